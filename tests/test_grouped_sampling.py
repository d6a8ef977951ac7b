"""The Python layer over per-chain observations, on the CPU (TEST-ONLY emulation build): GridWorkload bookkeeping and
sharding, per-group step-size adaptation in both samplers, per-group summaries, the SBC rank statistics, and two gloo ranks
whose boundary cuts through a group."""
import os
import subprocess
import sys
import numpy as np
import pytest
from test_emu_logic import emu_lib  # noqa: F401  (fixture)
from test_distributed_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))


def _cells(sigmas, T=6):
    from manifold_mcmc_for_diffusions_amd import example_models as em
    return [(em.simulate_fhn_observations(T, 0.2, 50, seed=5 + i, sigma=s)[:, 0], s) for i, s in enumerate(sigmas)]


def _grid(sigmas, n, **kw):
    from manifold_mcmc_for_diffusions_amd.workload import GridWorkload
    return GridWorkload(_cells(sigmas), n, num_steps_per_obs=4, num_obs_per_subseq=2, seed=7, **kw)


def test_grid_workload_bookkeeping_and_sharding(emu_lib):  # noqa: F811
    """groups, chain_offset and total_chains; every chain carries its cell's (y, sigma) and starts on the manifold of its own
    data; a shard that cuts through a cell holds the same chains, bit for bit, as the whole grid."""
    sig = (0.05, 0.1, 0.2)
    w = _grid(sig, 2)
    assert (w.total_chains, w.n_groups, w.B, w.chain_offset) == (6, 3, 6, 0)
    assert np.array_equal(w.groups, [0, 0, 1, 1, 2, 2]) and np.array_equal(w.cell_chains(1), [2, 3])
    y, s = w.ctx.observations()
    assert np.array_equal(y, w.cell_y[w.groups]) and np.array_equal(s, np.asarray(sig)[w.groups])
    assert np.abs(y[0] - y[2]).max() > 0 and np.abs(w.ctx.constr()).max() < 1e-9
    q, _, xo, _ = w.ctx.get_state()
    assert np.array_equal(xo[:, :, 0], y)  # x_obs_seq_init = [y of the chain's own cell, 0.5 N(0, 1)]
    w.ctx.close()
    for off, cnt in ((0, 3), (3, 3), (1, 4)):
        part = _grid(sig, 2, chain_offset=off, num_chains=cnt)
        assert (part.total_chains, part.B) == (6, cnt) and np.array_equal(part.groups, np.arange(off, off + cnt) // 2)
        assert np.array_equal(part.ctx.get_state()[0], q[off:off + cnt])
        assert np.array_equal(part.ctx.observations()[0], y[off:off + cnt])
        part.ctx.close()
    with pytest.raises(ValueError, match="shard"):
        _grid(sig, 2, chain_offset=4, num_chains=3)
    with pytest.raises(ValueError, match="sigma must be a number for every cell"):
        from manifold_mcmc_for_diffusions_amd.workload import GridWorkload
        GridWorkload([(np.zeros(6), 0.1), (np.zeros(6), None)], 2)


def test_static_sampler_adapts_one_step_size_per_group(emu_lib):  # noqa: F811
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.adapters import OnlineBlockDiagonalMetricAdapter
    w = _grid((0.02, 0.5), 3)
    res = sample_static_chmc(w.ctx, 30, 2, 0.05, seed=3, n_adapt=26, groups=w.groups, n_groups=2)
    assert res["step_size"].shape == (30, 2) and res["group_accept_stat"].shape == (30, 2)
    assert res["final_step_size"].shape == (2,) and res["final_step_size"][0] != res["final_step_size"][1]
    assert (res["group_accept_stat"][:, 0] != res["group_accept_stat"][:, 1]).any()  # ... each on its own accept statistic
    assert np.abs(w.ctx.constr()).max() < 1e-8
    with pytest.raises(ValueError, match="one M_0 per context"):
        sample_static_chmc(w.ctx, 4, 2, 0.05, seed=3, n_adapt=4, groups=w.groups, metric_adapter=OnlineBlockDiagonalMetricAdapter(4))
    with pytest.raises(ValueError, match="groups must"):
        sample_static_chmc(w.ctx, 4, 2, 0.05, seed=3, groups=w.groups[:-1])
    w.ctx.close()


def _one_group_runs(sampler, **kw):
    """The same sampler call on two identical one-cell grids: with groups = 0 for every chain, and without `groups`."""
    out = []
    for grouped in (True, False):
        w = _grid((0.1,), 4)
        extra = dict(groups=w.groups, n_groups=1) if grouped else {}
        out.append(sampler(w.ctx, seed=3, **kw, **extra))
        w.ctx.close()
    return out


def test_static_sampler_single_group_reproduces_the_ungrouped_call(emu_lib):  # noqa: F811
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    a, b = _one_group_runs(sample_static_chmc, n_iter=12, n_step=2, step_size=0.05, n_adapt=8)
    assert np.array_equal(a["heads"], b["heads"]) and np.array_equal(a["accept_stat"], b["accept_stat"])
    assert np.array_equal(a["step_size"][:, 0], b["step_size"]) and a["final_step_size"][0] == b["final_step_size"]
    assert np.array_equal(a["group_accept_stat"][:, 0], b["accept_stat"])


def test_dynamic_sampler_group_step_sizes(emu_lib):  # noqa: F811
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    w = _grid((0.02, 0.5), 3)
    res = sample_dynamic_chmc(w.ctx, 14, 0.05, seed=3, n_adapt=12, max_tree_depth=3, groups=w.groups, n_groups=2)
    eps = res["group_step_sizes"]
    assert eps.shape == (2,) and eps[0] != eps[1]
    for g in range(2):  # the main-phase step size of a group: the mean of ITS chains' adapted step sizes
        assert eps[g] == res["adapted_step_sizes"][w.groups == g].sum() / 3
    assert np.isfinite(res["heads"]).all()
    w.ctx.close()
    a, b = _one_group_runs(sample_dynamic_chmc, n_iter=8, step_size=0.05, n_adapt=6, max_tree_depth=3)
    assert np.array_equal(a["heads"], b["heads"]) and np.array_equal(a["step_size"], b["step_size"])
    assert a["final_step_size"] == b["final_step_size"] and a["group_step_sizes"][0] == b["final_step_size"]


def test_summaries_per_group(emu_lib, tmp_path):  # noqa: F811
    """traces.summarize(groups=...) against per-group calls of the function as it was; summary.json of a grouped run holds
    one table per cell."""
    import json
    from manifold_mcmc_for_diffusions_amd.traces import summarize
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    rng = np.random.default_rng(0)
    traces = {"a": rng.standard_normal((7, 40)) + np.arange(7)[:, None], "b": rng.standard_normal((7, 40, 2))}
    groups = np.array([0, 0, 0, 2, 2, 5, 5])
    got = summarize(traces, groups=groups)
    assert sorted(got) == [0, 2, 5]
    for g in (0, 2, 5):
        assert got[g] == summarize({k: v[groups == g] for k, v in traces.items()})
    assert got[0]["mean"]["a"] != got[5]["mean"]["a"]
    assert summarize(traces, ["a"], groups=groups)[2] == summarize({"a": traces["a"][groups == 2]})
    w = _grid((0.05, 0.2), 2)
    d = str(tmp_path / "out")
    res = sample_static_chmc(w.ctx, 8, 2, 0.05, seed=3, n_adapt=4, trace_dir=d, groups=w.groups, n_groups=2)
    s = json.load(open(os.path.join(d, "summary.json")))
    assert sorted(s["groups"]) == ["0", "1"] and s["final_integrator_step_size"] == list(res["final_step_size"])
    pos = np.load(os.path.join(d, "trace_pos_head.npy"))[:, 4:]
    assert s["groups"]["1"]["mean"]["pos_head[0]"] == float(pos[2:, :, 0].mean())
    assert s["total_leapfrog_step_calls"] == 8 * 2
    w.ctx.close()


def test_sbc_ranks_and_uniformity():
    from manifold_mcmc_for_diffusions_amd import sbc
    post = np.arange(10.0).reshape(1, 10, 1) * np.ones((3, 1, 2))           # draws 0 .. 9 for 3 data sets, 2 parameters
    prior = np.array([[-1.0, 9.5], [4.5, 0.0], [3.0, 100.0]])
    assert np.array_equal(sbc.ranks(prior, post), [[0, 10], [5, 0], [3, 10]])  # (a tie is not "below")
    with pytest.raises(ValueError):
        sbc.ranks(prior[:2], post)
    # known chi^2 values: L = 7 (8 rank values), 4 bins of 2 values each, 8 data sets
    r = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [5, 0], [6, 0], [7, 0]])
    stat, p = sbc.uniformity(r, L=7, bins=4)
    assert stat[0] == 0.0 and p[0] == 1.0 and abs(stat[1] - 24.0) < 1e-12   # (8 - 2)^2 / 2 + 3 (0 - 2)^2 / 2
    assert abs(p[1] - 2.4982e-05) < 1e-8                                      # P(chi^2(3) >= 24)
    assert abs(sbc.chi2_sf(3.84145882, 1) - 0.05) < 1e-8 and abs(sbc.chi2_sf(16.9189776, 9) - 0.05) < 1e-8
    assert abs(sbc.chi2_sf(2.0, 2) - np.exp(-1.0)) < 1e-14
    # uniform ranks pass, constant ranks do not
    rng = np.random.default_rng(2024)
    L, D = 63, 400
    stat, p = sbc.uniformity(rng.integers(0, L + 1, size=(D, 5)), L, bins=16)
    assert (p > 0.01).all(), p
    stat, p = sbc.uniformity(np.zeros((D, 5), dtype=np.int64), L, bins=16)
    assert (p < 1e-6).all() and np.allclose(stat, D * 15.0)
    # unequal bins (L + 1 = 10 values in 4 bins of 2, 3, 2, 3): the expected counts follow the bin widths
    stat, p = sbc.uniformity(np.repeat(np.arange(10), 4)[:, None], L=9, bins=4)
    assert abs(stat[0]) < 1e-12 and p[0] == 1.0
    with pytest.raises(ValueError):
        sbc.uniformity(np.array([[8]]), L=7, bins=4)


def test_sbc_on_simulated_observations(emu_lib):  # noqa: F811
    """The pieces of examples/fhn_sbc.py together: the prior draw of every chain is the position simulate_observations
    leaves (u = the first components), and ranks() takes it with the thinned posterior draws.  No statistical assertion."""
    from manifold_mcmc_for_diffusions_amd import sbc
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    ctx = ChmcContext("fhn", 0.2, 4, 2, np.zeros(6), sigma=0.3, num_chains=5)
    ctx.simulate_observations(11)
    prior_u = ctx.get_head(4)
    assert np.abs(ctx.constr()).max() <= 1e-12
    res = sample_dynamic_chmc(ctx, 6, 0.1, seed=3, n_adapt=2, max_tree_depth=3, groups=np.arange(5), n_groups=5, n_head=4)
    r = sbc.ranks(prior_u, res["heads"][2:].transpose(1, 0, 2))
    assert r.shape == (5, 4) and r.min() >= 0 and r.max() <= 4
    ctx.close()


def test_two_ranks_adapt_the_step_size_of_every_group(emu_lib, tmp_path):  # noqa: F811
    """Two gloo ranks of 3 chains over 3 cells x 2 chains: the middle cell has a chain on either rank.  The group accept
    statistics are summed over ranks (one vector of 2 G numbers per transition), so both ranks use the same G step sizes,
    equal to the single-rank run's."""
    import grouped_dist_worker as gw
    n_iter, G = 12, len(gw.SIGMAS)
    single = gw.run_sampler(n_iter, 0, 1)
    out = str(tmp_path / "gathered.npy")
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "grouped_dist_worker.py"), out, str(n_iter)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, o.decode()[-2000:]
    gathered = np.load(out)
    hist = gathered[:, 6:]
    assert (hist == hist[0]).all()                                   # every chain / rank saw the same histories
    eps = hist[0, :n_iter * G].reshape(n_iter, G)
    assert len({tuple(e) for e in eps[:n_iter - 2]}) > 2 and (eps[-1] != eps[-1, 0]).any()  # adapted, and apart
    np.testing.assert_allclose(gathered, single, rtol=1e-12, atol=1e-12)


def test_finder_rows_stay_with_their_chain_under_per_chain_data():
    """init._adam_on_device with the stand-ins of test_keyed_init: in a context with per-chain observations row c is judged
    against chain c's data, so every try of a chain runs in the chain's own row -- and the winners (try numbers, points) are
    those of the schedule that hands rows around (shared data)."""
    from types import SimpleNamespace
    from manifold_mcmc_for_diffusions_amd import init
    from test_keyed_init import stand_ins
    B, T, nuv, off = 48, 6, 12, 100
    res = {}
    for own in (False, True):
        ctx = SimpleNamespace(B=B, Q=nuv + T, T=T, U=3, sigma=np.full(B, 1.0) if own else 1.0, variable_sigma=False,
                              per_chain_observations=own)
        rec = []
        u_v, tries, status = init._adam_on_device(ctx, None, 0.1, 1000, 100, 1.0, 0.8, 100, 10, None, max_parallel_tries=16,
                                                  _calls=stand_ins(B, T, nuv, rec), seed=5, chain_offset=off)
        res[own] = (u_v.numpy().copy(), tries.copy(), rec)
    assert all(r == s - off for r, s, k in res[True][2]) and any(r != s - off for r, s, k in res[False][2])
    assert res[True][1].max() >= 3 and len(res[True][2]) == int(res[True][1].sum())  # tries one after the other, none wasted
    assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][0], res[False][0])
