"""Carrying chains to a longer data record (ChmcContext.extended, sequential.extend_state, sequential_static_chmc) and the
log predictive score through the samplers (paths.FutureScore, `future_score=`).

extend_state is judged by what it promises: the head columns [u | v_0 | v_seq] of the longer record's position are the
source's, bit for bit; the tail's step normals are the picked candidate's keyed row (ctx.fill_normal, bitwise); `moved` --
the destination's own scan against the recursion that produced the spliced n -- stays under TOL max(1, |o|) / sigma, the
project's per-operator bound divided by sigma as the definition divides (o: the obs channel of the destination's path, from
oracle/py/models.py); the constraint is at rounding level (1e-9, the bound test_resolution.check_on_the_manifold holds
transfer_state to); the state is bitwise that of chmc_set_state on what chmc_get_state returns.  The drivers are re-derived
by hand with the documented seeds and compared bitwise.

Every GPU body has a `*_host_logic` twin on the TEST-ONLY emulation build."""
import os
import numpy as np
import pytest
from test_paths import path_by_models
from test_predictive import CASES as PCASES, prepared, sigma_of, key0, SEED, OFFSET
from test_resolution import make_ctx as plain_ctx, state_ops
from test_emu_logic import emu_lib  # noqa: F401
from manifold_mcmc_for_diffusions_amd import example_models as em

TOL = 1e-10
CONSTR = 1e-9  # test_resolution.check_on_the_manifold's bound on max |constraint| after transfer_state


def head_len(ctx):
    return ctx.U + ctx.V0 + ctx.T * ctx.S * ctx.V


def new_observations(case, ctx, H, per_chain):
    """y_new [H] or [B, H]: near the last observation, so that the candidates' weights are neither equal nor degenerate."""
    rng = np.random.default_rng(77)
    sig = 1.0 if case["model"] == "sir" else 0.1
    return case["y"][-1] + sig * rng.standard_normal((ctx.B, H) if per_chain else H)


def extend_body(name, H, n_cand, per_chain_y=False, per_chain_sigma=False):
    from manifold_mcmc_for_diffusions_amd.sequential import extend_state
    case, src = prepared(PCASES[name][0], per_chain_sigma=per_chain_sigma)
    B, T, S, V = src.B, src.T, src.S, src.V
    y_new = new_observations(case, src, H, per_chain_y)
    dst = src.extended(y_new)
    assert (dst.T, dst.B, dst.S, dst.Q) == (T + H, B, S, src.Q + H * S * V + H)
    y_src, sg_src = src.observations()
    y_dst, sg_dst = dst.observations()
    assert np.array_equal(y_dst[:, :T], y_src) and np.array_equal(y_dst[:, T:], np.broadcast_to(y_new, (B, H)))
    assert np.array_equal(sg_dst, sg_src) and (not per_chain_sigma or len(set(sg_dst.tolist())) == B)
    q_src = src.get_state(want_p=False, want_x_obs=False)[0]
    before = src.get_state()
    tr = extend_state(src, dst, SEED, draw=3, chain_offset=OFFSET, n_cand=n_cand)
    after = src.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]  # src is untouched
    st = state_ops(dst)
    q = st["q"]
    assert st["part"] == src.partition and not st["p"].any()
    h, nv = head_len(src), H * S * V
    assert q[:, :h].tobytes() == q_src[:, :h].tobytes()  # [u | v_0 | v_seq]: bit for bit
    rows = np.arange(B, dtype=np.int32)
    keys = np.array([key0(3) | int(r) for r in tr["picked"]], dtype=np.uint64)
    v_ref = src.fill_normal(SEED, rows, OFFSET + rows, keys, np.zeros((B, nv)))
    assert q[:, h:h + nv].tobytes() == v_ref.tobytes()  # the tail: the picked candidate's keyed normals
    assert (tr["picked"] >= 0).all() and (tr["picked"] < n_cand).all() and np.isfinite(tr["log_pred"]).all()
    assert ((tr["ess_cand"] >= 1 - 1e-12) & (tr["ess_cand"] <= n_cand + 1e-9)).all()
    # moved: dst's own scan against the recursion that produced the spliced n
    sig = sigma_of(dst, case, q) if not per_chain_sigma else sg_dst
    path = path_by_models(case["model"], q, dst.T, S, case["obs_interval"], dst.U)[:, S::S]
    o = em.MODELS[case["model"]].obs_func(path)[..., 0]
    bound = TOL * np.maximum(1.0, np.abs(o).max(1)) / sig
    n_ref = (y_dst - o) / sig[:, None]
    out = dict(moved=float((tr["moved"] / bound).max()), n=float(np.abs(q[:, h + nv:] - n_ref).max()),
               max_constr=tr["max_constr"], ess_min=float(tr["ess_cand"].min()), ess_max=float(tr["ess_cand"].max()))
    print(f"\n{name} H {H} n_cand {n_cand}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()) + " (moved: in units of its bound)")
    assert out["moved"] <= 1.0 and out["n"] <= 1e-9, out
    assert tr["max_constr"] < CONSTR and np.abs(st["constr"]).max() < CONSTR
    # bitwise the state chmc_set_state gives for what chmc_get_state returns
    dst.set_state(st["q"], None, st["xo"], int(st["part"]))
    again = state_ops(dst)
    for k in st:
        assert np.array_equal(st[k], again[k]), k
    r = dst.leapfrog_step(0.02)
    assert (r["status"] == 0).mean() > 0.7, r
    dst.close(), src.close()


def carried_and_refused_body():
    from manifold_mcmc_for_diffusions_amd.sequential import extend_state
    src = plain_ctx("fhn", 4, 2, 0.1, 4, R=2)
    src.simulate_observations(SEED)
    y, sg = src.observations()
    y_new = y[:, -1:] + 0.05
    # the metric is carried: per chain, through groups, shared, and none
    rng = np.random.default_rng(5)
    G = rng.standard_normal((2, src.U, src.U))
    src.set_metric(np.einsum("bij,bkj->bik", G, G) + 2 * np.eye(src.U), groups=np.array([0, 1, 1, 0]))
    dst = src.extended(y_new)
    assert dst.per_chain_metric and np.array_equal(dst.metrics(), src.metrics())
    assert np.array_equal(dst.observations()[0], np.concatenate([y, y_new], 1)) and np.array_equal(dst.observations()[1], sg)
    tr = extend_state(src, dst, SEED, n_cand=16)
    assert tr["max_constr"] < CONSTR and np.array_equal(dst.metrics(), src.metrics())
    again = dst.extended(np.array([0.1, 0.2, 0.3]))  # a 1-d array is [H]: the same new observations for every chain
    assert again.T == dst.T + 3 and np.array_equal(again.observations()[0][:, -3:], np.tile([0.1, 0.2, 0.3], (4, 1)))
    again.close()
    src.set_metric(np.diag([1.0, 2.0, 3.0, 4.0]))
    d2 = src.extended(y_new)
    assert not d2.per_chain_metric and np.array_equal(d2.metrics(), src.metrics())
    src.set_metric(None)
    d3 = src.extended(y_new)
    assert d3.M_0 is None
    # pairs that do not match are refused
    other_S = plain_ctx("fhn", 5, 4, 0.1, 4, R=2)
    other_B = plain_ctx("fhn", 5, 2, 0.1, 3, R=2)
    other_data = plain_ctx("fhn", 5, 2, 0.1, 4, R=2)  # zeros where src has its simulated data
    other_sigma = plain_ctx("fhn", 5, 2, 0.2, 4, R=2)
    other_model = plain_ctx("fhn_nb", 5, 2, 0.1, 4, R=2)
    same_T = src.sibling(2)
    for bad in (other_S, other_B, other_data, other_sigma, other_model, same_T):
        with pytest.raises(ValueError, match="extend_state"):
            extend_state(src, bad, SEED)
    with pytest.raises(ValueError, match="extend_state"):
        extend_state(dst, src, SEED)  # shorter
    with pytest.raises(ValueError):
        src.extended(np.zeros((3, 1)))
    noiseless = plain_ctx("fhn", 4, 2, None, 2, R=2)
    with pytest.raises(ValueError, match="observation noise"):
        extend_state(noiseless, noiseless.extended(np.zeros(1)), SEED)
    for c in (dst, d2, d3, other_S, other_B, other_data, other_sigma, other_model, same_T, noiseless, src):
        c.close()


def small_fit(B=4, T=4, T_all=6):
    """(ctx with T observations and on-manifold states, y_batches): the first T observations of a T_all-record simulated from
    a prior draw per chain (the longer context's own simulation), and the position truncated to them."""
    big = plain_ctx("fhn", T_all, 2, 0.1, B, R=2)
    big.simulate_observations(SEED)
    y, _ = big.observations()
    q, _, xo, _ = big.get_state()
    h = big.U + big.V0
    nvb = T_all * big.S * big.V
    ctx = plain_ctx("fhn", T, 2, 0.1, B, R=2)
    ctx.set_observations(y[:, :T])
    q_small = np.concatenate([q[:, :h + T * big.S * big.V], q[:, h + nvb:h + nvb + T]], 1)
    ctx.set_state(q_small, None, xo[:, :T], 0)
    assert np.abs(ctx.constr()).max() < 1e-12
    big.close()
    return ctx, [y[:, T + i:T + i + 1] for i in range(T_all - T)]


def driver_body():
    """T = 4 -> 5 -> 6, two warm-up transitions and two draws per stage; then every stage again by hand with seed + i."""
    from manifold_mcmc_for_diffusions_amd.sequential import sequential_static_chmc, extend_state
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_metric
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    seed = 11
    ctx, batches = small_fit()
    out = sequential_static_chmc(ctx, batches, n_warm_first=2, n_warm_next=2, n_main=2, n_step=2, step_size=0.05, seed=seed,
                                 n_cand=16, chain_offset=OFFSET)
    stages = out["stages"]
    keys = {"T", "seconds", "first_step_size", "final_step_size", "mean_accept_stat", "log_pred", "chain_log_pred", "ess_cand",
            "moved", "max_constr", "first_head"}
    assert [s["T"] for s in stages] == [4, 5, 6] and all(set(s) == keys for s in stages)
    assert out["heads"].shape[:2] == (4, 4) and out["ctx"].T == 6
    assert stages[0]["log_pred"] is None and stages[0]["moved"] is None and stages[0]["first_step_size"] == 0.05
    for prev, s in zip(stages, stages[1:]):
        assert s["first_step_size"] == prev["final_step_size"]  # the step sizes are handed on
        assert np.isfinite(s["log_pred"]) and np.isfinite(s["chain_log_pred"]).all() and s["chain_log_pred"].shape == (4,)
        assert np.isfinite(s["moved"]).all() and (s["ess_cand"] >= 1 - 1e-12).all() and (s["ess_cand"] <= 16 + 1e-9).all()
        assert s["max_constr"] < CONSTR
    for s in stages:
        assert s["seconds"] > 0 and 0 <= s["mean_accept_stat"] <= 1 and np.isfinite(s["final_step_size"])
    assert out["final_step_size"] == stages[-1]["final_step_size"]
    assert np.abs(out["ctx"].constr()).max() < 1e-8  # every chain on its manifold at the end
    # by hand
    cur, _ = small_fit()
    eps = 0.05
    for i in range(3):
        if i:
            nxt = cur.extended(batches[i - 1])
            transfer_metric(cur, nxt)
            tr = extend_state(cur, nxt, seed, draw=i, chain_offset=OFFSET, n_cand=16)
            assert tr["log_pred"].tobytes() == stages[i]["chain_log_pred"].tobytes()
            cur.close()
            cur = nxt
        assert cur.get_head(6).tobytes() == stages[i]["first_head"].tobytes(), i  # the stage's first state
        hand = sample_static_chmc(cur, 4, 2, eps, seed + i, n_adapt=2, chain_offset=OFFSET)
        eps = hand["final_step_size"]
        assert eps == stages[i]["final_step_size"], i
    for k in ("heads", "accept_stat", "step_size"):
        assert np.asarray(hand[k]).tobytes() == np.asarray(out[k]).tobytes(), k
    cur.close(), out["ctx"].close(), ctx.close()


def samplers_body(tmp_path):
    """FutureScore through both samplers: its [n_main, B] array is what direct calls give at the same states with the same
    draws, and the chain is bitwise what it is without it."""
    from manifold_mcmc_for_diffusions_amd.paths import FutureScore, log_mean_exp
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    ctx, batches = small_fit()
    q0, _, xo0, _ = ctx.get_state()
    y = np.concatenate(batches, 1)  # [B, 2]
    samplers = {"static": lambda **kw: sample_static_chmc(ctx, 4, 2, 0.03, seed=3, n_adapt=2, chain_offset=OFFSET, **kw),
                "dynamic": lambda **kw: sample_dynamic_chmc(ctx, 4, 0.03, seed=3, n_adapt=2, max_tree_depth=2,
                                                            chain_offset=OFFSET, **kw)}
    for name, run in samplers.items():
        ctx.set_state(q0, None, xo0, 0)
        plain = run()
        assert "future_score" not in plain
        ctx.set_state(q0, None, xo0, 0)
        fs = FutureScore(ctx, y, n_cand=70, seed=19)
        direct = []

        def by_hand(it, *rest):
            if it >= 2:
                direct.append(ctx.score_future_device(19, it, OFFSET, y, 70)[0])

        scored = run(future_score=fs, callback=by_hand)
        for k in ("heads", "accept_stat", "step_size"):
            assert np.asarray(plain[k]).tobytes() == np.asarray(scored[k]).tobytes(), (name, k)
        lp = fs.log_pred
        assert lp.shape == (2, 4) and lp.tobytes() == np.stack(direct).tobytes() and np.isfinite(lp).all()
        assert scored["future_log_pred"].tobytes() == lp.tobytes()
        pool = fs.pooled()
        assert set(pool) == {"log_pred", "chain_log_pred", "mcse", "n_draws"} == set(scored["future_score"])
        m = lp.max()
        assert abs(pool["log_pred"] - (m + np.log(np.exp(lp - m).mean()))) <= 1e-12
        np.testing.assert_allclose(pool["chain_log_pred"], [log_mean_exp(lp[:, c]) for c in range(4)], rtol=0, atol=1e-12)
        assert pool["n_draws"] == 2 and pool["mcse"] >= 0
        path = fs.save(str(tmp_path / name))
        assert os.path.basename(path) == "future_score.npz"
        z = np.load(path)
        assert z["log_pred"].tobytes() == lp.tobytes() and float(z["pooled_log_pred"]) == pool["log_pred"]
    assert log_mean_exp(np.array([-np.inf, -np.inf])) == -np.inf and log_mean_exp(np.array([0.0, -np.inf])) == -np.log(2.0)
    with pytest.raises(ValueError):
        FutureScore(ctx, np.zeros((3, 1)))
    with pytest.raises(ValueError):
        FutureScore(ctx, np.array([np.nan]))
    ctx.close()


EXTEND = [("fhn_v2", 1, 70, False, False), ("fhn_v2", 2, 5, True, False), ("fhn_v2", 2, 64, True, True),
          ("sir_v3", 1, 70, False, False), ("fhn_varsigma", 2, 130, True, False)]


# ------------------------------------------------------------------------------------------------------ emulation build
@pytest.mark.parametrize("name,H,n_cand,per_chain_y,per_chain_sigma", EXTEND)
def test_extend_state_host_logic(emu_lib, name, H, n_cand, per_chain_y, per_chain_sigma):  # noqa: F811
    extend_body(name, H, n_cand, per_chain_y, per_chain_sigma)


def test_metric_is_carried_and_mismatches_are_refused_host_logic(emu_lib):  # noqa: F811
    carried_and_refused_body()


def test_sequential_driver_host_logic(emu_lib):  # noqa: F811
    driver_body()


def test_future_score_through_the_samplers_host_logic(emu_lib, tmp_path):  # noqa: F811
    samplers_body(tmp_path)


# ---------------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("name,H,n_cand,per_chain_y,per_chain_sigma", EXTEND)
def test_extend_state(name, H, n_cand, per_chain_y, per_chain_sigma):
    _hip()
    extend_body(name, H, n_cand, per_chain_y, per_chain_sigma)


@pytest.mark.gpu
def test_metric_is_carried_and_mismatches_are_refused():
    _hip()
    carried_and_refused_body()


@pytest.mark.gpu
def test_sequential_driver():
    _hip()
    driver_body()


@pytest.mark.gpu
def test_future_score_through_the_samplers(tmp_path):
    _hip()
    samplers_body(tmp_path)
