"""The latent path x(t) of a chain (chmc_generate_x_seq*, generate_from_model's x_seq) and its running posterior moments
(chmc_path_stats_update_device, paths.PathPosterior), judged by two references that share no code with the device scan:

  (a) at the observation points, c_oracle.OracleSystem.generate_x_obs_seq(q);
  (b) at every emitted point, a loop over oracle.py.models' hand-written forward_func / generate_z / generate_x_0.

Bound: 1e-10 relative in the infinity norm with scale max(1, |ref|) (the per-operator bound).  Fair-case
condition, asserted for every case, state and chain: (a) and (b) agree to 1e-11.  No chain is dropped from a comparison.
The seeds were screened on the emulation build (every `*_host_logic` test below); seeds that failed and must not be
used: REPLACED.

Every GPU body has a `*_host_logic` twin on the TEST-ONLY emulation build (generic functors: KPath for both forms, the host
sequencing, the Python layer and the reference side of every comparison, to the same bounds)."""
import math
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx
from test_hip_autodiff_parity import distinct_on_manifold_chains, spread_chains_by_stepping
from test_emu_logic import emu_lib  # noqa: F401
from test_distributed_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL, FAIR = 1e-10, 1e-11

# id: model, T, S, R, noisy, gaussian, var_sigma, obs_interval, chains, strides, seed
CASES = {
    "fhn_l48_idle_lanes": ("fhn", 6, 8, 2, True, False, False, None, 5, (1, 4, 8), 31),        # fewer steps than lanes
    "fhn_l64_one_step_per_lane": ("fhn", 8, 8, 3, True, False, False, None, 5, (1, 2, 8), 32),
    "fhn_l65_s13": ("fhn", 5, 13, 2, True, False, False, None, 5, (1, 13), 33),  # m = 2, trailing lanes empty, S % 8 != 0
    "fhn_l520_m9": ("fhn", 13, 40, 5, True, False, False, None, 5, (1, 4, 8, 40), 34),  # segment ends, emit indices interleave
    "fhn_noiseless_gauss": ("fhn", 7, 8, 3, False, True, False, None, 5, (1, 4, 8), 35),
    "fhn_nb_noiseless_gauss": ("fhn_nb", 7, 8, 3, False, True, False, None, 5, (1, 4, 8), 36),
    "fhn_varsigma": ("fhn", 12, 16, 5, True, False, True, None, 5, (1, 4, 16), 37),             # U = 5
    "sir_one_block": ("sir", 14, 8, 14, True, False, False, 0.25, 5, (1, 2, 8), 38),             # X = V = 3
    "sir_two_blocks": ("sir", 26, 24, 13, True, False, False, 0.1, 5, (1, 6, 24), 39),
    "fhn_b130": ("fhn", 12, 16, 5, True, False, False, None, 130, (1, 4, 16), 40),  # several workgroups, the last one partial
}
REPLACED = {}  # id: {seed: why}; no seed failed the screening
MOMENTS = {"fhn": ("fhn", 6, 8, 2, True, 4, 2, 41), "fhn_nb": ("fhn_nb", 6, 8, 2, True, 4, 4, 42),
           "sir": ("sir", 6, 8, 3, True, 4, 2, 43)}  # model, T, S, R, noisy, chains, stride, seed
SAMPLER = ("fhn", 8, 8, 3, 4, 44)  # noiseless; model, T, S, R, chains, seed


def build_case(cfg):
    model, T, S, R, noisy, gaussian, var_sigma, oi, B, _, seed = cfg
    if noisy:
        return distinct_on_manifold_chains(model, T, S, R, B, seed, obs_interval=oi, var_sigma=var_sigma, gaussian=gaussian)
    return make_case(model, T, S, R, False, B=B, seed=seed, obs_interval=oi, gaussian=gaussian)


def on_manifold_points(ctx, case, rng):
    """Distinct on-manifold points of all chains in partition 0 (noisy data: the case's own; noiseless: reached by stepping)."""
    if case["noisy"]:
        return case["q"], case["x_obs"]
    return spread_chains_by_stepping(ctx, case, 0, rng)


def rel(a, ref):
    return float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref))))


def path_by_models(model, q, T, S, obs_interval, U):
    """Reference (b): [B, T S + 1, X] by a loop over the hand-written closed forms of oracle/py/models.py (all chains of `q`
    advance together, one forward_func call per step)."""
    import torch
    from oracle.py import models as om
    m = om.MODELS[model]
    dl = obs_interval / S
    qt = torch.from_numpy(np.ascontiguousarray(q))
    zs = [m.generate_z(qc[:U]) for qc in qt]
    x = torch.stack([m.generate_x_0(z, qc[U:U + m.dim_v_0]) for z, qc in zip(zs, qt)], 1)  # [X, B]
    z = torch.stack(zs, 1)
    v = qt[:, U + m.dim_v_0:U + m.dim_v_0 + T * S * m.dim_v].reshape(len(q), T * S, m.dim_v)
    out = [x]
    for s in range(T * S):
        x = m.forward_func(z, x, v[:, s].T, dl)
        out.append(x)
    return torch.stack(out, 0).permute(2, 0, 1).numpy().copy()


def references(ctx, case, q):
    full = path_by_models(case["model"], q, ctx.T, ctx.S, case["obs_interval"], ctx.U)
    at_obs = np.stack([case["osys"].generate_x_obs_seq(q[c]) for c in range(ctx.B)])
    fair = rel(full[:, ctx.S::ctx.S], at_obs)
    assert fair <= FAIR, f"the two references differ by {fair:.2e}: not a fair case"
    return full, at_obs


def check_state(ctx, case, strides, label, on_device, par, settled, switched=False):
    """The checks of one state: both forms against both references for every stride; the launch counters and sweeps.
    switched: the state comes right out of a partition switch, so the context's x_obs is fresh (k_xobs_par; KXobs on the
    emulation build) and is held against the C oracle and against the path at stride S."""
    q, _, x_obs, _ = ctx.get_state(want_p=False, want_x_obs=switched)
    full, at_obs = references(ctx, case, q)
    worst = 0.0
    for stride in strides:
        n_p, times = ctx.path_points(stride)
        per_obs = ctx.S // stride
        assert n_p == ctx.T * per_obs + 1 and times[per_obs] == pytest.approx(case["obs_interval"])
        d0 = ctx.diagnostics()
        cur, sw = ctx.generate_x_seq(stride, return_sweeps=True)
        d1 = ctx.diagnostics()
        given = ctx.generate_x_seq(stride, q=q)
        d2 = ctx.diagnostics()
        assert cur.shape == given.shape == (ctx.B, n_p, ctx.X)
        for name, x in (("current", cur), ("given q", given)):
            e_b, e_a = rel(x, full[:, ::stride]), rel(x[:, per_obs::per_obs], at_obs)
            worst = max(worst, e_a, e_b)
            print(f"  {label} stride {stride} {name}: vs models {e_b:.2e}, vs C oracle at the observations {e_a:.2e}")
            assert e_b <= TOL and e_a <= TOL, (label, stride, name, e_a, e_b)
        if switched and stride == ctx.S:
            e_o, e_p = rel(x_obs, at_obs), rel(x_obs, cur[:, per_obs::per_obs])
            worst = max(worst, e_o, e_p)
            print(f"  {label}: x_obs of the switch vs C oracle {e_o:.2e}, vs the path at stride {stride} {e_p:.2e}")
            assert e_o <= TOL and e_p <= 1e-12, (label, e_o, e_p)
        assert d2["path_seq_launches"] == d1["path_seq_launches"] + 1 and d2["path_par_launches"] == d1["path_par_launches"]
        if on_device:
            agree = rel(cur, given)
            print(f"  {label} stride {stride}: forms agree to {agree:.2e}; sweeps {sw.tolist() if ctx.B <= 8 else np.bincount(sw)}")
            assert agree <= 1e-12
            if par:
                assert d1["path_par_launches"] == d0["path_par_launches"] + 1 and d1["path_seq_launches"] == d0["path_seq_launches"]
                assert ((sw >= 0) & (sw <= 8)).all(), sw
                if settled:
                    assert (sw <= 3).all(), sw
            else:  # CHMC_COMPACT_ROWS=0: the sequential pass
                assert d1["path_seq_launches"] == d0["path_seq_launches"] + 1 and d1["path_par_launches"] == d0["path_par_launches"]
                assert not sw.any()
        else:
            assert d1["path_seq_launches"] == d0["path_seq_launches"] + 1 and d1["path_par_launches"] == 0
            np.testing.assert_array_equal(cur, given)
    return worst


def path_body(name, on_device=True, par=True):
    cfg = CASES[name]
    case = build_case(cfg)
    ctx = make_ctx(case)
    strides = cfg[9]
    assert all(ctx.S % s == 0 for s in strides) and 1 in strides and ctx.S in strides
    rng = np.random.default_rng(cfg[10] + 1000)
    q_on, xo = on_manifold_points(ctx, case, rng)
    B = ctx.B
    # 1: on the manifold, two integrator steps
    ctx.set_state(q_on, rng.standard_normal((B, ctx.Q)), xo, 0)
    ctx.project_onto_cotangent_space()
    dt = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 if case["model"] == "sir" else 0.04)
    for _ in range(2):
        r = ctx.leapfrog_step(dt)
    print(f"\n{name}: L={ctx.T * ctx.S} K={ctx.K} RM={ctx.RM}; steps ended with status {np.bincount(r['status'] + 1)}")
    worst = check_state(ctx, case, strides, "after two steps", on_device, par, True)
    # 2, 3: right after a partition switch, and after the second one
    ctx.switch_partition()
    worst = max(worst, check_state(ctx, case, strides, "after a switch", on_device, par, True, switched=True))
    ctx.switch_partition()
    worst = max(worst, check_state(ctx, case, strides, "after two switches", on_device, par, True, switched=True))
    # 4: off the manifold: large junction defects in the stored trajectory
    ctx.set_state(q_on + 0.01 * rng.standard_normal(q_on.shape), None, xo, 0)
    worst = max(worst, check_state(ctx, case, strides, "off the manifold", on_device, par, False))
    ctx.close()
    return worst


def welford(xs, masks, obs):
    """The recurrence of KPathWelford in NumPy over stacked paths xs [draw][B, NP, X] with masks [draw][B]."""
    v0 = np.concatenate([xs[0], obs(xs[0])], -1)
    n, mean, m2 = np.zeros(v0.shape[0], dtype=np.int64), np.zeros_like(v0), np.zeros_like(v0)
    for x, mk in zip(xs, masks):
        v = np.concatenate([x, obs(x)], -1)
        mk = np.asarray(mk) != 0
        n = n + mk
        nn = np.maximum(n, 1)[:, None, None].astype(np.float64)
        d = v - mean
        mean_new = mean + d / nn
        m2_new = m2 + d * (v - mean_new)
        mean = np.where(mk[:, None, None], mean_new, mean)
        m2 = np.where(mk[:, None, None], m2_new, m2)
    return n, mean, m2


def moments_body(model):
    from manifold_mcmc_for_diffusions_amd import example_models as em
    from manifold_mcmc_for_diffusions_amd.paths import PathPosterior
    m_, T, S, R, noisy, B, stride, seed = MOMENTS[model]
    case = distinct_on_manifold_chains(m_, T, S, R, B, seed)
    ctx = make_ctx(case)
    rng = np.random.default_rng(seed + 1000)
    ctx.set_state(case["q"], rng.standard_normal((B, ctx.Q)), case["x_obs"], 0)
    ctx.project_onto_cotangent_space()
    pp = PathPosterior(ctx, stride)
    xs, masks = [], []
    dt = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 if model == "sir" else 0.04)
    for k in range(4):
        if k:
            assert (ctx.leapfrog_step(dt)["status"] == 0).all()
        mask = np.array([1, 0, 1, 1], dtype=np.int32) if k == 2 else None
        before = pp.moments()
        pp.update(mask)
        after = pp.moments()
        if k == 2:  # chain 1 sat this one out: its buffers are bitwise what they were
            for a, b in zip(before, after):
                assert a[1].tobytes() == b[1].tobytes()
            assert after[0].tolist() == [3, 2, 3, 3]
        xs.append(ctx.generate_x_seq(stride))
        np.testing.assert_array_equal(pp.last_paths(), xs[-1])
        masks.append(np.ones(B, dtype=np.int32) if mask is None else mask)
    obs = em.MODELS[model].obs_func
    n_ref, mean_ref, m2_ref = welford(xs, masks, obs)
    n, mean, m2 = pp.moments()
    assert n.tolist() == n_ref.tolist() == [4, 3, 4, 4]
    e_mean, e_m2 = rel(mean, mean_ref), rel(m2, m2_ref)
    print(f"\n{model}: mean {e_mean:.2e}, m2 {e_m2:.2e}")
    assert e_mean <= 1e-12 and e_m2 <= 1e-12
    n2, mean2, var = pp.per_chain()
    np.testing.assert_array_equal(n2, n), np.testing.assert_array_equal(mean2, mean)
    np.testing.assert_array_equal(var, m2 / (n - 1)[:, None, None])
    # pooled: NumPy's mean and variance over all (chain, draw) paths
    draws = np.stack([np.concatenate([x[c], obs(x[c])], -1) for x, mk in zip(xs, masks) for c in range(B) if mk[c]])
    pool = pp.pooled()
    assert pool["n"] == len(draws) == 15
    e_pm, e_pv = rel(pool["mean"], draws.mean(0)), rel(pool["var"], draws.var(0, ddof=1))
    print(f"  pooled mean {e_pm:.2e}, variance {e_pv:.2e}")
    assert e_pm <= 1e-12 and e_pv <= 1e-12
    np.testing.assert_array_equal(pool["sd"], np.sqrt(pool["var"]))
    ctx.close()


def shard_body():
    """6 chains as one context and as 2 x 3: paths and moments bitwise the same chain for chain."""
    from manifold_mcmc_for_diffusions_amd.paths import PathPosterior
    case = distinct_on_manifold_chains("fhn", 8, 8, 3, 6, 45)
    dts = np.array([0.04, -0.04, 0.05, 0.03, -0.05, 0.02])
    mom = np.random.default_rng(46).standard_normal((6, case["q"].shape[1]))

    def run(sl):
        sub = dict(case, B=sl.stop - sl.start)
        ctx = make_ctx(sub)
        ctx.set_state(case["q"][sl], mom[sl], case["x_obs"][sl], 0)
        ctx.project_onto_cotangent_space()
        pp = PathPosterior(ctx, 2)
        for _ in range(2):
            ctx.leapfrog_step(dts[sl])
            ctx.switch_partition()
            pp.update()
        out = (ctx.generate_x_seq(2),) + pp.moments()
        ctx.close()
        return out

    whole = run(slice(0, 6))
    assert whole[1].tolist() == [2] * 6
    for h in range(2):
        sl = slice(3 * h, 3 * h + 3)
        for a, b in zip(whole, run(sl)):
            assert np.array_equal(a[sl], b)


def samplers_body(tmp_path):
    """Both samplers on fhn noiseless T=8, S=8, R=3 with a PathPosterior: the chain is what it is without one, bitwise; every
    post-warm-up state was counted; the observed channel of every chain's mean path hits the data at the observation times
    (noiseless observations: the constraint pins it at every draw, to the junction defects of the retraction.  Measured
    maximum on the emulation build: 2.6e-15 static, 1.1e-15 dynamic -- Newton's last iteration leaves the constraint far
    below its tolerance; 1.7e-15 / 1.8e-15 on the device.  The body also holds it below 1e-8, 100 x under the bound 1e-6)."""
    from manifold_mcmc_for_diffusions_amd.paths import PathPosterior
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    model, T, S, R, B, seed = SAMPLER
    case = make_case(model, T, S, R, False, B=B, seed=seed)
    ctx = make_ctx(case)
    q_on, xo = spread_chains_by_stepping(ctx, case, 0, np.random.default_rng(seed + 1000))
    samplers = {"static": lambda **kw: sample_static_chmc(ctx, 6, 3, 0.03, seed=3, n_adapt=2, **kw),
                "dynamic": lambda **kw: sample_dynamic_chmc(ctx, 6, 0.03, seed=3, n_adapt=2, max_tree_depth=2, **kw)}
    for name, run in samplers.items():
        ctx.set_state(q_on, None, xo, 0)
        plain = run()
        assert "path_posterior" not in plain
        ctx.set_state(q_on, None, xo, 0)
        pp = PathPosterior(ctx, 4)
        with_pp = run(path_posterior=pp)
        for k in ("heads", "accept_stat", "step_size"):
            assert np.asarray(plain[k]).tobytes() == np.asarray(with_pp[k]).tobytes(), (name, k)
        assert plain["final_step_size"] == with_pp["final_step_size"]
        n, mean, _ = pp.per_chain()
        assert n.tolist() == [4] * B
        pool = pp.pooled()
        assert set(with_pp["path_posterior"]) == set(pool) and with_pp["path_posterior"]["n"] == pool["n"] == 4 * B
        for k in ("mean", "var", "sd", "m2"):
            np.testing.assert_array_equal(with_pp["path_posterior"][k], pool[k])
        per_obs = S // 4
        defect = np.abs(mean[:, per_obs::per_obs, -1] - case["y"][None, :]).max()
        print(f"\n{name}: observed channel of the per-chain mean paths vs y at the observations: max {defect:.2e}; "
              f"moved {not np.array_equal(with_pp['heads'][-1], with_pp['heads'][0])}")
        assert defect <= 1e-6
        assert defect <= 1e-8, "less than 100 x margin under 1e-6: choose another seed"
        path = pp.save(str(tmp_path / name))
        assert os.path.basename(path) == "path_posterior.npz"
        z = np.load(path)
        np.testing.assert_array_equal(z["times"], pp.times), np.testing.assert_array_equal(z["n"], n)
        np.testing.assert_array_equal(z["mean"], pool["mean"]), np.testing.assert_array_equal(z["sd"], pool["sd"])
        np.testing.assert_array_equal(z["chain_mean"], mean)
        assert int(z["pooled_n"]) == 4 * B and int(z["stride"]) == 4
    ctx.close()


def surface_body():
    """system.generate_from_model for one state and for a batch larger than the context."""
    import manifold_mcmc_for_diffusions_amd as mm
    from manifold_mcmc_for_diffusions_amd import example_models as em
    case = distinct_on_manifold_chains("fhn", 6, 8, 2, 3, 47)
    system = mm.ConditionedDiffusionConstrainedSystem(
        0.2, 8, 2, case["y"][:, None], em.fhn.dim_z, em.fhn.dim_x, em.fhn.dim_v, em.fhn.forward_func, em.fhn.generate_x_0,
        em.fhn.generate_z, em.fhn.obs_func, generate_σ=0.1, dim_v_0=em.fhn.dim_v_0, num_chains=2)
    full = path_by_models("fhn", case["q"], 6, 8, 0.2, 4)
    x_seq, y_seq, z, x_0 = mm.generate_from_model(system, case["q"], stride=2)
    assert x_seq.shape == (3, 25, 2) and y_seq.shape == (3, 6, 1) and z.shape == (3, 4) and x_0.shape == (3, 2)
    assert rel(x_seq, full[:, ::2]) <= TOL and rel(x_0, full[:, 0]) <= 1e-14
    np.testing.assert_array_equal(y_seq, x_seq[:, 4::4, :1])
    assert rel(y_seq[..., 0], case["y"][None, :] - 0.1 * case["q"][:, -6:]) <= TOL  # y = obs + sigma n on the manifold
    one = mm.generate_from_model(system, case["q"][2])
    assert one[0].shape == (49, 2) and rel(one[0], full[2]) <= TOL and one[1].shape == (6, 1) and one[2].shape == (4,)
    system.ctx.close()


def misuse_body():
    case = make_case("fhn", 6, 8, 2, True, B=2, seed=48)
    ctx = make_ctx(case)
    with pytest.raises(RuntimeError, match="chmc_generate_x_seq.*no state"):
        ctx.generate_x_seq(1)
    ctx.generate_x_seq(1, q=case["q"])  # a caller's q needs no state
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    for bad in (0, -1, 3, 16):
        with pytest.raises(RuntimeError, match="chmc_generate_x_seq.*stride"):
            ctx.generate_x_seq(bad)
    buf = np.zeros(2 * 49 * 3 * 3)
    with pytest.raises(RuntimeError, match="chmc_path_stats_update_device.*stride"):
        ctx.path_stats_update_device(3, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    with pytest.raises(ValueError):
        ctx.path_points(3)
    ctx.close()


# ------------------------------------------------------------------------------------------------------ emulation build
@pytest.mark.parametrize("name", list(CASES))
def test_paths_host_logic(emu_lib, name):  # noqa: F811
    path_body(name, on_device=False)


@pytest.mark.parametrize("model", list(MOMENTS))
def test_moments_host_logic(emu_lib, model):  # noqa: F811
    moments_body(model)


def test_shards_host_logic(emu_lib):  # noqa: F811
    shard_body()


def test_samplers_host_logic(emu_lib, tmp_path):  # noqa: F811
    samplers_body(tmp_path)


def test_generate_from_model_host_logic(emu_lib):  # noqa: F811
    surface_body()


def test_api_misuse_host_logic(emu_lib):  # noqa: F811
    misuse_body()


def test_pooled_over_two_gloo_ranks_equals_one_process(emu_lib, tmp_path):  # noqa: F811
    """pooled() over two ranks of 3 chains (merged in rank order) against the single-process 6-chain result."""
    import paths_dist_worker
    single = paths_dist_worker.run(6, 0, 1)
    out = str(tmp_path / "pooled.npy")
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "paths_dist_worker.py"), out, "6"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, o.decode()[-2000:]
    both = np.load(out)
    assert both.shape == single.shape and both[0] == single[0] == 12
    assert rel(both, single) <= 1e-12


# ---------------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_paths(name):
    _hip()
    path_body(name)


_SEQ_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_paths as tp
from manifold_mcmc_for_diffusions_amd import _lib
assert _lib.lib().chmc_backend() == b"hip:gfx950"
for name in tp.CASES:
    print("SEQ_WORST", name, tp.path_body(name, on_device=True, par=False))
print("SEQ_OK")
"""


@pytest.mark.gpu
def test_paths_without_the_compact_rows():
    """CHMC_COMPACT_ROWS=0 (latched per process: a child): no stored trajectory seeds a time-parallel pass, the current-state
    form runs KPath -- every case, the same bound, out80[75] moves and out80[74] does not."""
    _hip()
    script = _SEQ_SCRIPT.format(root=ROOT, tests=HERE)
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, "CHMC_COMPACT_ROWS": "0"}, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "SEQ_OK" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(MOMENTS))
def test_moments(model):
    _hip()
    moments_body(model)


@pytest.mark.gpu
def test_results_do_not_depend_on_the_shard_size():
    _hip()
    shard_body()


@pytest.mark.gpu
def test_samplers(tmp_path):
    _hip()
    samplers_body(tmp_path)


@pytest.mark.gpu
def test_generate_from_model():
    _hip()
    surface_body()


@pytest.mark.gpu
def test_api_misuse():
    _hip()
    misuse_body()
