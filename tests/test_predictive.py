"""Posterior predictive simulation on the device (chmc_predict_points / chmc_predict_device, paths.PredictivePosterior):
forecasts beyond the last observation and replicated data sets, folded into running moments and CDF counts.

References, none of which shares code with the kernels:
  paths      the device's own normals (ctx.fill_normal with the replicate's stream and draw key, themselves held against
             test_rng.reference_normals to its rtol 1e-9 / atol 1e-10) integrated by a loop over the hand-written closed forms
             of oracle/py/models.py from the start state that test_paths.path_by_models gives for the current q.  Bound 1e-10
             in test_paths.rel's norm (scale max(1, |ref|)), the per-operator bound.  Fair-case condition, asserted for
             every chain: that start state and the last point of ctx.generate_x_seq(stride = S) agree to 1e-11.  Every case
             takes two leapfrog steps with no partition switch before the call, so x_obs_seq is stale when the forecast
             starts (the freshness check).
  reduction  moments and counts recomputed in NumPy from the device's own kept values by the grouped two-pass definition
             and ordered Chan merges of include/chmc.h.  Counts and n exactly; mean and m2 to 1e-12 in the form
             test_paths' moment check uses: rel(), i.e. scale max(1, |ref|) for both.
  AR(1)      SIR's third state component under its Euler-Maruyama step is an exact Gaussian AR(1) (stated below).
No chain and no replicate is left out of a comparison.  The seeds were screened on the emulation build (every
`*_host_logic` test); seeds that failed and must not be used: REPLACED.

Every GPU body has a `*_host_logic` twin on the TEST-ONLY emulation build (the generic functors KPredict / KPredictFold)."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx
from test_rng import reference_normals
from test_paths import path_by_models, rel, build_case, on_manifold_points
from test_emu_logic import emu_lib  # noqa: F401
from test_distributed_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL, FAIR, MOM = 1e-10, 1e-11, 1e-12
PREDICT_DRAW = 1 << 61
SEED, OFFSET = 20240607, 3

# id: build_case's tuple (model, T, S, R, noisy, gaussian, var_sigma, obs_interval, chains, _, seed), then the runs
# (origin, horizon, stride, n_rep)
CASES = {
    # a partial group, exactly one group, two groups with the second partial, three groups; every stride
    "fhn_v2": (("fhn", 6, 8, 2, True, False, False, None, 5, None, 61),
               [(0, 2, st, nr) for st in (1, 4, 8) for nr in (5, 64, 70, 130)]),
    # V = 3: Philox pairs straddle steps; stride 6: H S V + NPF = 19 normals, the last pair half used; replication, H = T.
    # The replication starts at I = 1, where whole replicates run towards extinction: x1 passes through values like -5e129
    # before the clip at -500 holds it, and the reference itself moves by more than FAIR there.  Runs that failed the
    # fair-case condition of run_checks (a property of the reference alone) and must not be used: UNFAIR.
    "sir_v3": (("sir", 5, 6, None, True, False, False, None, 5, None, 62), [(0, 1, 1, 70), (0, 1, 6, 70), (1, 5, 6, 5)]),
    "fhn_varsigma": (("fhn", 12, 16, 5, True, False, True, None, 5, None, 63), [(0, 1, 4, 70), (1, 12, 16, 64)]),
    "fhn_nb": (("fhn_nb", 7, 8, 3, False, True, False, None, 5, None, 64), [(0, 2, 4, 70), (1, 7, 8, 5)]),  # y_rep = obs
    "fhn_b130": (("fhn", 12, 16, 5, True, False, False, None, 130, None, 65), [(0, 1, 4, 64)]),  # the last workgroup partial
}
REPLACED = {}  # id: {seed: why}; no seed failed the screening
UNFAIR = {"sir_v3": {(1, 5, 6, 70): "the reference moves by 1.5e-11 (draw 7) and 1.5e-10 (draw 12345678901) under a 1-ulp change",
                     (1, 5, 1, 5): "9.0e-12 and 3.0e-11: stride 1 emits the transient values of an extinction"}}
AR1_SEED = 66
AR1_REPLACED = {}  # seed: why; no seed failed the screening


def key0(draw):
    return PREDICT_DRAW | (draw << 16)


def device_normals(ctx, seed, draw, off, n_rep, n):
    """[B, n_rep, n]: the library's own keyed normals of every (chain, replicate) stream of a predictive call."""
    out = np.empty((ctx.B, n_rep, n))
    rows = np.arange(ctx.B, dtype=np.int32)
    for r in range(n_rep):
        buf = np.zeros((ctx.B, n))
        ctx.fill_normal(seed, rows, off + rows, key0(draw) | r, buf)
        out[:, r] = buf
    return out


def sigma_of(ctx, case, q):
    if not case["noisy"]:
        return np.zeros(ctx.B)
    if case["sigma"] == "variable":
        return np.exp(q[:, ctx.U - 1])
    return np.broadcast_to(np.asarray(ctx.sigma, dtype=np.float64), (ctx.B,)).copy()


def integrate(model, q, start, W, HS, stride, dl, U, noisy, sig):
    """[B, n_rep, NPF, X + 2] by a loop over oracle/py/models.py's forward_func from `start` [B, X] over the normals W."""
    import torch
    from oracle.py import models as om
    m = om.MODELS[model]
    B, n_rep = W.shape[:2]
    V = m.dim_v
    qt = torch.from_numpy(np.ascontiguousarray(q))
    z = torch.stack([m.generate_z(qc[:U]) for qc in qt], 1).repeat_interleave(n_rep, 1)  # [Z, B n_rep]
    x = torch.from_numpy(np.ascontiguousarray(start)).T.repeat_interleave(n_rep, 1)
    v = torch.from_numpy(np.ascontiguousarray(W[..., :HS * V])).reshape(B * n_rep, HS, V)
    eps = W[..., HS * V:]
    pts = []
    for s in range(HS):
        x = m.forward_func(z, x, v[:, s].T, dl)
        if (s + 1) % stride == 0:
            pts.append(x.T.numpy().copy())
    xs = np.stack(pts, 1).reshape(B, n_rep, len(pts), -1)
    obs = m.obs_func(torch.from_numpy(xs)).numpy()
    y = obs + sig[:, None, None, None] * eps[..., None] if noisy else obs
    return np.concatenate([xs, obs, y], -1)


def fold(state, vals, levels, mask=None):
    """include/chmc.h's definition in NumPy: groups of 64 consecutive replicates of vals [B, n_rep, NPF, XC], two passes per
    group, Chan merges in group order; state = [n, mean, m2, cdf]."""
    n, mean, m2, cdf = state
    on = np.ones(len(n), dtype=bool) if mask is None else np.asarray(mask) != 0
    for g in range(0, vals.shape[1], 64):
        grp = vals[:, g:g + 64]
        R = grp.shape[1]
        mg = np.add.reduce(grp, 1) / R
        sg = np.add.reduce((grp - mg[:, None]) ** 2, 1)
        nn = n.astype(np.float64)[:, None, None]
        n1 = nn + R
        d = mg - mean
        mean = np.where(on[:, None, None], mean + d * R / n1, mean)
        m2 = np.where(on[:, None, None], m2 + sg + d * d * nn * R / n1, m2)
        cdf = cdf + on[:, None, None] * (grp[..., -1][..., None] <= levels).sum(1)
        n = n + on * R
    return [n, mean, m2, cdf]


def prepared(cfg, per_chain_sigma=False):
    """The case's context two leapfrog steps away from an on-manifold state, no partition switch behind them."""
    case = build_case(cfg)
    ctx = make_ctx(case)
    rng = np.random.default_rng(cfg[10] + 1000)
    B = ctx.B
    if per_chain_sigma:  # every chain its own noise level; the n part puts the chain on the manifold of the shared data
        from manifold_mcmc_for_diffusions_amd import example_models as em
        sig = 0.05 + 0.03 * np.arange(B)
        ctx.set_observations(np.repeat(case["y"][None], B, 0), sig)
        case["q"][:, -ctx.T:] = (case["y"][None] - em.MODELS[case["model"]].obs_func(case["x_obs"])[..., 0]) / sig[:, None]
    q_on, xo = on_manifold_points(ctx, case, rng)
    ctx.set_state(q_on, rng.standard_normal((B, ctx.Q)), xo, 0)
    ctx.project_onto_cotangent_space()
    dt = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 if case["model"] == "sir" else 0.04)
    for _ in range(2):
        r = ctx.leapfrog_step(dt)
    assert (r["status"] == 0).mean() > 0.9
    return case, ctx


def run_checks(case, ctx, origin, H, stride, n_rep, label):
    """Checks 1, 2 and 5 of one (origin, horizon, stride, n_rep): two calls with different draws, everything kept."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    from oracle.py import models as om
    B, S, T, X = ctx.B, ctx.S, ctx.T, ctx.X
    V, noisy = om.MODELS[case["model"]].dim_v, bool(case["noisy"])
    q = ctx.get_state(want_p=False, want_x_obs=False)[0]
    full = path_by_models(case["model"], q, T, S, case["obs_interval"], ctx.U)
    at_end = ctx.generate_x_seq(S)[:, -1]
    for c in range(B):  # the fair-case condition, every chain
        assert rel(full[c, -1], at_end[c]) <= FAIR, (label, c)
    start = full[:, -1] if origin == 0 else full[:, 0]
    HS, NPF = H * S, H * S // stride
    n_norm = HS * V + (NPF if noisy else 0)
    sig = sigma_of(ctx, case, q)
    dl = case["obs_interval"] / S
    # levels: spread over the range the replicates of the first call take (inputs of the call, fixed before it runs)
    W0 = device_normals(ctx, SEED, 7, OFFSET, n_rep, n_norm)
    ref0 = integrate(case["model"], q, start, W0, HS, stride, dl, ctx.U, noisy, sig)
    levels = np.unique(np.quantile(ref0[..., -1], [0.02, 0.1, 0.3, 0.5, 0.7, 0.9, 0.98]))
    pp = PredictivePosterior(ctx, H, stride, n_rep, "end" if origin == 0 else "start", levels=levels, n_keep=n_rep)
    n_p, times = ctx.predict_points(H, stride, origin)
    t0 = T * case["obs_interval"] if origin == 0 else 0.0
    assert n_p == NPF == pp.NPF and np.allclose(times, t0 + np.arange(1, NPF + 1) * stride * dl, rtol=1e-14, atol=0)
    state = [np.zeros(B, dtype=np.int64), np.zeros((B, NPF, X + 2)), np.zeros((B, NPF, X + 2)),
             np.zeros((B, NPF, len(levels)), dtype=np.int64)]
    worst = dict(fair=0.0, paths=0.0, eps=0.0, mean=0.0, m2=0.0)
    for draw in (7, 12345678901):
        W = W0 if draw == 7 else device_normals(ctx, SEED, draw, OFFSET, n_rep, n_norm)
        for c in range(B):
            for r in range(n_rep):
                np.testing.assert_allclose(W[c, r], reference_normals(n_norm, OFFSET + c, SEED, key0(draw) | r), rtol=1e-9,
                                           atol=1e-10)
        ref = ref0 if draw == 7 else integrate(case["model"], q, start, W, HS, stride, dl, ctx.U, noisy, sig)
        # the fair-case condition of the replicates, from the reference alone: moving its start state by one unit in the
        # last place moves no value by more than FAIR (a replicate that runs away -- SIR's I towards extinction, where
        # exp(-x1) amplifies every rounding error until the clip at -500 -- would make the 1e-10 bound a matter of luck)
        moved = integrate(case["model"], q, start * (1.0 + 2.0 ** -52), W, HS, stride, dl, ctx.U, noisy, sig)
        worst["fair"] = max(worst["fair"], rel(moved, ref))
        pp.update(SEED, draw, OFFSET)
        dev = pp.last_paths()
        assert dev.shape == ref.shape == (B, n_rep, NPF, X + 2)
        worst["paths"] = max(worst["paths"], rel(dev, ref))
        if noisy:
            e = rel((dev[..., -1] - dev[..., -2]) / sig[:, None, None], W[..., HS * V:])
            worst["eps"] = max(worst["eps"], e)
        else:
            np.testing.assert_array_equal(dev[..., -1], dev[..., -2])
        state = fold(state, dev, levels)
        n, mean, m2 = pp.moments()
        assert n.tolist() == state[0].tolist()
        np.testing.assert_array_equal(pp.counts(), state[3])
        worst["mean"], worst["m2"] = max(worst["mean"], rel(mean, state[1])), max(worst["m2"], rel(m2, state[2]))
    print(f"  {label} origin {origin} H {H} stride {stride} n_rep {n_rep}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["fair"] <= FAIR, f"{label}: the reference moves by {worst['fair']:.2e} under a 1-ulp change of its start: not a fair case"
    assert worst["paths"] <= TOL and worst["eps"] <= TOL, (label, worst)
    assert worst["mean"] <= MOM and worst["m2"] <= MOM, (label, worst)
    assert state[0].tolist() == [2 * n_rep] * B
    # the Python summaries on top of the buffers
    pool = pp.pooled()
    allv = state  # pooled over chains: NumPy's mean / variance are not available (the replicates of call 1 are gone), so
    from manifold_mcmc_for_diffusions_amd.paths import merge_moments  # the chains' reference moments merged in chain order
    acc = (0, 0.0, 0.0)
    for c in range(B):
        acc = merge_moments(acc, (int(allv[0][c]), allv[1][c], allv[2][c]))
    assert pool["n"] == acc[0] == 2 * n_rep * B
    assert rel(pool["mean"], acc[1]) <= MOM and rel(pool["m2"], acc[2]) <= MOM
    np.testing.assert_array_equal(pool["cdf"], state[3].sum(0) / pool["n"])
    qs = pp.quantiles([0.5])
    F = pool["cdf"]
    for p in range(NPF):
        if F[p, 0] < 0.5 <= F[p, -1]:
            k = int(np.searchsorted(F[p], 0.5))
            assert levels[k - 1] <= qs[p, 0] <= levels[k]
        else:
            assert np.isnan(qs[p, 0]) or F[p, 0] == 0.5
    return worst


def case_body(name, on_device=True):
    cfg, runs = CASES[name]
    case, ctx = prepared(cfg)
    print(f"\n{name}: L={ctx.T * ctx.S} K={ctx.K} B={ctx.B}")
    d0 = ctx.diagnostics()
    for origin, H, stride, n_rep in runs:
        run_checks(case, ctx, origin, H, stride, n_rep, name)
    d1 = ctx.diagnostics()
    wave, seq = d1["predict_wave_launches"] - d0["predict_wave_launches"], d1["predict_seq_launches"] - d0["predict_seq_launches"]
    assert (wave, seq) == ((2 * len(runs), 0) if on_device else (0, 2 * len(runs)))
    ctx.close()


def per_chain_sigma_body():
    cfg = ("fhn", 6, 8, 2, True, False, False, None, 5, None, 67)
    case, ctx = prepared(cfg, per_chain_sigma=True)
    assert len(set(np.asarray(ctx.sigma).tolist())) == 5
    run_checks(case, ctx, 0, 2, 4, 70, "per-chain sigma")
    run_checks(case, ctx, 1, 6, 8, 5, "per-chain sigma")
    ctx.close()


def collect(pp):
    return (pp.last_paths(),) + pp.moments() + (pp.counts(),)


def shard_body():
    """Six chains as one context against 2 x 3 with chain_offset 0 and 3: every output bitwise equal chain for chain."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    from test_hip_autodiff_parity import distinct_on_manifold_chains
    case = distinct_on_manifold_chains("fhn", 6, 8, 2, 6, 68)
    dts = np.array([0.04, -0.04, 0.05, 0.03, -0.05, 0.02])
    mom = np.random.default_rng(69).standard_normal((6, case["q"].shape[1]))
    levels = np.linspace(-2.0, 2.0, 9)

    def run(sl):
        ctx = make_ctx(dict(case, B=sl.stop - sl.start))
        ctx.set_state(case["q"][sl], mom[sl], case["x_obs"][sl], 0)
        ctx.project_onto_cotangent_space()
        pp = PredictivePosterior(ctx, 2, 4, 70, levels=levels, n_keep=70)
        for it in range(2):
            ctx.leapfrog_step(dts[sl])
            pp.update(SEED, it, sl.start)
        out = collect(pp)
        ctx.close()
        return out

    whole = run(slice(0, 6))
    assert whole[1].tolist() == [140] * 6 and whole[4].any()
    for h in range(2):
        sl = slice(3 * h, 3 * h + 3)
        for a, b in zip(whole, run(sl)):
            assert a[sl].tobytes() == b.tobytes()


def mask_and_misuse_body():
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    case = make_case("fhn", 6, 8, 2, True, B=4, seed=70)
    ctx = make_ctx(case)
    buf = np.zeros(4 * 8 * 2 * 4 * 4)
    i64 = np.zeros(4 * 16 * 4, dtype=np.int64)
    ptrs = (i64.ctypes.data, buf.ctypes.data, buf.ctypes.data)

    def call(seed=1, draw=0, off=0, H=1, stride=8, origin=0, n_rep=4, **kw):
        ctx.predict_device(seed, draw, off, H, stride, origin, n_rep, *ptrs, **kw)

    with pytest.raises(RuntimeError, match="chmc_predict_device.*no state"):
        call()
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    for kw, msg in ((dict(H=0), "horizon"), (dict(H=-1), "horizon"), (dict(stride=0), "stride"), (dict(stride=3), "stride"),
                    (dict(stride=16), "stride"), (dict(origin=2), "origin"), (dict(origin=-1), "origin"),
                    (dict(n_rep=0), "n_rep"), (dict(n_rep=65537), "n_rep"), (dict(n_keep=5, paths_dev_ptr=buf.ctypes.data), "n_keep"),
                    (dict(n_keep=-1, paths_dev_ptr=buf.ctypes.data), "n_keep"), (dict(draw=1 << 45), "draw"),
                    (dict(levels=[0.0, 1.0]), "levels and cdf_dev"),
                    (dict(levels=[0.0, 0.0], cdf_dev_ptr=i64.ctypes.data), "increasing"),
                    (dict(levels=[1.0, 0.0], cdf_dev_ptr=i64.ctypes.data), "increasing")):
        with pytest.raises(RuntimeError, match="chmc_predict_device.*" + msg):
            call(**kw)
    import ctypes as C
    with pytest.raises(RuntimeError, match="chmc_predict_device.*levels and cdf_dev"):  # n_levels > 0 with NULL levels
        from manifold_mcmc_for_diffusions_amd._lib import check
        check(ctx.L.chmc_predict_device(ctx.h, 1, 0, 0, 1, 8, 0, 4, None, 2, None, C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]),
                                        C.c_void_p(ptrs[2]), C.c_void_p(i64.ctypes.data), None, 0), "chmc_predict_device")
    for kw, msg in ((dict(horizon=0), "horizon"), (dict(horizon=1, stride=3), "stride")):
        with pytest.raises(RuntimeError, match="chmc_predict_points.*" + msg):
            PredictivePosterior(ctx, **kw)
    assert not buf.any() and not i64.any()  # a refused call writes nothing
    # the buffers of a chain that sits a call out are bitwise what they were
    levels = np.linspace(-1.5, 1.5, 5)
    for n_rep in (5, 70):  # one group (the wave kernel merges itself) and two (the fold does)
        pp = PredictivePosterior(ctx, 2, 4, n_rep, levels=levels, n_keep=3)
        pp.update(SEED, 0)
        before = collect(pp)
        pp.update(SEED, 1, mask=np.array([1, 0, 1, 0], dtype=np.int32))
        after = collect(pp)
        for a, b in zip(before, after):
            for c in (1, 3):
                assert a[c].tobytes() == b[c].tobytes()
            for c in (0, 2):
                assert a[c].tobytes() != b[c].tobytes()
        assert after[1].tolist() == [2 * n_rep, n_rep, 2 * n_rep, n_rep]
    with pytest.raises(ValueError):
        PredictivePosterior(ctx, 1, origin="middle")
    with pytest.raises(ValueError):
        PredictivePosterior(ctx, 1, levels=[1.0, 1.0])
    ctx.close()


def ar1_body():
    """Known answer.  SIR's third component under its step (models_gen.h, oracle/py/models.py) is
        x2' = x2 + gamma (zeta - x2) dl + eps sqrt(dl) v,   v ~ N(0, 1),
    a Gaussian AR(1): with a = 1 - gamma dl, after k steps from x2_T
        E = zeta + a^k (x2_T - zeta),   Var = eps^2 dl (1 - a^(2k)) / (1 - a^2).
    16 updates x 64 replicates = 1024 per chain.  Thresholds, derived: the mean of n Gaussians has standard error
    sqrt(Var / n): 5 of them; the unbiased variance estimate of n Gaussians has relative standard deviation sqrt(2 / (n - 1)):
    5 of them (22 % at n = 1024).  4 chains x 12 points x 2 checks at 5 sigma: a false alarm has probability below 1e-4."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    cfg = ("sir", 5, 6, None, True, False, False, None, 4, None, AR1_SEED)
    case, ctx = prepared(cfg)
    q = ctx.get_state(want_p=False, want_x_obs=False)[0]
    full = path_by_models("sir", q, ctx.T, ctx.S, case["obs_interval"], ctx.U)
    pp = PredictivePosterior(ctx, 2, 1, 64)
    for it in range(16):
        pp.update(AR1_SEED, it, OFFSET)
    n, mean, var = pp.per_chain()
    assert n.tolist() == [1024] * 4
    dl = case["obs_interval"] / ctx.S
    gam, zet = np.exp(q[:, 1]), q[:, 2]
    eps = np.exp(np.sqrt(0.75) * q[:, 3] + 0.5 * q[:, 1] - 3.0)
    a = 1.0 - gam * dl
    k = np.arange(1, pp.NPF + 1)[None, :]
    e_ref = zet[:, None] + a[:, None] ** k * (full[:, -1, 2] - zet)[:, None]
    v_ref = (eps ** 2 * dl)[:, None] * (1.0 - a[:, None] ** (2 * k)) / (1.0 - a ** 2)[:, None]
    z_mean = (mean[..., 2] - e_ref) / np.sqrt(v_ref / 1024)
    r_var = (var[..., 2] - v_ref) / v_ref
    print(f"\nAR(1): mean within {np.abs(z_mean).max():.2f} standard errors, variance within {np.abs(r_var).max():.3f} relative "
          f"(bound {5 * np.sqrt(2 / 1023):.3f})")
    assert (np.abs(z_mean) <= 5.0).all() and (np.abs(r_var) <= 5.0 * np.sqrt(2.0 / 1023.0)).all()
    ctx.close()


def samplers_body(tmp_path):
    """Both samplers on a tiny FHN case, four iterations, two of them warm-up: the chain and its traces are what they are
    without a predictive, bitwise; n = 2 n_rep per chain; the result is what update() by hand gives at the same states (a
    second PredictivePosterior driven from the callback, which runs behind the sampler's own update of the iteration)."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    from test_hip_autodiff_parity import distinct_on_manifold_chains
    B, n_rep, seed = 4, 70, 3
    case = distinct_on_manifold_chains("fhn", 6, 8, 2, B, 71)
    ctx = make_ctx(case)
    levels = np.linspace(-2.0, 2.0, 9)
    samplers = {"static": lambda **kw: sample_static_chmc(ctx, 4, 2, 0.03, seed=seed, n_adapt=2, chain_offset=OFFSET, **kw),
                "dynamic": lambda **kw: sample_dynamic_chmc(ctx, 4, 0.03, seed=seed, n_adapt=2, max_tree_depth=2,
                                                            chain_offset=OFFSET, **kw)}
    for name, run in samplers.items():
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        plain = run(trace_dir=str(tmp_path / (name + "_plain")))
        assert "predictive" not in plain
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        pp = PredictivePosterior(ctx, 2, 4, n_rep, levels=levels, n_keep=2)
        hand = PredictivePosterior(ctx, 2, 4, n_rep, levels=levels, n_keep=2)

        def by_hand(it, *rest):
            if it >= 2:
                hand.update(seed, it, OFFSET)

        with_pp = run(predictive=pp, callback=by_hand, trace_dir=str(tmp_path / (name + "_pp")))
        for k in ("heads", "accept_stat", "step_size"):
            assert np.asarray(plain[k]).tobytes() == np.asarray(with_pp[k]).tobytes(), (name, k)
        assert sorted(plain["trace_files"]) == sorted(with_pp["trace_files"])
        for k in plain["trace_files"]:
            assert np.load(plain["trace_files"][k]).tobytes() == np.load(with_pp["trace_files"][k]).tobytes(), (name, k)
        assert pp.moments()[0].tolist() == [2 * n_rep] * B
        for a, b in zip(collect(pp), collect(hand)):
            assert a.tobytes() == b.tobytes()
        pool = pp.pooled()
        assert set(with_pp["predictive"]) == set(pool) and with_pp["predictive"]["n"] == 2 * n_rep * B
        for k in ("mean", "var", "sd", "m2", "cdf"):
            np.testing.assert_array_equal(with_pp["predictive"][k], pool[k])
        path = pp.save(str(tmp_path / name))
        assert os.path.basename(path) == "predictive.npz"
        z = np.load(path)
        np.testing.assert_array_equal(z["times"], pp.times), np.testing.assert_array_equal(z["mean"], pool["mean"])
        np.testing.assert_array_equal(z["cdf"], pool["cdf"]), np.testing.assert_array_equal(z["levels"], levels)
        assert int(z["pooled_n"]) == 2 * n_rep * B
    # groups: the per-group pooled results are those of the groups' chains
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    pp = PredictivePosterior(ctx, 1, 8, 5, levels=levels)
    groups = np.array([0, 1, 0, 1])
    out = sample_static_chmc(ctx, 3, 2, 0.03, seed=seed, n_adapt=1, predictive=pp, groups=groups)
    assert len(out["predictive_groups"]) == 2
    for g in range(2):
        want = pp.pooled(np.flatnonzero(groups == g))
        assert out["predictive_groups"][g]["n"] == want["n"] == 20
        np.testing.assert_array_equal(out["predictive_groups"][g]["mean"], want["mean"])
    ctx.close()


# ------------------------------------------------------------------------------------------------------ emulation build
@pytest.mark.parametrize("name", list(CASES))
def test_predictive_host_logic(emu_lib, name):  # noqa: F811
    case_body(name, on_device=False)


def test_per_chain_sigma_host_logic(emu_lib):  # noqa: F811
    per_chain_sigma_body()


def test_shards_host_logic(emu_lib):  # noqa: F811
    shard_body()


def test_mask_and_misuse_host_logic(emu_lib):  # noqa: F811
    mask_and_misuse_body()


def test_ar1_known_answer_host_logic(emu_lib):  # noqa: F811
    ar1_body()


def test_samplers_host_logic(emu_lib, tmp_path):  # noqa: F811
    samplers_body(tmp_path)


def test_pooled_over_two_gloo_ranks_equals_one_process(emu_lib, tmp_path):  # noqa: F811
    """pooled() over two ranks of 3 chains (merged in rank order) against the single-process 6-chain result."""
    import predictive_dist_worker
    single = predictive_dist_worker.run(6, 0, 1)
    out = str(tmp_path / "pooled.npy")
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "predictive_dist_worker.py"), out, "6"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, o.decode()[-2000:]
    both = np.load(out)
    assert both.shape == single.shape and both[0] == single[0] == 6 * 2 * 70
    assert rel(both, single) <= 1e-12


# ---------------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_predictive(name):
    _hip()
    case_body(name)


@pytest.mark.gpu
def test_per_chain_sigma():
    _hip()
    per_chain_sigma_body()


@pytest.mark.gpu
def test_results_do_not_depend_on_the_shard_size():
    _hip()
    shard_body()


@pytest.mark.gpu
def test_mask_and_misuse():
    _hip()
    mask_and_misuse_body()


@pytest.mark.gpu
def test_ar1_known_answer():
    _hip()
    ar1_body()


@pytest.mark.gpu
def test_samplers(tmp_path):
    _hip()
    samplers_body(tmp_path)


AB_RUNS = {"fhn_v2": [(0, 2, 1, 5), (0, 2, 1, 64), (0, 2, 4, 70), (0, 2, 8, 130)], "sir_v3": [(0, 1, 6, 70), (1, 5, 6, 5)],
           "fhn_varsigma": [(0, 1, 4, 70)], "fhn_nb": [(0, 2, 4, 70)]}


def ab_dump(out):
    """One process' outputs of AB_RUNS (the switch is latched at the first create): arrays and the launch counters."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    res = {}
    for name, runs in AB_RUNS.items():
        case, ctx = prepared(CASES[name][0])
        for i, (origin, H, stride, n_rep) in enumerate(runs):
            pp = PredictivePosterior(ctx, H, stride, n_rep, "end" if origin == 0 else "start", levels=np.linspace(-1.0, 1.0, 5),
                                     n_keep=n_rep)
            for draw in (7, 12345678901):  # (the draws of run_checks, whose replicates passed the fair-case condition)
                pp.update(SEED, draw, OFFSET)
            for k, v in zip(("paths", "n", "mean", "m2", "cdf"), collect(pp)):
                res[f"{name}/{i}/{k}"] = v
        d = ctx.diagnostics()
        res[f"{name}/launches"] = np.array([d["predict_wave_launches"], d["predict_seq_launches"]])
        ctx.close()
    np.savez(out, **res)


_AB_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_predictive as tp
from manifold_mcmc_for_diffusions_amd import _lib
assert _lib.lib().chmc_backend() == b"hip:gfx950"
tp.ab_dump({out!r})
print("AB_OK")
"""


@pytest.mark.gpu
def test_wave_kernel_equals_the_functor_form(tmp_path):
    """The default (k_predict) against CHMC_COMPACT_ROWS=0 (KPredict / KPredictFold), a child process per setting: kept paths
    bitwise or to 1e-14 (printed which), moments to 1e-12, counts and n exactly; out80[76] moves in the one, [77] in the other."""
    _hip()
    got = {}
    for tag, env in (("wave", {}), ("seq", {"CHMC_COMPACT_ROWS": "0"})):
        out = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", _AB_SCRIPT.format(root=ROOT, tests=HERE, out=out)], env={**os.environ, **env},
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "AB_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        got[tag] = np.load(out)
    for name, runs in AB_RUNS.items():
        assert got["wave"][f"{name}/launches"].tolist() == [2 * len(runs), 0]
        assert got["seq"][f"{name}/launches"].tolist() == [0, 2 * len(runs)]
        for i in range(len(runs)):
            w, s = (got["wave"][f"{name}/{i}/paths"], got["seq"][f"{name}/{i}/paths"])
            bitwise = w.tobytes() == s.tobytes()
            e_p = rel(w, s)
            e_m = rel(got["wave"][f"{name}/{i}/mean"], got["seq"][f"{name}/{i}/mean"])
            e_s = rel(got["wave"][f"{name}/{i}/m2"], got["seq"][f"{name}/{i}/m2"])
            print(f"  {name} run {runs[i]}: paths {'bitwise equal' if bitwise else f'agree to {e_p:.2e}'}, mean {e_m:.2e}, m2 {e_s:.2e}")
            assert e_p <= 1e-14 and e_m <= MOM and e_s <= MOM
            for k in ("n", "cdf"):
                np.testing.assert_array_equal(got["wave"][f"{name}/{i}/{k}"], got["seq"][f"{name}/{i}/{k}"])
