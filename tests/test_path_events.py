"""Path-wise event summaries on the device (chmc_path_events_device / chmc_predict_events_device, paths.PathEvents and the
`events=` of paths.PredictivePosterior): extremes and their times, the trapezoid integral and, per threshold, up-crossings,
first passage and time above, of one channel over a window of points.

The reference is `events_ref` below: NumPy written from the definition in include/chmc.h; it shares no code with the kernels.
Bounds: max, min, t_max, t_min, every up-crossing count and every t_first are equal bit for bit, the NaN pattern included;
integral, time_above and every folded mean and m2 agree to 1e-12 in test_paths.rel's norm (the project's bound for moment
checks, MOM in tests/test_predictive.py); folded counts are exact.  No chain, replicate or entry is left out of a comparison.
The reference's inputs v_p are NumPy's: the path buffer's components, and obs_func in NumPy for the observed channel -- but
for SIR, whose obs_func is exp(x_1): NumPy's exp and the library's differ in the last bit of some values (1 of the first 20
on the host build), so there the inputs are read from the library point by point and held to two units in the last place
(`channel_values`); every check of a window then stays exact.
The seeds were screened on the emulation build (every `*_host_logic` test); seeds that failed the reference-only conditions
and must not be used: REPLACED.

Every GPU body has a `*_host_logic` twin on the TEST-ONLY emulation build (the generic functors KPathEvents, KPredictEvents,
KEventFold)."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx
from test_paths import build_case, on_manifold_points, rel
import test_predictive as tpred
from test_predictive import prepared, SEED, OFFSET, MOM
from test_emu_logic import emu_lib  # noqa: F401
from test_distributed_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXED = (0, 1, 2, 3)  # max, t_max, min, t_min: exact; 4: the integral


def exact_entries(L):
    return list(FIXED) + [5 + 3 * l for l in range(L)] + [6 + 3 * l for l in range(L)]


def close_entries(L):
    return [4] + [7 + 3 * l for l in range(L)]


def events_ref(v, times, h, p0, p1, thetas):
    """The event vector of include/chmc.h of the values v [NP] at the times `times` over the window p0 .. p1."""
    L = len(thetas)
    w = np.asarray(v[p0:p1 + 1], dtype=np.float64)
    out = np.full(5 + 3 * L, np.nan)
    if not np.isfinite(w).all():
        return out
    imax = int(np.flatnonzero(w == w.max())[0])
    imin = int(np.flatnonzero(w == w.min())[0])
    out[0], out[1], out[2], out[3] = w[imax], times[p0 + imax], w[imin], times[p0 + imin]
    out[4] = h * (w.sum() - 0.5 * (w[0] + w[-1])) if p1 > p0 else 0.0
    for l, th in enumerate(thetas):
        ge = w >= th
        out[5 + 3 * l] = float(np.count_nonzero((w[:-1] < th) & ge[1:]))
        out[6 + 3 * l] = times[p0 + int(np.argmax(ge))] if ge.any() else np.nan
        out[7 + 3 * l] = h * float(np.count_nonzero(ge[1:]))
    return out


def compare(dev, ref, L, label):
    """Exact where the definition is exact, 1e-12 for integral and time_above; returns the worst of the latter."""
    assert dev.shape == ref.shape, (label, dev.shape, ref.shape)
    ex, cl = exact_entries(L), close_entries(L)
    np.testing.assert_array_equal(dev[..., ex], ref[..., ex], err_msg=str(label))
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), label
    e = rel(np.nan_to_num(dev[..., cl]), np.nan_to_num(ref[..., cl]))
    assert e <= MOM, (label, e)
    return e


def is_hip(ctx):
    return ctx.L.chmc_backend() == b"hip:gfx950"


def to_dev(ctx, a):
    """(keep-alive object, pointer, read-back) of a device copy of `a` (host memory on the emulation build)."""
    if is_hip(ctx):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))
        torch.cuda.synchronize()
        return t, t.data_ptr(), lambda: t.cpu().numpy()
    b = np.ascontiguousarray(a).copy()
    return b, b.ctypes.data, lambda: b.copy()


def obs_of(model, x):
    from manifold_mcmc_for_diffusions_amd import example_models as em
    return np.asarray(em.MODELS[model].obs_func(x))[..., 0]


TWO_ULP = 2.0 ** -51


def channel_values(model, x, ch, dev=None):
    """The channel's values v [B, NP] of the paths x [B, NP, X]: a state component, or obs_func(x) in NumPy.
    SIR's obs_func is exp(x_1), and two correct exp implementations need not agree in the last bit (NumPy's and the C
    library's do not: the host-build screening met a 1-ulp difference in 1 of 20 values), so no NumPy value can be the
    bitwise input of an exact check there.  With dev = (ctx, x_ptr, stride) the inputs of that channel are read from the
    library instead, point by point, as the `max` of the one-point window (p, p) -- a pass-through of v_p that involves no
    reduction, no threshold and no neighbour -- and held against NumPy's to two units in the last place (each exp documents
    an error below one).  Every check of a longer window then rests on exactly the values the library evaluates."""
    if ch < x.shape[-1]:
        return x[..., ch]
    v = obs_of(model, x)
    if model != "sir" or dev is None:
        return v
    ctx, x_ptr, stride = dev
    B, NP = v.shape
    keep, ev_ptr, ev_host = to_dev(ctx, np.zeros((B, 5)))
    got = np.empty_like(v)
    for p in range(NP):
        ctx.path_events_device(x_ptr, NP, stride, ch, p, p, (), ev_ptr)
        got[:, p] = ev_host()[:, 0]
    fin = np.isfinite(v)
    assert np.array_equal(np.isfinite(got), fin)
    assert (np.abs(got[fin] - v[fin]) <= TWO_ULP * np.abs(v[fin])).all()
    return np.where(fin, got, v)


def launches(ctx):
    d = ctx.diagnostics()
    return d["path_events_wave_launches"], d["path_events_seq_launches"]


# ------------------------------------------------------------------------------------------------------- synthetic paths
WINDOWS = [(49, 3, 3), (49, 5, 6), (65, 1, 63), (129, 2, 65), (129, 1, 65), (193, 7, 135)]  # lengths 1, 2, 63, 64, 65, 129
SYNTH = [("fhn", 5), ("fhn", 130), ("sir", 5), ("sir", 130)]  # X = 2 and 3; one wavefront per chain, several workgroups
N_SHAPES = 9


def synthetic_paths(shapes, NP, X, p0, p1, rng):
    """[B, NP, X] of dyadic numbers (exact sums); chain c has shape shapes[c]: 0 constant; 1 alternating +-1; 2, 3 increasing
    and decreasing ramps; 4, 8 random; 5, 6 random with a NaN, with a +inf inside the window; 7 random with both just outside."""
    p = np.arange(NP, dtype=np.float64)
    base = np.empty((len(shapes), NP))
    for c, k in enumerate(shapes):
        if k == 0:
            base[c] = 0.5
        elif k == 1:
            base[c] = np.where((np.arange(NP) + c) % 2 == 0, 1.0, -1.0)
        elif k == 2:
            base[c] = (p - NP // 2) / 64.0
        elif k == 3:
            base[c] = (NP // 2 - p) / 64.0
        else:
            base[c] = rng.integers(-96, 97, NP) / 64.0
    x = base[:, :, None] + 0.25 * np.arange(X)[None, None, :]
    for c, k in enumerate(shapes):
        if k == 5:
            x[c, p0 + (p1 - p0) // 2] = np.nan
        elif k == 6:
            x[c, p1] = np.inf
        elif k == 7:
            x[c, p0 - 1], x[c, p1 + 1] = np.nan, np.inf
    return x


def synthetic_thresholds(model, v, shapes, X, ch, p0, p1, L, pick):
    """From the reference values v [B, NP] of the channel: bitwise the constant path's value, bitwise an interior value of a
    random chain, the upper level of the alternating path, one above and one below every finite value; L = 1 takes one of
    them in turn, L = 8 all of them and three more."""
    w = v[:, p0:p1 + 1]
    fin = w[np.isfinite(w)]
    probe = np.array([[0.5, 1.0]])[:, :, None] + 0.25 * np.arange(X)[None, None, :]  # a constant and an alternating point
    v_const, v_upper = (float(a) for a in channel_values(model, probe, ch)[0])  # (used where no chain has the shape)
    for c, k in enumerate(shapes):
        if k == 0:
            v_const = float(v[c, p0])
        elif k == 1:
            v_upper = float(max(v[c, p0], v[c, p0 + 1]))
    rnd = [c for c, k in enumerate(shapes) if k in (4, 8)]
    v_inner = float(v[rnd[0] if rnd else 0, p0 + (p1 - p0) // 2])
    above, below = float(fin.max() + 1.0), float(fin.min() - 1.0)
    must = [v_const, v_inner, v_upper, above, below]
    if L == 0:
        return np.zeros(0), must
    if L == 1:
        return np.array([must[pick % 5]]), must
    th = list(np.unique(must))
    for e in (float(np.median(fin)), above + 1.0, below - 1.0, 0.125, -0.125, 0.3, -0.3):
        if len(th) < L and e not in th:
            th.append(e)
    assert len(th) == L
    return np.sort(np.array(th)), must


def check_reference_situations(ref, v, shapes, times, p0, p1, th, must):
    """What the reference itself gives in the listed situations (a check of the test's inputs, not of the device)."""
    v_const, _, v_upper, above, _ = must
    l_const, l_upper, l_above = (int(np.flatnonzero(th == t)[0]) for t in (v_const, v_upper, above))
    for c, k in enumerate(shapes):
        w = v[c, p0:p1 + 1]
        if k in (5, 6):
            assert np.isnan(ref[c]).all()
            continue
        assert np.isfinite(ref[c, :5]).all()  # shape 7 included: the NaN and the inf just outside the window do not matter
        assert ref[c, 5 + 3 * l_above] == 0.0 and np.isnan(ref[c, 6 + 3 * l_above]) and ref[c, 7 + 3 * l_above] == 0.0
        if k == 0:  # ties give the first point; a threshold equal to the constant is reached at once and never crossed
            assert ref[c, 1] == ref[c, 3] == times[p0]
            assert ref[c, 5 + 3 * l_const] == 0.0 and ref[c, 6 + 3 * l_const] == times[p0]
        elif k == 1:
            assert ref[c, 5 + 3 * l_upper] == np.count_nonzero(np.diff(w) > 0)
        elif k == 2:
            assert ref[c, 1] == times[p1] and ref[c, 3] == times[p0]
        elif k == 3:
            assert ref[c, 1] == times[p0] and ref[c, 3] == times[p1]


def synthetic_body(model, B, on_device=True):
    case = make_case(model, 6, 8, 2, True, B=B, seed=81)
    ctx = make_ctx(case)
    X, stride = ctx.X, 2
    h = stride * (case["obs_interval"] / ctx.S)
    rng = np.random.default_rng(82)
    worst, calls, covered = 0.0, 0, set()
    l0 = launches(ctx)
    for wi, (NP, p0, p1) in enumerate(WINDOWS):
        assert 0 < p0 <= p1 < NP - 1
        shapes = [(c + 2 * wi) % N_SHAPES for c in range(B)]  # B = 5 meets every shape over the six windows
        covered.update(shapes)
        x = synthetic_paths(shapes, NP, X, p0, p1, rng)
        times = np.arange(NP) * h
        keep, x_ptr, _ = to_dev(ctx, x)
        for ch in range(X + 1):
            n_calls = launches(ctx)
            v = channel_values(model, x, ch, (ctx, x_ptr, stride))
            calls += sum(launches(ctx)) - sum(n_calls)
            for L in (0, 1, 8):
                th, must = synthetic_thresholds(model, v, shapes, X, ch, p0, p1, L, wi + ch)
                NE = 5 + 3 * L
                ref = np.stack([events_ref(v[c], times, h, p0, p1, th) for c in range(B)])
                if L == 8:
                    check_reference_situations(ref, v, shapes, times, p0, p1, th, must)
                ev_keep, ev_ptr, ev_host = to_dev(ctx, np.full((B, NE), 777.0))
                ctx.path_events_device(x_ptr, NP, stride, ch, p0, p1, th, ev_ptr)
                calls += 1
                dev = ev_host()
                worst = max(worst, compare(dev, ref, L, (model, B, NP, p0, p1, ch, L)))
                if L == 8:  # a masked chain's row keeps the sentinel, the others are what they were
                    mask = np.ones(B, dtype=np.int32)
                    mask[1::7] = 0
                    ev2_keep, ev2_ptr, ev2_host = to_dev(ctx, np.full((B, NE), 777.0))
                    ctx.path_events_device(x_ptr, NP, stride, ch, p0, p1, th, ev2_ptr, mask=mask)
                    calls += 1
                    dev2 = ev2_host()
                    assert (dev2[mask == 0] == 777.0).all()
                    assert dev2[mask != 0].tobytes() == dev[mask != 0].tobytes()
    l1 = launches(ctx)
    print(f"\nsynthetic {model} B={B}: {calls} calls, integral / time_above within {worst:.2e} of the reference")
    assert covered == set(range(N_SHAPES))
    assert (l1[0] - l0[0], l1[1] - l0[1]) == ((calls, 0) if on_device else (0, calls))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ real paths
# build_case's tuples: model, T, S, R, noisy, gaussian, var_sigma, obs_interval, chains, _, seed
REAL = {
    "fhn": ("fhn", 6, 8, 2, True, False, False, None, 5, None, 514),
    "fhn_varsigma": ("fhn", 12, 16, 5, True, False, True, None, 5, None, 94),
    "fhn_nb_noiseless": ("fhn_nb", 7, 8, 3, False, True, False, None, 5, None, 105),
    "sir": ("sir", 5, 6, None, True, False, False, None, 5, None, 86),
}
# id: {seeds: why}.  The condition (real_body: the median threshold of chain 0 is up-crossed in at least half the chains, at
# stride 1 and at stride S) is a property of the reference path alone; at stride S the window of "fhn" has five points.
REPLACED = {
    "fhn": {tuple(range(83, 474, 10)) + tuple(range(500, 514)): "fewer than 3 of 5 chains up-cross at stride 1 or at stride S"},
    "fhn_varsigma": {(84,): "1 of 5 chains up-crosses at stride 1, none at stride S"},
    "fhn_nb_noiseless": {(85, 95): "no chain up-crosses at stride S"},
}


def stepped_ctx(cfg):
    case = build_case(cfg)
    ctx = make_ctx(case)
    rng = np.random.default_rng(cfg[10] + 1000)
    q_on, xo = on_manifold_points(ctx, case, rng)
    B = ctx.B
    ctx.set_state(q_on, rng.standard_normal((B, ctx.Q)), xo, 0)
    ctx.project_onto_cotangent_space()
    dt = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 if case["model"] == "sir" else 0.04)
    for _ in range(2):
        ctx.leapfrog_step(dt)
    return case, ctx


def real_thresholds(v, p0, p1):
    w = v[:, p0:p1 + 1]
    return np.array([w.min() - 1.0, float(np.median(w[0])), w.max() + 1.0])


def real_body(name, on_device=True, wave=True):
    from manifold_mcmc_for_diffusions_amd.paths import PathEvents, PathPosterior
    case, ctx = stepped_ctx(REAL[name])
    model, B, X = case["model"], ctx.B, ctx.X
    worst, out = 0.0, {}
    for stride in (1, ctx.S):
        x = ctx.generate_x_seq(stride)
        NP = x.shape[1]
        p0, p1 = 1, NP - 2
        pp = PathPosterior(ctx, stride)
        pp.update()
        x_keep, x_ptr, _ = to_dev(ctx, x)
        for ch in range(X + 1):
            v = channel_values(model, x, ch, (ctx, x_ptr, stride))
            th = real_thresholds(v, p0, p1)
            pe = PathEvents(ctx, ch, th, stride=stride, window=(p0, p1))
            assert pe.NP == NP and pe.names[:5] == ["max", "t_max", "min", "t_min", "integral"] and len(pe.names) == pe.NE == 14
            h = pe.times[1]
            ref = np.stack([events_ref(v[c], pe.times, h, p0, p1, th) for c in range(B)])
            if ch == X:  # the condition on the reference: the median threshold is up-crossed in at least half the chains
                assert np.count_nonzero(ref[:, 8] >= 1) * 2 >= B, (name, stride, ref[:, 8])
            assert np.isnan(ref[:, 12]).all() and (ref[:, 6] == pe.times[p0]).all()  # never reached; reached at once
            l0 = launches(ctx)
            dev = pe.update()
            l1 = launches(ctx)
            worst = max(worst, compare(dev, ref, 3, (name, stride, ch)))
            shared = PathEvents(ctx, ch, th, stride=stride, window=(p0, p1), path_posterior=pp).update()
            assert shared.tobytes() == dev.tobytes(), (name, stride, ch)
            assert (l1[0] - l0[0], l1[1] - l0[1]) == ((1, 0) if on_device and wave else (0, 1))
            out[f"{name}/{stride}/{ch}"] = dev
    print(f"\n{name}: integral / time_above within {worst:.2e} of the reference")
    ctx.close()
    return out


def misuse_body():
    from manifold_mcmc_for_diffusions_amd.paths import PathEvents
    case = make_case("fhn", 6, 8, 2, True, B=2, seed=87)
    ctx = make_ctx(case)
    keep, x_ptr, _ = to_dev(ctx, np.zeros((2, 49, 2)))
    ev_keep, ev_ptr, ev_host = to_dev(ctx, np.full((2, 29), 777.0))

    def call(NP=49, stride=1, ch=0, p0=0, p1=48, th=(), x=x_ptr, ev=ev_ptr):
        ctx.path_events_device(x, NP, stride, ch, p0, p1, th, ev)

    for kw, msg in ((dict(stride=0), "stride"), (dict(stride=3), "stride"), (dict(ch=-1), "channel"), (dict(ch=3), "channel"),
                    (dict(p0=-1), "window"), (dict(p0=5, p1=4), "window"), (dict(p1=49), "window"), (dict(NP=0), "n_points"),
                    (dict(th=[0.0, 0.0]), "increasing"), (dict(th=[1.0, 0.0]), "increasing"), (dict(th=[np.nan]), "increasing"),
                    (dict(th=np.arange(9.0)), "thresholds"), (dict(x=None), "null"), (dict(ev=None), "null")):
        with pytest.raises(RuntimeError, match="chmc_path_events_device.*" + msg):
            call(**kw)
    assert (ev_host() == 777.0).all()  # a refused call writes nothing
    call(th=np.arange(8.0))  # needs no state: any path buffer
    assert (ev_host() != 777.0).all()
    for kw in (dict(channel=3), dict(channel=0, thresholds=[1.0, 1.0]), dict(channel=0, window=(0, 49)),
               dict(channel=0, stride=3)):
        with pytest.raises(ValueError):
            PathEvents(ctx, **kw)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ predictive
def fold_events(state, raw, mask=None):
    """include/chmc.h's fold in NumPy from raw events [B, n_rep, NE]: groups of 64 consecutive replicates, two passes over
    the finite values of each entry, Chan merges in group order with the entry's own count; state = [en, emean, em2]."""
    en, emean, em2 = (a.copy() for a in state)
    B, n_rep, NE = raw.shape
    for c in range(B):
        if mask is not None and not mask[c]:
            continue
        for i in range(NE):
            for g in range(0, n_rep, 64):
                vals = raw[c, g:g + 64, i]
                vals = vals[np.isfinite(vals)]
                R = len(vals)
                if R == 0:
                    continue
                mg = np.add.reduce(vals) / R
                sg = np.add.reduce((vals - mg) ** 2)
                nn = float(en[c, i])
                n1 = nn + R
                d = mg - emean[c, i]
                emean[c, i] += d * R / n1
                em2[c, i] += sg + d * d * nn * R / n1
                en[c, i] += R
    return [en, emean, em2]


def predictive_run(case, ctx, origin, H, stride, n_rep, label, on_device):
    """One (origin, horizon, stride, n_rep): the events call beside chmc_predict_device, two accumulating draws and a masked
    third; raw events against NumPy on the kept paths, the fold against NumPy on the device's raw events."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    B, X = ctx.B, ctx.X
    org = "end" if origin == 0 else "start"
    levels = np.linspace(-1.0, 1.0, 5)
    plain = PredictivePosterior(ctx, H, stride, n_rep, org, levels=levels, n_keep=n_rep)
    NPF = plain.NPF
    p0, p1 = min(1, NPF - 1), max(NPF - 2, min(1, NPF - 1))
    ch = X + 1
    plain.update(SEED, 7, OFFSET)
    first = plain.last_paths()[..., ch]  # the replicates of the first draw: thresholds are fixed from them before the events call
    peak = first[:, :, p0:p1 + 1].max(-1)
    th = np.unique([first.min() - 1.0, float(np.median(first[0, 0, p0:p1 + 1])), float(np.median(peak))])
    L = len(th)
    pp = PredictivePosterior(ctx, H, stride, n_rep, org, levels=levels, n_keep=n_rep,
                             events=dict(channel=ch, thresholds=th, window=(p0, p1)), keep_events=True)
    assert pp.event_names == ["max", "t_max", "min", "t_min", "integral"] + [f"{k}_{l}" for l in range(L)
                                                                               for k in ("upcross", "t_first", "time_above")]
    h = stride * (case["obs_interval"] / ctx.S)
    NE = 5 + 3 * L
    state = [np.zeros((B, NE), dtype=np.int64), np.zeros((B, NE)), np.zeros((B, NE))]
    worst = dict(raw=0.0, emean=0.0, em2=0.0)
    reached = [0, 0]
    d0 = ctx.diagnostics()
    for k, draw in enumerate((7, 12345678901, 5)):
        mask = np.array([c % 3 != 1 for c in range(B)], dtype=np.int32) if k == 2 else None
        if k:
            plain.update(SEED, draw, OFFSET, mask=mask)
        before = tpred.collect(pp) + tuple(pp.event_moments()) + (pp.last_events(),)
        pp.update(SEED, draw, OFFSET, mask=mask)
        for a, b in zip(tpred.collect(pp), tpred.collect(plain)):  # paths, n, mean, m2, cdf: those of chmc_predict_device
            assert a.tobytes() == b.tobytes(), (label, draw)
        paths, raw = pp.last_paths(), pp.last_events()
        assert raw.shape == (B, n_rep, NE)
        ref = np.stack([[events_ref(paths[c, r, :, ch], pp.times, h, p0, p1, th) for r in range(n_rep)] for c in range(B)])
        worst["raw"] = max(worst["raw"], compare(raw, ref, L, (label, draw)))
        top = ref[..., 6 + 3 * (L - 1)]
        reached[0] += int(np.isfinite(top).sum())
        reached[1] += int(np.isnan(top).sum())
        state = fold_events(state, raw, mask)
        en, emean, em2 = pp.event_moments()
        np.testing.assert_array_equal(en, state[0])
        worst["emean"], worst["em2"] = max(worst["emean"], rel(emean, state[1])), max(worst["em2"], rel(em2, state[2]))
        if mask is not None:  # a chain that sits the call out keeps every buffer
            for a, b in zip(before, tpred.collect(pp) + tuple(pp.event_moments()) + (pp.last_events(),)):
                assert a[mask == 0].tobytes() == b[mask == 0].tobytes()
            assert (en[mask != 0] > before[5][mask != 0]).any(1).all()
    d1 = ctx.diagnostics()
    wave, seq = d1["predict_wave_launches"] - d0["predict_wave_launches"], d1["predict_seq_launches"] - d0["predict_seq_launches"]
    assert (wave, seq) == ((5, 0) if on_device else (0, 5))
    print(f"  {label} origin {origin} H {H} stride {stride} n_rep {n_rep}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; highest threshold reached by {reached[0]} replicates, not by {reached[1]}")
    assert reached[0] > 0 and reached[1] > 0, (label, reached)  # on the reference: both kinds occur
    assert worst["emean"] <= MOM and worst["em2"] <= MOM, (label, worst)
    assert (state[0][:, 0] == [3 * n_rep if c % 3 != 1 else 2 * n_rep for c in range(B)]).all()
    # the Python summaries: chains merged in chain order with per-entry counts
    from manifold_mcmc_for_diffusions_amd.paths import merge_moments
    pool = pp.pooled()["events"]
    n_paths = int(pp.moments()[0].sum())
    for i in range(NE):
        acc = (0, 0.0, 0.0)
        for c in range(B):
            acc = merge_moments(acc, (int(state[0][c, i]), state[1][c, i], state[2][c, i]))
        assert pool["n"][i] == acc[0] and pool["reached"][i] == acc[0] / n_paths
        assert rel(pool["mean"][i], acc[1]) <= MOM and rel(pool["m2"][i], acc[2]) <= MOM
    assert pool["names"] == pp.event_names and pool["reached"][0] == 1.0 and 0.0 < pool["reached"][6 + 3 * (L - 1)] < 1.0
    return pp


def predictive_body(name, on_device=True, tmp_path=None):
    cfg, runs = tpred.CASES[name]
    case, ctx = prepared(cfg)
    print(f"\n{name}: L={ctx.T * ctx.S} B={ctx.B}")
    for origin, H, stride, n_rep in runs:
        pp = predictive_run(case, ctx, origin, H, stride, n_rep, name, on_device)
    if tmp_path is not None:
        z = np.load(pp.save(str(tmp_path)))
        pool = pp.pooled()["events"]
        assert z["event_names"].tolist() == pp.event_names
        np.testing.assert_array_equal(z["event_n"], pool["n"]), np.testing.assert_array_equal(z["event_mean"], pool["mean"])
        np.testing.assert_array_equal(z["event_reached"], pool["reached"])
        np.testing.assert_array_equal(z["event_chain_n"], pp.event_moments()[0])
    ctx.close()


def predictive_misuse_body():
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    case = make_case("fhn", 6, 8, 2, True, B=2, seed=88)
    ctx = make_ctx(case)
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    for ev, msg in ((dict(channel=4), None), (dict(channel=0, window=(0, 2)), None), (dict(channel=0, thresholds=[1, 1]), None),
                    (dict(thresholds=[1.0]), None), (dict(channel=0, level=1), None)):
        with pytest.raises(ValueError):
            PredictivePosterior(ctx, 1, 4, 5, events=ev)
    with pytest.raises(ValueError):
        PredictivePosterior(ctx, 1, 4, 5, keep_events=True)
    pp = PredictivePosterior(ctx, 1, 4, 5)
    with pytest.raises(ValueError):
        pp.event_moments()
    pp = PredictivePosterior(ctx, 1, 4, 5, events=dict(channel=3))
    with pytest.raises(ValueError):
        pp.last_events()
    args = (1, 0, 0, 1, 4, 0, 5, pp._ptr("n"), pp._ptr("mean"), pp._ptr("m2"))
    evb = (pp._ptr("en"), pp._ptr("emean"), pp._ptr("em2"))
    for a, msg in (((4, 0, 1, ()) + evb, "channel"), ((-1, 0, 1, ()) + evb, "channel"), ((0, 0, 2, ()) + evb, "window"),
                   ((0, 1, 0, ()) + evb, "window"), ((0, 0, 1, (1.0, 1.0)) + evb, "increasing"),
                   ((0, 0, 1, np.arange(9.0)) + evb, "thresholds"), ((0, 0, 1, (), None, evb[1], evb[2]), "null")):
        with pytest.raises(RuntimeError, match="chmc_predict_events_device.*" + msg):
            ctx.predict_events_device(*args, *a)
    with pytest.raises(RuntimeError, match="chmc_predict_events_device.*n_rep"):
        ctx.predict_events_device(1, 0, 0, 1, 4, 0, 0, *args[7:], 0, 0, 1, (), *evb)
    assert not pp.event_moments()[0].any() and not pp.moments()[0].any()  # a refused call writes nothing
    ctx.close()


# --------------------------------------------------------------------------------------------------------------- sharding
def shard_body():
    """13 chains as one context and as 4 | 5 | 4: latent-path events, the predictive's raw events and its folded events are
    bitwise equal chain for chain."""
    from manifold_mcmc_for_diffusions_amd.paths import PathEvents, PredictivePosterior
    from test_hip_autodiff_parity import distinct_on_manifold_chains
    N = 13
    case = distinct_on_manifold_chains("fhn", 6, 8, 2, N, 89)
    dts = np.where(np.arange(N) % 2 == 0, 1.0, -1.0) * (0.02 + 0.002 * np.arange(N))
    mom = np.random.default_rng(90).standard_normal((N, case["q"].shape[1]))
    th = np.array([-0.5, 0.0, 0.5])

    def run(sl):
        ctx = make_ctx(dict(case, B=sl.stop - sl.start))
        ctx.set_state(case["q"][sl], mom[sl], case["x_obs"][sl], 0)
        ctx.project_onto_cotangent_space()
        pe = PathEvents(ctx, 2, th, stride=2, window=(1, 23))
        pp = PredictivePosterior(ctx, 2, 4, 70, events=dict(channel=3, thresholds=th, window=(0, 3)), keep_events=True)
        latent = []
        for it in range(2):
            ctx.leapfrog_step(dts[sl])
            ctx.switch_partition()
            latent.append(pe.update())
            pp.update(SEED, it, sl.start)
        out = (np.stack(latent, 1), pp.last_events()) + tuple(pp.event_moments())
        ctx.close()
        return out

    whole = run(slice(0, N))
    assert np.isfinite(whole[0]).any() and (whole[2][:, 0] == 140).all()
    for sl in (slice(0, 4), slice(4, 9), slice(9, 13)):
        for a, b in zip(whole, run(sl)):
            assert a[sl].tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------------------------- samplers
def samplers_body():
    """Both samplers with path_events=: the traced events are those recomputed from generate_x_seq at the same states (a
    callback, which runs behind the sampler's own update), the summary carries the names, and the chain is bitwise the chain
    of the call without path_events."""
    from manifold_mcmc_for_diffusions_amd.paths import PathEvents, PathPosterior
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    from test_hip_autodiff_parity import distinct_on_manifold_chains
    B, seed, stride = 4, 3, 4
    case = distinct_on_manifold_chains("fhn", 6, 8, 2, B, 91)
    ctx = make_ctx(case)
    th = np.array([-0.25, 0.5])
    samplers = {"static": lambda **kw: sample_static_chmc(ctx, 5, 2, 0.03, seed=seed, n_adapt=2, **kw),
                "dynamic": lambda **kw: sample_dynamic_chmc(ctx, 5, 0.03, seed=seed, n_adapt=2, max_tree_depth=2, **kw)}
    for name, run in samplers.items():
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        plain = run()
        assert "path_events" not in plain
        for share in (False, True):
            ctx.set_state(case["q"], None, case["x_obs"], 0)
            pp = PathPosterior(ctx, stride) if share else None
            pe = PathEvents(ctx, ctx.X, th, stride=stride, window=(1, 11), path_posterior=pp)
            seen = []

            def recompute(it, *rest):
                if it >= 2:
                    v = channel_values("fhn", ctx.generate_x_seq(stride), ctx.X)
                    seen.append(np.stack([events_ref(v[c], pe.times, pe.times[1], 1, 11, th) for c in range(B)]))

            kw = dict(path_posterior=pp) if share else {}
            got = run(path_events=pe, callback=recompute, **kw)
            for k in ("heads", "accept_stat", "step_size"):
                assert np.asarray(plain[k]).tobytes() == np.asarray(got[k]).tobytes(), (name, k)
            assert plain["final_step_size"] == got["final_step_size"]
            assert got["path_events"].shape == (3, B, pe.NE) and len(seen) == 3
            for i in range(3):
                compare(got["path_events"][i], seen[i], 2, (name, share, i))
            summ = got["path_events_summary"]
            assert set(summ) == {"mean", "sd", "r_hat", "ess_bulk"} and list(summ["mean"]) == pe.names
            assert summ["mean"]["max"] == pytest.approx(float(got["path_events"][:, :, 0].mean()), rel=1e-13)
    groups = np.array([0, 1, 0, 1])
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    out = sample_static_chmc(ctx, 3, 2, 0.03, seed=seed, n_adapt=1, path_events=PathEvents(ctx, 0), groups=groups)
    assert sorted(out["path_events_summary"]) == [0, 1] and list(out["path_events_summary"][1]["mean"]) == PathEvents(ctx, 0).names
    ctx.close()


# ------------------------------------------------------------------------------------------------------ emulation build
@pytest.mark.parametrize("model,B", SYNTH)
def test_synthetic_paths_host_logic(emu_lib, model, B):  # noqa: F811
    synthetic_body(model, B, on_device=False)


@pytest.mark.parametrize("name", list(REAL))
def test_real_paths_host_logic(emu_lib, name):  # noqa: F811
    real_body(name, on_device=False)


def test_api_misuse_host_logic(emu_lib):  # noqa: F811
    misuse_body()
    predictive_misuse_body()


@pytest.mark.parametrize("name", list(tpred.CASES))
def test_predictive_events_host_logic(emu_lib, name, tmp_path):  # noqa: F811
    predictive_body(name, on_device=False, tmp_path=tmp_path)


def test_shards_host_logic(emu_lib):  # noqa: F811
    shard_body()


def test_samplers_host_logic(emu_lib):  # noqa: F811
    samplers_body()


def test_pooled_events_over_two_gloo_ranks_equal_one_process(emu_lib, tmp_path):  # noqa: F811
    """pooled()["events"] over two ranks of 3 chains (merged in rank order, per-entry counts) against one process of 6."""
    import path_events_dist_worker
    single = path_events_dist_worker.run(6, 0, 1)
    out = str(tmp_path / "pooled.npy")
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "path_events_dist_worker.py"), out, "6"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, o.decode()[-2000:]
    both = np.load(out)
    NE = 11
    assert both.shape == single.shape == (1 + 4 * NE,) and both[0] == single[0] == 6 * 2 * 70
    np.testing.assert_array_equal(both[1:1 + NE], single[1:1 + NE])  # the per-entry counts
    assert 0 < both[1 + 6] < both[0] or 0 < both[1 + 9] < both[0]  # a threshold only some replicates reach
    assert rel(np.nan_to_num(both), np.nan_to_num(single)) <= 1e-12 and np.array_equal(np.isnan(both), np.isnan(single))


# ---------------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("model,B", SYNTH)
def test_synthetic_paths(model, B):
    _hip()
    synthetic_body(model, B)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REAL))
def test_real_paths(name):
    _hip()
    real_body(name)


@pytest.mark.gpu
def test_api_misuse():
    _hip()
    misuse_body()
    predictive_misuse_body()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tpred.CASES))
def test_predictive_events(name, tmp_path):
    _hip()
    predictive_body(name, tmp_path=tmp_path)


@pytest.mark.gpu
def test_results_do_not_depend_on_the_shard_size():
    _hip()
    shard_body()


@pytest.mark.gpu
def test_samplers():
    _hip()
    samplers_body()


AB_PREDICT = {"fhn_v2": [(0, 2, 1, 5), (0, 2, 4, 70), (0, 2, 8, 130)], "sir_v3": [(0, 1, 6, 70), (1, 5, 6, 5)],
              "fhn_nb": [(0, 2, 4, 70)]}


def ab_fixed_paths(out):
    """The real-path cases' paths at both strides with their thresholds, written by the parent: the two children evaluate the
    SAME buffers (their own path scans differ by rounding: k_path_par against KPath, test_paths)."""
    res = {}
    for name in REAL:
        case, ctx = stepped_ctx(REAL[name])
        for stride in (1, ctx.S):
            x = ctx.generate_x_seq(stride)
            res[f"{name}/{stride}/x"] = x
            for ch in range(ctx.X + 1):
                res[f"{name}/{stride}/th{ch}"] = real_thresholds(channel_values(case["model"], x, ch), 1, x.shape[1] - 2)
        ctx.close()
    np.savez(out, **res)


def ab_dump(out, wave, fixed):
    """One process' events (the switch is latched at the first create): the real-path cases against the reference on the
    process' own paths (real_body, with the launch counters per call), the events of the parent's fixed paths, the
    predictive runs of AB_PREDICT with their kept paths, and the launch counters."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    res = {}
    fixed = np.load(fixed)
    for name in REAL:
        real_body(name, on_device=True, wave=wave)
        ctx = make_ctx(build_case(REAL[name]))
        l0, calls = launches(ctx), 0
        for stride in (1, ctx.S):
            x = fixed[f"{name}/{stride}/x"]
            keep, x_ptr, _ = to_dev(ctx, x)
            for ch in range(ctx.X + 1):
                th = fixed[f"{name}/{stride}/th{ch}"]
                ev_keep, ev_ptr, ev_host = to_dev(ctx, np.zeros((ctx.B, 14)))
                ctx.path_events_device(x_ptr, x.shape[1], stride, ch, 1, x.shape[1] - 2, th, ev_ptr)
                calls += 1
                res[f"fixed/{name}/{stride}/{ch}"] = ev_host()
        l1 = launches(ctx)
        assert (l1[0] - l0[0], l1[1] - l0[1]) == ((calls, 0) if wave else (0, calls))
        ctx.close()
    for name, runs in AB_PREDICT.items():
        case, ctx = prepared(tpred.CASES[name][0])
        for i, (origin, H, stride, n_rep) in enumerate(runs):
            NPF = H * ctx.S // stride
            th = np.array([-0.5, 0.25, 1.0])
            pp = PredictivePosterior(ctx, H, stride, n_rep, "end" if origin == 0 else "start", n_keep=n_rep,
                                     events=dict(channel=ctx.X + 1, thresholds=th, window=(0, NPF - 1)), keep_events=True)
            for draw in (7, 12345678901):
                pp.update(SEED, draw, OFFSET)
            paths, raw = pp.last_paths(), pp.last_events()
            h = stride * (case["obs_interval"] / ctx.S)
            ref = np.stack([[events_ref(paths[c, r, :, -1], pp.times, h, 0, NPF - 1, th) for r in range(n_rep)]
                            for c in range(ctx.B)])
            compare(raw, ref, 3, (name, i))  # this form's events against the reference on this form's own paths
            for k, v in zip(("paths", "raw", "en", "emean", "em2"), (paths, raw) + tuple(pp.event_moments())):
                res[f"{name}/{i}/{k}"] = v
        d = ctx.diagnostics()
        res[f"{name}/launches"] = np.array([d["predict_wave_launches"], d["predict_seq_launches"]])
        ctx.close()
    np.savez(out, **res)


_AB_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_path_events as te
from manifold_mcmc_for_diffusions_amd import _lib
assert _lib.lib().chmc_backend() == b"hip:gfx950"
te.ab_dump({out!r}, {wave!r}, {fixed!r})
print("AB_OK")
"""


@pytest.mark.gpu
def test_wave_kernels_equal_the_functor_forms(tmp_path):
    """The default (k_path_events, k_predict_events) against CHMC_COMPACT_ROWS=0 (KPathEvents, KPredictEvents), a child process
    per setting.  Each child holds the events of its own paths against the reference at the module's bounds, with out80[78] /
    [79] and the predictive counters as witnesses of the form that ran.  Across the two:
    latent-path events of the SAME path buffers (written by this process): every entry but `integral` identical, the
    integral to 1e-12;
    predictive: where the two forms' kept paths are bitwise equal (printed) the raw events at the module's bounds and the
    folded counts exactly; where the paths differ in the last bits (they agree to 1e-14, test_predictive) an exact
    comparison across the forms has no common input, and the raw events are held to 1e-12 with the same NaN pattern;
    folded means and m2 to 1e-12 either way."""
    _hip()
    fixed = str(tmp_path / "fixed.npz")
    ab_fixed_paths(fixed)
    got = {}
    for tag, env in (("wave", {}), ("seq", {"CHMC_COMPACT_ROWS": "0"})):
        out = str(tmp_path / (tag + ".npz"))
        script = _AB_SCRIPT.format(root=ROOT, tests=HERE, out=out, wave=tag == "wave", fixed=fixed)
        r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "AB_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        got[tag] = np.load(out)
    assert sorted(got["wave"].files) == sorted(got["seq"].files)
    for k in got["wave"].files:
        w, s = got["wave"][k], got["seq"][k]
        if k.startswith("fixed/"):
            other = [i for i in range(w.shape[-1]) if i != 4]
            np.testing.assert_array_equal(w[..., other], s[..., other], err_msg=k)
            e = rel(w[..., 4], s[..., 4])
            print(f"  {k}: identical but for the integral, which agrees to {e:.2e}")
            assert e <= MOM
        elif k.endswith("/launches"):
            n = 2 * len(AB_PREDICT[k.split("/")[0]])
            assert w.tolist() == [n, 0] and s.tolist() == [0, n]
        elif k.endswith(("/emean", "/em2")):
            assert rel(np.nan_to_num(w), np.nan_to_num(s)) <= MOM and np.array_equal(np.isnan(w), np.isnan(s)), k
        elif k.endswith("/raw"):
            same = got["wave"][k[:-3] + "paths"].tobytes() == got["seq"][k[:-3] + "paths"].tobytes()
            if same:
                e = compare(w, s, 3, k)
                np.testing.assert_array_equal(got["wave"][k[:-3] + "en"], got["seq"][k[:-3] + "en"])
            else:
                e = rel(np.nan_to_num(w), np.nan_to_num(s))
                assert e <= MOM and np.array_equal(np.isnan(w), np.isnan(s)), k
            print(f"  {k}: kept paths {'bitwise equal' if same else 'differ in the last bits'}, raw events agree to {e:.2e}")
