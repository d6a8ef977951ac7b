"""Scoring observations that arrived behind the fit (chmc_score_future_device, include/chmc.h): forecast candidates weighed by
the new observations, the log predictive score, the pick and the tail of the longer record's position.

References, none of which shares code with the kernels:
  forecasts   the candidates ARE the forecast replicates of chmc_predict_device: logw recomputed in NumPy from the obs
              channel of its kept paths (n_keep = n_cand, same seed / draw / offset, stride = S).  The inputs o_p are the
              same bits, so the bound is that of the sum and the log alone: 1e-13 in rel()'s norm.
  restatement the device's own normals (device_normals) integrated by integrate() over oracle/py/models.py from
              path_by_models' start state.  Bound per n_p: TOL max(1, |o|) / sigma (the project's per-operator bound, 1e-10,
              divided by sigma as the definition divides), propagated to logw as sum_p |n_p| dn_p; the arithmetic of the sum
              and the log (the 1e-13 of the first reference, in its norm) is added.  Fair-case condition, asserted for every
              chain: that start state and the last point of ctx.generate_x_seq(stride = S) agree to FAIR.
  definition  log_pred from the device's logw by the definition, to 1e-12; picked from the definition with u = Phi(z), z from
              ctx.fill_normal under the pick key.  A chain could be excused from the `picked` comparison only if the
              reference's own u s lies within 1e-9 relative of a running-sum boundary; the committed seeds have no such
              chain (asserted: the cap is zero).
  tail        v: ctx.fill_normal under the picked candidate's key, bitwise; n: (y - o) / sigma of the picked candidate's
              kept path, bitwise.
Every case starts two leapfrog steps away from an on-manifold state with no partition switch behind them (prepared), so
x_obs_seq is stale.  y_future is simulated from the model -- the obs channel of one reference path continued from the
chain's state under a draw key of its own (Y_DRAW) -- and shifted by 0.3 sigma, so that the weights are neither equal nor
degenerate.  No chain and no candidate is left out.  The seeds were screened on the emulation build (every `*_host_logic`
test); seeds that failed and must not be used: REPLACED.

Every GPU body has a `*_host_logic` twin on the TEST-ONLY emulation build (the generic functors KFutureScore / KFuturePick)."""
import math
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx
from test_paths import path_by_models, rel
from test_predictive import CASES as PCASES, prepared, device_normals, integrate, sigma_of, key0, SEED, OFFSET
from test_resolution import Dev
from test_emu_logic import emu_lib  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL, FAIR, SUM, SCORE, EDGE = 1e-10, 1e-11, 1e-13, 1e-12, 1e-9
FUTURE_DRAW = 1 << 59  # CHMC_FUTURE_DRAW (include/chmc.h)
Y_DRAW = 999           # the draw key y_future is simulated under
DRAWS = (7, 12345678901)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)

# id: test_predictive's case tuple, then the runs (H, n_cand): a partial group, exactly one candidate, exactly one group, a
# partial second and a partial third group
CASES = {
    "fhn_v2": (PCASES["fhn_v2"][0], [(H, nc) for H in (1, 2) for nc in (1, 5, 64, 70, 130)]),
    "sir_v3": (PCASES["sir_v3"][0], [(1, 70), (2, 5)]),            # V = 3: Philox pairs straddle steps
    "fhn_varsigma": (PCASES["fhn_varsigma"][0], [(1, 70), (2, 64)]),  # sigma = exp(u[Z])
    "fhn_b130": (PCASES["fhn_b130"][0], [(1, 64)]),                # the last workgroup of the per-chain launches partial
}
REPLACED = {}  # id: {seed: why}; no seed failed the screening


def simulated_y(case, ctx, q, start, sig, H):
    """y_future [B, H]: the obs channel of one reference path per chain under Y_DRAW, shifted by 0.3 sigma."""
    V = ctx.V
    W = device_normals(ctx, SEED, Y_DRAW, OFFSET, 1, H * ctx.S * V + H)
    ref = integrate(case["model"], q, start, W, H * ctx.S, ctx.S, case["obs_interval"] / ctx.S, ctx.U, True, sig)
    return np.ascontiguousarray(ref[:, 0, :, ctx.X] + 0.3 * sig[:, None])


def logw_of(y, o, sig):
    """(logw [B, n_cand], n [B, n_cand, H]) by the definition from the obs channel o [B, n_cand, H]; the sum in ascending p."""
    n = (y[:, None, :] - o) / sig[:, None, None]
    ss = np.zeros(n.shape[:2])
    for p in range(n.shape[2]):
        ss = ss + n[..., p] * n[..., p]
    lw = -0.5 * ss - n.shape[2] * (np.log(sig) + HALF_LOG_2PI)[:, None]
    return np.where(np.isfinite(o).all(-1), lw, -np.inf), n


def score_of(lw):
    """(log_pred [B], s [B], running sums [B, n_cand]) by the definition from logw [B, n_cand] (finite maxima)."""
    m = lw.max(1)
    e = np.exp(lw - m[:, None])
    run = np.zeros_like(e)
    acc = np.zeros(len(lw))
    for r in range(lw.shape[1]):  # ascending r, one order
        acc = acc + e[:, r]
        run[:, r] = acc
    return m + np.log(acc) - math.log(lw.shape[1]), acc, run


def pick_of(ctx, draw, lw, off=OFFSET, seed=SEED):
    """(picked [B], near [B]: the reference's own u s within EDGE relative of a running-sum boundary)."""
    rows = np.arange(ctx.B, dtype=np.int32)
    z = ctx.fill_normal(seed, rows, off + rows, np.uint64(FUTURE_DRAW | draw), np.zeros((ctx.B, 2)))[:, 0]
    u = np.array([0.5 * math.erfc(-zz / math.sqrt(2.0)) for zz in z])
    _, s, run = score_of(lw)
    thr = u * s
    picked = np.empty(ctx.B, dtype=np.int32)
    for c in range(ctx.B):
        over = np.flatnonzero(run[c] > thr[c])
        picked[c] = over[0] if len(over) else np.flatnonzero(np.isfinite(lw[c]))[-1]
    near = (np.abs(run - thr[:, None]) <= EDGE * thr[:, None]).any(1)
    return picked, near


def picked_keys(draw, picked):
    return np.array([key0(draw) | int(r) for r in picked], dtype=np.uint64)


def call(ctx, draw, y, n_cand, off=OFFSET, seed=SEED, mask=None, fill=-7.5, lp=None, pk=None):
    """One score call into sentinel-filled buffers: (log_pred, picked, logw [B, n_cand], tail [B, H S V + H])."""
    H = y.shape[-1]
    logw = Dev(ctx, np.full((ctx.B, n_cand), fill))
    tail = Dev(ctx, np.full((ctx.B, H * ctx.S * ctx.V + H), fill))
    lp, pk = ctx.score_future_device(seed, draw, off, y, n_cand, mask=mask, logw_dev_ptr=logw.ptr, tail_dev_ptr=tail.ptr,
                                     log_pred=lp, picked=pk)
    return lp, pk, logw.get(), tail.get()


def state_bytes(ctx):
    q, p, xo, part = ctx.get_state()
    return q.tobytes() + p.tobytes() + xo.tobytes() + bytes([part])


def run_checks(case, ctx, H, n_cand, label):
    """Checks 1 - 4 of one (H, n_cand): two calls with different draws."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    B, S, T, X, V = ctx.B, ctx.S, ctx.T, ctx.X, ctx.V
    q = ctx.get_state(want_p=False, want_x_obs=False)[0]
    full = path_by_models(case["model"], q, T, S, case["obs_interval"], ctx.U)
    at_end = ctx.generate_x_seq(S)[:, -1]
    for c in range(B):  # the fair-case condition, every chain
        assert rel(full[c, -1], at_end[c]) <= FAIR, (label, c)
    start = full[:, -1]
    sig = sigma_of(ctx, case, q)
    y = simulated_y(case, ctx, q, start, sig, H)
    nv = H * S * V
    pp = PredictivePosterior(ctx, H, S, n_cand, "end", n_keep=n_cand)
    rows = np.arange(B, dtype=np.int32)
    worst = dict(forecast=0.0, restated=0.0, score=0.0)
    before = state_bytes(ctx)
    for draw in DRAWS:
        lp, pk, lw, tail = call(ctx, draw, y, n_cand)
        assert state_bytes(ctx) == before  # the chain state is not changed
        # 1. the candidates are the forecasts
        pp.update(SEED, draw, OFFSET)
        o = pp.last_paths()[..., X]
        lw_ref, n_ref = logw_of(y, o, sig)
        assert np.isfinite(lw).all() and lw.shape == lw_ref.shape == (B, n_cand)
        worst["forecast"] = max(worst["forecast"], rel(lw, lw_ref))
        # 2. the independent restatement, every chain and candidate
        W = device_normals(ctx, SEED, draw, OFFSET, n_cand, nv + H)
        o2 = integrate(case["model"], q, start, W, H * S, S, case["obs_interval"] / S, ctx.U, True, sig)[..., X]
        lw2, n2 = logw_of(y, o2, sig)
        bound = (np.abs(n2) * TOL * np.maximum(1.0, np.abs(o2)) / sig[:, None, None]).sum(-1) + SUM * np.maximum(1.0, np.abs(lw2))
        worst["restated"] = max(worst["restated"], float((np.abs(lw - lw2) / bound).max()))
        # 3. score and pick from the definition, on the device's own weights
        lp_ref, _, _ = score_of(lw)
        worst["score"] = max(worst["score"], rel(lp, lp_ref))
        pk_ref, near = pick_of(ctx, draw, lw)
        assert not near.any(), (label, draw, np.flatnonzero(near))  # cap: no chain is excused
        assert pk.tolist() == pk_ref.tolist(), (label, draw)
        if n_cand == 1:
            assert pk.tolist() == [0] * B and lp.tobytes() == lw[:, 0].tobytes()
        # 4. the tail: the picked candidate's step normals and its n, bitwise
        v_ref = ctx.fill_normal(SEED, rows, OFFSET + rows, picked_keys(draw, pk), np.zeros((B, nv)))
        assert tail[:, :nv].tobytes() == v_ref.tobytes(), (label, draw)
        assert tail[:, nv:].tobytes() == np.ascontiguousarray(n_ref[rows, pk]).tobytes(), (label, draw)
    print(f"  {label} H {H} n_cand {n_cand}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + " (restated: in units of its bound)")
    assert worst["forecast"] <= SUM and worst["restated"] <= 1.0 and worst["score"] <= SCORE, (label, worst)
    return worst


def case_body(name, wave_predictive=True):
    """wave_predictive: the predictive calls of the checks run k_predict (the HIP library with the compact rows on); the
    score calls run the functor form by default in every build."""
    cfg, runs = CASES[name]
    case, ctx = prepared(cfg)
    print(f"\n{name}: L={ctx.T * ctx.S} K={ctx.K} B={ctx.B}")
    d0 = ctx.diagnostics()
    for H, n_cand in runs:
        run_checks(case, ctx, H, n_cand, name)
    d1 = ctx.diagnostics()
    wave, seq = d1["predict_wave_launches"] - d0["predict_wave_launches"], d1["predict_seq_launches"] - d0["predict_seq_launches"]
    calls = len(DRAWS) * len(runs)  # a score call and a predictive call per draw share the two counters
    assert (wave, seq) == ((calls, calls) if wave_predictive else (0, 2 * calls))
    ctx.close()


def degenerate_body():
    """Every weight -inf (y_future pushed to 1e200): log_pred = -inf, picked = -1, the tail row untouched; only in the chains
    it happens to."""
    case, ctx = prepared(PCASES["fhn_v2"][0])
    q = ctx.get_state(want_p=False, want_x_obs=False)[0]
    start = path_by_models(case["model"], q, ctx.T, ctx.S, case["obs_interval"], ctx.U)[:, -1]
    y = simulated_y(case, ctx, q, start, sigma_of(ctx, case, q), 2)
    far = y.copy()
    far[[1, 3]] = 1e200
    lp0, pk0, lw0, tail0 = call(ctx, 7, y, 70)
    lp, pk, lw, tail = call(ctx, 7, far, 70)
    for c in range(ctx.B):
        if c in (1, 3):
            assert lp[c] == -np.inf and pk[c] == -1 and (lw[c] == -np.inf).all() and (tail[c] == -7.5).all()
        else:
            assert lp[c] == lp0[c] and pk[c] == pk0[c] and lw[c].tobytes() == lw0[c].tobytes() and tail[c].tobytes() == tail0[c].tobytes()
    from manifold_mcmc_for_diffusions_amd.sequential import extend_state
    dst = ctx.extended(far)
    with pytest.raises(ValueError, match=r"chains \[1, 3\]"):
        extend_state(ctx, dst, SEED, draw=7, chain_offset=OFFSET, n_cand=70)
    dst.close(), ctx.close()


def shard_body():
    """Six chains as one context against 2 x 3 with chain_offset 0 and 3: every output bitwise equal chain for chain."""
    from test_hip_autodiff_parity import distinct_on_manifold_chains
    case = distinct_on_manifold_chains("fhn", 6, 8, 2, 6, 72)
    dts = np.array([0.04, -0.04, 0.05, 0.03, -0.05, 0.02])
    mom = np.random.default_rng(73).standard_normal((6, case["q"].shape[1]))
    y = case["y"][-1] + 0.05 * np.random.default_rng(74).standard_normal((6, 2))

    def run(sl):
        ctx = make_ctx(dict(case, B=sl.stop - sl.start))
        ctx.set_state(case["q"][sl], mom[sl], case["x_obs"][sl], 0)
        ctx.project_onto_cotangent_space()
        out = []
        for it in range(2):
            ctx.leapfrog_step(dts[sl])
            out += list(call(ctx, it, y[sl], 70, off=sl.start))
        ctx.close()
        return out

    whole = run(slice(0, 6))
    assert np.isfinite(whole[0]).all() and (whole[1] >= 0).all()
    for h in range(2):
        sl = slice(3 * h, 3 * h + 3)
        for a, b in zip(whole, run(sl)):
            assert a[sl].tobytes() == b.tobytes()


def mask_and_misuse_body():
    import ctypes as C
    case = make_case("fhn", 6, 8, 2, True, B=4, seed=75)
    ctx = make_ctx(case)
    y = np.tile(case["y"][-1:], (4, 1)) + 0.01
    with pytest.raises(RuntimeError, match="chmc_score_future_device.*no state"):
        ctx.score_future_device(1, 0, 0, y, 4)
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    good = dict(seed=1, draw=0, chain_offset=0, y_future=y, n_cand=4)
    for kw, msg in ((dict(n_cand=0), "n_cand"), (dict(n_cand=65537), "n_cand"), (dict(draw=1 << 45), "draw"),
                    (dict(chain_offset=-1), "chain_offset"), (dict(y_future=np.full((4, 1), np.nan)), "finite"),
                    (dict(y_future=np.array([[0.0], [np.inf], [0.0], [0.0]])), "finite")):
        with pytest.raises(RuntimeError, match="chmc_score_future_device.*" + msg):
            ctx.score_future_device(**{**good, **kw})
    lp, pk = np.zeros(4), np.zeros(4, dtype=np.int32)
    args = (ctx.h, 1, 0, 0)
    for horizon in (0, -1):
        assert ctx.L.chmc_score_future_device(*args, horizon, y.ctypes.data_as(C.POINTER(C.c_double)), 4, None,
                                              lp.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) != 0
        assert b"horizon" in ctx.L.chmc_last_error()
    assert ctx.L.chmc_score_future_device(*args, 1, None, 4, None, lp.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) != 0
    assert b"null" in ctx.L.chmc_last_error()
    assert ctx.L.chmc_score_future_device(*args, 1, y.ctypes.data_as(C.POINTER(C.c_double)), 4, None, None, None, None, None) != 0
    assert b"null" in ctx.L.chmc_last_error()
    assert not lp.any() and not pk.any()  # a refused call writes nothing
    ctx.score_future_device(1, (1 << 45) - 1, 0, y, 4)  # the largest draw; picked, logw_dev and tail_dev may all be NULL
    # the buffers and entries of a chain that sits a call out are bitwise what they were
    mask = np.array([1, 0, 1, 0], dtype=np.int32)
    for n_cand in (5, 70):
        lp, pk = np.full(4, -3.25), np.full(4, -9, dtype=np.int32)
        lp, pk, lw, tail = call(ctx, 1, y, n_cand, off=0, mask=mask, lp=lp, pk=pk)
        lp1, pk1, lw1, tail1 = call(ctx, 1, y, n_cand, off=0)
        for c in (1, 3):
            assert lp[c] == -3.25 and pk[c] == -9 and (lw[c] == -7.5).all() and (tail[c] == -7.5).all()
        for c in (0, 2):
            assert lp[c] == lp1[c] and pk[c] == pk1[c] and lw[c].tobytes() == lw1[c].tobytes() and tail[c].tobytes() == tail1[c].tobytes()
    ctx.close()
    # without observation noise: refused
    case = make_case("fhn", 6, 8, 2, False, B=2, seed=76)
    ctx = make_ctx(case)
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    with pytest.raises(RuntimeError, match="chmc_score_future_device.*not supported"):
        ctx.score_future_device(1, 0, 0, np.zeros((2, 1)), 4)
    ctx.close()


# ------------------------------------------------------------------------------------------------------ emulation build
@pytest.mark.parametrize("name", list(CASES))
def test_future_score_host_logic(emu_lib, name):  # noqa: F811
    case_body(name, wave_predictive=False)


def test_degenerate_weights_host_logic(emu_lib):  # noqa: F811
    degenerate_body()


def test_shards_host_logic(emu_lib):  # noqa: F811
    shard_body()


def test_mask_and_misuse_host_logic(emu_lib):  # noqa: F811
    mask_and_misuse_body()


# ---------------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_future_score(name):
    _hip()
    case_body(name)


@pytest.mark.gpu
def test_degenerate_weights():
    _hip()
    degenerate_body()


@pytest.mark.gpu
def test_results_do_not_depend_on_the_shard_size():
    _hip()
    shard_body()


@pytest.mark.gpu
def test_mask_and_misuse():
    _hip()
    mask_and_misuse_body()


AB_RUNS = {"fhn_v2": [(1, 1), (1, 5), (2, 64), (2, 70), (2, 130)], "sir_v3": [(1, 70), (2, 5)], "fhn_varsigma": [(1, 70)],
           "fhn_b130": [(1, 64)]}


@pytest.mark.gpu
def test_wave_kernel_equals_the_functor_form():
    """k_future_score against KFutureScore on the SAME chain states and start states: the call under CHMC_FUTURE_WAVE=1 (read on
    entry to every call, chmc_plan.h) against the default call.  logw, log_pred, picked and tail bitwise equal; out80[76]
    moves in the one, [77] in the other.
    (Why not a child process per CHMC_COMPACT_ROWS setting, as test_predictive's A/B test runs: that switch also selects
    the stepping kernels and the path scan, so the two processes do not hold the same inputs.  Measured on an MI355X with
    these cases: after `prepared`'s two leapfrog steps q differs by 7e-16 .. 8e-14 between the settings, x_T by 4e-16 ..
    5e-14, and with them logw by 1e-14 .. 3e-12 and log_pred by 3e-15 .. 7e-13, all in rel()'s norm; picked was equal.
    No bitwise statement about the two KERNELS can be read off such a pair.  The setting itself is covered by the next test.)"""
    _hip()
    for name, runs in AB_RUNS.items():
        case, ctx = prepared(CASES[name][0])
        q = ctx.get_state(want_p=False, want_x_obs=False)[0]
        start = path_by_models(case["model"], q, ctx.T, ctx.S, case["obs_interval"], ctx.U)[:, -1]
        for H, n_cand in runs:
            y = simulated_y(case, ctx, q, start, sigma_of(ctx, case, q), H)
            for draw in DRAWS:
                d0 = ctx.diagnostics()
                assert "CHMC_FUTURE_WAVE" not in os.environ
                os.environ["CHMC_FUTURE_WAVE"] = "1"
                try:
                    wave = call(ctx, draw, y, n_cand)
                finally:
                    del os.environ["CHMC_FUTURE_WAVE"]
                d1 = ctx.diagnostics()
                seq = call(ctx, draw, y, n_cand)
                d2 = ctx.diagnostics()
                moved = [(b["predict_wave_launches"] - a["predict_wave_launches"], b["predict_seq_launches"] - a["predict_seq_launches"])
                         for a, b in ((d0, d1), (d1, d2))]
                assert moved == [(1, 0), (0, 1)], (name, H, n_cand, moved)
                for k, a, b in zip(("log_pred", "picked", "logw", "tail"), wave, seq):
                    assert a.tobytes() == b.tobytes(), (name, H, n_cand, draw, k)
        ctx.close()


_ROWS_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_future_score as tf
from manifold_mcmc_for_diffusions_amd import _lib
assert _lib.lib().chmc_backend() == b"hip:gfx950"
for name in {names!r}:
    tf.case_body(name, wave_predictive=False)
print("ROWS_OK")
"""


@pytest.mark.gpu
def test_functor_form_under_stored_rows():
    """CHMC_COMPACT_ROWS=0 (latched at the first create, hence a child process): the functor form serves the call on the GPU
    (out80[77] moves, [76] does not) and passes checks 1 - 4 against the references at its own states."""
    _hip()
    names = ["fhn_v2", "sir_v3", "fhn_varsigma"]
    r = subprocess.run([sys.executable, "-c", _ROWS_SCRIPT.format(root=ROOT, tests=HERE, names=names)],
                       env={**os.environ, "CHMC_COMPACT_ROWS": "0"}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ROWS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
