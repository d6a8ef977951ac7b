"""The unconstrained comparator target on every scan and model its plan can pick, on the GPU.

`chmc_neg_log_dens_and_grad[_device]` (conditioned_diffusion_neg_log_dens_and_grad, sde/mici_extensions.py:82-205) and
`chmc_adam_objective_device`, which shares its core (nld_core, csrc/chmc_api.inc): one forward scan over the whole chain --
KFullScan (S % 8 != 0), k_fwd_scan (S % 8 == 0) or the time-parallel k_fwd_par on 1, 2 or 4 wavefronts per chain
(KernelPlan::nld, csrc/chmc_plan.h) -- then the adjoint sweep k_nld_grad_wave (one wavefront per chain, four chains per
workgroup, 64-step tiles).  Every case is judged per chain by the autodiff oracle (oracle/py/neg_log_dens.py, in the worker
pool of autodiff_checks) at the bounds of test_hip_parity.test_unconstrained_hmc_target_matches_autodiff_oracle:

    value     |v - v_o|        <= 1e-10 max(1, |v_o|)
    gradient  max|g - g_o|     <= 1e-9  max(1, max|g_o|)

and, where the time-parallel scan runs, by the library's own sequential scan (CHMC_PAR_SCAN=0) on the same inputs at 1e-12
relative (the claim of test_hip_parity's docstring: "the scans agree to 1e-12"), with equal NaN patterns.  Where the oracle
is not finite the library must not be finite either; every chain handed to the oracle is judged.

  1. MATRIX     model x noise x splitting x row slots, T S <= 300, 9 chains (three workgroups of the adjoint sweep, the last
                with one chain), one S % 8 != 0 and one S % 8 == 0 shape per combination; contexts created with a partition so
                that dispatch() instantiates the scan with every row-slot count the family has (fhn 6 / 7 / 8 / 16, fhn with
                variable noise 8 / 16, fhn_nb 6 / 8 / 16, sir 8 / 16: chmc_create gives no other).  R = 4 (six rows with noisy
                observations) is in no table of test_hip_layout_edges / test_hip_fhn16, whose six-row layouts are noiseless;
                the target needs observation noise.  The notebook model has no generate_sigma: fixed noise only.
                The target does not depend on R: R_INDEPENDENCE, equal bits at equal ctx.RM, 1e-12 otherwise.
  2. TILES      S = 63 / 64 / 65 / 128 / 1 of the adjoint sweep's 64-step tiles.
  3. SEGMENTS   CHMC_PAR_SCAN=1, CHMC_PAR_WAVES=W, L = T S = 64 W - 1 (lanes without a segment), 64 W (one step per lane, the
                last lane has no junction), 64 W + 1 (two steps per segment: for W = 4 the last two wavefronts own nothing).
                fhn with 8 row slots, sir as T = 1 cases (one row: 8 row slots) and, where L has a factor 9 <= T <= 16, in a
                16-row single-block context (chain16: sweeps until settled, no in-launch recursion); 127, 129 and 257 have
                no such factor.
  4. LONG       the default plan on FitzHugh-Nagumo chains of 1 024 (W = 1), 2 048 (W = 2) and 4 100 steps (W = 4, m = 17, 15
                empty lanes), 8 row slots, five calls in one context (healthy, healthy + 0.01 noise, wild, wild reversed over
                the chains, healthy): every scan is seeded with the trajectory the previous call left in that row.  The last
                call must reproduce the first to 1e-12.
  5.            par_scan[0] (the in-launch sequential recursion of lane 0, after 12 sweeps) must rise over the wild calls.
  6. ADAM       chmc_adam_objective_device on one case of 4 and one of 3.

Wild points are scale * N(0, 1) in every coordinate, scale 4, 4, 4, 8, 8, 16 over the six chains (WILD_SCALES: at 4 alone
five of six chains of the longer cases stay finite in most seeds).  Screened with tools/screen_nld_paths.py (the oracle alone, no
GPU): every chain of parts 1 - 3 has a finite oracle value and gradient; finite chains of the six of every wild call in
WILD_FINITE (at least two finite and two not, required by the test).

Screened finite chains of the wild calls (of 6): fhn_w1 2, fhn_vs_w1 4, fhn_nb_w1 3, fhn_w2 3, fhn_vs_w2 2, fhn_nb_w2 4, fhn_w4 3,
fhn_vs_w4 4, fhn_nb_w4 3, fhn_gauss_w4 3; the wild calls of part 6: 2 of 6 (fhn_w1) and 4 of 6 ((2, 64) forced W = 2).  No chain
had a finite value with a gradient that is not.  On the device the library was finite in exactly those chains.

MEASURED on an MI355X (75 tests, 19 s), worst relative distance per part; library against the oracle | time-parallel against
sequential scan:
  1. value 3.7e-13 (fhn_vs_gauss_rm16_functor), gradient 5.2e-13 (fhn_vs_rm8_functor); contexts that differ in R: equal bits,
     also across different RM
  2. value 2.4e-14 ((5, 1)), gradient 5.4e-14 ((3, 65))
  3. value 4.0e-14 (fhn W = 4, 255 steps), gradient 1.0e-12 (fhn W = 4, 257 steps) | value 1.3e-15, gradient 2.9e-14; every scan
     of every case settled, par_scan[0] stayed 0
  4. value 7.3e-13 (fhn_gauss_w4), gradient 1.8e-11 (fhn_vs_w4) | value 1.3e-13 (fhn_gauss_w4), gradient 2.5e-13 (fhn_vs_w4), the
     kernel comment's "about 1e-15" holds for the trajectory, not for a sum over 4 100 steps; the last call against the first
     value 8.4e-15, gradient 1.3e-14.  The sequential scan is judged by the oracle on the same chains at the same bounds,
     and the project's bounds stand as they are for the long cases (a fiftieth of the gradient bound is used).
     par_scan[0:16] after the five calls (index 0: lane 0's recursion; 1 + s: scans settled after s + 1 sweeps) and par_scan[0]
     after every call:
       fhn_w1        [12, 2, 6, 0, 6, 0, 0, 2, 1, 0, 0, 0, 1, 0, 0, 0]   6, 6, 6, 8, 12
       fhn_vs_w1     [12, 0, 4, 2, 8, 1, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0]   5, 5, 5, 7, 12
       fhn_nb_w1     [14, 2, 4, 0, 6, 0, 0, 0, 3, 0, 0, 0, 1, 0, 0, 0]   6, 6, 7, 10, 14
       fhn_w2        [10, 0, 4, 1, 6, 0, 0, 1, 3, 3, 2, 0, 0, 0, 0, 0]   1, 1, 2, 6, 10
       fhn_vs_w2     [9, 0, 6, 0, 5, 1, 1, 0, 3, 3, 2, 0, 0, 0, 0, 0]    0, 0, 2, 5, 9
       fhn_nb_w2     [8, 0, 4, 1, 7, 0, 0, 3, 3, 2, 1, 0, 1, 0, 0, 0]    1, 1, 3, 6, 8
       fhn_w4        [11, 2, 4, 0, 8, 1, 0, 0, 2, 1, 0, 1, 0, 0, 0, 0]   6, 6, 6, 7, 11
       fhn_vs_w4     [13, 0, 4, 0, 7, 2, 0, 0, 0, 0, 1, 3, 0, 0, 0, 0]   5, 5, 6, 9, 13
       fhn_nb_w4     [9, 2, 4, 0, 6, 0, 1, 2, 1, 1, 0, 3, 1, 0, 0, 0]    5, 5, 5, 6, 9
       fhn_gauss_w4  [11, 2, 4, 0, 8, 1, 0, 0, 2, 1, 0, 1, 0, 0, 0, 0]   6, 6, 6, 7, 11
     par_scan[0] rose over the two wild calls and again in the last call of every case (a row whose carried guess is NaN gains one
     exact segment per sweep); in the first call, from the guess of zeros, 5 or 6 of the 6 chains of the cases over 0.8 time units
     (T = 4) went to the recursion, 0 or 1 of those over 0.4 (T = 2).
  6. value 1.2e-14, gradient 5.1e-13; objective and gradient bitwise the target's, |u_v|^2 within 1e-14, flags as the oracle's.

That the tests can fail, with a scratch build: without the `(gaussian ? 0.0 : q[Z])` term of variable sigma, and with the
hand-over of the third wavefront's last start state to the fourth left out of fwd_par_sweeps, exactly these failed of parts 1 and
3: the four MATRIX ids with variable sigma and standard splitting (gradient entry 4 off by 6e-3 to 2e-1), and every W = 4 case
whose fourth wavefront owns a segment (255, 256 steps, (4, 64), (15, 17), (16, 16); 257 steps, where it owns none, passed)."""
import numpy as np
import pytest
import autodiff_checks as ac
from helpers import make_case, make_ctx

pytestmark = pytest.mark.gpu

VAL_TOL, GRAD_TOL = 1e-10, 1e-9  # library against the autodiff oracle
SCAN_TOL = 1e-12                 # time-parallel against sequential scan; contexts that differ in RM
WILD_SCALES = np.array([4.0, 4.0, 4.0, 8.0, 8.0, 16.0])[:, None]  # per chain of a wild call (LONG_B chains)

# ---------------------------------------------------------------------------------------------------------------------
# tables (tools/screen_nld_paths.py reads them)

# 1. id: model, var_sigma, gaussian, T, S, R, expected ctx.RM
MATRIX = {
    "fhn_rm6_functor": ("fhn", False, False, 12, 25, 4, 6),
    "fhn_rm7_wave": ("fhn", False, False, 12, 24, 5, 7),
    "fhn_gauss_rm8_functor": ("fhn", False, True, 7, 41, 2, 8),
    "fhn_gauss_rm16_wave": ("fhn", False, True, 12, 24, 10, 16),
    "fhn_vs_rm8_functor": ("fhn", True, False, 7, 41, 3, 8),
    "fhn_vs_rm16_wave": ("fhn", True, False, 12, 24, 10, 16),
    "fhn_vs_gauss_rm16_functor": ("fhn", True, True, 14, 21, 12, 16),
    "fhn_vs_gauss_rm8_wave": ("fhn", True, True, 7, 40, 2, 8),
    "fhn_nb_rm6_functor": ("fhn_nb", False, False, 12, 25, 4, 6),
    "fhn_nb_rm8_wave": ("fhn_nb", False, False, 7, 40, 2, 8),
    "fhn_nb_gauss_rm16_functor": ("fhn_nb", False, True, 14, 21, 12, 16),
    "fhn_nb_gauss_rm8_wave": ("fhn_nb", False, True, 12, 24, 5, 8),
    "sir_rm8_functor": ("sir", False, False, 6, 41, 2, 8),
    "sir_rm16_wave": ("sir", False, False, 14, 16, 14, 16),
    "sir_gauss_rm16_functor": ("sir", False, True, 14, 21, 14, 16),
    "sir_gauss_rm8_wave": ("sir", False, True, 6, 40, 2, 8),
    "sir_vs_rm16_functor": ("sir", True, False, 12, 25, 6, 16),
    "sir_vs_rm8_wave": ("sir", True, False, 6, 40, 3, 8),
    "sir_vs_gauss_rm8_functor": ("sir", True, True, 6, 41, 5, 8),
    "sir_vs_gauss_rm16_wave": ("sir", True, True, 14, 16, 14, 16),
}
MATRIX_B, MATRIX_SEED = 9, 161
SIR_DT = 0.05  # between observations, as the many-block SIR cases of test_hip_layout_edges (at 0.25 the epidemic runs out)

# model: var_sigma, T, S, [(R, expected RM)]: one target, contexts that differ in R only
R_INDEPENDENCE = {
    "fhn": (False, 12, 24, [(2, 8), (3, 8), (4, 6), (5, 7), (10, 16), (None, 16)]),
    "fhn_nb": (False, 12, 25, [(2, 8), (5, 8), (4, 6), (10, 16)]),
    "sir": (True, 12, 24, [(2, 8), (5, 8), (6, 16), (None, 16)]),
}

# 2. fhn, fixed sigma, 5 chains, default plan
TILES = [(3, 63), (3, 64), (3, 65), (2, 128), (5, 1), (1, 1), (1, 64)]
TILES_SEED = 471  # (171, 271, 371, 571: (5, 1), a step of 0.2, diverges in the oracle itself for one to five of the chains)

# 3. W: [(T, S)] with T S = 64 W - 1, 64 W, 64 W + 1 as T = 1 cases and 64 W once more with T > 1
SEGMENTS = {1: [(1, 63), (1, 64), (1, 65), (2, 32)], 2: [(1, 127), (1, 128), (1, 129), (2, 64)],
            4: [(1, 255), (1, 256), (1, 257), (4, 64)]}
# the same lengths with 9 <= T <= 16: sir in a 16-row single-block context
SEGMENTS_SIR16 = {1: [(9, 7), (16, 4), (13, 5)], 2: [(16, 8)], 4: [(15, 17), (16, 16)]}
SEGMENTS_SEED = 181

# 4. id: model, T, S, R, var_sigma, gaussian, W of the default plan, seed
LONG = {
    "fhn_w1": ("fhn", 4, 256, 2, False, False, 1, 191),
    "fhn_vs_w1": ("fhn", 4, 256, None, True, False, 1, 191),
    "fhn_nb_w1": ("fhn_nb", 4, 256, None, False, False, 1, 191),
    "fhn_w2": ("fhn", 2, 1024, 2, False, False, 2, 191),
    "fhn_vs_w2": ("fhn", 2, 1024, None, True, False, 2, 191),
    "fhn_nb_w2": ("fhn_nb", 2, 1024, None, False, False, 2, 291),
    "fhn_w4": ("fhn", 4, 1025, 2, False, False, 4, 191),
    "fhn_vs_w4": ("fhn", 4, 1025, None, True, False, 4, 291),
    "fhn_nb_w4": ("fhn_nb", 4, 1025, None, False, False, 4, 191),
    "fhn_gauss_w4": ("fhn", 4, 1025, 2, False, True, 4, 191),
}
LONG_B = 6
# id: chains of the wild call (call 2; call 3 holds the same points in reverse order) whose oracle value and gradient are
# finite, as tools/screen_nld_paths.py prints them
WILD_FINITE = {
    "fhn_w1": (0, 2),
    "fhn_vs_w1": (0, 1, 2, 4),
    "fhn_nb_w1": (1, 2, 3),
    "fhn_w2": (1, 2, 5),
    "fhn_vs_w2": (0, 2),
    "fhn_nb_w2": (0, 1, 2, 4),
    "fhn_w4": (0, 2, 3),
    "fhn_vs_w4": (0, 1, 2, 3),
    "fhn_nb_w4": (0, 2, 3),
    "fhn_gauss_w4": (0, 2, 3),
}
# seeds that failed the screening (five of the six chains of the wild call finite)
REPLACED = {"fhn_nb_w2": (191,), "fhn_vs_w4": (191,)}

# 6. (table, id or (W, T, S))
ADAM = [("long", "fhn_w1"), ("segments", (2, 2, 64))]


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def build(model, T, S, R, var_sigma, B, seed, obs_interval=None):
    """The case (data from chain 0) and the B points [B, U + NV] of the target: the case's chain states without their
    observation-noise components."""
    if obs_interval is None and model == "sir":
        obs_interval = SIR_DT
    case = make_case(model, T, S, R, True, B=B, seed=seed, var_sigma=var_sigma, obs_interval=obs_interval)
    return case, np.ascontiguousarray(case["q"][:, :case["q"].shape[1] - T])


def long_calls(cid):
    """The case of LONG[cid] and its five calls."""
    model, T, S, R, var_sigma, _, _, seed = LONG[cid]
    case, healthy = build(model, T, S, R, var_sigma, LONG_B, seed)
    rng = np.random.default_rng(seed + 1)
    warm = healthy + 0.01 * rng.standard_normal(healthy.shape)
    wild = WILD_SCALES * rng.standard_normal(healthy.shape)
    return case, [healthy, warm, wild, wild[::-1].copy(), healthy]


def segment_case(model, T, S, B=5):
    """FitzHugh-Nagumo: 0.2 time units per CHAIN whatever T (the cases with T = 1 have that anyway).  The first scan of a context
    starts from a guess of zeros; measured on the device, over 0.8 time units (4, 64) it left all five chains unsettled after
    12 sweeps, over 0.4 (2, 32) / (2, 64) four and three of five, and every one of them went to lane 0's recursion -- which
    says nothing about the segments (the long cases meet that branch: 5 or 6 of 6 chains in their first call)."""
    return build(model, T, S, None, False, B, SEGMENTS_SEED + T + S, obs_interval=0.2 / T if model == "fhn" else None)


# ---------------------------------------------------------------------------------------------------------------------
# judging

def submit(case, q, gaussian, chains):
    """Oracle jobs for the chosen chains of one call: {chain: future of (value, gradient)}."""
    spec = ac.spec_of(case)
    return {c: ac.pool().submit(ac.nld_job, spec, np.array(q[c]), bool(gaussian)) for c in chains}


def all_finite(v, g):
    return bool(np.isfinite(v) and np.isfinite(g).all())


def judge(val, g, futs, worst, what, must_be_finite=True):
    """The library's (val [B], g [B, QH]) against the collected oracle results, chain by chain; updates worst["value"],
    worst["grad"] (relative distances) and worst["finite"] / worst["not_finite"] (oracle chains of either kind)."""
    for c, fut in futs.items():
        vo, go = fut.result(timeout=600)
        if all_finite(vo, go):
            worst["finite"] = worst.get("finite", 0) + 1
        else:
            assert not must_be_finite, f"{what} chain {c}: the oracle itself is not finite (value {vo}): pick another seed"
            worst["not_finite"] = worst.get("not_finite", 0) + 1
            assert not all_finite(val[c], g[c]), f"{what} chain {c}: the oracle is not finite, the library is (value {val[c]})"
        if np.isfinite(vo):
            ev = abs(val[c] - vo) / max(1.0, abs(vo)) if np.isfinite(val[c]) else np.inf
            worst["value"] = max(worst.get("value", 0.0), ev)
            assert ev <= VAL_TOL, f"{what} chain {c}: value {val[c]!r} against the oracle's {vo!r}: {ev:.2e}"
        eg, _ = ac.distance(g[c], go)  # over the oracle's finite entries; inf where the library is not finite there
        worst["grad"] = max(worst.get("grad", 0.0), eg)
        k = int(np.nanargmax(np.where(np.isfinite(go), np.abs(g[c] - go), 0.0)))
        assert eg <= GRAD_TOL, f"{what} chain {c}: gradient {eg:.2e} from the oracle's, worst entry {k}: {g[c][k]!r} / {go[k]!r}"
    return worst


def scan_distance(a, b, what):
    """(value, gradient) relative distances of two library results [(val [B], g [B, QH])] whose non-finite patterns must be
    equal; per chain, scale max(1, |.|) of the second."""
    (v, g), (v0, g0) = a, b
    np.testing.assert_array_equal(np.isnan(v), np.isnan(v0), err_msg=f"{what}: NaN pattern of the values")
    np.testing.assert_array_equal(np.isfinite(v), np.isfinite(v0), err_msg=f"{what}: finite pattern of the values")
    np.testing.assert_array_equal(np.isnan(g), np.isnan(g0), err_msg=f"{what}: NaN pattern of the gradients")
    np.testing.assert_array_equal(np.isfinite(g), np.isfinite(g0), err_msg=f"{what}: finite pattern of the gradients")
    ev = eg = 0.0
    for c in range(len(v0)):
        if np.isfinite(v0[c]):
            ev = max(ev, abs(v[c] - v0[c]) / max(1.0, abs(v0[c])))
        fin = np.isfinite(g0[c])
        if fin.any():
            eg = max(eg, float(np.abs(g[c][fin] - g0[c][fin]).max()) / max(1.0, float(np.abs(g0[c][fin]).max())))
    return ev, eg


def show(what, worst):
    print(f"  {what}:", {k: (f"{v:.1e}" if isinstance(v, float) else v) for k, v in worst.items()})


def scan_env(monkeypatch, par=None, waves=None):
    for k, v in (("CHMC_PAR_SCAN", par), ("CHMC_PAR_WAVES", waves)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


# ---------------------------------------------------------------------------------------------------------------------
# 1. model x noise x splitting x row slots

@pytest.mark.parametrize("cid", list(MATRIX))
def test_matrix_of_models_noise_splitting_and_row_slots(monkeypatch, cid):
    """Nine chains (the third workgroup of k_nld_grad_wave holds one), every chain against the oracle; the scan is KFullScan
    for the `functor` ids and k_fwd_scan for the `wave` ids, instantiated for the context's row-slot count."""
    scan_env(monkeypatch)
    model, var_sigma, gaussian, T, S, R, rm = MATRIX[cid]
    assert T * S <= 300 and (S % 8 == 0) == cid.endswith("wave")
    case, q = build(model, T, S, R, var_sigma, MATRIX_B, MATRIX_SEED)
    futs = submit(case, q, gaussian, range(MATRIX_B))
    ctx = make_ctx(case)
    assert ctx.RM == rm, (ctx.RM, ctx.K)
    val, g = ctx.neg_log_dens_and_grad(q, use_gaussian_splitting=gaussian)
    assert int(ctx.diagnostics()["par_scan"][:48].sum()) == 0  # neither of the two is the time-parallel scan
    ctx.close()
    worst = judge(val, g, futs, {}, cid)
    show(cid, worst)
    assert worst["finite"] == MATRIX_B


@pytest.mark.parametrize("model", list(R_INDEPENDENCE))
@pytest.mark.parametrize("gaussian", [False, True])
def test_target_does_not_depend_on_the_partition(monkeypatch, model, gaussian):
    """Contexts that differ in R only: equal bits where ctx.RM is equal (the same instantiation), 1e-12 otherwise."""
    scan_env(monkeypatch)
    var_sigma, T, S, rs = R_INDEPENDENCE[model]
    out = []
    for R, rm in rs:
        case, q = build(model, T, S, R, var_sigma, MATRIX_B, MATRIX_SEED + 1)
        ctx = make_ctx(case)
        assert ctx.RM == rm, (R, ctx.RM)
        out.append((rm, R, ctx.neg_log_dens_and_grad(q, use_gaussian_splitting=gaussian)))
        ctx.close()
    assert np.isfinite(out[0][2][0]).all() and np.isfinite(out[0][2][1]).all()
    worst = 0.0
    for i, (rm, R, res) in enumerate(out):
        for rm2, R2, res2 in out[i + 1:]:
            if rm == rm2:
                np.testing.assert_array_equal(res[0], res2[0], err_msg=f"values, R = {R} / {R2}")
                np.testing.assert_array_equal(res[1], res2[1], err_msg=f"gradients, R = {R} / {R2}")
            else:
                ev, eg = scan_distance(res2, res, f"R = {R2} / {R}")
                worst = max(worst, ev, eg)
                assert ev <= SCAN_TOL and eg <= SCAN_TOL, (R, R2, ev, eg)
    print(f"  {model}: worst distance between contexts of different RM {worst:.1e}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. tile edges of the adjoint sweep

@pytest.mark.parametrize("T,S", TILES)
def test_adjoint_sweep_tile_edges(monkeypatch, T, S):
    """S one lane short of a 64-step tile, exactly one, one lane over, two tiles, and S = 1 (63 idle lanes per tile)."""
    scan_env(monkeypatch)
    case, q = build("fhn", T, S, None, False, 5, TILES_SEED)
    futs = submit(case, q, False, range(5))
    ctx = make_ctx(case)
    val, g = ctx.neg_log_dens_and_grad(q)
    ctx.close()
    worst = judge(val, g, futs, {}, f"({T}, {S})")
    show(f"({T}, {S})", worst)
    assert worst["finite"] == 5


# ---------------------------------------------------------------------------------------------------------------------
# 3. segment edges of the forced time-parallel scan

def segments_body(monkeypatch, model, W, T, S, rm):
    case, q = segment_case(model, T, S)
    futs = submit(case, q, False, range(5))
    scan_env(monkeypatch, 1, W)
    ctx = make_ctx(case)
    assert ctx.RM == rm and ctx.K == [1], (ctx.RM, ctx.K)
    par = ctx.neg_log_dens_and_grad(q)
    ps = ctx.diagnostics()["par_scan"]
    assert int(ps[1:48].sum()) > 0, ps[:48]
    ctx.close()
    scan_env(monkeypatch, 0)
    ctx = make_ctx(case)
    seq = ctx.neg_log_dens_and_grad(q)
    assert int(ctx.diagnostics()["par_scan"][:48].sum()) == 0
    ctx.close()
    what = f"{model} W={W} ({T}, {S})"
    worst = judge(par[0], par[1], futs, {}, what)
    worst["scan_value"], worst["scan_grad"] = scan_distance(par, seq, what)
    worst["fallbacks"], worst["settled"] = int(ps[0]), int(ps[1:48].sum())
    show(what, worst)
    assert worst["finite"] == 5
    assert worst["scan_value"] <= SCAN_TOL and worst["scan_grad"] <= SCAN_TOL, worst
    if rm == 16:
        assert worst["fallbacks"] == 0 and worst["settled"] == 5  # chain16: the sweeps go on until settled
    return worst


@pytest.mark.parametrize("model", ["fhn", "sir"])
@pytest.mark.parametrize("W,T,S", [(W, T, S) for W, shapes in SEGMENTS.items() for T, S in shapes])
def test_time_parallel_scan_segment_edges(monkeypatch, model, W, T, S):
    """64 W segments of m = ceil(L / 64 W) steps with L = 64 W - 1, 64 W, 64 W + 1: lanes (and, for W = 4 at 257 steps, two
    whole wavefronts) without a segment still take part in the prefix scan, the LDS hand-over and the barriers.  Against the
    oracle and against the sequential scan."""
    assert T * S in (64 * W - 1, 64 * W, 64 * W + 1)
    segments_body(monkeypatch, model, W, T, S, 8)


@pytest.mark.parametrize("W,T,S", [(W, T, S) for W, shapes in SEGMENTS_SIR16.items() for T, S in shapes])
def test_time_parallel_scan_segment_edges_sixteen_row_context(monkeypatch, W, T, S):
    """The same lengths in a 16-row single-block SIR context (RM > 8 and Kmax == 1: k_fwd_par sweeps until settled)."""
    assert T * S in (64 * W - 1, 64 * W, 64 * W + 1) and 9 <= T <= 16
    segments_body(monkeypatch, "sir", W, T, S, 16)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the default plan on long FitzHugh-Nagumo chains, carried guesses, the in-launch sequential recursion

def wild_chains(cid, call):
    """(finite, not finite) chains of wild call 2 or 3 by the screening."""
    fin = [c for c in range(LONG_B) if c in WILD_FINITE[cid]]
    bad = [c for c in range(LONG_B) if c not in WILD_FINITE[cid]]
    if call == 3:  # the same points, reversed over the chains
        fin, bad = sorted(LONG_B - 1 - c for c in fin), sorted(LONG_B - 1 - c for c in bad)
    return fin, bad


@pytest.mark.parametrize("cid", list(LONG))
def test_default_plan_on_long_chains_with_carried_guesses(monkeypatch, cid):
    """Five calls in one context with no switch set; every call against CHMC_PAR_SCAN=0 in a second context (all chains,
    1e-12, equal NaN patterns) and two chains per call against the oracle (the wild calls: one finite and one that is not).
    The finite pattern of every wild call is the screened one; par_scan[0] rises over the wild calls; the last call equals
    the first to 1e-12."""
    model, T, S, R, var_sigma, gaussian, W, _ = LONG[cid]
    assert (W, T * S >= 1024, T * S >= 2048, T * S >= 4096) in ((1, True, False, False), (2, True, True, False), (4, True, True, True))
    case, calls = long_calls(cid)
    assert len(WILD_FINITE[cid]) >= 2 and LONG_B - len(WILD_FINITE[cid]) >= 2  # both regimes in every wild call
    chains = [(0, LONG_B - 1), (0, LONG_B - 1), None, None, (0, LONG_B - 1)]
    for i in (2, 3):
        fin, bad = wild_chains(cid, i)
        chains[i] = (fin[0], bad[0])
    futs = [submit(case, calls[i], gaussian, chains[i]) for i in range(4)]
    futs.append(futs[0])  # the same points
    scan_env(monkeypatch)
    ctx = make_ctx(case)
    assert ctx.RM <= 8, ctx.RM
    par, fallbacks = [], [int(ctx.diagnostics()["par_scan"][0])]
    for q in calls:
        par.append(ctx.neg_log_dens_and_grad(q, use_gaussian_splitting=gaussian))
        fallbacks.append(int(ctx.diagnostics()["par_scan"][0]))
    hist = ctx.diagnostics()["par_scan"][:16].tolist()
    ctx.close()
    scan_env(monkeypatch, 0)
    ctx = make_ctx(case)
    seq = [ctx.neg_log_dens_and_grad(q, use_gaussian_splitting=gaussian) for q in calls]
    assert int(ctx.diagnostics()["par_scan"][:48].sum()) == 0
    ctx.close()
    print(f"  {cid}: par_scan[0:16] {hist}, par_scan[0] after every call {fallbacks[1:]}")
    assert sum(hist[1:]) > 0
    worst = {}
    for i in range(5):
        ev, eg = scan_distance(par[i], seq[i], f"{cid} call {i}")
        worst["scan_value"], worst["scan_grad"] = max(worst.get("scan_value", 0.0), ev), max(worst.get("scan_grad", 0.0), eg)
        assert ev <= SCAN_TOL and eg <= SCAN_TOL, (cid, i, ev, eg)
        judge(par[i][0], par[i][1], futs[i], worst, f"{cid} call {i}", must_be_finite=i not in (2, 3))
        judge(seq[i][0], seq[i][1], futs[i], {}, f"{cid} call {i}, sequential scan", must_be_finite=i not in (2, 3))
    for i in (2, 3):  # every chain of a wild call: finite exactly where the screened oracle is
        fin, _ = wild_chains(cid, i)
        lib = [c for c in range(LONG_B) if all_finite(par[i][0][c], par[i][1][c])]
        assert lib == fin, (cid, i, lib, fin)
    worst["again_value"], worst["again_grad"] = scan_distance(par[4], par[0], f"{cid} healthy again")
    show(cid, worst)
    assert worst["again_value"] <= SCAN_TOL and worst["again_grad"] <= SCAN_TOL, worst  # else the guess leaked into the result
    assert worst["finite"] == 8 and worst["not_finite"] == 2
    assert fallbacks[4] > fallbacks[2], fallbacks  # 5.: chains that did not settle in 12 sweeps went to lane 0's recursion


# ---------------------------------------------------------------------------------------------------------------------
# 6. chmc_adam_objective_device

@pytest.mark.parametrize("table,key", ADAM)
def test_adam_objective_on_the_same_paths(monkeypatch, table, key):
    """out3 [B, 3] of chmc_adam_objective_device at a healthy and a wild point, call by call beside
    chmc_neg_log_dens_and_grad_device in a second context that has seen the same calls (the same carried guesses): objective
    bitwise the target's value, gradient bitwise, |u_v|^2 to 1e-14, and the flag 0 exactly where the oracle's gradient is
    not finite (1 elsewhere)."""
    import torch
    if table == "long":
        case, calls = long_calls(key)
        calls = [calls[0], calls[2]]
        scan_env(monkeypatch)
    else:
        W, T, S = key
        case, healthy = segment_case("fhn", T, S, B=LONG_B)
        calls = [healthy, WILD_SCALES * np.random.default_rng(SEGMENTS_SEED).standard_normal(healthy.shape)]
        scan_env(monkeypatch, 1, W)
    B = case["B"]
    futs = [submit(case, q, False, range(B)) for q in calls]
    a, b = make_ctx(case), make_ctx(case)
    n_bad = 0
    for i, q in enumerate(calls):
        qd = torch.from_numpy(q).cuda()
        g1, g2 = torch.empty_like(qd), torch.empty_like(qd)
        torch.cuda.synchronize()
        out3 = a.adam_objective_device(qd.data_ptr(), g1.data_ptr())
        val = b.neg_log_dens_and_grad_device(qd.data_ptr(), g2.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out3[:, 0], val)
        np.testing.assert_array_equal(g1.cpu().numpy(), g2.cpu().numpy())
        sq = np.array([float(np.sum(np.asarray(q[c], dtype=np.longdouble) ** 2)) for c in range(B)])
        assert np.abs(out3[:, 1] - sq).max() <= 1e-14 * np.maximum(1.0, sq).max(), (out3[:, 1], sq)
        worst = judge(val, g2.cpu().numpy(), futs[i], {}, f"{key} call {i}", must_be_finite=i == 0)
        for c in range(B):
            fin = bool(np.isfinite(futs[i][c].result()[1]).all())
            n_bad += not fin
            assert out3[c, 2] == (1.0 if fin else 0.0), (i, c, out3[c], fin)
        show(f"{key} call {i}", worst)
    assert int(a.diagnostics()["par_scan"][:16].sum()) > 0 and n_bad >= 1
    a.close(), b.close()
