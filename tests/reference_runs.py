"""Helper of test_reference_runs.py / test_hip_reference_runs.py: the fixtures of tests/golden/reference_runs (numbers
computed by the reference's own programs, tests/golden/generate_reference_runs.py) and the one way a copy of the model is
judged against them.

Bounds
  paths and model functions   distance from the 50-digit values <= FACTOR x max(e_ref64, 2^-52) of that array, e_ref64
                              being the reference's own double-precision distance from them on the same inputs.  FACTOR =
                              10: another evaluation order changes the constant of the rounding error, not its order; a
                              decimal digit over the yardstick, not a measured figure.
  J w, J^T lam                1e-9 (the project's operator bound, tests/test_golden.py).
distance(a, ref) = max |a - ref| / max(1, max |ref|) over the whole array, every entry of every chain."""
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = os.path.join(HERE, "golden", "reference_runs")
CASES = ("fhn_3x8", "fhn_9x8", "fhn_3x5", "fhn_nb_4x8", "sir_3x8", "sir_3x5", "sir_12x8", "sir_absorbed", "fhn_varsigma_3x8")
FACTOR = 10.0
OPERATOR_TOL = 1e-9
MAX_FILE_BYTES = 120709  # the largest file under tests/golden before these fixtures

# predict_device: the replicates' key, as tests/test_predictive.py states it; one interval beyond the last observation
PREDICT_CASES = ("fhn_3x8", "sir_3x8")
PREDICT = dict(seed=20240607, draw=7, offset=3, n_rep=2, horizon=1, stride=1)
PREDICT_DRAW = 1 << 61

_cache = {}


def predict_normals(ctx, n):
    """[B, n_rep, n]: the library's keyed normals of every (chain, replicate) stream of the PREDICT call."""
    P = PREDICT
    out = np.empty((ctx.B, P["n_rep"], n))
    rows = np.arange(ctx.B, dtype=np.int32)
    for r in range(P["n_rep"]):
        buf = np.zeros((ctx.B, n))
        ctx.fill_normal(P["seed"], rows, P["offset"] + rows, PREDICT_DRAW | (P["draw"] << 16) | r, buf)
        out[:, r] = buf
    return out


def load(cid):
    """The case's file as a dict of arrays (read once, handed out read-only)."""
    if cid not in _cache:
        with np.load(os.path.join(RUNS, cid + ".npz")) as f:
            d = {k: f[k] for k in f.files}
        for v in d.values():
            v.setflags(write=False)
        _cache[cid] = d
    return _cache[cid]


def meta(f):
    """(model, T, S, R, sigma as ChmcContext / OracleSystem take it, obs_interval)."""
    noise = int(f["noise"])
    sigma = None if noise == 0 else "variable" if noise == 2 else float(f["sigma"])
    return str(f["model"]), int(f["T"]), int(f["S"]), int(f["R"]), sigma, float(f["obs_interval"])


def single_partition(f):
    return int(f["R"]) >= int(f["T"])


def q_of(f):
    """q [B, Q] = (u, v_0, v_seq, n)."""
    B = len(f["u"])
    return np.ascontiguousarray(np.concatenate([f["u"], f["v_0"], f["v_seq"].reshape(B, -1), f["n"]], 1))


def distance(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not np.isfinite(a).all():
        return np.inf
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def bound(f, name, factor=FACTOR):
    return factor * max(float(f["e_ref64_" + name]), 2.0 ** -52)


def judge(copy, cid, name, value, factor=FACTOR, tol=None):
    """Prints and asserts: `value`, some copy's result for the fixture array `name` of case `cid`.  tol: an absolute bound
    (the derivative products) instead of factor x the reference's own error."""
    f = load(cid)
    d = distance(value, f[name])
    b = bound(f, name, factor) if tol is None else tol
    print(f"REFRUN {copy} {cid} {name} {d:.2e} bound {b:.2e}")
    assert d <= b, f"{copy}, {cid}: {name} is {d:.2e} from the reference's 50-digit run, bound {b:.2e}"
    return d


def own_data(f):
    """y [B, T]: data of its own for every chain, y + c in double precision, on whose manifold the chain's fixture point
    lies to rounding; and the constraint value that leaves, c - (y_own - y), a residual of the size of an ulp of y."""
    y_own = f["y"][None] + f["c"]
    return y_own, f["c"] - (y_own - f["y"][None])


def make_ctx(cid, per_chain_data=False, **kw):
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    f = load(cid)
    model, T, S, R, sigma, obs_interval = meta(f)
    y = own_data(f)[0] if per_chain_data else f["y"]
    ctx = ChmcContext(model, obs_interval, S, R, y, sigma=sigma, num_chains=len(f["u"]), **kw)
    assert (ctx.num_partition == 1) == single_partition(f)
    return ctx


NULL_STEP = 1e-10  # step size of judge_after_null_step
# The null step's own factor.  Its retraction starts from a residual that is the first scan's rounding error e0 and solves
# J dq = -e0: that error becomes a displacement of q, and the final evaluation at q + dq adds its own error e1, so what is
# read back differs from the fixture by e1 - e0, two evaluations' rounding errors: twice FACTOR.  Measured on the
# emulation build at FACTOR alone: c of fhn_varsigma_3x8 3.0e-15 against 2.2e-15 (the plain evaluation: 9.6e-16).
NULL_STEP_FACTOR = 2 * FACTOR


def judge_after_null_step(copy, cid, ctx, factor=NULL_STEP_FACTOR):
    """The state evaluation that ends a leapfrog step, put on a fixture point: a context made with per_chain_data=True (every
    chain on the manifold of its own data), momentum zero, one step of size NULL_STEP.  The kick is h / 2 times the projected
    gradient and the flow moves q by h times that, 5e-21 times the gradient: below the rounding of q.  The retraction starts
    on the manifold, so its one Newton update moves q by rounding error (the distance is returned and bounded at 1e-13);
    what the step leaves is the forward scan of its rounds and of its final state evaluation at (to rounding) the fixture
    point: the scan with a guess trajectory, KernelPlan::fwd -- k_fwd_par under CHMC_PAR_SCAN=1.  Judged: constr() (one
    partition), which reads that scan's trajectory, and the current path, which k_path_par seeds with it, both at
    NULL_STEP_FACTOR."""
    f = load(cid)
    q = q_of(f)
    ctx.set_state(q, np.zeros_like(q), np.ascontiguousarray(f["x_obs"]), 0)
    r = ctx.leapfrog_step(NULL_STEP)
    assert (r["status"] == 0).all(), (cid, r["status"], r["iters_fwd"], r["iters_bwd"])
    dq = ctx.get_state(want_p=False, want_x_obs=False)[0] - q
    moved = float(np.abs(dq).max())
    print(f"REFRUN {copy}:null_step {cid} q_moved {moved:.2e} bound 1.00e-13 iters {r['iters_fwd'].tolist()}")
    assert moved <= 1e-13, (cid, moved)
    if single_partition(f):
        # scale: that of the fixture's c, the one its e_ref64 was measured with (the values here are residuals near zero)
        d = float(np.abs(ctx.constr() - own_data(f)[1]).max() / max(1.0, np.abs(f["c"]).max()))
        b = bound(f, "c", factor)
        print(f"REFRUN {copy}:null_step:constr {cid} c {d:.2e} bound {b:.2e}")
        assert d <= b, f"{copy}, {cid}: c after the null step is {d:.2e} from the reference's 50-digit run, bound {b:.2e}"
    x, sw = ctx.generate_x_seq(return_sweeps=True)
    judge(copy + ":null_step:current_path", cid, "x_seq", x, factor)
    return moved, sw


def judge_context(copy, cid, ctx, paths=True, factor=FACTOR):
    """The entry points of one context (emulation build or device) that produce fixture arrays, in the order: sequential
    path pass, set_state, update_x_obs_seq, constr, J w, J^T lam (the last three where the case has one partition)."""
    f = load(cid)
    q = q_of(f)
    if paths:
        judge(copy + ":generate_x_seq(q)", cid, "x_seq", ctx.generate_x_seq(q=q), factor)
    ctx.set_state(q, None, np.ascontiguousarray(f["x_obs"]), 0)
    ctx.update_x_obs_seq()
    judge(copy + ":update_x_obs_seq", cid, "x_obs", ctx.get_state(want_p=False)[2], factor)
    if single_partition(f):
        judge(copy + ":constr", cid, "c", ctx.constr(), factor)
        judge(copy + ":lmult_by_jacob_constr", cid, "Jw", ctx.lmult_by_jacob_constr(f["w"]), tol=OPERATOR_TOL)
        judge(copy + ":rmult_by_jacob_constr", cid, "JTlam", ctx.rmult_by_jacob_constr(f["lam"]), tol=OPERATOR_TOL)
