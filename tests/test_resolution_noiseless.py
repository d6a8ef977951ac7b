"""Carrying chains between time resolutions WITHOUT observation noise (chmc_set_state_project_device, the noiseless leg of
resolution.transfer_state, the two coarse-to-fine drivers), on the CPU through the TEST-ONLY emulation build.  The placed
states are judged by the constraint, by chmc_set_state, by the C oracle's projection from the NumPy-pinned x_obs_seq, and by
the identity that makes the correction a projection.  The check functions are shared with the GPU tests
(test_hip_resolution_noiseless.py)."""
import numpy as np
import pytest
import test_resolution as tr
from test_resolution import Dev, SEED, DT, state_ops
from test_emu_logic import emu_lib  # noqa: F401
from manifold_mcmc_for_diffusions_amd import example_models as em

# (model, T, S_c, m, R): R = None is a single partition.  m = 2, 3, 8, 65: the tilings of the refinement; R = 5: the 6-row
# instantiation of BASELINE configs[2]; fhn_nb: the notebook model, with R = 3 for both splittings of T = 7; R = 15 = T: one
# 16-row block; T S_dst = 1024 on the last
SHAPES = [("fhn", 6, 5, 2, 2), ("fhn", 6, 5, 3, 2), ("fhn", 4, 1, 8, 2), ("fhn", 4, 1, 65, 2), ("fhn", 10, 5, 2, 5),
          ("fhn_nb", 10, 5, 2, 5), ("fhn_nb", 7, 4, 2, 3), ("fhn", 15, 4, 2, 15), ("fhn", 5, 4, 2, None), ("fhn", 8, 16, 8, 3)]
FIRST = SHAPES[0]
# half of its chains are not placed -- an ordinary result of the solver, nothing provoked.  Measured on both builds: chains
# 0, 4, 5, 6 converge (4 to 6 iterations), 1, 3, 7 stop at max_iters = 50 (status 1), and chain 2 cannot be pinned (status 2,
# the solver not run): its refined path has x_1 = -191 against log y = -8.8 and Newton on exp from below overflows.  The
# issue's prototype pinned by assignment in NumPy and so saw four chains with status 1; its own rule for KPinObs gives this.
FAILING = ("sir", 4, 4, 2, None)
OBSERVED = {"fhn": 0, "fhn_nb": 0, "sir": 1}  # the coordinate obs_func reads


def shape_id(s):
    return f"{s[0]}-T{s[1]}-S{s[2]}-m{s[3]}-R{s[4]}"


def make_ctx(model, T, S, R, B):
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    return ChmcContext(model, DT[model], S, R, np.zeros(T), sigma=None, num_chains=B)


def pin(model, xo, y):
    """The issue's pinning rule restated: x_t moves along obs_grad, x <- x + g (y - obs(x)) / (g . g), at most 8 rounds, done
    when |y - obs(x)| <= 8 eps max(1, |y|).  obs_func reads one coordinate (x[0] itself for FitzHugh-Nagumo, exp(x[1]) for
    SIR), so the rule moves that coordinate alone: onto y in one round, or by Newton on exp.  Returns (x_obs_seq [B, T, X]
    pinned, ok [B]); a chain with an observation that does not get there has status 2 and the solver is not run for it."""
    xo, k, sir = xo.copy(), OBSERVED[model], model == "sir"
    x = xo[..., k]
    tol = 8 * np.finfo(float).eps * np.maximum(1.0, np.abs(y))
    with np.errstate(all="ignore"):
        r = y - (np.exp(x) if sir else x)
        for _ in range(8):
            todo = ~(np.abs(r) <= tol)
            if not todo.any():
                break
            g = np.exp(x) if sir else np.ones_like(x)
            x = np.where(todo, x + g * (r / (g * g)), x)
            r = y - (np.exp(x) if sir else x)
    ok = (np.abs(r) <= tol).all(1)
    xo[..., k] = x
    # where the rule gets there, the observed coordinate is the data's (the issue's "set to y")
    want = np.log(np.maximum(y, 1e-300)) if sir else y
    seen = np.abs(r) <= tol
    assert np.abs((xo[..., k] - want)[seen & (y > 1e-12)]).max() <= 1e-12
    return xo, ok


def start(shape, B=8, rows=slice(None)):
    """The coarse context at the issue's start states: q0 = 0.3 N(0, I) with the u-part a further third, the data of a chain
    obs_func of its own coarse path.  rows: the chains of the B drawn that the context holds."""
    from test_paths import path_by_models
    model, T, Sc, m, R = shape
    probe = make_ctx(model, T, Sc, R, 1)
    Q, U = probe.Q, probe.U
    probe.close()
    q0 = 0.3 * np.random.default_rng(5).standard_normal((B, Q))
    q0[:, :U] /= 3.0
    q0 = q0[rows]
    path = path_by_models(model, q0, T, Sc, DT[model], U)[:, Sc::Sc]
    y = em.MODELS[model].obs_func(path)[..., 0]
    coarse = make_ctx(model, T, Sc, R, len(q0))
    coarse.set_observations(y)
    coarse.set_state(q0, None, path, 0)
    assert np.abs(coarse.constr()).max() < 1e-12
    return coarse, y


def refined(coarse, fine, draw=9, chain_offset=0):
    """(device buffer, host copy) of the coarse states refined to fine's resolution."""
    src = Dev(coarse, coarse.get_state()[0])
    dst = Dev(fine, np.zeros((fine.B, fine.Q)))
    fine.resample_q_device(src.ptr, coarse.S, SEED, dst.ptr, draw=draw, chain_offset=chain_offset)
    return dst, dst.get()


def assert_placed(ctx, part, chains=None):
    """Assertion (1) on the chains listed (default all): on the manifold, at rest, bitwise the state chmc_set_state gives."""
    st = state_ops(ctx)
    sel = slice(None) if chains is None else chains
    assert st["part"] == part and not st["p"].any()
    assert np.abs(st["constr"][sel]).max() < 1e-9, np.abs(st["constr"]).max(1)
    ctx.set_state(st["q"], None, st["xo"], part)
    again = state_ops(ctx)
    for k in st:
        assert np.array_equal(st[k], again[k], equal_nan=True), k
    return st


def check_placed(shape, part, B=8):
    """Assertion (1): transfer_state puts every chain on the fine manifold of its data in the partition asked for."""
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state
    model, T, Sc, m, R = shape
    coarse, y = start(shape, B)
    fine = coarse.sibling(Sc * m)
    assert np.array_equal(fine.observations()[0], y)
    assert part < fine.num_partition
    out = transfer_state(coarse, fine, SEED, draw=9, partition=part)
    print(shape_id(shape), "partition", part, "iters", out["iters"].tolist(), "tries", out["tries"].tolist(),
          f"defect {out['defect'].min():.1e} .. {out['defect'].max():.1e}  moved {out['moved'].max():.1e}  "
          f"max|c| {out['max_constr']:.1e}")
    assert (out["status"] == 0).all() and out["max_constr"] < 1e-9 and (out["tries"] >= 1).all()
    assert sorted(out) == ["defect", "iters", "max_constr", "moved", "status", "tries"]
    assert_placed(fine, part)
    r = fine.leapfrog_step(0.02)
    assert (r["status"] == 0).all(), r
    fine.close(), coarse.close()
    return out


def oracle_projection(shape, fine, y, q_given, **solver):
    """The NumPy pin and the C oracle's project(q_prev = q, q, x_obs pinned, partition 0, dt = 1), a system per chain's data.
    Returns (defect [B], x_obs pinned [B, T, X], status [B], iters [B], q [B, Q])."""
    from oracle import c_oracle
    from test_paths import path_by_models
    model, T, Sc, m, R = shape
    okw = {dict(constraint_tol="ctol", position_tol="ptol", divergence_tol="dtol", max_iters="max_iters")[k]: v
           for k, v in solver.items() if k != "newton"}
    xo = path_by_models(model, q_given, T, fine.S, DT[model], fine.U)[:, fine.S::fine.S]
    defect = np.abs(y - em.MODELS[model].obs_func(xo)[..., 0]).max(1)
    xo, pinned = pin(model, xo, y)
    st, it, qs = [], [], []
    for c in range(len(q_given)):
        if not pinned[c]:
            st.append(2), it.append(0), qs.append(q_given[c])
            continue
        osys = c_oracle.OracleSystem(model, DT[model], fine.S, R, y[c], sigma=None)
        s, q, _, i, _, _ = osys.project(solver.get("newton", True), q_given[c], q_given[c], xo[c], 0, 1.0, **okw)
        st.append(s), it.append(i), qs.append(q)
    return defect, xo, np.array(st), np.array(it), np.array(qs)


def check_against_oracle(shape, B=8, expect_all=True, **solver):
    """Assertion (2), and for FAILING the per-chain statuses of (5)."""
    model, T, Sc, m, R = shape
    coarse, y = start(shape, B)
    fine = coarse.sibling(Sc * m)
    dst, q_given = refined(coarse, fine)
    r = fine.set_state_project(dst.ptr, 0, **solver)
    defect, xo, st, it, qo = oracle_projection(shape, fine, y, q_given, **solver)
    q, p, xo_dev, part = fine.get_state()
    print(shape_id(shape), solver, "status", r["status"].tolist(), "oracle", st.tolist(), "iters", r["iters"].tolist(),
          "oracle", it.tolist(), f"defect {defect.min():.1e} .. {defect.max():.1e}")
    assert np.abs(r["defect"] - defect).max() <= 1e-10
    assert r["status"].tolist() == st.tolist() and r["iters"].tolist() == it.tolist()
    assert np.array_equal(dst.get(), q_given)  # the caller's rows are never written
    ok = st == 0
    if expect_all:
        assert ok.all()
    for c in range(B):
        if ok[c]:
            assert np.abs(q[c] - qo[c]).max() <= 1e-9 * max(1.0, np.abs(qo[c]).max()), c
            assert r["moved"][c] == np.abs(q[c] - q_given[c]).max()
        else:  # the pinned, unprojected state
            assert np.array_equal(q[c], q_given[c]) and r["moved"][c] == 0
            assert r["iters"][c] == 0 if st[c] == 2 and not np.isfinite(xo[c]).all() else np.abs(xo_dev[c] - xo[c]).max() <= 1e-12
    out = dict(r, ok=ok, q=q, q_given=q_given, xo_pinned=xo)
    fine.close(), coarse.close()
    return out


def check_is_a_projection(shape, B=8, metric=False):
    """Assertion (3): the correction d = q placed - q given is the solver's M^-1 J^T lambda with J at the pinned, unprojected
    state, so M d = J^T lambda lies in the normal space there: normal_space_component (J^T G^-1 J M^-1, the complement of
    project_onto_cotangent_space) returns it unchanged.  With the identity metric that is d itself, as the issue states it;
    with a block metric M_0 the vector the identity holds for is d with its u-part multiplied by the chain's M_0 (d itself
    fails it by 0.93 relative on this shape, which is the metric at work, not an error of the placement)."""
    model, T, Sc, m, R = shape
    coarse, y = start(shape, B)
    if metric:
        G = np.random.default_rng(5).standard_normal((B, coarse.U, coarse.U))
        coarse.set_metric(np.einsum("bij,bkj->bik", G, G) + 2 * np.eye(coarse.U))  # a matrix per chain
    fine, at = coarse.sibling(Sc * m), coarse.sibling(Sc * m)
    dst, q_given = refined(coarse, fine)
    r = fine.set_state_project(dst.ptr, 0)
    assert (r["status"] == 0).all()
    d = fine.get_state()[0] - q_given
    from test_paths import path_by_models
    xo, _ = pin(model, path_by_models(model, q_given, T, fine.S, DT[model], fine.U)[:, fine.S::fine.S], y)
    at.set_state(q_given, None, xo, 0)
    md = d.copy()
    if metric:
        md[:, :fine.U] = np.einsum("bij,bj->bi", fine.metrics(), d[:, :fine.U])
    ns = at.normal_space_component(md)
    scale = np.abs(md).max(1)
    fig = float((np.abs(ns - md).max(1) / scale).max())
    print(shape_id(shape), "metric" if metric else "identity", f"max |M d| {scale.max():.1e}  |N M d - M d| / |M d| {fig:.1e}  "
          f"u moved {np.abs(d[:, :fine.U]).max():.1e}")
    assert scale.min() > 0 and fig <= 1e-9
    assert np.abs(d[:, :fine.U]).max() > 0  # u moves with the rest
    for c in (fine, at, coarse):
        c.close()
    return fig


def check_shards(shape, max_tries=3, want_retry=False, draw=4, **solver):
    """Assertions (4) and the retry contract of (5): six chains in one context against 2 x 3 with chain_offset.
    want_retry: the solver settings force retries (max_iters = 2 on FitzHugh-Nagumo; no listed shape retries by itself).  A
    chain's iteration count hangs on its coarse state far more than on xi, so some chains are retried and placed and some
    stay unplaced after every try: the call then raises, and what its tries left (the error's `result`) is held to the same
    contract -- tries, statuses, iterations and the states in the context, bitwise by global chain."""
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state
    model, T, Sc, m, R = shape

    def run(rows, offset):
        coarse, _ = start(shape, 6, rows)
        fine = coarse.sibling(Sc * m)
        try:
            out = transfer_state(coarse, fine, SEED, draw=draw, chain_offset=offset, max_tries=max_tries, solver=solver)
        except RuntimeError as err:
            assert want_retry
            out = err.result
            bad = np.flatnonzero(out["status"] != 0)
            assert f"chains {bad.tolist()} " in str(err) and (out["tries"][bad] == max_tries).all()
        res = dict(q=fine.get_state()[0], status=out["status"], iters=out["iters"], tries=out["tries"])
        fine.close(), coarse.close()
        return res
    whole = run(slice(None), 10)
    print(shape_id(shape), solver, "tries", whole["tries"].tolist(), "iters", whole["iters"].tolist(), "status",
          whole["status"].tolist())
    if want_retry:  # a chain placed at once, and a chain placed by a retry
        assert whole["tries"].min() == 1 and ((whole["tries"] > 1) & (whole["status"] == 0)).any(), whole
    else:
        assert (whole["status"] == 0).all()
    for lo in (0, 3):
        part = run(slice(lo, lo + 3), 10 + lo)
        for k in whole:
            assert np.array_equal(part[k], whole[k][lo:lo + 3]), (k, lo)
    return whole


def check_failure_contract(B=8):
    """Assertion (5) on FAILING: statuses as the oracle's, both kinds; converged chains placed, the others flagged and pinned."""
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state
    model, T, Sc, m, R = FAILING
    res = check_against_oracle(FAILING, B, expect_all=False)
    ok = res["ok"]
    assert ok.any() and (~ok).any() and set(res["status"][~ok].tolist()) <= {1, 2}
    coarse, _ = start(FAILING, B)
    fine = coarse.sibling(Sc * m)
    bad = np.flatnonzero(~ok).tolist()
    with pytest.raises(RuntimeError) as err:
        transfer_state(coarse, fine, SEED, draw=9, max_tries=1)
    assert f"chains {bad} " in str(err.value) and f"status {res['status'][~ok].tolist()}" in str(err.value)
    # the context holds what the failed call left: the converged chains placed, the others pinned and unprojected
    st = assert_placed(fine, 0, np.flatnonzero(ok))
    assert np.array_equal(st["q"][~ok], res["q_given"][~ok]) and np.abs(st["constr"][~ok]).max() > 1e-9
    r = fine.leapfrog_step(0.02, active=ok.astype(np.int32))
    assert (r["status"][ok] == 0).all(), r
    fine.close(), coarse.close()
    return res


def check_errors():
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state
    noisy = tr.make_ctx("fhn", 4, 2, 0.1, 2, R=2)
    q = Dev(noisy, np.zeros((2, noisy.Q)))
    with pytest.raises(RuntimeError, match="chmc_set_state_solve_noise_device"):
        noisy.set_state_project(q.ptr, 0)
    noisy.close()
    coarse, _ = start(FIRST, 2)
    fine = coarse.sibling(10)
    dst, _ = refined(coarse, fine)
    with pytest.raises(RuntimeError, match="null"):
        fine.set_state_project(0, 0)
    with pytest.raises(RuntimeError, match="partition"):
        fine.set_state_project(dst.ptr, 5)
    with pytest.raises(RuntimeError, match="max_iters"):
        fine.set_state_project(dst.ptr, 0, max_iters=-1)
    with pytest.raises(RuntimeError, match="no state"):
        fine.set_state_project(dst.ptr, 0, mask=[1, 0])
    with pytest.raises(ValueError, match="2\\^32"):
        transfer_state(coarse, fine, SEED, draw=1 << 32)
    transfer_state(coarse, fine, SEED, draw=1 << 32, max_tries=1)  # a single try takes any draw below 2^45
    # a partial mask on a context with a state: the other chain keeps position, momentum and x_obs_seq
    fine.sample_momentum(SEED, 1, 0)
    q0, p0, x0, _ = fine.get_state()
    dst, q_given = refined(coarse, fine, draw=11)
    r = fine.set_state_project(dst.ptr, 0, mask=[0, 1])
    q1, p1, x1, _ = fine.get_state()
    assert r["status"].tolist() == [-1, 0] and r["iters"][0] == 0
    assert np.array_equal(q1[0], q0[0]) and np.array_equal(p1[0], p0[0]) and np.array_equal(x1[0], x0[0])
    assert not np.array_equal(q1[1], q0[1]) and not p1[1].any() and np.abs(fine.constr()).max() < 1e-9
    # ... and into the other partition: the call's chain is placed there, the other one is evaluated there from what it holds
    dst, _ = refined(coarse, fine, draw=12)
    r = fine.set_state_project(dst.ptr, 1, mask=[1, 0])
    st = state_ops(fine)
    assert r["status"].tolist() == [0, -1] and st["part"] == 1 and np.abs(st["constr"]).max() < 1e-9
    assert np.array_equal(st["q"][1], q1[1]) and np.array_equal(st["p"][1], p1[1]) and np.array_equal(st["xo"][1], x1[1])
    assert np.array_equal(st["p"][0], np.zeros(fine.Q)) and not np.array_equal(st["q"][0], q1[0])
    fine.set_state(st["q"], st["p"], st["xo"], 1)
    again = state_ops(fine)
    for k in st:
        assert np.array_equal(st[k], again[k]), k
    fine.close(), coarse.close()


DYNAMIC_KEYS = ("n_step", "integrator_error", "adapted_step_sizes", "chain_outcomes_dynamic", "per_chain")


def check_driver(dynamic):
    """Assertion (7): S = 2 -> 4 -> 8, noiseless FHN T = 4, B = 4, a matrix per chain, a handful of transitions."""
    from manifold_mcmc_for_diffusions_amd.resolution import coarse_to_fine_static_chmc, coarse_to_fine_dynamic_chmc
    coarse, y = start(("fhn", 4, 2, 2, 2), 4)
    G = np.random.default_rng(5).standard_normal((4, coarse.U, coarse.U))
    coarse.set_metric(np.einsum("bij,bkj->bik", G, G) + 2 * np.eye(coarse.U))
    ladder = [coarse.sibling(4), coarse.sibling(8)]
    if dynamic:
        out = coarse_to_fine_dynamic_chmc(coarse, ladder, n_warm_coarse=4, n_warm_fine=2, n_main=3, step_size=0.05, seed=SEED,
                                          max_tree_depth=3)
        assert all(k in out for k in DYNAMIC_KEYS)
    else:
        out = coarse_to_fine_static_chmc(coarse, ladder, n_warm_coarse=4, n_warm_fine=2, n_main=3, n_step=2, step_size=0.05,
                                         seed=SEED)
        assert "fail_rate" in out
    rungs = out["rungs"]
    keys = sorted(["S", "seconds", "first_step_size", "final_step_size", "mean_accept_stat", "moved", "max_constr", "defect",
                   "tries", "proj_iters"])
    assert [r["S"] for r in rungs] == [2, 4, 8] and len(out["accept_stat"]) == 5 and out["heads"].shape[:2] == (5, 4)
    assert all(sorted(r) == keys for r in rungs)
    for prev, r in zip(rungs, rungs[1:]):
        assert r["first_step_size"] == prev["final_step_size"]  # the step sizes are handed on
        assert r["max_constr"] < 1e-9 and (r["tries"] >= 1).all() and (r["proj_iters"] >= 1).all()
        assert r["moved"].shape == r["defect"].shape == (4,) and (r["defect"] > 0).all() and (r["moved"] > 0).all()
    assert all(rungs[0][k] is None for k in ("moved", "defect", "tries", "proj_iters")) and rungs[0]["first_step_size"] == 0.05
    assert out["final_step_size"] == rungs[-1]["final_step_size"] and out["step_size"][0] == rungs[1]["final_step_size"]
    print("dynamic" if dynamic else "static", [(r["S"], r["final_step_size"], r["max_constr"]) for r in rungs])
    for ctx in ladder:
        assert ctx.per_chain_metric and np.array_equal(ctx.metrics(), coarse.metrics())  # the metric arrives
        assert np.array_equal(ctx.observations()[0], y)                                 # and the data
        assert np.abs(ctx.constr()).max() < 1e-8
    for c in ladder + [coarse]:
        c.close()


# ---- the tests
# both partitions where the layout has two
PLACED = [(s, p) for s in SHAPES for p in ((0, 1) if s[4] is not None and s[4] < s[1] else (0,))]


def placed_id(sp):
    return f"{shape_id(sp[0])}-p{sp[1]}"


@pytest.mark.parametrize("shape_part", PLACED, ids=placed_id)
def test_placed_on_the_manifold(emu_lib, shape_part):  # noqa: F811
    check_placed(*shape_part)


def test_last_pin_workgroup_is_partial(emu_lib):  # noqa: F811
    check_placed(FIRST, 1, B=130)


@pytest.mark.parametrize("newton", [True, False])
def test_against_the_oracle(emu_lib, newton):  # noqa: F811
    check_against_oracle(FIRST, newton=newton)


@pytest.mark.parametrize("shape", [SHAPES[5], SHAPES[7]], ids=shape_id)
def test_against_the_oracle_other_layouts(emu_lib, shape):  # noqa: F811
    check_against_oracle(shape, B=3)


@pytest.mark.parametrize("metric", [False, True])
def test_the_correction_is_a_projection(emu_lib, metric):  # noqa: F811
    check_is_a_projection(FIRST, metric=metric)


def test_shard_independence(emu_lib):  # noqa: F811
    check_shards(FIRST)


def test_retries_depend_on_the_global_chain_alone(emu_lib):  # noqa: F811
    check_shards(SHAPES[9], want_retry=True, max_iters=2)


def test_failure_contract(emu_lib):  # noqa: F811
    check_failure_contract()


def test_errors(emu_lib):  # noqa: F811
    check_errors()


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_coarse_to_fine_drivers(emu_lib, dynamic):  # noqa: F811
    check_driver(dynamic)
