"""Helpers for the tests of per-chain block metrics (chmc_set_metrics): the groups of tests/grouped_obs.py, every group with
its own data (y_g, sigma_g) AND its own M_0, in ONE context -- against one context per group that holds the group's data as
shared data and its matrix through set_metric(M_g), the way every other test of the suite runs.

Test infrastructure only (may import oracle/)."""
import threading
import numpy as np
import pytest
import grouped_obs as go
from helpers import random_metric

LAYOUTS = sorted(n for n in go.LAYOUTS if not go.LAYOUTS[n][5])  # without Gaussian splitting (no metric there)
A, C_, D, E, F, G = LAYOUTS
MIN_M_GAP = 1.0  # the groups' matrices differ by at least this much in some entry


def group_metrics(U, n=len(go.SIZES)):
    """M_g = random_metric(default_rng(100 + g), U); pairwise apart by MIN_M_GAP in some entry, so that a broadcast of chain
    0's metric cannot pass."""
    Ms = np.stack([random_metric(np.random.default_rng(100 + g), U) for g in range(n)])
    for a in range(n):
        for b in range(a + 1, n):
            assert np.abs(Ms[a] - Ms[b]).max() >= MIN_M_GAP, (a, b, np.abs(Ms[a] - Ms[b]).max())
    return Ms


def grouped_metric_ctx(gc, Ms):
    """ONE context of all B chains with per-chain data and per-chain metrics; metrics() returns exactly what was set."""
    ctx = go.grouped_ctx(gc)
    ctx.set_metric(Ms, groups=gc["groups"])
    assert ctx.per_chain_metric and np.array_equal(ctx.metrics(), Ms[gc["groups"]]) and np.array_equal(ctx.M_0, Ms[gc["groups"]])
    return ctx


def run_grouped_vs_separate(gc, nld=True):
    """Test 1 (and its host-logic twin).  Control first: the 13 chains with ONE shared data set and ONE shared metric as one
    context and as the 4 | 5 | 4 split; then one context with per-chain (y, sigma, M_0) against one context per group with
    that group's data as shared data and set_metric(M_g); last the grouped data with group 0's matrix on every chain, from
    which groups 1 and 2 must differ (the metrics reached the kernels).
    Returns (control differences, grouped differences, the grouped run, the grouped context's diagnostics)."""
    p, dts, active, failing = go.sequence_inputs(gc)
    c0 = gc["cases"][0]
    if gc["noisy"] and gc["model"] != "sir":
        q_ctl = go.on_manifold(gc["model"], gc["q"], gc["x_obs"], c0["y"], c0["sigma"], gc["var_sigma"])
        xo_ctl = gc["x_obs"]
    else:
        q_ctl, xo_ctl = np.repeat(c0["q"][:1], gc["B"], 0), np.repeat(c0["x_obs"][:1], gc["B"], 0)
    ctx = go.shared_ctx(gc, c0["y"], c0["sigma"], gc["B"])
    Ms = group_metrics(ctx.U)
    ctx.set_metric(Ms[0])
    assert not ctx.per_chain_metric and np.array_equal(ctx.metrics(), np.repeat(Ms[:1], gc["B"], 0))
    whole = go.run_sequence(ctx, q_ctl, p, xo_ctl, dts, active, failing, nld)
    ctx.close()
    parts = []
    for sl in gc["slices"]:
        ctx = go.shared_ctx(gc, c0["y"], c0["sigma"], sl.stop - sl.start)
        ctx.set_metric(Ms[0])
        parts.append(go.run_sequence(ctx, q_ctl[sl], p[sl], xo_ctl[sl], dts[sl], active[sl], failing[sl], nld))
        ctx.close()
    control_bad = go.split_equals_whole(whole, parts, gc["slices"])
    # -- per-chain data and metrics
    go.assert_groups_differ(gc)
    ctx = grouped_metric_ctx(gc, Ms)
    whole = go.run_sequence(ctx, gc["q"], p, gc["x_obs"], dts, active, failing, nld)
    diag = ctx.diagnostics()
    ctx.close()
    parts = []
    for g, (sl, case) in enumerate(zip(gc["slices"], gc["cases"])):
        ctx = go.shared_ctx(gc, case["y"], case["sigma"], sl.stop - sl.start)
        ctx.set_metric(Ms[g])
        parts.append(go.run_sequence(ctx, gc["q"][sl], p[sl], gc["x_obs"][sl], dts[sl], active[sl], failing[sl], nld))
        ctx.close()
    bad = go.split_equals_whole(whole, parts, gc["slices"])
    # -- group 0's matrix on every chain: groups 1 and 2 must come out differently
    ctx = go.grouped_ctx(gc)
    ctx.set_metric(Ms[0])
    flat = dict(go.run_sequence(ctx, gc["q"], p, gc["x_obs"], dts, active, failing, nld))
    ctx.close()
    rec = dict(whole)
    for key in ("set.log_det", "pre.q"):
        assert np.array_equal(rec[key][gc["slices"][0]], flat[key][gc["slices"][0]]), key
        for sl in gc["slices"][1:]:
            a, b = rec[key][sl].reshape(sl.stop - sl.start, -1), flat[key][sl].reshape(sl.stop - sl.start, -1)
            assert (a != b).any(1).all(), (key, sl)
    return control_bad, bad, whole, diag


def assert_status_pattern(whole):
    rec = dict(whole)
    status0 = rec["step0.status"]
    assert status0[5] == -1 and (status0[[2, 7]] > 0).all() and (np.delete(status0, [2, 5, 7]) == 0).all(), status0
    assert (rec["steps.n_done"] == 2).all()


def check_against_oracle(name, seed=42):
    """Test 2: go.check_grouped_against_oracle on a context with per-chain metrics, every group's oracle system carrying the
    group's M_g (reset afterwards)."""
    gc = go.make_groups(name, seed=seed)
    Ms = None
    try:
        ctx = go.grouped_ctx(gc)
        Ms = group_metrics(ctx.U)
        ctx.set_metric(Ms, groups=gc["groups"])
        for g, case in enumerate(gc["cases"]):
            case["osys"].set_metric(Ms[g])
        worst = go.check_grouped_against_oracle(ctx, gc)
        ctx.close()
    finally:
        for case in gc["cases"]:
            case["osys"].set_metric(None)
    return worst


def check_momentum(name=A, seed=49):
    """Test 4: sample_momentum on a grouped context: per chain metric.sqrt @ n with the chain's own chol(M_g) on the u-part
    of the keyed normals, projected with J M^-1 of the chain's own system."""
    from test_rng import reference_normals
    gc = go.make_groups(name, seed=seed)
    ctx = go.grouped_ctx(gc)
    Ms = group_metrics(ctx.U)
    ctx.set_metric(Ms, groups=gc["groups"])
    assert np.array_equal(ctx.metrics(), Ms[gc["groups"]])
    U, worst = ctx.U, 0.0
    try:
        for g, case in enumerate(gc["cases"]):
            case["osys"].set_metric(Ms[g])
        ctx.set_state(gc["q"], None, gc["x_obs"], 0)
        ctx.sample_momentum(77, 2, 1)
        p = ctx.get_state()[1]
        for c in range(gc["B"]):
            g = gc["groups"][c]
            n = reference_normals(ctx.Q, c + 1, 77, 2)
            n[:U] = np.linalg.cholesky(Ms[g]) @ n[:U]
            expect = n - gc["cases"][g]["osys"].jacob_products(gc["q"][c], gc["x_obs"][c], 0, n, np.zeros(ctx.dim_c))[3]
            np.testing.assert_allclose(p[c], expect, rtol=1e-9, atol=1e-10)
            worst = max(worst, float(np.abs(p[c] - expect).max()))
    finally:
        for case in gc["cases"]:
            case["osys"].set_metric(None)
    ctx.close()
    return worst


def _three_steps(ctx, gc):
    p, dts, _, _ = go.sequence_inputs(gc)
    ctx.set_state(gc["q"], p, gc["x_obs"], 0)
    out = []
    for _ in range(3):
        r = ctx.leapfrog_step(dts, max_iters=12)
        q1, p1, _, _ = ctx.get_state()
        out += [r["status"].copy(), r["iters_fwd"].copy(), r["rev_err"].copy(), q1, p1, ctx.hamiltonian(), ctx.log_det_sqrt_gram()]
    return out


def check_api_misuse(lib):
    """Test 5: each misuse returns a negative value with a chmc_last_error text and leaves the context (and its metrics) as
    they were; set_metric(M) / set_metric(None) after set_metrics equal contexts that only ever had M / the identity."""
    from manifold_mcmc_for_diffusions_amd._lib import ptr
    gc = go.make_groups(A, seed=44)
    B = gc["B"]
    ctx = go.grouped_ctx(gc)
    U = ctx.U
    Ms = group_metrics(U)
    per_chain = np.ascontiguousarray(Ms[gc["groups"]])
    ctx.set_metric(per_chain)  # [B, U, U]
    assert ctx.per_chain_metric

    def usable():
        assert np.array_equal(ctx.metrics(), per_chain)
        ctx.set_state(gc["q"], None, gc["x_obs"], 0)
        assert np.isfinite(ctx.constr()).all() and (ctx.leapfrog_step(0.02)["status"] >= 0).all()

    bad = per_chain.copy()
    bad[6, 0, 1] += 0.5  # not symmetric, chain 6
    assert lib.chmc_set_metrics(ctx.h, ptr(bad)) < 0 and b"chain 6 is not symmetric" in lib.chmc_last_error()
    bad = per_chain.copy()
    bad[9] -= 10.0 * np.eye(U)  # indefinite, chain 9
    assert lib.chmc_set_metrics(ctx.h, ptr(bad)) < 0 and b"chain 9 is not positive definite" in lib.chmc_last_error()
    with pytest.raises(RuntimeError, match="chain 9"):
        ctx.set_metric(bad)
    assert lib.chmc_set_metrics(ctx.h, None) < 0 and b"null" in lib.chmc_last_error()
    assert lib.chmc_get_metric(ctx.h, None) < 0 and b"null" in lib.chmc_last_error()
    res = {}

    def other():
        res["rc"] = lib.chmc_set_metrics(ctx.h, ptr(per_chain))
        res["err"] = lib.chmc_last_error()  # (the text is thread-local)
        res["rc_get"] = lib.chmc_get_metric(ctx.h, ptr(np.empty_like(per_chain)))

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert res["rc"] < 0 and res["rc_get"] < 0 and b"thread" in res["err"]
    with pytest.raises(ValueError, match="M_0 must have shape"):
        ctx.set_metric(per_chain[:-1])
    with pytest.raises(ValueError, match="groups must be"):
        ctx.set_metric(Ms, groups=gc["groups"] + 1)
    usable()
    # Gaussian splitting: refused, as one metric is
    g2 = go.make_groups("b_fhn_noiseless_gauss", seed=45)
    cg = go.grouped_ctx(g2)
    assert lib.chmc_set_metrics(cg.h, ptr(per_chain)) < 0 and b"Gaussian splitting" in lib.chmc_last_error()
    assert np.array_equal(cg.metrics(), np.repeat(np.eye(U)[None], B, 0))
    cg.set_state(g2["q"], None, g2["x_obs"], 0)
    assert (cg.leapfrog_step(0.02)["status"] >= 0).all()
    cg.close()
    # back to one shared matrix, and to the identity: bitwise a context that never had per-chain metrics
    for M in (Ms[1], None):
        ctx.set_metric(per_chain)
        ctx.set_metric(M)
        assert not ctx.per_chain_metric
        assert np.array_equal(ctx.metrics(), np.repeat((np.eye(U) if M is None else M)[None], B, 0))
        got = _three_steps(ctx, gc)
        fresh = go.grouped_ctx(gc)
        if M is not None:
            fresh.set_metric(M)
        want = _three_steps(fresh, gc)
        fresh.close()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want)), M
    ctx.close()


def check_transitions(name, seed, eps, depth=3, n_step=3, screening=False):
    """Test 3: grouped_obs.check_transitions on a context with per-chain metrics: one no-U-turn transition and one static
    transition, every chain judged by oracle_tree_transition(.., W=inv(M_g)) / oracle_static_transition(.., M0=M_g) on its own
    oracle system.  Decisions equal with no allowance, accept statistic and log weight to 1e-9, positions to 1e-9 max(1, |q|)
    per leaf; every oracle margin must pass test_hip_tree_oracle.admissible (seeds screened on the CPU; with `screening` the
    inadmissible margins are returned instead of asserted).  No chain is left out."""
    from helpers import oracle_static_transition, oracle_tree_transition
    from test_hip_tree_oracle import admissible
    from manifold_mcmc_for_diffusions_amd.dynamic import DynamicTransition, TreeUniforms
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    solver = go.TRANSITION_SOLVER
    gc = go.make_groups(name, seed=48)
    go.assert_groups_differ(gc)
    B = gc["B"]
    osys_of = [gc["cases"][g]["osys"] for g in gc["groups"]]
    ctx = go.grouped_ctx(gc)
    Ms = group_metrics(ctx.U)
    M_of = Ms[gc["groups"]]
    ctx.set_metric(Ms, groups=gc["groups"])
    problems, worst = [], dict(position=0.0, accept_stat=0.0, logw=0.0)
    try:
        for g, case in enumerate(gc["cases"]):
            case["osys"].set_metric(Ms[g])
        # ---- one dynamic transition
        ctx.set_state(gc["q"], None, gc["x_obs"], 0)
        tr = DynamicTransition(ctx, eps, seed, max_tree_depth=depth, max_delta_h=1000.0, solver=dict(solver))
        ctx.sample_momentum(seed, 1)
        q0, p0, xo0, part = ctx.get_state()
        st = tr.sample(0)
        logw = ctx.tree_get_doubling()["logw"]
        q1 = ctx.get_state()[0]
        un = TreeUniforms(seed, 0, B, 0, B)
        leaves = []
        for c in range(B):
            r = oracle_tree_transition(osys_of[c], q0[c], p0[c], xo0[c], part, lambda kind, d, k, c=c: un.get(kind, d, k)[c],
                                       eps, depth, 1000.0, dict(solver), np.linalg.inv(M_of[c]))
            bad = admissible(r["margins"])
            if bad:
                problems.append(("tree", c, bad))
                continue
            got = (st["n_step"][c], st["depth"][c], bool(st["moved"][c]), bool(st["integrator_error"][c]), bool(st["diverged"][c]))
            want = (r["n_step"], r["depth"], r["moved"], r["event"][0] == "error", r["event"][0] == "diverged")
            assert got == want, (c, got, want, r["event"])
            acc = r["sum_acc"] / max(r["n_step"], 1)
            e_acc = abs(st["accept_stat"][c] - acc) / max(1.0, abs(acc))
            e_logw = abs(logw[c] - r["logw"]) / max(1.0, abs(r["logw"]))
            assert e_acc <= 1e-9 and e_logw <= 1e-9, (c, e_acc, e_logw)
            e_q = np.abs(q1[c] - r["q"]).max() / max(1.0, np.abs(r["q"]).max())
            assert e_q <= 1e-9 * abs(r["offset"]) if r["offset"] else np.array_equal(q1[c], q0[c]), (c, e_q, r["offset"])
            worst["accept_stat"], worst["logw"] = max(worst["accept_stat"], e_acc), max(worst["logw"], e_logw)
            worst["position"] = max(worst["position"], e_q / max(abs(r["offset"]), 1))
            leaves.append(r["n_step"])
        # ---- one static transition: the sampler's own draws, restated
        ctx.set_state(gc["q"], None, gc["x_obs"], 0)
        res = sample_static_chmc(ctx, 1, n_step, eps, seed, n_adapt=0, solver=dict(solver), n_head=ctx.Q)
        rng = np.random.default_rng(seed)
        dt = np.where(rng.random(B) < 0.5, eps, -eps)
        u = rng.random(B)
        accepted = []
        for c in range(B):
            r = oracle_static_transition(osys_of[c], gc["q"][c], gc["x_obs"][c], 0, c, seed, 1, M_of[c], dt[c], n_step, u[c],
                                         dict(solver))
            bad = admissible(r["margins"])
            if bad:
                problems.append(("static", c, bad))
                continue
            outcome = res["chain_outcomes"][c]
            want_col = 1 + min(max(r["status"], 1), 3) if r["status"] > 0 else (0 if r["accepted"] else 1)
            assert outcome[want_col] == 1 and outcome.sum() == 1, (c, outcome, r["status"], r["accepted"])
            if r["accepted"]:
                e_q = np.abs(res["heads"][0, c] - r["q"]).max() / max(1.0, np.abs(r["q"]).max())
                assert e_q <= 1e-9 * n_step, (c, e_q)
                worst["position"] = max(worst["position"], e_q / n_step)
            else:
                assert np.array_equal(res["heads"][0, c], gc["q"][c]), c
            accepted.append(r["accepted"])
    finally:
        for case in gc["cases"]:
            case["osys"].set_metric(None)
        ctx.close()
    if screening:
        return problems, leaves, accepted
    assert not problems, f"the oracle's own decision margins (screening): {problems}"
    assert max(leaves) >= 3 and any(accepted), (leaves, accepted)  # (trees that grew, trajectories that were accepted)
    return dict(worst, leaves=leaves, accepted=accepted)
