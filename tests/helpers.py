"""Shared test helpers: synthetic cases for the conditioned-diffusion system and oracle access.

Test infrastructure only (may import oracle/)."""
import numpy as np
from oracle import c_oracle
from autodiff_checks import UNJUDGED, distance, failures
from manifold_mcmc_for_diffusions_amd import example_models as em

FHN_U = np.array([-1.2, -2.0, 0.4, 0.8])  # log sigma, log eps, log gamma, beta  (sigma 0.3, eps 0.135, gamma 1.5)
SIR_U = np.array([-1.0, -1.0, 1.0, 0.0])
FHN_NB_U = np.array([-0.4, -0.0, 1.0, -0.4])  # notebook priors: sigma 0.30, eps 0.135, gamma 1.5, beta 0.8


def random_q(model, T, S, noisy, B, rng, v_scale=0.3, u_scale=0.1, var_sigma=False):
    """var_sigma: variable observation noise, u gets a fifth component log sigma (dim_u = dim_z + 1)."""
    m = em.MODELS[model]
    U = m.dim_z + int(var_sigma)
    Q = U + m.dim_v_0 + T * S * m.dim_v + (T if noisy else 0)
    q = np.zeros((B, Q))
    u0 = FHN_U if model == "fhn" else FHN_NB_U if model == "fhn_nb" else SIR_U
    q[:, :4] = u_scale * rng.standard_normal((B, 4)) + u0
    if var_sigma:
        q[:, 4] = (np.log(0.1) if model in ("fhn", "fhn_nb") else 0.0) + u_scale * rng.standard_normal(B)
    if model in ("fhn", "fhn_nb"):
        q[:, U:U + 2] = 0.5 * rng.standard_normal((B, 2))
    else:
        q[:, U:U + 1] = 1.0 + 0.1 * rng.standard_normal((B, 1))
    nv = T * S * m.dim_v
    o = U + m.dim_v_0
    q[:, o:o + nv] = v_scale * rng.standard_normal((B, nv))
    if noisy:
        q[:, o + nv:] = rng.standard_normal((B, T))
    return q


def make_case(model, T, S, R, noisy, B, seed, obs_interval=None, gaussian=False, var_sigma=False):
    """Random chain states; the data are generated from chain 0 so that chain 0 lies on the manifold
    (c(q_0) = 0 in every partition).  Returns dict with q [B,Q], x_obs [B,T,X], y [T], sigma, oracle system.
    var_sigma: sigma = generate_sigma(u) = exp(u[dim_z]) (noisy observations only); case["sigma"] is then "variable"."""
    rng = np.random.default_rng(seed)
    m = em.MODELS[model]
    if obs_interval is None:
        obs_interval = 0.2 if model in ("fhn", "fhn_nb") else 0.25
    sigma = (0.1 if model in ("fhn", "fhn_nb") else 1.0) if noisy else None
    if var_sigma:
        assert noisy
        sigma = "variable"
    q = random_q(model, T, S, noisy, B, rng, var_sigma=var_sigma)
    tmp = c_oracle.OracleSystem(model, obs_interval, S, R, np.zeros(T), sigma=sigma, use_gaussian_splitting=gaussian)
    xo = np.stack([tmp.generate_x_obs_seq(q[c]) for c in range(B)])
    y = m.obs_func(xo[0])[:, 0] + ((np.exp(q[0, m.dim_z]) if var_sigma else sigma) * q[0, -T:] if noisy else 0.0)
    osys = c_oracle.OracleSystem(model, obs_interval, S, R, y, sigma=sigma, use_gaussian_splitting=gaussian)
    return dict(model=model, T=T, S=S, R=R, noisy=noisy, B=B, q=q, x_obs=xo, y=y, sigma=sigma,
                obs_interval=obs_interval, gaussian=gaussian, osys=osys, rng=rng)


def make_ctx(case, **kw):
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    return ChmcContext(case["model"], case["obs_interval"], case["S"], case["R"], case["y"], sigma=case["sigma"],
                       use_gaussian_splitting=case["gaussian"], num_chains=case["B"], **kw)


def _upd(worst, k, a, b):
    """worst[k] = the larger of itself and the distance of the library's `a` from the reference `b` (inf where `a` is not
    finite and `b` is); returns whether every entry of the reference was finite, i.e. whether all of `a` was judged."""
    e, judged = distance(a, b)
    worst[k] = max(worst.get(k, 0.0), e)
    return judged


def _count_unjudged(worst, judged):
    """worst[UNJUDGED] += the chains of `judged` (one flag per chain) with a reference value that was not finite."""
    worst[UNJUDGED] = worst.get(UNJUDGED, 0) + sum(not j for j in judged)


def _ops_at_point(ctx, osys, q, xo, part, rng, worst):
    """Every per-op entry point of the C ABI at the context's current state, which the caller says is (q, xo, part)."""
    B = ctx.B

    judged = [True] * B  # per chain: every reference value finite

    def upd(k, a, b):
        judged[c] &= _upd(worst, k, a, b)

    c_h = ctx.constr()
    du_h, dv_h = ctx.jacob_constr_blocks()
    cC, cD = ctx.chol_gram_blocks()
    ld = ctx.log_det_sqrt_gram()
    g = ctx.grad_log_det_sqrt_gram()
    w = rng.standard_normal((B, ctx.Q))
    lam = rng.standard_normal((B, ctx.dim_c))
    Jw, JTl = ctx.lmult_by_jacob_constr(w), ctx.rmult_by_jacob_constr(lam)
    Gil, nsc = ctx.lmult_by_inv_gram(lam), ctx.normal_space_component(w)
    for c in range(B):
        c_o, du_o, dv_o = osys.jacob_constr_blocks(q[c], xo[c], part)
        cCo, cDo, ldo, go = osys.gram_ops(q[c], xo[c], part)
        Jwo, JTlo, Gilo, nsco = osys.jacob_products(q[c], xo[c], part, w[c], lam[c])
        rm = osys.rmax
        upd("constr", c_h[c], c_o)
        upd("dc_du", du_h[c], du_o)
        upd("dc_dv", dv_h[c][:rm], dv_o)
        if ctx.RM > rm:
            upd("dc_dv_pad", dv_h[c][rm:], np.zeros_like(dv_h[c][rm:]))
        upd("chol_C", cC[c], cCo)
        for b in range(ctx.num_blocks):
            r = osys.block_info(part, b)["nrows"]
            upd("chol_D", cD[c][b][:r, :r], cDo[b][:r, :r])
        upd("log_det", np.array([ld[c]]), np.array([ldo]))
        upd("grad_log_det", g[c], go)
        upd("lmult_jacob", Jw[c], Jwo)
        upd("rmult_jacob", JTl[c], JTlo)
        upd("inv_gram", Gil[c], Gilo)
        upd("normal_space", nsc[c], nsco)
    return judged


def check_ops_against_oracle(ctx, case, tol=1e-10, parts=None):
    """Every per-op entry point of the C ABI against the C oracle, for every partition; returns max rel errors and, under
    "unjudged_chains", how many (partition, chain) points the oracle itself had a non-finite value at (not compared there).
    parts: the partitions to visit (default: all, in order)."""
    osys, q, xo, B = case["osys"], case["q"], case["x_obs"], case["B"]
    rng = case["rng"]
    worst = {}
    for part in range(ctx.num_partition) if parts is None else parts:
        p = rng.standard_normal((B, ctx.Q))
        ctx.set_state(q, p, xo, part)
        _count_unjudged(worst, _ops_at_point(ctx, osys, q, xo, part, rng, worst))
    bad = failures(worst, tol)
    assert not bad, f"op parity failures (rel err): {bad}; all: {worst}"
    return worst


def check_ops_at_current_state(ctx, osys, tol=1e-10, x_obs_current=True, rng=None):
    """The body of check_ops_against_oracle WITHOUT its set_state: the state caches the context holds right now (after a
    restore, a tree, a partition switch) are judged at the point the context reports.  Reads (q, p, x_obs, partition) back
    with get_state(); every per-op entry point, chain by chain, against the C oracle at those points; hamiltonian()
    against OracleChain.hamiltonian() of a chain set to the reported (q, p); the reported x_obs_seq against
    osys.generate_x_obs_seq(q).  The library refreshes x_obs_seq in set_state and in switch_partition only (as the oracle's
    chain does): `x_obs_current` says, for all chains or per chain, whether the position has moved since; for a chain that
    has, the conditioned entries of x_obs_seq are still judged, through `constr`.  osys carries the context's metric."""
    q, p, xo, part = ctx.get_state()
    assert (ctx.M_0 is None) == (getattr(osys, "M0", None) is None), "oracle and context must have the same metric"
    worst = {}
    judged = _ops_at_point(ctx, osys, q, xo, part, np.random.default_rng(0) if rng is None else rng, worst)
    h = ctx.hamiltonian()
    current = np.broadcast_to(np.asarray(x_obs_current, dtype=bool), (ctx.B,))
    for c in range(ctx.B):
        ch = c_oracle.OracleChain(osys)
        ch.set(q[c], p[c], xo[c], part)
        judged[c] &= _upd(worst, "hamiltonian", np.array([h[c, 0]]), np.array([ch.hamiltonian()]))
        if current[c]:
            judged[c] &= _upd(worst, "x_obs_seq", xo[c], osys.generate_x_obs_seq(q[c]))
    _count_unjudged(worst, judged)
    bad = failures(worst, tol)
    assert not bad, f"op parity failures at the current state (rel err): {bad}; all: {worst}"
    return worst


def check_steps_against_oracle(ctx, case, dts, newton=True, n_steps=1, tol=1e-9, part=0, project=True, n_inner=1,
                               step_kw=None):
    """Fused leapfrog steps against the C oracle chain by chain, starting from chain 0's on-manifold state with
    independent momenta (project=False: momenta that are NOT in the cotangent space, which the first half-kick of
    the integrator has to project -- the library then cannot use its projected-gradient shortcut)."""
    osys, B = case["osys"], case["B"]
    rng = case["rng"]
    qq = np.repeat(case["q"][:1], B, 0)
    xx = np.repeat(case["x_obs"][:1], B, 0)
    ctx.set_state(qq, rng.standard_normal((B, ctx.Q)), xx, part)
    if project:
        ctx.project_onto_cotangent_space()
    _, p0, _, _ = ctx.get_state()
    chains = []
    for c in range(B):
        ch = c_oracle.OracleChain(osys)
        ch.set(qq[c], p0[c], xx[c], part)
        chains.append(ch)
    h = ctx.hamiltonian()
    for c in range(B):
        assert abs(h[c, 0] - chains[c].hamiltonian()) <= 1e-10 * max(1.0, abs(h[c, 0]))
    out = []
    dts = np.broadcast_to(np.asarray(dts, dtype=np.float64), (B,))
    step_kw = step_kw or {}
    okw = {{"max_iters": "max_iters", "reverse_check_tol": "rev_tol", "constraint_tol": "ctol", "position_tol": "ptol",
            "divergence_tol": "dtol"}[k]: v for k, v in step_kw.items()}
    for _ in range(n_steps):
        res = ctx.leapfrog_step(dts, newton=newton, n_inner_step=n_inner, **step_kw)
        q1, p1, _, _ = ctx.get_state()
        h1 = ctx.hamiltonian()
        for c in range(B):
            st, itf, itb, rev = chains[c].step(dts[c], newton=newton, n_inner=n_inner, **okw)
            qo, po, _, _ = chains[c].get()
            assert res["status"][c] == st, (c, res["status"][c], st)
            assert res["iters_fwd"][c] == itf and (st != 0 or res["iters_bwd"][c] == itb), (c, res, itf, itb)
            sq, sp = max(1.0, np.abs(qo).max()), max(1.0, np.abs(po).max())
            assert np.abs(q1[c] - qo).max() <= tol * sq, (c, np.abs(q1[c] - qo).max())
            assert np.abs(p1[c] - po).max() <= tol * sp, (c, np.abs(p1[c] - po).max())
            assert abs(h1[c, 0] - chains[c].hamiltonian()) <= 1e-9 * max(1.0, abs(h1[c, 0]))
            out.append((st, itf, itb))
    return out


def random_metric(rng, n=4):
    a = rng.standard_normal((n, n))
    return a @ a.T / n + 0.5 * np.eye(n)


def check_block_metric_against_oracle(ctx, case, newton, dts, n_steps=2, tol=1e-9):
    """metric = blockdiag(M_0, I) (sde/mici_extensions.py:279-315): per-op entry points, the retraction's multiplier
    output, momentum sampling and fused leapfrog steps against the C oracle with the same M_0."""
    from test_rng import reference_normals
    osys, rng, B = case["osys"], case["rng"], case["B"]
    U = ctx.U
    M0 = random_metric(rng, U)
    osys.set_metric(M0)
    try:
        ctx.set_metric(M0)
        worst = check_ops_against_oracle(ctx, case)  # Woodbury cores, log-det (- log det M_0 / 2), gradient, normal space
        # projection from a flowed point: position, multiplier term mu = M dq / dt, iteration counts
        q0, x0 = case["q"][0], case["x_obs"][0]
        qq, xx = np.repeat(q0[None], B, 0), np.repeat(x0[None], B, 0)
        ctx.set_state(qq, None, xx, 0)
        mv = 0.03 * rng.standard_normal((B, ctx.Q))
        mv[:, :U] = mv[:, :U] @ np.linalg.inv(M0).T
        dt = np.full(B, 0.05)
        r = ctx.project(qq + mv, dt, newton=newton)
        for c in range(B):
            st, q1, mu, it, ndq, err = osys.project(newton, q0, qq[c] + mv[c], x0, 0, 0.05)
            assert st == r["status"][c] == 0 and it == r["iters"][c]
            np.testing.assert_allclose(r["q"][c], q1, rtol=0, atol=tol * max(1.0, np.abs(q1).max()))
            np.testing.assert_allclose(r["mu"][c], mu, rtol=0, atol=1e-8 * max(1.0, np.abs(mu).max()))
        # sample_momentum: metric.sqrt @ n, projected with J M^-1
        ctx.sample_momentum(77, 2, 1)
        _, p, _, _ = ctx.get_state()
        Lc = np.linalg.cholesky(M0)
        for c in range(B):
            n = reference_normals(ctx.Q, c + 1, 77, 2)
            n[:U] = Lc @ n[:U]
            expect = n - osys.jacob_products(q0, x0, 0, n, np.zeros(ctx.dim_c))[3]
            np.testing.assert_allclose(p[c], expect, rtol=1e-9, atol=1e-10)
        # fused steps (tangent momenta: projected-kick shortcut; then from unprojected momenta)
        for part in range(ctx.num_partition):
            check_steps_against_oracle(ctx, case, dts, newton=newton, n_steps=n_steps, tol=tol, part=part)
        check_steps_against_oracle(ctx, case, dts, newton=newton, n_steps=1, tol=tol, project=False)
        # back to the identity: same results as a context that never had a metric
        ctx.set_metric(None)
    finally:
        osys.set_metric(None)
    check_ops_against_oracle(ctx, case)
    return worst


def check_tree_leaf(ctx, case, device, with_metric):
    """chmc_tree_leaf (fused per-leaf bookkeeping of the batched no-U-turn trees) against plain numpy on the same
    buffers: momentum sum, proposal update, checkpoint store and the criterion values of the checked spans."""
    import torch
    rng, B, Q = case["rng"], ctx.B, ctx.Q
    D = 4
    M0 = random_metric(rng) if with_metric else None
    ctx.set_metric(M0)
    p = rng.standard_normal((B, Q))
    ctx.set_state(case["q"], p, case["x_obs"], 0)
    q0, p0, _, _ = ctx.get_state()
    t = lambda a: torch.from_numpy(np.array(a, copy=True)).to(device)  # noqa: E731  (a copy: on the CPU the tensor would alias `a`)
    sub_prop = rng.standard_normal((B, Q))
    sub_sum = rng.standard_normal((B, Q))
    ck_p, ck_sum, ck_end = (rng.standard_normal((D, B, Q)) for _ in range(3))
    run = (np.arange(B) % 3 != 1).astype(np.int32)
    take = (np.arange(B) % 2 == 0).astype(np.int32) & run
    W = np.eye(Q)
    if with_metric:
        W[:4, :4] = np.linalg.inv(M0)
    dot = lambda a, rho: ((a @ W.T) * rho).sum(1) * run  # noqa: E731  dh_dmom(a) . rho

    def expect(store, lo, n, extra):
        S = sub_sum + p0 * run[:, None]
        prop = np.where((take == 1)[:, None], q0, sub_prop)
        cp, cs, ce = ck_p.copy(), ck_sum.copy(), ck_end.copy()
        if store >= 0:
            cp[store] = np.where((run == 1)[:, None], p0, cp[store])
            cs[store] = np.where((run == 1)[:, None], S, cs[store])
        crit = np.zeros((B, n, 6))
        for k in range(n):
            a, csa = ck_p[lo + k], ck_sum[lo + k]
            span = S - csa + a
            crit[:, k, 0], crit[:, k, 1] = dot(a, span), dot(p0, span)
            if extra and k < n - 1:  # the span of slot lo + k + 1 is the right half
                ar, csr, pm = ck_p[lo + k + 1], ck_sum[lo + k + 1], ck_end[lo + k]
                rho1 = csr - csa + a          # momenta of the left half + first momentum of the right half
                rho2 = S - csr + ar + pm      # momenta of the right half + last momentum of the left half
                crit[:, k, 2], crit[:, k, 3] = dot(a, rho1), dot(ar, rho1)
                crit[:, k, 4], crit[:, k, 5] = dot(pm, rho2), dot(p0, rho2)
        if extra and n > 0:
            ce[lo] = np.where((run == 1)[:, None], p0, ce[lo])
        return S, prop, cp, cs, ce, crit

    for store, lo, n, extra in ((2, 0, 0, True), (-1, 1, 3, True), (-1, 0, 1, True), (-1, 0, 4, True), (-1, 1, 3, False)):
        d_prop, d_sum, d_cp, d_cs, d_ce = t(sub_prop), t(sub_sum), t(ck_p), t(ck_sum), t(ck_end)
        if device != "cpu":
            torch.cuda.synchronize()
        crit = ctx.tree_leaf(run, take, d_prop.data_ptr(), d_sum.data_ptr(), d_cp.data_ptr(), d_cs.data_ptr(), store, lo, n,
                             ck_end_ptr=d_ce.data_ptr() if extra else None)
        S, prop, cp, cs, ce, ecrit = expect(store, lo, n, extra)
        np.testing.assert_allclose(d_sum.cpu().numpy(), S, rtol=0, atol=1e-14)
        np.testing.assert_array_equal(d_prop.cpu().numpy(), prop)
        np.testing.assert_array_equal(d_cp.cpu().numpy(), cp)
        np.testing.assert_array_equal(d_ce.cpu().numpy(), ce)
        np.testing.assert_allclose(d_cs.cpu().numpy(), cs, rtol=0, atol=1e-14)
        np.testing.assert_allclose(crit, ecrit, rtol=1e-11, atol=1e-9)
    ctx.set_metric(None)


def _half_batch_inputs(case, masked, failing):
    """One start point for every chain, momenta and step sizes of mixed sign per chain; `failing` chains get a step size
    no retraction survives, `masked` ones are inactive."""
    B = case["B"]
    rng = np.random.default_rng(99)
    p = rng.standard_normal(case["q"].shape)
    qq = np.repeat(case["q"][:1], B, 0)
    xx = np.repeat(case["x_obs"][:1], B, 0)
    dts = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 + 0.06 * rng.random(B))
    dts[list(failing)] = 5.0
    act = np.ones(B, dtype=np.int32)
    act[list(masked)] = 0
    return qq, p, xx, dts, act


def rounds_follow_from_iteration_counts(case, monkeypatch, part=0, newton=True, n_steps=3, cap=12):
    """The lock-step Newton loop (run_lockstep, csrc/chmc_api.inc) enqueues rounds by a fixed protocol, so while no loop
    predicts -- a fresh context and at most 3 steps: proj_stable < 3 -- the rounds of a step follow from its iteration counts.
    A problem is the batch (CHMC_HALVES=1) or one of the chain ranges [0, B // 2), [B // 2, B) (CHMC_HALVES=2); with m its
    largest iteration count in a retraction and `cap` = max_iters it has work in `cap if m >= cap else max(m, 2)` rounds (the
    first count the host looks at is round 1's) and is enqueued for one speculative round more, up to the cap:
      newton_rounds (enqueued, per problem) grows by the sum over both retractions and their problems of the second figure,
      projection_iterations (rounds with work, once per batch) by the sum over both retractions of the largest first figure.
    Inputs of halves_vs_single_batch with chain 1 masked in the first step and chain 2 failing.  Prints each figure before
    it asserts; returns the number of (step, mode) pairs checked."""
    B = case["B"]
    qq, p, xx, dts, act = _half_batch_inputs(case, masked=(1,), failing=(2,))
    checked = 0
    for halves in ("1", "2"):
        monkeypatch.setenv("CHMC_HALVES", halves)
        ctx = make_ctx(case)
        ctx.set_state(qq, p, xx, part)
        problems = [slice(0, B)] if halves == "1" else [slice(0, B // 2), slice(B // 2, B)]
        for k in range(n_steps):
            d0, c0 = ctx.diagnostics()["newton_rounds"], ctx.counters()["projection_iterations"]
            r = ctx.leapfrog_step(dts, active=act if k == 0 else None, newton=newton, max_iters=cap)
            enqueued = ctx.diagnostics()["newton_rounds"] - d0
            counted = ctx.counters()["projection_iterations"] - c0
            want_enqueued = want_counted = 0
            for iters in (r["iters_fwd"], r["iters_bwd"]):
                ms = [int(iters[s].max()) for s in problems]
                worked = [cap if m >= cap else max(m, 2) for m in ms]
                want_enqueued += sum(min(w + 1, cap) for w in worked)
                want_counted += max(worked)
            print(f"  halves={halves} part={part} step={k} fwd={r['iters_fwd'].tolist()} bwd={r['iters_bwd'].tolist()}: "
                  f"enqueued {enqueued} (expected {want_enqueued}), counted {counted} (expected {want_counted})")
            assert enqueued == want_enqueued and counted == want_counted, (halves, part, k)
            checked += 1
        assert r["status"][2] > 0
        ctx.close()
    return checked


def halves_vs_single_batch(case, monkeypatch, part=0, n_steps=2, newton=True, masked=(), failing=()):
    """The same leapfrog steps with the step run as ONE batch (CHMC_HALVES=1) and as two overlapped half-batches on two
    streams (CHMC_HALVES=2).  Chains are independent and every per-chain reduction has a fixed order, so the two runs
    must agree BITWISE: positions, momenta, statuses, iteration counts, reverse-check distances."""
    qq, p, xx, dts, act = _half_batch_inputs(case, masked, failing)
    out = []
    for halves in ("1", "2"):
        monkeypatch.setenv("CHMC_HALVES", halves)
        ctx = make_ctx(case)
        ctx.set_state(qq, p, xx, part)
        res = []
        for k in range(n_steps):  # first step from unprojected momenta (full projection path), then the shortcut
            res.append(ctx.leapfrog_step(dts, active=act if k == 0 else None, newton=newton, max_iters=12))
        q1, p1, _, _ = ctx.get_state()
        out.append((q1, p1, res, ctx.hamiltonian()))
        ctx.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for ra, rb in zip(a[2], b[2]):
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
    assert (a[2][0]["status"][list(masked)] == -1).all() and (a[2][0]["status"][list(failing)] > 0).all()
    return a


def check_late_inner_failure(ctx, case, dts, n_inner=2):
    """A chain whose step fails in a LATER inner h2-flow step (n_inner_step > 1) has already moved to an intermediate
    point: the library must hand back the step's start state with valid caches.  The failure is provoked with a
    reverse_check_tol between the round-off distances of the first and of the last inner step (both measured with
    the library itself, whose round-off differs from the oracle's in the last bits)."""
    osys, B = case["osys"], case["B"]
    rng = case["rng"]
    qq = np.repeat(case["q"][:1], B, 0)
    xx = np.repeat(case["x_obs"][:1], B, 0)
    p_raw = rng.standard_normal((B, ctx.Q))
    dts = np.broadcast_to(np.asarray(dts, dtype=np.float64), (B,))

    def reset():
        ctx.set_state(qq, p_raw, xx, 0)
        ctx.project_onto_cotangent_space()
        return ctx.get_state()[:2]

    reset()
    rd_first = ctx.leapfrog_step(dts / n_inner, reverse_check_tol=1.0)["rev_err"]
    reset()
    rd_last = ctx.leapfrog_step(dts, n_inner_step=n_inner, reverse_check_tol=1.0)["rev_err"]
    ratio = rd_last / np.maximum(rd_first, 1e-300)
    c_late = int(np.argmax(ratio))
    if not ratio[c_late] > 1.5:
        return None  # no chain with a clearly larger round-off in the last inner step: the caller tries another case
    tol = float(np.sqrt(rd_first[c_late] * rd_last[c_late]))  # inner step 1 passes, the last one fails for c_late
    q0, p0 = reset()
    res = ctx.leapfrog_step(dts, n_inner_step=n_inner, reverse_check_tol=tol)
    q1, p1, _, _ = ctx.get_state()
    assert res["status"][c_late] == 3 and rd_first[c_late] <= tol < res["rev_err"][c_late]
    failed = res["status"] > 0
    assert np.array_equal(q1[failed], q0[failed]) and np.array_equal(p1[failed], p0[failed])
    # every chain (moved or restored) has valid caches: the next ordinary step agrees with an oracle chain started from
    # the state the library reports
    res = ctx.leapfrog_step(dts, n_inner_step=n_inner)
    q2, p2, _, _ = ctx.get_state()
    for c in range(B):
        ch = c_oracle.OracleChain(osys)
        ch.set(q1[c], p1[c], xx[c], 0)
        st, itf, itb, _ = ch.step(dts[c], n_inner=n_inner)
        qo, po, _, _ = ch.get()
        assert res["status"][c] == st == 0 and res["iters_fwd"][c] == itf and res["iters_bwd"][c] == itb
        assert np.abs(q2[c] - qo).max() <= 1e-9 * max(1.0, np.abs(qo).max())
        assert np.abs(p2[c] - po).max() <= 1e-8 * max(1.0, np.abs(po).max())
    return c_late


_SOLVER_TO_ORACLE = {"max_iters": "max_iters", "reverse_check_tol": "rev_tol", "constraint_tol": "ctol", "position_tol": "ptol",
                     "divergence_tol": "dtol", "newton": "newton", "n_inner_step": "n_inner"}


def oracle_static_transition(osys, q, x_obs, part, c, seed, draw, M0, dt, length, u_accept, solver=None):
    """One transition of sampling.sample_static_chmc for ONE chain with the oracle alone: the keyed momentum of global chain
    `c` and draw `draw` (test_hip_tree_oracle.oracle_momentum), h0, up to `length` OracleChain.step calls of step size `dt`
    that stop at the first non-zero status, and the acceptance probability and decision as the sampler writes them: prob =
    exp(min(0, -dh)) for a complete trajectory with a finite dh = h1 - h0, else 0; accept = u_accept < prob.  `osys` carries
    the metric M0 (None: identity); `solver` is the sampler's dict.

    Returns a dict: `q` (the end point if accepted, else the start), `q_end` (where the trajectory ended), `accepted`, `prob`,
    `status` (0, or the failing step's code), `n_done`, `iters_fwd` / `iters_bwd` (summed over the steps, the failing one
    included), `dh` (None unless the trajectory is complete) and `margins`, the smallest margin of every kind of decision:
      accept                        |u_accept - prob| of a complete trajectory (a failed one is rejected whatever the draw)
      finite_dh                     0 for a complete trajectory whose dh is not finite (never admitted), else absent
      constraint_tol, position_tol  relative distance of every retraction residual (OracleChain.trace: every iteration of
                                    both retractions of the last inner step of every step) from its tolerance
      reverse_check                 relative distance of every step's reversibility error from reverse_check_tol."""
    from oracle import c_oracle as co
    from test_hip_tree_oracle import oracle_momentum
    had = getattr(osys, "M0", None)
    assert (M0 is None) == (had is None) and (M0 is None or np.array_equal(had, M0)), "osys must carry the metric M0"
    solver = dict(solver or {})
    okw = {_SOLVER_TO_ORACLE[k]: v for k, v in solver.items()}
    ctol, ptol, rtol = okw.get("ctol", 1e-9), okw.get("ptol", 1e-8), okw.get("rev_tol", 2e-8)
    margins = {}

    def note(kind, v):
        if v == v:  # (a residual that is NaN is on no side of a tolerance)
            margins[kind] = min(margins.get(kind, np.inf), float(v))

    ch = co.OracleChain(osys)
    ch.set(q, oracle_momentum(osys, q, x_obs, part, c, seed, draw, M0), x_obs, part)
    h0 = ch.hamiltonian()
    status, n_done, itf, itb = 0, 0, 0, 0
    for _ in range(int(length)):
        status, f, b, rev = ch.step(float(dt), **okw)
        itf, itb = itf + f, itb + b
        for direction in (0, 1):
            err, ndq = ch.trace(direction)
            for e, n in zip(err, ndq):
                note("constraint_tol", abs(e - ctol) / ctol), note("position_tol", abs(n - ptol) / ptol)
        if status in (0, 3):
            note("reverse_check", abs(rev - rtol) / rtol)
        if status != 0:
            break
        n_done += 1
    dh, prob = None, 0.0
    if status == 0:
        dh = ch.hamiltonian() - h0
        if np.isfinite(dh):
            prob = float(np.exp(min(0.0, -dh)))
        else:
            margins["finite_dh"] = 0.0
        note("accept", abs(u_accept - prob))
    accepted = bool(u_accept < prob)
    q_end = ch.get()[0]
    return dict(q=q_end if accepted else np.array(q, copy=True), q_end=q_end, accepted=accepted, prob=prob, status=status,
                n_done=n_done, iters_fwd=itf, iters_bwd=itb, dh=dh, h0=h0, margins=margins)


def oracle_tree_transition(osys, q, p, x_obs, part, draw, eps, depth, max_delta_h, solver=None, W=None, extra=True):
    """One dynamic (no-U-turn, multinomial) transition of ONE chain, every leaf an OracleChain.step and every Hamiltonian an
    OracleChain.hamiltonian(): tests/test_dynamic.py::_reference_transition without the library.  `draw(kind, depth, leaf)`
    hands out the chain's keyed uniforms (dynamic.TreeUniforms), `solver` is DynamicTransition's dict (its n_inner_step is
    the oracle's n_inner), `W` the inverse of the block metric M_0 (None: identity), applied to the oracle with
    osys.set_metric for the duration of the call unless osys already carries that metric.

    Returns a dict: `q` the selected position, `n_step`, `sum_acc` = sum of min(1, exp(h0 - h)) over the leaves, `depth`
    (doublings completed), `moved`, `logw` (the tree's log weight), `offset` (signed leaf index of the selected position
    along the trajectory, 0 = the start), `event` -- what ended the tree: ("subtree",) a span criterion inside the new
    sub-tree, ("extra",) one of the additional sub-tree checks while every plain span criterion of that leaf passed,
    ("tree",) the whole-tree criterion, ("max_depth",), ("error", status, leaves taken before, doubling, leaf in it),
    ("diverged", leaves taken before, doubling, leaf in it) --, `dirs` (direction per doubling, True = forward),
    `edge_switches` (doublings that extend the tree from the edge the state is not sitting on), `leaves` (every
    (doubling, leaf) the integrator was run for), `dh` (h - h0 of every leaf that was integrated without error), `ck_end`
    (checkpoint slot: (momentum, leaves from the start) that the additional checks' buffer holds after the transition) and
    `margins`, the smallest margin of every kind of decision taken:
      direction / leaf / accept   |u - probability| of the draws
      criterion                   |value| / (|dh_dmom(edge)|_2 |rho|_2) of every criterion value
      delta_h                     |dh - max_delta_h| / max(1, |max_delta_h|)
      constraint_tol, position_tol  relative distance of every retraction residual (OracleChain.trace: every iteration of
                                  both retractions of the last inner step of every leaf) from its tolerance
      reverse_check               relative distance of the step's reversibility error from reverse_check_tol."""
    from oracle import c_oracle as co
    from manifold_mcmc_for_diffusions_amd.dynamic import _ckpt_range
    solver = dict(solver or {})
    okw = {_SOLVER_TO_ORACLE[k]: v for k, v in solver.items()}
    ctol, ptol, rtol = okw.get("ctol", 1e-9), okw.get("ptol", 1e-8), okw.get("rev_tol", 2e-8)
    margins = {}

    def note(kind, v):
        if v == v:  # (a residual that is NaN is on no side of a tolerance)
            margins[kind] = min(margins.get(kind, np.inf), float(v))

    def vel(pp):  # dh_dmom = metric.inv @ mom
        if W is None:
            return pp
        v = pp.copy()
        v[:W.shape[0]] = W @ pp[:W.shape[0]]
        return v

    def crit(edge, rho):
        v = vel(edge)
        val = float(v @ rho)
        note("criterion", abs(val) / (np.linalg.norm(v) * np.linalg.norm(rho)))
        return val < 0

    had = getattr(osys, "M0", None)
    if W is not None and not (had is not None and np.allclose(np.linalg.inv(had), W, rtol=1e-13, atol=0)):
        osys.set_metric(np.linalg.inv(W))
    elif W is None and had is not None:
        osys.set_metric(None)
    try:
        neg, pos = co.OracleChain(osys), co.OracleChain(osys)
        neg.set(q, p, x_obs, part), pos.set(q, p, x_obs, part)
        h0 = pos.hamiltonian()
        out = dict(q=np.array(q, copy=True), n_step=0, sum_acc=0.0, depth=0, moved=False, logw=-h0, offset=0, event=("max_depth",),
                   dirs=[], edge_switches=[], leaves=[], dh=[], margins=margins, h0=h0, ck_end={})
        sum_mom = np.array(p, copy=True)
        p_neg, p_pos = sum_mom.copy(), sum_mom.copy()
        n_neg = n_pos = 0   # leaves on either side of the start
        at_neg = at_pos = True
        for d in range(depth):
            u = draw(0, d, 0)
            note("direction", abs(u - 0.5))
            fwd = bool(u < 0.5)
            out["dirs"].append(fwd)
            if not (at_pos if fwd else at_neg):
                out["edge_switches"].append(d)
            at_pos, at_neg = fwd, not fwd
            ch = pos if fwd else neg
            leaves, sub_logw, sub_prop, sub_off = [], -np.inf, None, 0
            ended = None
            for k in range(1 << d):
                out["leaves"].append((d, k))
                st, _, _, rev = ch.step((1.0 if fwd else -1.0) * eps, **okw)
                for direction in (0, 1):
                    err, ndq = ch.trace(direction)
                    for e, n in zip(err, ndq):
                        note("constraint_tol", abs(e - ctol) / ctol), note("position_tol", abs(n - ptol) / ptol)
                if st in (0, 3):
                    note("reverse_check", abs(rev - rtol) / rtol)
                if st != 0:
                    ended = ("error", st, out["n_step"], d, k)
                    break
                h = ch.hamiltonian()
                out["dh"].append(h - h0)
                note("delta_h", abs(h - h0 - max_delta_h) / max(1.0, abs(max_delta_h)))
                if not (h - h0 <= max_delta_h):
                    ended = ("diverged", out["n_step"], d, k)
                    break
                q2, p2, _, _ = ch.get()
                out["n_step"] += 1
                out["sum_acc"] += min(1.0, np.exp(min(0.0, h0 - h)))
                off = (n_pos + k + 1) if fwd else -(n_neg + k + 1)
                leaves.append(p2)
                new = np.logaddexp(sub_logw, -h)
                prob = np.exp(-h - new)
                u = draw(2, d, k)
                note("leaf", abs(u - prob))
                if u < prob:
                    sub_prop, sub_off = q2, off
                sub_logw = new
                if extra and k % 2 == 1:  # KTreeLeaf / KTreeLeafFinish: the last leaf of the left half of the next larger span
                    out["ck_end"][_ckpt_range(k)[0]] = (p2, abs(off))
                plain = more = False
                j = 1
                while (k + 1) % (1 << j) == 0 and j <= d:  # aligned spans of 2^j leaves that end at this leaf
                    a = k + 1 - (1 << j)
                    span = np.sum(leaves[a:k + 1], axis=0)
                    plain |= crit(leaves[a], span) | crit(leaves[k], span)
                    if extra and j >= 2:  # the additional checks across the two halves of the span
                        m = a + (1 << (j - 1)) - 1
                        rho1 = np.sum(leaves[a:m + 1], axis=0) + leaves[m + 1]
                        rho2 = np.sum(leaves[m + 1:k + 1], axis=0) + leaves[m]
                        more |= crit(leaves[a], rho1) | crit(leaves[m + 1], rho1)
                        more |= crit(leaves[m], rho2) | crit(leaves[k], rho2)
                    j += 1
                if plain or more:
                    ended = ("subtree",) if plain else ("extra",)
                    break
            if ended:
                out["event"] = ended
                break
            prob = np.exp(min(0.0, sub_logw - out["logw"]))
            u = draw(1, d, 0)
            note("accept", abs(u - prob))
            if u < prob:
                out["q"], out["offset"], out["moved"] = sub_prop, sub_off, True
            out["logw"] = float(np.logaddexp(out["logw"], sub_logw))
            out["depth"] = d + 1
            sum_mom = sum_mom + np.sum(leaves, axis=0)
            if fwd:
                p_pos, n_pos = leaves[-1], n_pos + (1 << d)
            else:
                p_neg, n_neg = leaves[-1], n_neg + (1 << d)
            if crit(p_neg, sum_mom) | crit(p_pos, sum_mom):
                out["event"] = ("tree",)
                break
        return out
    finally:
        if getattr(osys, "M0", None) is not had:
            osys.set_metric(had)
