"""The HIP library against the AUTODIFF oracle (oracle/py) on the kernel families the golden files do not reach: the
16-row family (SIR, a block of more than 8 rows), the forward-scan kernel (steps per observation S % 8 == 0), the
M_0 != I branches, n_inner_step > 1, unprojected start momenta, many DISTINCT chains (partial wavefronts, several
workgroups) and the BASELINE sizes.  The C oracle that judges the other GPU tests shares its generated model code with
the device; the autodiff oracle shares nothing with it (tests/autodiff_checks.py).

Every case is built once (`plan`) and used twice:
  * test_references_agree (CPU): C oracle vs autodiff oracle on the very inputs of the GPU test, operators and steps to
    1e-10 relative (a tenth of the GPU bound), equal iteration counts, status 0, and no retraction residual within 1e-2
    (relative) of its tolerance -- so that "equal counts" is a fair demand on the library;
  * the gpu tests: library vs autodiff oracle, operators 1e-9, q 1e-9, p 1e-8, Hamiltonian 1e-9 (the figures of
    tests/test_golden.py), statuses and both iteration counts equal, no edge allowance.

Seeds / step sizes: every step case below passes the edge condition with the seeds written here and no chain is dropped.
Seeds that were replaced: fhn_noisy_s16 106 -> 206 (chain 64, quasi-Newton: reverse |c| 9.92e-10 at the stop) and
metric_fhn_nb_6_4_2 125 -> 425 (125: chain 2, quasi-Newton, forward |c| 9.93e-10; 225 and 325: a chain whose
step does not succeed in either oracle); sir_two_16row_blocks 105 -> 205 (seed 105
puts a perturbed state where a 16-row Gram block is numerically singular: the autodiff oracle's Cholesky refuses it);
fhn_k65_rm7 111 -> 211 (chain 2, quasi-Newton: reverse |c| 9.96e-10 at the stop); sir16_k5_6_rows9 115 -> 215 (115: as 105, a
perturbed state whose Gram block the autodiff oracle's Cholesky refuses).  sir_two_16row_blocks has had its Newton and
quasi-Newton steps since the reference step was seen to succeed at its 0.1 between observations.  fhn_k65_rm7 is the 325-observation
layout (K = [65, 66], 7 row slots), not the smaller stand-in: its test_references_agree case takes 60 to 100 s here on
16 threads.

Wall time of this module on the MI355X host: 111 s for the gpu tests (full-size SIR 42 s, full-size FHN 23 s; the whole
`-m gpu` run 266 s); test_references_agree took about 170 s on the CPU before the four layout-edge cases and takes 330 s with them.  Measured distances: tests/golden/README.md."""
import numpy as np
import pytest
import autodiff_checks as ac
from helpers import make_case, make_ctx, random_metric
from test_emu_logic import emu_lib  # noqa: F401

REF_TOL = 1e-10  # reference vs reference: a tenth of the tightest GPU bound
EDGE = 1e-2


def distinct_on_manifold_chains(model, T, S, R, B, seed, obs_interval=None, var_sigma=False, gaussian=False):
    """test_hip_parity._distinct_on_manifold_chains, also for variable observation noise (sigma_c = exp(u_c[dim_z]))."""
    from manifold_mcmc_for_diffusions_amd import example_models as em
    case = make_case(model, T, S, R, True, B=B, seed=seed, obs_interval=obs_interval, var_sigma=var_sigma, gaussian=gaussian)
    m, q, xo, y = em.MODELS[model], case["q"], case["x_obs"], case["y"]
    sigma = np.exp(q[:, m.dim_z])[:, None] if var_sigma else case["sigma"]
    q[:, -T:] = (y[None, :] - m.obs_func(xo)[..., 0]) / sigma
    return case


def spread_chains_by_stepping(ctx, case, part, rng, n_pre=2):
    """test_hip_parity._spread_chains_by_stepping (noiseless data: distinct on-manifold states reached with the library;
    they are then the common INPUT of the library and of both oracles)."""
    B = case["B"]
    ctx.set_state(np.repeat(case["q"][:1], B, 0), rng.standard_normal((B, ctx.Q)), np.repeat(case["x_obs"][:1], B, 0), part)
    ctx.project_onto_cotangent_space()
    pre = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.03 + 0.05 * rng.random(B))
    for _ in range(n_pre):
        r = ctx.leapfrog_step(pre)
        assert (r["status"] == 0).mean() > 0.9
    q, _, xo, _ = ctx.get_state()
    assert np.abs(q - q[:1]).max(1).min(initial=np.inf, where=np.arange(B) > 0) > 1e-3
    return q, xo


# name: model, T, S, R, noisy, gaussian, var_sigma, B, chains, step variants (newton, n_inner, project), seed, h
NQ = [(True, 1, True), (False, 1, True)]
SIR16_STEPS = [(True, 1, True), (False, 1, True), (True, 2, True), (False, 2, True)]
C37, C70, C5 = [0, 1, 17, 31, 33, 36], [0, 1, 31, 63, 64, 69], [0, 1, 2, 3, 4]
MID = {
    "sir16_s8": ("sir", 14, 8, 14, True, False, False, 37, C37, SIR16_STEPS, 101, 0.02),
    "sir16_s16": ("sir", 14, 16, 14, True, False, False, 37, C37, SIR16_STEPS, 102, 0.02),
    "sir16_s8_varsigma": ("sir", 14, 8, 14, True, False, True, 37, C37, SIR16_STEPS, 103, 0.02),
    "sir16_s16_varsigma": ("sir", 14, 16, 14, True, False, True, 37, C37, SIR16_STEPS, 204, 0.02),
    "sir_two_16row_blocks": ("sir", 26, 24, 13, True, False, False, 5, [0, 2, 4], NQ, 205, 0.02),
    # 16 row slots with several blocks per chain (tests/test_hip_multiblock16.py), every chain judged: K = [4, 5] (the interval-
    # parallel and the stored-rows state evaluation in one context) and K = [5, 6] with 9 rows in 16 slots
    "sir16_k4_5": ("sir", 40, 8, 10, True, False, False, 5, C5, NQ, 114, 0.02),
    "sir16_k5_6_rows9": ("sir", 30, 8, 6, True, False, False, 5, C5, NQ, 215, 0.02),
    "fhn_noisy_s16": ("fhn", 12, 16, 5, True, False, False, 70, C70, NQ + [(True, 1, False)], 206, 0.05),
    "fhn_noiseless_gauss_s8": ("fhn", 7, 8, 3, False, True, False, 70, C70, NQ, 107, 0.05),
    "fhn_nb_noiseless_gauss_s8": ("fhn_nb", 7, 8, 3, False, True, False, 70, C70, NQ, 108, 0.05),
    "fhn_noisy_s40": ("fhn", 20, 40, 5, True, False, False, 70, C70, NQ, 109, 0.05),
    # the layout edges of tests/test_hip_layout_edges.py, every chain judged: 64 | 65 blocks per chain (the fused and the
    # unfused Newton round in one context), 65 | 66 blocks of 7 row slots, S = 64 (a full last tile), 16 rows with S = 65
    "fhn_k64_65": ("fhn", 128, 4, 2, True, False, False, 5, C5, NQ, 110, 0.05),
    "fhn_k65_rm7": ("fhn", 325, 8, 5, True, False, False, 5, C5, NQ, 211, 0.05),
    "fhn_s64": ("fhn", 4, 64, 2, True, False, False, 5, C5, NQ, 112, 0.05),
    "sir16_s65": ("sir", 14, 65, 14, True, False, False, 5, C5, NQ, 113, 0.02),
}
# M_0 != I: the parameter list of test_hip_parity.test_block_metric plus one 16-row case
METRIC = [("fhn", 6, 4, 2, True, 120), ("fhn", 12, 16, 5, True, 121), ("fhn", 7, 8, 3, False, 122), ("sir", 6, 8, 2, True, 123),
          ("sir", 14, 6, 14, True, 124), ("fhn_nb", 6, 4, 2, True, 425), ("sir", 14, 8, 14, True, 126)]
for _m, _T, _S, _R, _n, _seed in METRIC:
    MID[f"metric_{_m}_{_T}_{_S}_{_R}"] = (_m, _T, _S, _R, _n, False, False, 4, [0, 1, 2, 3], NQ, _seed, 0.02 if _m == "sir" else 0.05)
# BASELINE.json configs[3] at full size: 2 distinct chains, all operators and one Newton step each
FULL_SIR = ("sir", 14, 200, 14, True, False, False, 2, [0, 1], [(True, 1, True)], 141, 0.02)


INTERVALS = {"sir_two_16row_blocks": 0.1, "sir16_k4_5": 0.05, "sir16_k5_6_rows9": 0.05}  # time between observations, by name


def plan(name, cfg, ctx=None):
    """The inputs of one case: states for the operators (each chain its own OFF-manifold point), on-manifold states,
    raw momenta and step sizes for the steps.  Noiseless data need `ctx` (library) to spread the chains."""
    model, T, S, R, noisy, gaussian, var_sigma, B, chains, steps, seed, h = cfg
    # (SIR over 26 observations 0.25 apart: the prior draw's Gram matrix is so poorly conditioned that the two references
    # agree to 1e-9 only in inverse-Gram products; at 0.1 apart they agree to the bound asked of every other case)
    # (the layouts of tests/test_hip_multiblock16.py: 0.05 apart, as there)
    oi = INTERVALS.get(name, 0.25 if model == "sir" else None)
    rng = np.random.default_rng(seed)
    if noisy:
        case = distinct_on_manifold_chains(model, T, S, R, B, seed, obs_interval=oi, var_sigma=var_sigma)
        q_on, xo = case["q"], case["x_obs"]
    else:
        case = make_case(model, T, S, R, False, B=B, seed=seed, obs_interval=oi, gaussian=gaussian)
        q_on, xo = spread_chains_by_stepping(ctx, case, 0, rng)
    M_0 = random_metric(rng, 4) if name.startswith("metric") else None
    q_off = q_on + 0.01 * rng.standard_normal(q_on.shape)
    p_raw = rng.standard_normal(q_on.shape)
    if M_0 is not None:  # metric.sqrt @ n (sde/mici_extensions.py:1257)
        p_raw[:, :len(M_0)] = p_raw[:, :len(M_0)] @ np.linalg.cholesky(M_0).T
    dts = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.5 * h + h * rng.random(B))
    return dict(name=name, case=case, q_on=q_on, q_off=q_off, x_obs=xo, p_raw=p_raw, dts=dts, chains=chains, steps=steps,
                M_0=M_0, seed=seed)


def submit(pl, want=("grad", "products")):
    case = pl["case"]
    ops = ac.submit_ops(case, pl["chains"], pl["seed"] + 1000, M_0=pl["M_0"], q=pl["q_off"], x_obs=pl["x_obs"], want=want)
    steps = [ac.submit_steps(case, pl["q_on"], pl["p_raw"], pl["x_obs"], 0, pl["dts"], pl["chains"], newton=nw, n_inner=ni,
                             project=pr, M_0=pl["M_0"]) for nw, ni, pr in pl["steps"]]
    return ops, steps


def what(hs):
    return f"{'newton' if hs['newton'] else 'quasi-newton'} n_inner={hs['n_inner']} project={hs['project']}"


def library_side(ctx, pl, ops, steps):
    """library vs autodiff: all operators, then every step variant; returns the traj-kernel launches of the Newton,
    n_inner_step = 1, tangent-momentum steps."""
    if pl["M_0"] is not None:
        ctx.set_metric(pl["M_0"])
    print(f"\n{pl['name']}: Q={ctx.Q} B={ctx.B} RM={ctx.RM} K={ctx.K}")
    ac.check_ops(ctx, ops)
    traj = 0
    for hs in steps:
        d0 = ctx.diagnostics()["traj_kernel_launches"]
        ac.check_steps(ctx, hs, what=what(hs))
        if hs["newton"] and hs["n_inner"] == 1 and hs["project"]:
            traj += ctx.diagnostics()["traj_kernel_launches"] - d0
    return traj


def far_from_edge(err, ndq):
    return abs(err - 1e-9) > EDGE * 1e-9 and abs(ndq - 1e-8) > EDGE * 1e-8


def reference_side(pl, ops, steps):
    """C oracle vs autodiff oracle on the same inputs + the conditions that make equal iteration counts a fair demand."""
    from oracle import c_oracle
    case, osy = pl["case"], pl["case"]["osys"]
    osy.set_metric(pl["M_0"])
    worst = {}
    try:
        for part, d in ops["parts"].items():
            nrows = [osy.block_info(part, b)["nrows"] for b in range(osy.num_blocks(part))]
            for c, fut in d["futs"].items():
                q, xo = ops["q"][c], ops["x_obs"][c]
                ref = fut.result(timeout=900)
                cc, du, dv = osy.jacob_constr_blocks(q, xo, part)
                cC, cD, ld, grad = osy.gram_ops(q, xo, part)
                Jw, JTl, Gil, nsc = osy.jacob_products(q, xo, part, d["w"][c], d["lam"][c])
                ch = c_oracle.OracleChain(osy)
                ch.set(q, d["p"][c], xo, part)
                lib = {k: {c: v} for k, v in dict(c=cc, dc_du=du, dc_dv=dv, chol_C=cC, chol_D=cD, log_det=ld, grad=grad,
                                                 Jw=Jw, JTlam=JTl, Ginv_lam=Gil, nsc=nsc, h=ch.hamiltonian()).items()}
                ac.compare_ops(lib, ref, c, nrows, worst)
        print(f"\n{pl['name']}: C oracle vs autodiff, operators (rel):", {k: f"{v:.1e}" for k, v in worst.items()})
        bad = {k: v for k, v in worst.items() if not v < REF_TOL}
        assert not bad, (bad, worst)
        for hs in steps:
            ws = {}
            for c, fut in hs["futs"].items():
                ref = fut.result(timeout=900)
                assert ref["status"] == 0, (what(hs), c, ref)
                ch = c_oracle.OracleChain(osy)
                ch.set(hs["q"][c], hs["p"][c], hs["x_obs"][c], hs["part"])
                if hs["project"]:
                    ch.project_mom()
                _, p0, _, _ = ch.get()
                h0 = ch.hamiltonian()
                st, itf, itb, _ = ch.step(hs["dts"][c], n_inner=hs["n_inner"], newton=hs["newton"])
                q1, p1, _, _ = ch.get()
                assert (st, itf, itb) == (0,) + tuple(ref["iters"]), (what(hs), c, (st, itf, itb), ref["iters"])
                for fwd, bwd in ref["residuals"]:  # the (|c|, |dq|) each autodiff solver stopped at, every inner step
                    assert far_from_edge(*fwd) and far_from_edge(*bwd), (what(hs), c, ref["residuals"])
                for d in (0, 1):  # every iteration of the C oracle's last inner step
                    err, ndq = ch.trace(d)
                    assert all(far_from_edge(e, n) for e, n in zip(err, ndq)), (what(hs), c, d, err, ndq)
                for k, a, b in (("p0", p0, ref["p0"]), ("h0", [h0], [ref["h0"]]), ("q1", q1, ref["q1"]),
                                ("p1", p1, ref["p1"]), ("h1", [ch.hamiltonian()], [ref["h1"]])):
                    ws[k] = max(ws.get(k, 0.0), ac.rel(a, b))
            print(f"  C oracle vs autodiff, step {what(hs)} (rel):", {k: f"{v:.1e}" for k, v in ws.items()})
            assert all(v < REF_TOL for v in ws.values()), (what(hs), ws)
    finally:
        osy.set_metric(None)
    return worst


@pytest.mark.parametrize("name", list(MID))
def test_references_agree(emu_lib, name):  # noqa: F811  (the emulation build only spreads the noiseless chains)
    cfg = MID[name]
    ctx = None
    if not cfg[4]:
        ctx = make_ctx(make_case(*cfg[:4], False, B=cfg[7], seed=cfg[10], gaussian=cfg[5]))
    pl = plan(name, cfg, ctx)
    if ctx is not None:
        ctx.close()
    reference_side(pl, *submit(pl))


def _gpu_case(name, cfg, want=("grad", "products")):
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"
    noisy = cfg[4]
    if noisy:
        pl = plan(name, cfg)
        handles = submit(pl, want)  # the oracle works while the library runs
        ctx = make_ctx(pl["case"])
    else:
        ctx = make_ctx(make_case(*cfg[:4], False, B=cfg[7], seed=cfg[10], gaussian=cfg[5]))
        pl = plan(name, cfg, ctx)
        handles = submit(pl, want)
    traj = library_side(ctx, pl, *handles)
    return ctx, traj


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in MID if n.startswith("sir16_s")])
def test_sixteen_row_kernels(name):
    """SIR T = 14, R = 14 (one 16-row block per chain: k_traj_chain, k_retract_chain, k_fwd_par, k_newton_ivl /
    k_newton_comb_wg, state_factor16 / newton_factor16, k_gld_ivl_*), S = 8 and 16, fixed and variable sigma, 37 distinct
    chains of which 6 are judged (first, last, two past index 32): every operator; steps with Newton and quasi-Newton,
    n_inner_step 1 and 2, +dt and -dt.  sir16_s65: S = 65 (the 64-lane tile of an interval one lane over), 5 chains, all
    judged, n_inner_step 1."""
    ctx, traj = _gpu_case(name, MID[name])
    assert ctx.RM == 16 and ctx.K == [1]
    assert traj == 1  # k_traj_chain did the Newton, n_inner_step = 1 step
    ctx.close()


@pytest.mark.gpu
def test_two_sixteen_row_blocks_both_partitions():
    """SIR T = 26, R = 13, S = 24: two 16-row blocks per chain, both partitions, every operator, 3 chains; Newton and
    quasi-Newton steps in partition 0."""
    ctx, _ = _gpu_case("sir_two_16row_blocks", MID["sir_two_16row_blocks"])
    assert ctx.RM == 16 and ctx.num_partition == 2
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sir16_k4_5", "sir16_k5_6_rows9"])
def test_sixteen_row_blocks_several_per_chain(name):
    """SIR (40, 8, 10), K = [4, 5], and (30, 8, 6), K = [5, 6] (9 rows in 16 slots), 0.05 between observations: all 5 distinct
    chains, every operator in both partitions (interval-parallel state evaluation up to 4 blocks per chain, stored rows beyond),
    Newton and quasi-Newton steps in partition 0, judged by the oracle that shares no model code with the device."""
    ctx, traj = _gpu_case(name, MID[name])
    d = ctx.diagnostics()
    assert ctx.RM == 16 and ctx.K == {"sir16_k4_5": [4, 5], "sir16_k5_6_rows9": [5, 6]}[name]
    assert traj == 0 and d["retract_kernel_launches"] == 0 and d["gram_valu_launches"] > 0, d
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in MID if n.startswith("fhn") and not n.startswith("fhn_k")])
def test_forward_scan_kernel(name):
    """S % 8 == 0 (k_fwd_scan), 70 distinct chains (more than one wavefront of chains) of which 6 are judged: every
    operator in both partitions, steps with both solvers; fhn_noisy_s16 also from an unprojected momentum.  fhn_s64:
    S = 64 (the last tile of an interval exactly full), 5 chains, all judged."""
    ctx, _ = _gpu_case(name, MID[name])
    assert ctx.S % 8 == 0 and ctx.num_partition == 2
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in MID if n.startswith("fhn_k")])
def test_block_count_boundary(name):
    """64 | 65 and 65 | 66 blocks per chain (tests/test_hip_layout_edges.py) judged by the oracle that shares no model code:
    every operator in both partitions (past 64 blocks lmult_by_inv_gram and normal_space_component solve with
    KSolveChain), Newton and quasi-Newton steps in partition 0, all 5 distinct chains.  The launch counters say which
    Newton round ran: k_newton_fsm_wave (out80[68]) with 64 blocks, KNewtonFactor (out80[69]) with 65."""
    ctx, _ = _gpu_case(name, MID[name])
    d = ctx.diagnostics()
    print(f"  K={ctx.K}: out80[68] = {d['newton_fsm_launches']}, out80[69] = {d['newton_factor8_launches']}")
    assert ctx.K == {"fhn_k64_65": [64, 65], "fhn_k65_rm7": [65, 66]}[name]
    if ctx.K[0] <= 64:  # (the steps of a case run in partition 0)
        assert d["newton_fsm_launches"] > 0 and d["newton_factor8_launches"] == 0, d
    else:
        assert d["newton_fsm_launches"] == 0 and d["newton_factor8_launches"] > 0, d
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in MID if n.startswith("metric")])
def test_block_metric(name):
    """metric = blockdiag(M_0, I): every operator in every partition and steps with both solvers against the autodiff
    oracle's own M_0 branches (restated from sde/mici_extensions.py, not from the C oracle)."""
    ctx, _ = _gpu_case(name, MID[name])
    ctx.close()


@pytest.mark.gpu
def test_full_size_sir_configs3():
    """BASELINE.json configs[3] (SIR T = 14, S = 200, R = 14, Q = 8419): 2 distinct chains, every operator and one Newton
    step each."""
    ctx, traj = _gpu_case("full_size_sir", FULL_SIR)
    assert ctx.Q == 8419 and ctx.RM == 16 and ctx.K == [1] and traj == 1
    ctx.close()


@pytest.mark.gpu
def test_full_size_fhn_configs1():
    """BASELINE.json configs[1] (FHN T = 100, S = 400, R = 5, Q = 80106): chain 1 of 2 (not chain 0), both partitions:
    constr, Jacobian (both parts) and Jacobian-vector product, chol_C, every chol_D block, log_det, lmult_by_inv_gram.
    LEFT OUT at this size: the log-det gradient (its autodiff sweep had not finished after 5 minutes for one partition
    on 8 threads) and a leapfrog step (at least two such sweeps plus 6 Jacobians of 40 s each): neither fits the time
    limit of the gpu run."""
    cfg = ("fhn", 100, 400, 5, True, False, False, 2, [1], [], 142, 0.05)
    ctx, _ = _gpu_case("full_size_fhn", cfg, want=())
    assert ctx.Q == 80106 and ctx.C == [138, 140]
    ctx.close()
