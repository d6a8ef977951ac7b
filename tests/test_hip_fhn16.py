"""FitzHugh-Nagumo layouts with 9 to 16 constraint rows per block (num_obs_per_subseq up to 14 with noisy, 15 with noiseless
observations) against the C oracle: the 16-row kernel family of csrc/chmc_plan.h, which the SIR tests
(tests/test_hip_multiblock16.py) only ever ran with three state components and three noise increments per step, instantiated
for FhnModel, FhnVsModel and FhnNbModel:

  * X = V = 2 in every 16-row kernel (k_rev_wave_ldsrows, k_gram_rows, k_gram_rows_mfma<16>, k_newton_comb,
    k_newton_factor_wave, k_newton_comb_wg, k_gld_ivl_*, k_gld_fwd_wave<compact> + k_gld_bwd_wave_ldsrows, k_jw_pb_wg);
  * noiseless observations with 16 row slots: a non-final block has nobs - 1 observation rows and then X state rows;
  * U = Z + 1 (FhnVsModel) with 16 row slots, and the notebook's parametrisation (FhnNbModel);
  * short, many 16-row blocks (K up to 7 blocks of 40 to 80 steps), all 16 rows in use (14 + 2), one block per chain (the
    batched _wg path with the time-parallel scan: the per-chain kernels k_retract_chain / k_traj_chain are SIR-only and
    must never run, whatever CHMC_RETRACT_KERNEL says), and blocks of 1040 steps under k_fwd_par.

Every case runs test_hip_multiblock16.run_case: operators partition by partition at 1e-10 with no chain unjudged, two Newton
and two quasi-Newton steps in every partition at 1e-9 with statuses and both iteration counts equal to the oracle's for every
chain, a step from unprojected momenta where `unproj` is set, and the launch-counter witnesses (device only).  Every case has
a `*_host_logic` twin on the TEST-ONLY emulation build (generic functors: the host sequencing, the layout tables and the
oracle side of every comparison, to the same bounds).  The further bodies are the sibling modules' own, imported.

Screened on the CPU with tools/screen_layout_edges.py (run_case and the switch, masked and trajectory bodies on the emulation
build, every oracle step traced: every step of run_case ends with status 0 and no retraction residual of any iteration lies
within 1e-2 relative of constraint_tol / position_tol) and, for the tree, with the method of tools/screen_tree_oracle.py
(--search on this module's TREE layout).  Seeds that failed a screening and must not be used: REPLACED."""
import os
import subprocess
import sys
import numpy as np
import pytest
from autodiff_checks import UNJUDGED
from helpers import make_case, make_ctx, check_block_metric_against_oracle
import test_hip_layout_edges as le
import test_hip_multiblock16 as mb
import test_hip_tree_oracle as to
from test_emu_logic import emu_lib  # noqa: F401

ROOT = le.ROOT

# id: model, T, S, R, noisy, gaussian, var_sigma, obs_interval, chains, expected K, expected RM, unproj, seed  (le.build_case)
CASES = {
    # 12-row blocks in 16 slots, K > 4 in both partitions: stored-rows state sweep; k_newton_factor_wave packs four blocks per
    # wavefront across chains
    "fhn16_k5_6": ("fhn", 50, 8, 10, True, False, False, None, 5, [5, 6], 16, True, 31),
    # partition 0 interval-parallel, partition 1 stored rows, in one context
    "fhn16_k4_5": ("fhn", 40, 8, 10, True, False, False, None, 5, [4, 5], 16, True, 31),
    # all 16 rows used (14 + 2), beside 14, 9 and 7
    "fhn16_k2_3_full": ("fhn", 28, 8, 14, True, False, False, None, 5, [2, 3], 16, True, 31),
    # noiseless, 14 + 2 = 16 rows, beside 15 and 8
    "fhn16_noiseless_k3_4_full": ("fhn", 45, 8, 15, False, False, False, None, 5, [3, 4], 16, False, 131),
    # noiseless, Gaussian splitting, stored-rows sweeps
    "fhn16_noiseless_gauss_k6_7": ("fhn", 60, 8, 10, False, True, False, None, 5, [6, 7], 16, False, 31),
    # FhnVsModel, U = 5
    "fhn16_varsigma_k4_5": ("fhn", 40, 8, 10, True, False, True, None, 5, [4, 5], 16, True, 331),
    # FhnNbModel
    "fhn_nb16_noiseless_k3_4": ("fhn_nb", 36, 8, 12, False, True, False, None, 5, [3, 4], 16, False, 31),
    # one 16-slot block per chain: the batched _wg path with the time-parallel scan; the per-chain kernels stay out
    "fhn16_single_block": ("fhn", 14, 16, 14, True, False, False, None, 5, [1], 16, True, 31),
    # longest block 13 x 80 = 1040 steps: k_fwd_par with several 16-row FHN blocks
    "fhn16_long_k2_3": ("fhn", 26, 80, 13, True, False, False, None, 5, [2, 3], 16, True, 331),
}
LONG = ("fhn16_single_block", "fhn16_long_k2_3")  # KernelPlan::par_scan
REPLACED = {  # id: seeds that failed the screening; shapes that failed it with every seed tried and are not in the table
    "fhn16_noiseless_k3_4_full": {31: "screening"},
    "fhn16_varsigma_k4_5": {31: "screening", 131: "screening", 231: "screening"},
    "fhn16_long_k2_3": {31: "near-edge", 231: "near-edge",
                        131: "the emulation build itself is 1.5e-10 from the oracle in chol_C / grad_log_det (ill-conditioned Gram)"},
    "fhn (42, 8, 14)": {s: "near-edge" for s in range(31, 732, 100)},
    # (the momenta / points of the further bodies, not the cases)
    "switch_body momenta on fhn16_k4_5": {5: "forward |dq| 1.0060e-08"},
    "masked_body momenta on fhn16_long_k2_3": {16: "quasi-Newton: reverse |c| 9.925e-10"},
    "metric_case": {31: "quasi-Newton: reverse |c| 9.996e-10, reverse |dq| 9.954e-09", 231: "quasi-Newton: reverse |dq| 9.913e-09"},
}
# masked_body: (step-size scale, max_iters Newton, max_iters quasi-Newton, momenta seed), screened on the CPU: the three
# ordinary chains end with status 0 within max_iters in both partitions, the chain at dt = 5.0 does not
MASKED = {"fhn16_k5_6": (0.25, 6, 12, 16), "fhn16_long_k2_3": (0.25, 6, 12, 36)}
SWITCH = (0.25, 15)  # switch_body on fhn16_k4_5: step-size scale, momenta seed
METRIC = ("fhn", 40, 8, 10, 4, 131)  # check_block_metric_against_oracle: model, T, S, R, chains, seed
# transitions_body / restore_body on fhn16_k4_5's layout: seed and step sizes chosen by tools/screen_tree_oracle.py's search
TREE = dict(layout=("fhn", 40, 8, 10, True, False, False, None), K=[4, 5], metric=False, env={}, n_inner=1, restore_scale=0.25,
            seed=31, eps=np.array([0.03, 0.8, 0.6, 0.5, 0.5]))
BUILD = le.build_case
dts_of = le.dts_of


def run_case(ctx, case, cfg, on_device=True, long=False):
    """mb.run_case (tools/screen_layout_edges.py calls it through this module)."""
    return mb.run_case(ctx, case, cfg, on_device=on_device, long=long)


def switch_16(ctx, case, cfg, on_device=True):
    """mb.switch_16 with this module's screened step-size scale and momenta."""
    def counters(ctx, part, d0, d1):
        mb.witness(ctx, part, d0, d1, "step", True)

    def ops(ctx):
        d0 = ctx.diagnostics()
        w = mb.check_ops_at_current_state(ctx, case["osys"])
        part = ctx.get_state()[3]
        mb.witness(ctx, part, d0, ctx.diagnostics(), "operators after the switch", on_device, state_evals=False)
        print(f"  after the switch to partition {part} (rel):", {k: f"{v:.1e}" for k, v in w.items()})
        assert w[UNJUDGED] == 0, w

    le.switch_body(ctx, case, cfg, on_device, witness=counters, after_switch=ops, dt_scale=SWITCH[0], seed=SWITCH[1])


def masked_16(ctx, case, cfg, name, newton, on_device=True):
    scale, it_newton, it_quasi, seed = MASKED[name]
    f0 = mb.hist(ctx)
    le.masked_body(ctx, case, cfg, newton, dt_scale=scale, max_iters=it_newton if newton else it_quasi, seed=seed)
    f1 = mb.hist(ctx)
    print(f"  {name} newton={newton}: par_scan[0] {f0[0]} -> {f1[0]}, settled time-parallel scans {f0[1]} -> {f1[1]}")
    if on_device:
        assert (f1[1] > f0[1]) == (name in LONG)


trajectories = mb.trajectories


def metric_case():
    model, T, S, R, B, seed = METRIC
    return make_case(model, T, S, R, True, B=B, seed=seed)


def no_per_chain_kernels(ctx):
    d = ctx.diagnostics()
    assert d["retract_kernel_launches"] == 0 and d["traj_kernel_launches"] == 0, d


def shard_body(device_init=True):
    """fhn16_k5_6's layout with 6 chains as one context and as 2 x 3 with chain_offset: initial states by the library's
    linear-interpolation entry point, Philox momentum refresh, 3 steps -- bitwise the same chain for chain."""
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload
    kw = dict(num_steps_per_obs=8, num_obs=50, num_obs_per_subseq=10, num_steps_per_obs_data=200, device_init=device_init)
    dts = np.array([0.05, -0.05, 0.08, 0.02, -0.08, 0.04])

    def run(wl, sl):
        assert wl.ctx.K == [5, 6] and wl.ctx.RM == 16
        assert np.abs(wl.ctx.constr()).max() < 1e-9
        wl.refresh_momentum()
        res = [wl.step(dts[sl]) for _ in range(3)]
        q1, p1, _, _ = wl.ctx.get_state()
        wl.ctx.close()
        return res, q1, p1

    whole = run(FhnWorkload(6, **kw), slice(0, 6))
    n_ok = 0
    for h in range(2):
        sl = slice(3 * h, 3 * h + 3)
        part = run(FhnWorkload(3, chain_offset=3 * h, total_chains=6, **kw), sl)
        for ra, rb in zip(whole[0], part[0]):
            for k in ra:
                np.testing.assert_array_equal(ra[k][sl], rb[k], err_msg=f"{k} shard {h}")
        np.testing.assert_array_equal(whole[1][sl], part[1])
        np.testing.assert_array_equal(whole[2][sl], part[2])
        n_ok += int((part[0][-1]["status"] == 0).sum())
    assert n_ok >= 3  # (the comparison is of moving chains, not of failed steps that left their state alone)


def surface_body():
    """The wiring of the reference's scripts (tests/test_hip_surface.py::test_reference_style_script_single_chain) with
    num_obs_per_subseq = 10: 12-row blocks in 16 slots, one integrator step and a partition switch against oracle/py."""
    import manifold_mcmc_for_diffusions_amd as mm
    from manifold_mcmc_for_diffusions_amd import example_models as em
    from oracle.py import models as omodels, system as osys
    tols = dict(constraint_tol=1e-9, position_tol=1e-8, max_iters=50)
    rng = np.random.default_rng(20200710)
    y = em.simulate_fhn_observations(30, 0.2, 200, seed=1, sigma=0.1)
    system = mm.ConditionedDiffusionConstrainedSystem(
        0.2, 8, 10, y, em.fhn.dim_z, em.fhn.dim_x, em.fhn.dim_v, em.fhn.forward_func, em.fhn.generate_x_0,
        em.fhn.generate_z, em.fhn.obs_func, generate_σ=0.1, use_gaussian_splitting=False, dim_v_0=em.fhn.dim_v_0)
    assert system.ctx.RM == 16 and system.ctx.K == [3, 4]
    integrator = mm.ConstrainedLeapfrogIntegrator(
        system, n_inner_step=1, projection_solver=mm.jitted_solve_projection_onto_manifold_newton,
        reverse_check_tol=2e-8, projection_solver_kwargs=tols)
    integrator.step_size = 0.05
    gen = lambda r: np.concatenate((y, r.standard_normal(y.shape) * 0.5), -1)  # noqa: E731
    u, v_0 = rng.standard_normal(4), rng.standard_normal(2)
    state = mm.find_initial_state_by_linear_interpolation(system, rng, gen, u=u, v_0=v_0)
    assert abs(system.constr(state)).max() < 1e-9
    ref = osys.make_system(omodels.fhn, 0.2, 8, 10, y, sigma=0.1)
    rstate = osys.ConditionedDiffusionHamiltonianState(state.pos, state.x_obs_seq, 0, mom=state.mom)
    rinteg = osys.ConstrainedLeapfrogIntegrator(ref, step_size=0.05, projection_solver_kwargs=tols)
    state, rstate = integrator.step(state), rinteg.step(rstate)
    np.testing.assert_allclose(state.pos, rstate.pos, atol=1e-8)
    np.testing.assert_allclose(state.mom, rstate.mom, atol=1e-7)
    assert abs(system.h(state) - ref.h(rstate)) < 1e-7 * abs(ref.h(rstate))
    state, _ = mm.SwitchPartitionTransition(system).sample(state)
    rstate, _ = osys.SwitchPartitionTransition(ref).sample(rstate)
    np.testing.assert_allclose(state.x_obs_seq, rstate.x_obs_seq, atol=1e-9)
    state, rstate = integrator.step(state), rinteg.step(rstate)  # ... and a step in partition 1 (stored rows would need K > 4)
    np.testing.assert_allclose(state.pos, rstate.pos, atol=1e-8)
    np.testing.assert_allclose(state.mom, rstate.mom, atol=1e-7)


def samplers_body():
    """The static and the dynamic sampler on fhn16_k4_5's layout: a few transitions each; every chain stays on the manifold
    and some of them move: nothing on the samplers' path refuses or breaks on 16 row slots.  The arithmetic of whole
    transitions on this layout is judged against the C oracle elsewhere: the static sampler's loop (with the metric adapter)
    by tests/test_hip_static_oracle.py's case fhn16_k4_5, the dynamic transition by transitions_body / restore_body here."""
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc
    cfg = CASES["fhn16_k4_5"]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    r = sample_static_chmc(ctx, 4, 3, 0.02, seed=3)
    assert np.isfinite(r["heads"]).all() and np.abs(ctx.constr()).max() < 1e-8 and r["accept_stat"].max() > 0
    assert not np.array_equal(r["heads"][-1], case["q"][:, :6])
    r = sample_dynamic_chmc(ctx, 3, 0.02, seed=3, max_tree_depth=2)
    assert np.isfinite(r["heads"]).all() and np.abs(ctx.constr()).max() < 1e-8 and r["n_step"].max() > 0
    ctx.close()


# ------------------------------------------------------------------------------------------------------ emulation build
# (TEST-ONLY: generic functors only, so these say nothing about the device's kernels -- they hold the host side of these
# layouts, the oracle side of every comparison and the screening of the seeds to the same bounds)
@pytest.mark.parametrize("name", list(CASES))
def test_case_host_logic(emu_lib, name):  # noqa: F811
    cfg = CASES[name]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg, on_device=False)
    ctx.close()


def test_switch_host_logic(emu_lib):  # noqa: F811
    cfg = CASES["fhn16_k4_5"]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    switch_16(ctx, case, cfg, on_device=False)
    ctx.close()


@pytest.mark.parametrize("name", list(MASKED))
def test_masked_host_logic(emu_lib, name):  # noqa: F811
    cfg = CASES[name]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    for newton in (True, False):
        masked_16(ctx, case, cfg, name, newton, on_device=False)
    ctx.close()


def test_trajectories_host_logic(emu_lib):  # noqa: F811
    trajectories(BUILD(CASES["fhn16_k4_5"]), CASES["fhn16_k4_5"])


@pytest.mark.parametrize("newton", [True, False])
def test_block_metric_host_logic(emu_lib, newton):  # noqa: F811
    case = metric_case()
    ctx = make_ctx(case)
    assert ctx.K == [4, 5] and ctx.RM == 16
    w = check_block_metric_against_oracle(ctx, case, newton, le.FHN_DTS[:4])
    assert w[UNJUDGED] == 0
    ctx.close()


def test_transition_and_restore_host_logic(emu_lib):  # noqa: F811
    case = to.build_case(TREE)
    ctx = make_ctx(case)
    to.transitions_body(ctx, case, TREE)
    to.restore_body(ctx, case, TREE)
    ctx.close()


def test_shards_host_logic(emu_lib):  # noqa: F811
    shard_body()


def test_public_surface_host_logic(emu_lib):  # noqa: F811
    surface_body()


def test_samplers_host_logic(emu_lib):  # noqa: F811
    samplers_body()


def test_more_than_16_rows_are_still_refused(emu_lib):  # noqa: F811
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    for R, noisy in ((15, True), (16, False)):  # 15 + 2 and 15 + 2 rows
        with pytest.raises(RuntimeError, match="not supported"):
            ChmcContext("fhn", 0.2, 4, R, np.zeros(2 * R + 2), sigma=0.1 if noisy else None, num_chains=2)


# ---------------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    _hip()
    cfg = CASES[name]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg, long=name in LONG)
    no_per_chain_kernels(ctx)
    ctx.close()


@pytest.mark.gpu
def test_single_block_stays_on_the_batched_path_when_the_per_chain_kernels_are_asked_for(monkeypatch):
    """CHMC_RETRACT_KERNEL=1 (read on entry to every call): an FHN layout with one 16-slot block per chain has no per-chain
    kernels, so the switch changes nothing -- same checks, out80[66] and out80[67] stay 0."""
    _hip()
    monkeypatch.setenv("CHMC_RETRACT_KERNEL", "1")
    cfg = CASES["fhn16_single_block"]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg, long=True)
    no_per_chain_kernels(ctx)
    ctx.close()


@pytest.mark.gpu
def test_both_sixteen_row_state_evaluations_across_partition_switches():
    """fhn16_k4_5: step in partition 0 (interval-parallel, rows rebuilt on demand), switch, step in partition 1 (stored rows),
    switch back, step -- every chain against an oracle chain that does the same; all operators after every switch."""
    _hip()
    cfg = CASES["fhn16_k4_5"]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    switch_16(ctx, case, cfg)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MASKED))
@pytest.mark.parametrize("newton", [True, False])
def test_masked_and_failing_chains(name, newton):
    _hip()
    cfg = CASES[name]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    masked_16(ctx, case, cfg, name, newton)
    ctx.close()


@pytest.mark.gpu
def test_trajectories():
    """chmc_leapfrog_steps bitwise the host loop over chmc_leapfrog_step, and within 1e-9 of the oracle with equal counts."""
    _hip()
    trajectories(BUILD(CASES["fhn16_k4_5"]), CASES["fhn16_k4_5"])


@pytest.mark.gpu
@pytest.mark.parametrize("newton", [True, False])
def test_block_metric(newton):
    """metric = blockdiag(M_0, I) on FHN (40, 8, 10), K = [4, 5]: operators, projection with its multiplier term, momentum
    sampling and steps in both partitions."""
    _hip()
    case = metric_case()
    ctx = make_ctx(case)
    assert ctx.K == [4, 5] and ctx.RM == 16
    w = check_block_metric_against_oracle(ctx, case, newton, le.FHN_DTS[:4])
    print("  operators with M_0 (rel):", {k: f"{v:.1e}" for k, v in w.items()})
    assert w[UNJUDGED] == 0
    ctx.close()


@pytest.mark.gpu
def test_transition_and_restore_against_the_oracle():
    """No-U-turn transitions (depth 3, with partition switches between them) and the snapshot / restore body on fhn16_k4_5's
    layout, as tests/test_hip_tree_oracle.py runs them."""
    _hip()
    case = to.build_case(TREE)
    ctx = make_ctx(case)
    assert ctx.RM == 16
    to.transitions_body(ctx, case, TREE)
    to.restore_body(ctx, case, TREE)
    no_per_chain_kernels(ctx)
    ctx.close()


@pytest.mark.gpu
def test_results_do_not_depend_on_the_shard_size():
    _hip()
    shard_body()


@pytest.mark.gpu
def test_public_surface():
    _hip()
    surface_body()


@pytest.mark.gpu
def test_samplers():
    _hip()
    samplers_body()


# The other two row families are latched per process: a child process each, as tests/test_hip_multiblock16.py starts them.
_FAMILY_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_ctx, check_ops_against_oracle, check_steps_against_oracle
import test_hip_fhn16 as f16
cfg = f16.CASES["fhn16_k5_6"]
case = f16.BUILD(cfg)
ctx = make_ctx(case)
assert ctx.L.chmc_backend() == b"hip:gfx950" and ctx.K == [5, 6] and ctx.RM == 16
worst = check_ops_against_oracle(ctx, case)
print("OPS_WORST", worst)
assert worst[f16.UNJUDGED] == 0
for newton in (True, False):
    for part in range(2):
        print("STEPS", newton, part, check_steps_against_oracle(ctx, case, f16.dts_of(cfg), newton=newton, n_steps=2, part=part))
d1 = ctx.diagnostics()
assert d1["newton_fsm_launches"] == 0 and d1["newton_factor8_launches"] == 0, d1
assert d1["retract_kernel_launches"] == 0 and d1["traj_kernel_launches"] == 0, d1
assert (d1["gram_mfma_launches"] > 0) == {mfma} and (d1["gram_valu_launches"] > 0) == (not {mfma}), d1
print("FAMILY_OK", d1["gram_mfma_launches"], d1["gram_valu_launches"])
ctx.close()
"""


@pytest.mark.gpu
def test_stored_row_families():
    """CHMC_COMPACT_ROWS=0, then CHMC_GRAM_MFMA=1 (k_gram_rows_mfma<16> on FHN rows) on fhn16_k5_6: operators and steps in
    both partitions, the same bounds.  One child at a time, each under a time limit; nothing is started after a failure."""
    _hip()
    for env, mfma in (({"CHMC_COMPACT_ROWS": "0"}, False), ({"CHMC_GRAM_MFMA": "1"}, True)):
        script = _FAMILY_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mfma=mfma)
        r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True,
                           timeout=300)
        print(env, r.stdout[-1500:])
        assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
        assert "FAMILY_OK" in r.stdout
