"""16-row blocks with SEVERAL blocks per chain, and the time-parallel forward scan with several blocks per chain, against
the C oracle -- the launch sites of csrc/chmc_plan.h between the FitzHugh-Nagumo layouts (6, 7, 8 row slots, many blocks)
and the boarding-school layout (one 16-row block per chain):

  * K > 4 with 16 row slots: the default plan keeps the rows (state k_rev_wave_ldsrows + k_gram_rows, Newton round
    k_newton_ivl + k_newton_comb + k_newton_factor_wave + k_solve_chain_wave, k_gld_fwd_wave<compact> +
    k_gld_bwd_wave_ldsrows, k_jw_pb); k_newton_factor_wave / k_gld_prep_wave pack four blocks into a wavefront and k_gram_rows
    launches nbk RM / 4 wavefronts, so with 5 chains of 4 | 5, 5 | 6, 3 | 4 and 6 | 7 blocks a wavefront holds blocks of two chains
    and the last group is partial in both partitions;
  * K = [4, 5]: partition 0 interval-parallel (rebuild_rows), partition 1 stored rows, in ONE context -- shared Slots::Jv,
    rows_fresh and arrays strided by Kmax = 5 (the 16-row twin of K = [64, 65] of tests/test_hip_layout_edges.py);
  * SirVsModel (variable observation noise) with RM = 16 and K > 1;
  * k_fwd_par with K > 1 (few_long_blocks: K <= 4, longest block >= 1024 steps): blocks that start from x_obs, the end-of-block
    constraint rows, `out` strided by Kmax, no carry-over between rounds, 12 sweeps and then the recursion by lane 0 inside
    the launch, 1 and 2 wavefronts per block; 16 and 8 row slots.

Every case: check_ops_against_oracle partition by partition (1e-10, no chain unjudged), check_steps_against_oracle with Newton
and quasi-Newton, 2 steps, in every partition (1e-9; statuses and both iteration counts equal for every chain, no allowance)
and one step from unprojected momenta in the last partition.  Which path ran is asserted from ctx.diagnostics() around every
batch (device only): gram_valu_launches (k_gram_rows) rises exactly in the partitions with 16 row slots and K > 4, the
per-chain kernels (retract / traj) never run, out80[68] / out80[69] stay 0 for 16 rows, and the sweep histogram of the
time-parallel scan (par_scan[1:48]) has entries exactly for LONG.  par_scan[0] (recursions by lane 0 inside a launch) is printed.

All cases are noisy with DISTINCT on-manifold chains, 5 of them.  SIR: 0.05 between observations (diagonally scaled Gram
blocks of condition number 4e2 to 7e3; at 0.25 it is 3.8e7 for (26, 24, 13) and the CPU emulation build itself is 7.9e-9 from
the oracle in lmult_by_inv_gram).  Screened on the CPU with tools/screen_layout_edges.py (this module's run_case and the other
bodies on the emulation build, every oracle step traced): every step of run_case ends with status 0, no retraction residual
of any iteration lies within 1e-2 relative of constraint_tol / position_tol, and every operator agrees below 1e-11.  For LONG
the emulation build says nothing about k_fwd_par (it has no such kernel): the screening vouches for the oracle side only.
Seeds that failed the screening and must not be used: REPLACED."""
import os
import subprocess
import sys
import numpy as np
import pytest
from autodiff_checks import UNJUDGED
from helpers import make_case, make_ctx, check_ops_against_oracle, check_ops_at_current_state, check_block_metric_against_oracle
import test_hip_layout_edges as le
from test_emu_logic import emu_lib  # noqa: F401

ROOT = le.ROOT
SIR_DTS = le.SIR_DTS

# id: model, T, S, R, noisy, gaussian, var_sigma, obs_interval, chains, expected K, expected RM, unproj, seed  (le.build_case)
CASES = {
    # both 16-row state evaluations in one context; rows 13/13/13/10 and 8/13/13/13/5
    "sir16_k4_5": ("sir", 40, 8, 10, True, False, False, 0.05, 5, [4, 5], 16, True, 31),
    # 9 rows in 16 slots (7 padded), last blocks of 6 and 3 rows
    "sir16_k5_6_rows9": ("sir", 30, 8, 6, True, False, False, 0.05, 5, [5, 6], 16, True, 131),
    # full 16-row blocks beside 13, 9 and 7 rows; interval-parallel in both partitions
    "sir16_k3_4_full": ("sir", 39, 8, 13, True, False, False, 0.05, 5, [3, 4], 16, True, 31),
    # tests/test_kernel_plan.py's sir_16rows_7blocks: stored-rows state sweep in both partitions
    "sir16_k6_7": ("sir", 60, 8, 10, True, False, False, 0.05, 5, [6, 7], 16, True, 31),
    "sir16_k4_5_varsigma": ("sir", 40, 8, 10, True, False, True, 0.05, 5, [4, 5], 16, True, 31),
    # longest block 13 x 80 = 1040 steps: k_fwd_par<.., 1> with several 16-row blocks
    "sir16_long_k3_4": ("sir", 39, 80, 13, True, False, False, 0.05, 5, [3, 4], 16, True, 31),
    "sir16_long_k2_3": ("sir", 26, 80, 13, True, False, False, 0.05, 5, [2, 3], 16, True, 131),
    # 8 row slots, longest block 1024 steps; 2048 steps: two wavefronts per block
    "fhn_long_k2_3": ("fhn", 4, 512, 2, True, False, False, None, 5, [2, 3], 8, True, 431),
    "fhn_long_w2_k2_3": ("fhn", 4, 1024, 2, True, False, False, None, 5, [2, 3], 8, True, 31),
}
LONG = ("sir16_long_k3_4", "sir16_long_k2_3", "fhn_long_k2_3", "fhn_long_w2_k2_3")  # KernelPlan::par_scan
REPLACED = {  # id: seeds that failed the screening; shapes that failed it with seed 31 and are not in the table
    # (chain 1's latent path runs into the model's +-500 clip: in partition 1 the ORACLE's chol_C, the last chol_D block, log_det,
    # the gradient and the inverse-Gram products are NaN there -- a comparator that dropped NaN had let it pass)
    "sir16_k5_6_rows9": {31: "partition 1, chain 1: oracle not finite (unjudged_chains = 1)"},
    "fhn_long_k2_3": {31: "screening", 131: "screening", 331: "screening"},  # (231 is clean as well)
    "fhn_long_w2_k2_3": {131: "screening"},
    "sir (50, 8, 10) at 0.05": {31: "screening"},
    "sir (8, 512, 4) at 0.25": {31: "screening"},
}
# masked_body: (step-size scale, max_iters Newton, max_iters quasi-Newton, momenta seed), screened on the CPU: the three
# ordinary chains end with status 0 within max_iters in both partitions, the chain at dt = 5.0 does not
MASKED = {"sir16_k4_5": (1.0, 6, 8, 16), "sir16_k6_7": (1.0, 6, 8, 16), "sir16_long_k3_4": (1.0, 6, 8, 16),
          # (FHN from the chains' own points: at the full step sizes chain 4 needs more than 12 quasi-Newton iterations)
          "fhn_long_k2_3": (0.25, 6, 12, 16)}
SWITCH = (1.0, 5)  # switch_body on sir16_k4_5: step-size scale, momenta seed
BUILD = le.build_case
dts_of = le.dts_of


def hist(ctx):
    """(recursions by lane 0 inside a k_fwd_par launch, settled scans by number of sweeps and guess: par_scan[1:48])."""
    ps = ctx.diagnostics()["par_scan"]
    return int(ps[0]), int(ps[1:48].sum())


def witness(ctx, part, d0, d1, what, on_device, state_evals=True):
    """The launch counters around one batch of state evaluations / steps in partition `part` (state_evals: the batch evaluates
    the state at least once)."""
    gram = d1["gram_valu_launches"] - d0["gram_valu_launches"]
    print(f"  part {part} K={ctx.K[part]} {what}: gram_valu_launches +{gram}")
    if not on_device:  # (the emulation build has no wave kernels and counts nothing)
        return
    assert (gram > 0) == (state_evals and ctx.RM > 8 and ctx.K[part] > 4), (part, ctx.K, gram)  # stored-rows state sweep: k_gram_rows
    assert d1["retract_kernel_launches"] == 0 and d1["traj_kernel_launches"] == 0 and d1["gram_mfma_launches"] == 0, d1
    if ctx.RM > 8:
        assert d1["newton_fsm_launches"] == 0 and d1["newton_factor8_launches"] == 0, d1


def run_case(ctx, case, cfg, on_device=True, long=False):
    """Everything one case checks (also run by the CPU screening on the emulation build)."""
    K, rm, unproj = cfg[9], cfg[10], cfg[11]
    assert ctx.K == K and ctx.RM == rm and ctx.num_partition == len(K), (ctx.K, ctx.RM)
    print(f"\nQ={ctx.Q} B={ctx.B} K={ctx.K} RM={ctx.RM} C={ctx.C}")
    worst = {}
    for part in range(ctx.num_partition):
        d0 = ctx.diagnostics()
        w = check_ops_against_oracle(ctx, case, parts=[part])
        witness(ctx, part, d0, ctx.diagnostics(), "operators", on_device)
        print(f"  part {part} operators (rel):", {k: f"{v:.1e}" for k, v in w.items()})
        worst = {k: max(v, worst.get(k, 0)) for k, v in w.items()}
    print("  operators (rel):", {k: f"{v:.1e}" for k, v in worst.items()})
    assert worst[UNJUDGED] == 0, worst
    dts = dts_of(cfg)
    steps = [(newton, part, 2, True) for newton in (True, False) for part in range(ctx.num_partition)]
    if unproj:
        steps.append((True, ctx.num_partition - 1, 1, False))
    for newton, part, n, project in steps:
        d0 = ctx.diagnostics()
        le.counted_steps(ctx, case, dts, newton, part, on_device, n_steps=n, project=project)
        witness(ctx, part, d0, ctx.diagnostics(), "steps", on_device)
    fallbacks, sweeps = hist(ctx)
    print(f"  par_scan[0] (recursions by lane 0 inside a launch) = {fallbacks}; settled time-parallel scans = {sweeps}")
    if on_device:
        assert (sweeps > 0) == long, (long, ctx.diagnostics()["par_scan"])
    return worst


def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


def switch_16(ctx, case, cfg, on_device=True):
    """le.switch_body on K = [4, 5]: partition 0 evaluates its state interval-parallel and rebuilds the rows on demand,
    partition 1 keeps the rows of its state sweep; after every switch all operators at the state the context holds."""
    def counters(ctx, part, d0, d1):
        witness(ctx, part, d0, d1, "step", True)

    def ops(ctx):
        d0 = ctx.diagnostics()
        w = check_ops_at_current_state(ctx, case["osys"])
        part = ctx.get_state()[3]
        witness(ctx, part, d0, ctx.diagnostics(), "operators after the switch", on_device, state_evals=False)
        print(f"  after the switch to partition {part} (rel):", {k: f"{v:.1e}" for k, v in w.items()})
        assert w[UNJUDGED] == 0, w

    le.switch_body(ctx, case, cfg, on_device, witness=counters, after_switch=ops, dt_scale=SWITCH[0], seed=SWITCH[1])


def masked_16(ctx, case, cfg, name, newton, on_device=True):
    scale, it_newton, it_quasi, seed = MASKED[name]
    f0 = hist(ctx)
    le.masked_body(ctx, case, cfg, newton, dt_scale=scale, max_iters=it_newton if newton else it_quasi, seed=seed)
    f1 = hist(ctx)
    print(f"  {name} newton={newton}: par_scan[0] {f0[0]} -> {f1[0]}, settled time-parallel scans {f0[1]} -> {f1[1]}")
    if on_device:
        assert (f1[1] > f0[1]) == (name in LONG)


def trajectories(case, cfg, n_steps=3):
    """chmc_leapfrog_steps against the host loop over chmc_leapfrog_step (bitwise) and against the C oracle (1e-9), from chain
    0's point with independent momenta, both partitions."""
    from oracle import c_oracle
    from test_trajectories import lockstep_trajectories, assert_same
    B, dts = case["B"], dts_of(cfg)
    qq, xx = np.repeat(case["q"][:1], B, 0), np.repeat(case["x_obs"][:1], B, 0)
    p = np.random.default_rng(7).standard_normal(qq.shape)
    for part in range(len(cfg[9])):
        outs = []
        for engine in (True, False):
            ctx = make_ctx(case)
            ctx.set_state(qq, p, xx, part)
            ctx.project_onto_cotangent_space()
            p0 = ctx.get_state()[1]
            r = ctx.leapfrog_steps(dts, n_steps) if engine else lockstep_trajectories(ctx, dts, n_steps)
            q1, p1, _, _ = ctx.get_state()
            outs.append((r, q1, p1, ctx.hamiltonian()))
            ctx.close()
        assert_same(*outs)
        r, q1, p1, _ = outs[0]
        for c in range(B):
            ch = c_oracle.OracleChain(case["osys"])
            ch.set(qq[c], p0[c], xx[c], part)
            itf = itb = 0
            for _ in range(n_steps):
                st, f, b, _ = ch.step(dts[c])
                assert st == 0, (part, c, st)
                itf, itb = itf + f, itb + b
            qo, po, _, _ = ch.get()
            assert (r["n_done"][c], r["status"][c], r["iters_fwd"][c], r["iters_bwd"][c]) == (n_steps, 0, itf, itb), (part, c, r)
            assert np.abs(q1[c] - qo).max() <= 1e-9 * max(1.0, np.abs(qo).max()), (part, c)
            assert np.abs(p1[c] - po).max() <= 1e-9 * max(1.0, np.abs(po).max()), (part, c)
        print(f"  part {part}: iterations (forward, reverse) per chain {list(zip(r['iters_fwd'], r['iters_bwd']))}")


def metric_case():
    return make_case("sir", 40, 8, 10, True, B=4, seed=31, obs_interval=0.05)


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
    cfg = CASES["sir16_k4_5"]
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


@pytest.mark.parametrize("newton", [True, False])
def test_block_metric_host_logic(emu_lib, newton):  # noqa: F811
    case = metric_case()
    ctx = make_ctx(case)
    w = check_block_metric_against_oracle(ctx, case, newton, SIR_DTS[:4])
    assert w[UNJUDGED] == 0
    ctx.close()


@pytest.mark.parametrize("name", ["sir16_k4_5", "sir16_long_k3_4"])
def test_trajectories_host_logic(emu_lib, name):  # noqa: F811
    trajectories(BUILD(CASES[name]), CASES[name])


# ---------------------------------------------------------------------------------------------------------- HIP library
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    _hip()
    cfg = CASES[name]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg, long=name in LONG)
    ctx.close()


@pytest.mark.gpu
def test_both_sixteen_row_state_evaluations_across_partition_switches():
    """K = [4, 5]: step in partition 0, switch, step in partition 1, switch back, step in partition 0 -- every chain against an
    oracle chain that does the same; after every switch jacob_constr_blocks hands out rebuilt rows (partition 0) or the
    state sweep's own (partition 1), judged with every other operator at the current state."""
    _hip()
    cfg = CASES["sir16_k4_5"]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    switch_16(ctx, case, cfg)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MASKED))
@pytest.mark.parametrize("newton", [True, False])
def test_masked_and_failing_chains(name, newton):
    """One batched step in each partition with a masked chain (active = 0) and a chain at dt = 5.0 with a small max_iters:
    statuses as the oracle's, both chains' states bitwise unchanged, the others to 1e-9.  The diverging chain is the natural
    customer of the in-launch sequential recursion of k_fwd_par: par_scan[0] is printed before and after."""
    _hip()
    cfg = CASES[name]
    case = BUILD(cfg)
    ctx = make_ctx(case)
    masked_16(ctx, case, cfg, name, newton)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("newton", [True, False])
def test_block_metric(newton):
    """metric = blockdiag(M_0, I) on SIR (40, 8, 10), K = [4, 5]: operators, projection with its multiplier term, momentum
    sampling and steps in both partitions."""
    _hip()
    case = metric_case()
    ctx = make_ctx(case)
    assert ctx.K == [4, 5] and ctx.RM == 16
    w = check_block_metric_against_oracle(ctx, case, newton, SIR_DTS[:4])
    print("  operators with M_0 (rel):", {k: f"{v:.1e}" for k, v in w.items()})
    assert w[UNJUDGED] == 0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sir16_k4_5", "sir16_long_k3_4"])
def test_trajectories(name):
    """Paired retractions (k_fwd_scan<SirModel, 16, .., PAIR>) on K = [4, 5]; the time-parallel scan, which never pairs, on the
    long blocks."""
    _hip()
    trajectories(BUILD(CASES[name]), CASES[name])


# The other two row families are latched per process: a child process each, as tests/test_hip_layout_edges.py starts them.
_FAMILY_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_ctx, check_ops_against_oracle, check_steps_against_oracle
import test_hip_multiblock16 as mb
cfg = mb.CASES["sir16_k4_5"]
case = mb.BUILD(cfg)
ctx = make_ctx(case)
assert ctx.L.chmc_backend() == b"hip:gfx950" and ctx.K == [4, 5] and ctx.RM == 16
worst = check_ops_against_oracle(ctx, case)
print("OPS_WORST", worst)
assert worst[mb.UNJUDGED] == 0
for newton in (True, False):
    for part in range(2):
        print("STEPS", newton, part, check_steps_against_oracle(ctx, case, mb.dts_of(cfg), newton=newton, n_steps=2, part=part))
d1 = ctx.diagnostics()
assert d1["newton_fsm_launches"] == 0 and d1["newton_factor8_launches"] == 0, d1
assert (d1["gram_mfma_launches"] > 0) == {mfma} and (d1["gram_valu_launches"] > 0) == (not {mfma}), d1
print("FAMILY_OK", d1["gram_mfma_launches"], d1["gram_valu_launches"])
ctx.close()
"""


@pytest.mark.gpu
def test_stored_row_families():
    """CHMC_COMPACT_ROWS=0 (k_rev_wave_ldsrows + k_gram_rows in both partitions, Newton rounds included), then CHMC_GRAM_MFMA=1
    (k_gram_rows_mfma) on sir16_k4_5: operators and steps in both partitions.  One child at a time, each under a time limit;
    nothing is started after a failure."""
    for env, mfma in (({"CHMC_COMPACT_ROWS": "0"}, False), ({"CHMC_GRAM_MFMA": "1"}, True)):
        script = _FAMILY_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mfma=mfma)
        r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True,
                           timeout=300)
        print(env, r.stdout[-1500:])
        assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
        assert "FAMILY_OK" in r.stdout
