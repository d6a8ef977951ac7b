"""Layouts at the edges of the kernel plan (csrc/chmc_plan.h) against the C oracle, on the GPU:

  * more than 64 blocks per chain: a Newton round is k_newton_ivl + k_newton_comb, KNewtonFactor, the lane-per-chain
    KSolveChain (the K > 64 arm of solve_chain()) and KMuF as launches of their own, and all six call sites of the
    chain solve take KSolveChain;
  * exactly 64 blocks per chain: every lane of k_newton_fsm_wave / k_solve_chain_wave owns a block;
  * K = [64, 65]: one context switches between the two paths, per-block arrays strided by Kmax = 65;
  * S = 63, 64, 65, 128: the 64-lane tiles of the interval sweeps one lane short, exactly full, one lane over;
  * S = 1, 2, T = 1, T = 3 with R = 2: the degenerate sizes.

Every case: check_ops_against_oracle in every partition (1e-10), check_steps_against_oracle with Newton and quasi-Newton,
2 steps, in every partition (1e-9, statuses and both iteration counts equal for every chain); the cases marked `unproj`
also take one step from momenta that are not in the cotangent space.  Around every Newton / quasi-Newton batch of steps
the launch counters out80[68] (k_newton_fsm_wave) and out80[69] (KNewtonFactor, blocks of at most 8 rows) must move as
the plan says: K <= 64 raises [68] only, K > 64 raises [69] only, quasi-Newton and 16-row blocks neither.

Noisy cases have DISTINCT on-manifold chains (distinct_on_manifold_chains: the operators are judged at five different
points); the steps start, as the helper does it, from chain 0's point with independent momenta and step sizes.

Iteration counts are compared with no allowance, so every case was screened on the CPU (tools/screen_layout_edges.py:
this module's run_case on the emulation build, every oracle step traced): no retraction residual of any iteration of
any chain lies within 1e-2 relative of constraint_tol / position_tol, and every step ends with status 0.  All cases use
seed 31 unless the table says otherwise.  Seeds that were replaced: see REPLACED below."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx, check_ops_against_oracle, check_steps_against_oracle
from test_hip_autodiff_parity import distinct_on_manifold_chains
from test_emu_logic import emu_lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FHN_DTS = np.array([0.05, -0.05, 0.1, 0.02, -0.08])
SIR_DTS = np.array([0.02, -0.02, 0.04, 0.01, -0.03])

# id: model, T, S, R, noisy, gaussian, var_sigma, obs_interval, chains, expected K, expected RM, unproj, seed
BLOCK_COUNT = {
    "fhn_128_4_2_k64_65": ("fhn", 128, 4, 2, True, False, False, None, 5, [64, 65], 8, True, 31),
    "fhn_130_4_2_k65_66": ("fhn", 130, 4, 2, True, False, False, None, 5, [65, 66], 8, True, 31),
    "fhn_126_8_2_noiseless_gauss_k63_64": ("fhn", 126, 8, 2, False, True, False, None, 5, [63, 64], 8, False, 131),
    "fhn_325_8_5_k65_66_rm7": ("fhn", 325, 8, 5, True, False, False, None, 5, [65, 66], 7, True, 31),
    "fhn_330_4_5_noiseless_k66_67_rm6": ("fhn", 330, 4, 5, False, False, False, None, 5, [66, 67], 6, False, 31),
    "fhn_nb_130_4_2_noiseless_gauss_k65_66": ("fhn_nb", 130, 4, 2, False, True, False, None, 5, [65, 66], 8, False, 231),
    "fhn_130_4_2_varsigma_k65_66": ("fhn", 130, 4, 2, True, False, True, None, 5, [65, 66], 8, False, 331),
    # (SIR, 0.05 between observations: at 0.1 and above the epidemic has run out over this many observations and every
    # step of the oracle itself diverges)
    "sir_132_4_2_k66_67": ("sir", 132, 4, 2, True, False, False, 0.05, 5, [66, 67], 8, True, 31),
    "sir_130_3_2_varsigma_k65_66": ("sir", 130, 3, 2, True, False, True, 0.05, 5, [65, 66], 8, False, 31),
}
TILE_EDGE = {
    "fhn_4_64_2": ("fhn", 4, 64, 2, True, False, False, None, 5, [2, 3], 8, True, 131),
    "fhn_5_65_2": ("fhn", 5, 65, 2, True, False, False, None, 5, [3, 3], 8, True, 31),
    "fhn_5_63_3_gauss": ("fhn", 5, 63, 3, True, True, False, None, 5, [2, 3], 8, False, 31),
    "fhn_4_128_2_noiseless": ("fhn", 4, 128, 2, False, False, False, None, 5, [2, 3], 8, False, 131),
    "sir16_14_64": ("sir", 14, 64, 14, True, False, False, None, 5, [1], 16, True, 31),   # 16 rows, one block per chain
    "sir16_14_65": ("sir", 14, 65, 14, True, False, False, None, 5, [1], 16, True, 31),
}
DEGENERATE = {
    "sir16_14_1": ("sir", 14, 1, 14, True, False, False, None, 3, [1], 16, True, 31),
    "sir16_14_2": ("sir", 14, 2, 14, True, False, False, None, 3, [1], 16, False, 31),
    "sir_6_1_2": ("sir", 6, 1, 2, True, False, False, None, 3, [3, 4], 8, True, 31),
    "fhn_1_8": ("fhn", 1, 8, None, True, False, False, None, 3, [1], 8, True, 31),
    "fhn_1_1": ("fhn", 1, 1, None, True, False, False, None, 3, [1], 8, True, 31),
    "sir_1_8": ("sir", 1, 8, None, True, False, False, None, 3, [1], 8, False, 31),
    "fhn_3_8_2": ("fhn", 3, 8, 2, True, False, False, None, 3, [2, 2], 8, True, 31),   # rows 4 and 3
}
CASES = {**BLOCK_COUNT, **TILE_EDGE, **DEGENERATE}
REPLACED = {  # id: the seeds that failed the screening, and on what (direction 0 forward / 1 reverse, |c|, |dq| of the iteration)
    "fhn_126_8_2_noiseless_gauss_k63_64": {31: "forward |dq| 1.0005e-08"},
    "fhn_nb_130_4_2_noiseless_gauss_k65_66": {31: "reverse |dq| 9.982e-09", 131: "reverse |dq| 9.978e-09"},
    "fhn_130_4_2_varsigma_k65_66": {31: "forward |c| 9.930e-10, reverse |dq| 1.0036e-08", 131: "reverse |dq| 1.0046e-08, forward |c| "
                                    "1.0013e-09", 231: "forward |dq| 9.923e-09"},
    "fhn_4_64_2": {31: "reverse |c| 1.0085e-09"},
    "fhn_4_128_2_noiseless": {31: "reverse |c| 9.901e-10"},
    # (the momenta of masked_body, not the case: quasi-Newton, K = [65, 66])
    "masked_body momenta": {6: "reverse |dq| 9.994e-09", 26: "K = [64, 65]: reverse |c| 9.916e-10"},
}


def build_case(cfg):
    model, T, S, R, noisy, gaussian, var_sigma, oi, B, _, _, _, seed = cfg
    if noisy:
        return distinct_on_manifold_chains(model, T, S, R, B, seed, obs_interval=oi, var_sigma=var_sigma, gaussian=gaussian)
    return make_case(model, T, S, R, False, B=B, seed=seed, obs_interval=oi, gaussian=gaussian)


def dts_of(cfg):
    return (SIR_DTS if cfg[0] == "sir" else FHN_DTS)[:cfg[8]]


def counted_steps(ctx, case, dts, newton, part, on_device, **kw):
    """check_steps_against_oracle with the launch counters of the two Newton rounds read around it."""
    d0 = ctx.diagnostics()
    out = check_steps_against_oracle(ctx, case, dts, newton=newton, part=part, **kw)
    d1 = ctx.diagnostics()
    fsm = d1["newton_fsm_launches"] - d0["newton_fsm_launches"]
    factor8 = d1["newton_factor8_launches"] - d0["newton_factor8_launches"]
    print(f"  part {part} K={ctx.K[part]} {'newton' if newton else 'quasi-newton'}: out80[68] +{fsm}, out80[69] +{factor8}; "
          f"(status, iters_fwd, iters_bwd) {sorted(set(out))}")
    if on_device:  # (the emulation build has no wave kernels and counts neither)
        if not newton or ctx.RM > 8:
            assert (fsm, factor8) == (0, 0), (fsm, factor8)
        elif ctx.K[part] <= 64:
            assert fsm > 0 and factor8 == 0, (fsm, factor8)
        else:
            assert factor8 > 0 and fsm == 0, (fsm, factor8)
    return out


def run_case(ctx, case, cfg, on_device=True):
    """Everything one case checks (also run by the CPU screening on the emulation build)."""
    K, rm, unproj = cfg[9], cfg[10], cfg[11]
    assert ctx.K == K and ctx.RM == rm and ctx.num_partition == len(K), (ctx.K, ctx.RM)
    print(f"\nQ={ctx.Q} B={ctx.B} K={ctx.K} RM={ctx.RM} C={ctx.C}")
    worst = check_ops_against_oracle(ctx, case)
    print("  operators (rel):", {k: f"{v:.1e}" for k, v in worst.items()})
    dts = dts_of(cfg)
    for newton in (True, False):
        for part in range(ctx.num_partition):
            counted_steps(ctx, case, dts, newton, part, on_device, n_steps=2)
    if unproj:
        counted_steps(ctx, case, dts, True, ctx.num_partition - 1, on_device, n_steps=1, project=False)


def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


def test_k64_65_host_logic(emu_lib):  # noqa: F811
    """Without a GPU (TEST-ONLY emulation build: generic functors only, so this says nothing about the device's kernels):
    the host side of K = [64, 65] -- per-block arrays strided by Kmax = 65 with K[0] != K[1], both partitions, both
    solvers, the partition switches -- against the C oracle at the same bounds."""
    cfg = CASES["fhn_128_4_2_k64_65"]
    case = build_case(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg, on_device=False)
    switch_body(ctx, case, cfg, on_device=False)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BLOCK_COUNT))
def test_block_count_boundary(name):
    """63 to 67 blocks per chain of 8, 7 and 6 row slots, FitzHugh-Nagumo (both parametrisations, fixed and variable
    sigma, both splittings, k_fwd_scan for S = 8) and SIR."""
    _hip()
    cfg = CASES[name]
    case = build_case(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TILE_EDGE))
def test_tile_boundary(name):
    """S = 63, 64, 65 and 128 steps per observation: the last 64-lane tile of an interval one lane short, full, one lane
    over (k_newton_ivl, k_gld_*_ivl, k_state_lean, k_gld_fwd_qx / k_gld_bwd_lean, k_jw_pb)."""
    _hip()
    cfg = CASES[name]
    case = build_case(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_sizes(name):
    """Every (other) step an observation, one observation, blocks of 2 + 1 and 1 + 2 observations."""
    _hip()
    cfg = CASES[name]
    case = build_case(cfg)
    ctx = make_ctx(case)
    run_case(ctx, case, cfg)
    ctx.close()


@pytest.mark.gpu
def test_one_context_takes_both_newton_paths_across_a_partition_switch():
    """FHN T = 128, S = 4, R = 2 (K = [64, 65]): a Newton step in partition 0 raises out80[68] only, chmc_switch_partition,
    a Newton step in partition 1 raises out80[69] only -- distinct chains, each against an oracle chain that does the same."""
    _hip()
    cfg = CASES["fhn_128_4_2_k64_65"]
    case = build_case(cfg)
    ctx = make_ctx(case)
    switch_body(ctx, case, cfg)
    ctx.close()


def fsm_or_factor8(ctx, part, d0, d1):
    """The launch counters of the two Newton rounds of blocks of at most 8 rows, around a Newton step in `part`: K <= 64 raises
    out80[68] only, K > 64 out80[69] only."""
    fsm, factor8 = (d1[k] - d0[k] for k in ("newton_fsm_launches", "newton_factor8_launches"))
    print(f"  partition {part} (K = {ctx.K[part]}): out80[68] +{fsm}, out80[69] +{factor8}")
    assert (fsm > 0 and factor8 == 0) if ctx.K[part] <= 64 else (fsm == 0 and factor8 > 0), (fsm, factor8)


def switch_body(ctx, case, cfg, on_device=True, witness=fsm_or_factor8, after_switch=None, dt_scale=0.25, seed=5):
    """A step in partition 0, chmc_switch_partition, a step in partition 1, back, a step in partition 0: distinct chains from
    their own points, each against an oracle chain that does the same (status 0, both iteration counts, 1e-9).  On the device
    witness(ctx, part, diagnostics before, after) judges the launch counters around each step; after_switch(ctx), if given,
    runs after every switch (both sides have projected their momenta by then)."""
    from oracle import c_oracle
    B, dts = case["B"], dt_scale * dts_of(cfg)  # (FHN, from the chains' own, distinct points: chain 2 diverges in the oracle at 0.1)
    assert ctx.K == cfg[9] and ctx.num_partition == 2
    p_raw = np.random.default_rng(seed).standard_normal(case["q"].shape)
    ctx.set_state(case["q"], p_raw, case["x_obs"], 0)
    ctx.project_onto_cotangent_space()
    chains = []
    for c in range(B):
        ch = c_oracle.OracleChain(case["osys"])
        ch.set(case["q"][c], p_raw[c], case["x_obs"][c], 0)
        ch.project_mom()
        chains.append(ch)

    def step_and_compare(part):
        d0 = ctx.diagnostics()
        res = ctx.leapfrog_step(dts)
        d1 = ctx.diagnostics()
        q1, p1, _, got_part = ctx.get_state()
        assert got_part == part
        for c, ch in enumerate(chains):
            st, itf, itb, _ = ch.step(dts[c])
            qo, po, _, _ = ch.get()
            assert (res["status"][c], res["iters_fwd"][c], res["iters_bwd"][c]) == (st, itf, itb) and st == 0, (c, res, st, itf, itb)
            assert np.abs(q1[c] - qo).max() <= 1e-9 * max(1.0, np.abs(qo).max()), c
            assert np.abs(p1[c] - po).max() <= 1e-9 * max(1.0, np.abs(po).max()), c
        if on_device:
            witness(ctx, part, d0, d1)

    def switch():
        ctx.switch_partition()
        ctx.project_onto_cotangent_space()
        for ch in chains:
            ch.switch_partition()
            ch.project_mom()
        if after_switch is not None:
            after_switch(ctx)

    step_and_compare(0)
    switch()
    step_and_compare(1)
    switch()  # ... and back, with the arrays strided by Kmax
    step_and_compare(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fhn_128_4_2_k64_65", "fhn_130_4_2_k65_66"])
@pytest.mark.parametrize("newton", [True, False])
def test_masked_and_failing_chains_past_64_blocks(name, newton):
    """One batched step in each partition with a masked chain (active = 0) and a chain at dt = 5.0, max_iters = 3 (quasi-Newton: 8) (as
    test_hip_parity.test_failed_chains_keep_state): the unfused round masks per chain in four separate launches.  Status
    -1 and the failing status as the oracle's, both chains' states bitwise unchanged, the others to 1e-9."""
    _hip()
    cfg = CASES[name]
    case = build_case(cfg)
    ctx = make_ctx(case)
    masked_body(ctx, case, cfg, newton)
    ctx.close()


def masked_body(ctx, case, cfg, newton, dt_scale=0.25, max_iters=None, seed=16):
    from oracle import c_oracle
    B = case["B"]
    dts = dt_scale * dts_of(cfg)  # (as in switch_body)
    dts[1] = 5.0
    if max_iters is None:
        max_iters = 3 if newton else 8  # (FHN: quasi-Newton needs 4 to 7 iterations at these step sizes)
    active = np.ones(B, dtype=np.int32)
    active[3] = 0
    p_raw = np.random.default_rng(seed).standard_normal(case["q"].shape)
    for part in range(ctx.num_partition):
        ctx.set_state(case["q"], p_raw, case["x_obs"], part)
        ctx.project_onto_cotangent_space()
        q0, p0, _, _ = ctx.get_state()
        res = ctx.leapfrog_step(dts, newton=newton, max_iters=max_iters, active=active)
        q1, p1, _, _ = ctx.get_state()
        print(f"  part {part} K={ctx.K[part]} newton={newton}: status {res['status']}, iters_fwd {res['iters_fwd']}")
        assert res["status"][3] == -1
        for c in (1, 3):
            assert np.array_equal(q1[c], q0[c]) and np.array_equal(p1[c], p0[c]), c
        for c in range(B):
            if c == 3:
                continue
            ch = c_oracle.OracleChain(case["osys"])
            ch.set(case["q"][c], p0[c], case["x_obs"][c], part)
            st, itf, itb, _ = ch.step(dts[c], newton=newton, max_iters=max_iters)
            qo, po, _, _ = ch.get()
            assert res["status"][c] == st and res["iters_fwd"][c] == itf and (st != 0 or res["iters_bwd"][c] == itb), (c, res, st)
            if st == 0:
                assert np.abs(q1[c] - qo).max() <= 1e-9 * max(1.0, np.abs(qo).max()), c
                assert np.abs(p1[c] - po).max() <= 1e-9 * max(1.0, np.abs(po).max()), c
            else:
                assert np.array_equal(q1[c], q0[c]) and np.array_equal(p1[c], p0[c]), c
        assert res["status"][1] > 0 and (res["status"][[0, 2, 4]] == 0).all(), res["status"]


# The other two row families are latched per process: a child process each (as tests/test_mfma_gram_small_blocks.py starts
# its children).  Past 64 blocks they, too, take KSolveChain; their Newton rounds always use KNewtonFactor.
_FAMILY_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_ctx
import test_hip_layout_edges as le
cfg = le.CASES["fhn_128_4_2_k64_65"]
case = le.build_case(cfg)
ctx = make_ctx(case)
assert ctx.L.chmc_backend() == b"hip:gfx950" and ctx.K == [64, 65]
print("OPS_WORST", le.check_ops_against_oracle(ctx, case))
d0 = ctx.diagnostics()
for newton in (True, False):
    for part in range(2):
        print("STEPS", newton, part, le.check_steps_against_oracle(ctx, case, le.dts_of(cfg), newton=newton, n_steps=2, part=part))
d1 = ctx.diagnostics()
assert d1["newton_fsm_launches"] == 0 and d1["newton_factor8_launches"] > d0["newton_factor8_launches"], (d0, d1)
assert (d1["gram_mfma_launches"] > 0) == {mfma}, d1
print("FAMILY_OK", d1["newton_factor8_launches"], d1["gram_mfma_launches"])
ctx.close()
"""


@pytest.mark.gpu
def test_stored_row_families_past_64_blocks():
    """CHMC_COMPACT_ROWS=0, then CHMC_GRAM_MFMA=1, on FHN (128, 4, 2, noisy): operators and steps against the C oracle in
    both partitions.  One child at a time, each under a time limit; nothing is started after a failure."""
    for env, mfma in (({"CHMC_COMPACT_ROWS": "0"}, False), ({"CHMC_GRAM_MFMA": "1"}, True)):
        script = _FAMILY_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mfma=mfma)
        r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True,
                           timeout=300)
        print(env, r.stdout[-1500:])
        assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
        assert "FAMILY_OK" in r.stdout
