"""Which kernel family a layout gets (csrc/chmc_plan.h), stated on the CPU.

The plan is read through a TEST-ONLY probe (tests/emu/plan_probe.cpp, plain g++, wave kernels assumed compiled in), in a
fresh process per switch setting: the library reads its switches from the environment and latches two of them per process.

Expected values: `DEFAULT_PLANS` is written out by hand, and `parent_plan` transcribes the predicates of the commit
before the plan module existed (compact_rows, gram_mfma, compact_family, gram_mfma8, compact16, lean16, chain16,
rows_skipped, row_split_choice, few_long_blocks, par_waves_for, chain16_layout, step_fusions, mom_fix_in_jw,
rev_flow_in_update, retract_waves, traj_kernel of csrc/chmc_api.inc) and the ladders of its launch sites (now the passes of
csrc/chmc_passes.inc), one to one."""
import json
import os
import subprocess
import sys
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "manifold_mcmc_for_diffusions_amd", "csrc")
PROBE = os.path.join(HERE, "emu", "libchmc_plan_probe.so")

ROWS = ("compact", "stored", "stored_mfma")
FWD = ("k_fwd_par", "k_fwd_scan", "KFwd")
STATE = ("lean", "ivl+comb", "ivl+comb_wg", "ldsrows+gram", "ldsrows+gram_mfma", "rev_wave", "rev_wave_store+gram_mfma")
NEWTON = ("ivl+comb,fsm", "ivl+comb,factor,solve", "rev_wave,factor,solve", "rev_wave_store+gram_mfma,factor,solve",
          "ivl+comb_wg", "ivl+comb_factor", "ivl+comb,factor_wave,solve", "ldsrows+gram,factor_wave,solve",
          "ldsrows+gram_mfma,factor_wave,solve")
GLD = ("qx+lean", "ivl", "compact_fwd+ldsrows_bwd", "stored")
JP = ("k_jw_pb", "k_jw_pb_wg", "k_jw_wave")

DIMS = {"fhn": (2, 2, 4, 2), "fhn_nb": (2, 2, 4, 2), "sir": (3, 3, 4, 1)}  # X, V, Z, V0 (csrc/models_gen.h)


def layout(model, T, S, R, noisy, gaussian=False, varsig=False, chains=256, cus=256):
    """The integers chmc_create hands to the plan, from the block shape tables of the reference (build_partition)."""
    X, V, Z, V0 = DIMS[model]

    def blocks(init):
        if R is None or R <= 0 or R >= T:
            return [T]
        full, rem = divmod(T - init, R)
        return [init] + [R] * (full - 1 if rem == 0 else full) + [R if rem == 0 else rem]

    parts = [blocks(R)] if R is None or R <= 0 or R >= T else [blocks(R), blocks(R // 2)]
    rmax = 0
    for sizes in parts:
        for b, nobs in enumerate(sizes):
            last = b + 1 == len(sizes)
            rmax = max(rmax, (nobs if (last or noisy) else nobs - 1) + (0 if last else X))
    rmt = 8 if rmax <= 8 else 16
    if model != "sir" and not varsig and (rmax == 6 or (rmax == 7 and model == "fhn")):
        rmt = rmax
    U, NV = Z + int(varsig), V0 + T * S * V
    Q = U + NV + (T if noisy else 0)
    K = [len(s) for s in parts]
    return dict(rmt=rmt, npart=len(parts), K=K + K[:1] * (2 - len(K)), longest=max(max(s) for s in parts) * S,
                chain_steps=T * S, tiles8=S % 8 == 0, V=V, even=not ((Q | U | V0 | NV) & 1), gaussian=gaussian,
                chains=chains, cus=cus)


LAYOUTS = {
    "configs0_fhn_noisy_S50": layout("fhn", 100, 50, 5, True, chains=1),
    "configs1_fhn_noisy_S400": layout("fhn", 100, 400, 5, True),
    "configs2_fhn_noiseless_S400": layout("fhn", 100, 400, 5, False),
    "configs3_sir_S200_shard": layout("sir", 14, 200, 14, True),
    "configs4_fhn_noisy_S800_shard": layout("fhn", 100, 800, 5, True, chains=512),
    "fhn_noisy_R5_small": layout("fhn", 12, 10, 5, True, chains=4),
    "fhn_noiseless_R5_gaussian": layout("fhn", 12, 10, 5, False, gaussian=True, chains=4),
    "fhn_notebook": layout("fhn_nb", 100, 25, 5, False, gaussian=True, chains=4),
    "sir_14obs_single_block": layout("sir", 14, 6, 14, True, chains=3),
    "sir_single_block_2048_chains": layout("sir", 14, 200, 14, True, chains=2048),
    "sir_partitioned_8rows": layout("sir", 6, 8, 2, True, chains=3),
    "sir_16rows_7blocks": layout("sir", 60, 8, 10, True, chains=8),
    "sir_16rows_4blocks": layout("sir", 30, 8, 10, True, chains=8),
    "fhn_varsig": layout("fhn", 12, 10, 5, True, varsig=True, chains=4),
    "sir_varsig": layout("sir", 14, 6, 14, True, varsig=True, chains=3),
    # 64 blocks per chain and beyond (tests/test_hip_layout_edges.py runs them on the GPU)
    "fhn_k64_65": layout("fhn", 128, 4, 2, True, chains=5),
    "fhn_k65_66_rm7": layout("fhn", 325, 8, 5, True, chains=5),
    "sir_k66_67": layout("sir", 132, 4, 2, True, chains=5),
    # 16 row slots with 4 | 5 blocks per chain, and few long blocks with K > 1 (tests/test_hip_multiblock16.py runs them on the GPU)
    "sir16_k4_5": layout("sir", 40, 8, 10, True, chains=5),
    "sir16_long_k3_4": layout("sir", 39, 80, 13, True, chains=5),
    "fhn_long_k2_3": layout("fhn", 4, 512, 2, True, chains=5),
    "fhn_long_w2_k2_3": layout("fhn", 4, 1024, 2, True, chains=5),
}

SWITCHES = [{}, {"CHMC_COMPACT_ROWS": "0"}, {"CHMC_GRAM_MFMA": "1"}, {"CHMC_PAR_SCAN": "0"}, {"CHMC_PAR_SCAN": "1"},
            {"CHMC_PAR_WAVES": "1"}, {"CHMC_PAR_WAVES": "2"}, {"CHMC_PAR_WAVES": "4"}, {"CHMC_ROW_SPLIT": "1"},
            {"CHMC_ROW_SPLIT": "4"}, {"CHMC_NO_FWD_SCAN": "1"}, {"CHMC_STEP_FUSIONS": "0"}]
ALL_SWITCHES = ("CHMC_COMPACT_ROWS", "CHMC_GRAM_MFMA", "CHMC_PAR_SCAN", "CHMC_PAR_WAVES", "CHMC_ROW_SPLIT", "CHMC_HALVES",
                "CHMC_NO_FWD_SCAN", "CHMC_STEP_FUSIONS", "CHMC_RETRACT_KERNEL")


def parent_plan(L, env):
    """The parent commit's predicates and launch ladders, transcribed (wave kernels compiled in)."""
    get = env.get
    compact_rows = int(get("CHMC_COMPACT_ROWS", 1)) != 0
    gram_mfma = int(get("CHMC_GRAM_MFMA", 0)) != 0
    rmt, kmax = L["rmt"], max(L["K"][:L["npart"]])
    has_pb = compact_rows and not (gram_mfma and rmt <= 8)  # compact_family: Slots::PB allocated
    gram_mfma8 = gram_mfma and rmt <= 8 and not has_pb
    compact16 = has_pb and not gram_mfma
    chain16_layout = kmax == 1 and rmt > 8

    def few_long_blocks(nblocks, longest):
        return nblocks <= 4 and longest >= 1024

    def par_waves_for(longest):
        v = int(get("CHMC_PAR_WAVES", 0))
        return v if v in (1, 2, 4) else 4 if longest >= 4096 else 2 if longest >= 2048 else 1

    if "CHMC_PAR_SCAN" in env:
        par_scan = int(env["CHMC_PAR_SCAN"]) != 0
    else:
        par_scan = few_long_blocks(kmax, L["longest"]) or (chain16_layout and compact_rows and not gram_mfma)
    par_waves = 4 if chain16_layout and "CHMC_PAR_WAVES" not in env else par_waves_for(L["longest"])
    seq = "k_fwd_scan" if L["tiles8"] and "CHMC_NO_FWD_SCAN" not in env else "KFwd"
    nld_par = int(env["CHMC_PAR_SCAN"]) != 0 if "CHMC_PAR_SCAN" in env else few_long_blocks(1, L["chain_steps"])
    step_fusions = has_pb and not (get("CHMC_STEP_FUSIONS") is not None and int(get("CHMC_STEP_FUSIONS")) == 0)
    plan = dict(rows="compact" if (has_pb if rmt <= 8 else compact16) else "stored_mfma" if gram_mfma else "stored",
                pb_allocated=has_pb, par_scan=par_scan, fwd="k_fwd_par" if par_scan else seq, fwd_cold=seq,
                fwd_waves=par_waves, nld="k_fwd_par" if nld_par else "k_fwd_scan" if L["tiles8"] else "KFwd",
                nld_waves=par_waves_for(L["chain_steps"]),
                mom_fix_in_jp=step_fusions and rmt <= 8 and L["V"] == 2 and L["even"],
                rev_flow_in_update=step_fusions and rmt <= 8 and not L["gaussian"], part=[])
    for p in range(L["npart"]):
        K = L["K"][p]
        env_split = int(get("CHMC_ROW_SPLIT", 0))
        row_split = env_split if env_split in (1, 2, 4) else (4 if K <= 4 else 1)
        lean16 = rmt > 8 and compact16 and row_split > 1
        chain16 = chain16_layout and compact16 and lean16
        rows_skipped = has_pb and (rmt <= 8 or lean16)
        compact = has_pb if rmt <= 8 else compact16
        if rmt > 8:  # state_eval_core
            state = ("ivl+comb_wg" if chain16 else "ivl+comb") if lean16 else \
                ("ldsrows+gram_mfma" if gram_mfma else "ldsrows+gram")
            gld = "ivl" if lean16 else "compact_fwd+ldsrows_bwd" if compact16 else "stored"
        else:
            state = "lean" if rows_skipped else "rev_wave_store+gram_mfma" if gram_mfma8 else "rev_wave"
            gld = "qx+lean" if has_pb else "stored"
        fused = rmt <= 8 and K <= 64 and has_pb  # iteration_after_scan, newton
        fused16 = rmt > 8 and K == 1 and compact16
        if rmt > 8:
            if compact16:
                newton = "ivl+comb_wg" if fused16 and chain16 else "ivl+comb_factor" if fused16 else \
                    "ivl+comb,factor_wave,solve"
            else:
                newton = "ldsrows+gram_mfma,factor_wave,solve" if gram_mfma else "ldsrows+gram,factor_wave,solve"
        elif has_pb:
            newton = "ivl+comb,fsm" if fused else "ivl+comb,factor,solve"
        else:
            newton = "rev_wave_store+gram_mfma,factor,solve" if gram_mfma8 else "rev_wave,factor,solve"
        jp = "k_jw_pb_wg" if rmt > 8 and chain16 else "k_jw_pb" if compact else "k_jw_wave"
        if "CHMC_RETRACT_KERNEL" in env:
            want = int(env["CHMC_RETRACT_KERNEL"])
        else:
            want = 1 if L["chains"] <= L["cus"] else 2 if L["chains"] <= 4 * L["cus"] else 0
        if not (K == 1 and rmt > 8 and compact16):
            want = 0
        retract = 8 if want == 1 else 4 if want == 2 else 0
        plan["part"].append(dict(state=state, newton=newton, gld=gld, jp=jp, rebuild_rows=rows_skipped,
                                 retract_waves=retract, traj_waves=retract if lean16 else 0))
    return plan


def _part(state, newton, gld, jp, rebuild_rows, retract_waves=0, traj_waves=0):
    return dict(state=state, newton=newton, gld=gld, jp=jp, rebuild_rows=rebuild_rows, retract_waves=retract_waves,
                traj_waves=traj_waves)


def _plan(fwd, fwd_waves, nld, nld_waves, mom_fix, rev_flow, *parts, par_scan=False, fwd_cold=None):
    return dict(rows="compact", pb_allocated=True, par_scan=par_scan, fwd=fwd, fwd_cold=fwd_cold or fwd, fwd_waves=fwd_waves,
                nld=nld, nld_waves=nld_waves, mom_fix_in_jp=mom_fix, rev_flow_in_update=rev_flow, part=list(parts))


_FHN = _part("lean", "ivl+comb,fsm", "qx+lean", "k_jw_pb", True)
_COMB = _part("lean", "ivl+comb,factor,solve", "qx+lean", "k_jw_pb", True)  # more than 64 blocks per chain: the unfused round
_SIR1 = dict(par_scan=True, fwd_cold="k_fwd_scan")
DEFAULT_PLANS = {  # no switch set: every layout is on the compact rows
    "configs0_fhn_noisy_S50": _plan("KFwd", 1, "k_fwd_par", 4, True, True, _FHN, _FHN),
    "configs1_fhn_noisy_S400": _plan("k_fwd_scan", 1, "k_fwd_par", 4, True, True, _FHN, _FHN),
    "configs2_fhn_noiseless_S400": _plan("k_fwd_scan", 1, "k_fwd_par", 4, True, True, _FHN, _FHN),
    "configs3_sir_S200_shard": _plan("k_fwd_par", 4, "k_fwd_par", 2, False, False,
                                     _part("ivl+comb_wg", "ivl+comb_wg", "ivl", "k_jw_pb_wg", True, 8, 8), **_SIR1),
    "configs4_fhn_noisy_S800_shard": _plan("k_fwd_scan", 2, "k_fwd_par", 4, True, True, _FHN, _FHN),
    "fhn_noisy_R5_small": _plan("KFwd", 1, "KFwd", 1, True, True, _FHN, _FHN),
    "fhn_noiseless_R5_gaussian": _plan("KFwd", 1, "KFwd", 1, True, False, _FHN, _FHN),
    "fhn_notebook": _plan("KFwd", 1, "k_fwd_par", 2, True, False, _FHN, _FHN),
    "sir_14obs_single_block": _plan("k_fwd_par", 4, "KFwd", 1, False, False,
                                    _part("ivl+comb_wg", "ivl+comb_wg", "ivl", "k_jw_pb_wg", True, 8, 8), par_scan=True,
                                    fwd_cold="KFwd"),
    "sir_single_block_2048_chains": _plan("k_fwd_par", 4, "k_fwd_par", 2, False, False,
                                          _part("ivl+comb_wg", "ivl+comb_wg", "ivl", "k_jw_pb_wg", True, 0, 0), **_SIR1),
    "sir_partitioned_8rows": _plan("k_fwd_scan", 1, "k_fwd_scan", 1, False, True, _FHN, _FHN),
    "sir_16rows_7blocks": _plan("k_fwd_scan", 1, "k_fwd_scan", 1, False, False,
                                *[_part("ldsrows+gram", "ivl+comb,factor_wave,solve", "compact_fwd+ldsrows_bwd", "k_jw_pb",
                                        False)] * 2),
    "sir_16rows_4blocks": _plan("k_fwd_scan", 1, "k_fwd_scan", 1, False, False,
                                *[_part("ivl+comb", "ivl+comb,factor_wave,solve", "ivl", "k_jw_pb", True)] * 2),
    "fhn_varsig": _plan("KFwd", 1, "KFwd", 1, False, True, _FHN, _FHN),
    "sir_varsig": _plan("k_fwd_par", 4, "KFwd", 1, False, False,
                        _part("ivl+comb_wg", "ivl+comb_wg", "ivl", "k_jw_pb_wg", True, 8, 8), par_scan=True, fwd_cold="KFwd"),
    "fhn_k64_65": _plan("KFwd", 1, "KFwd", 1, True, True, _FHN, _COMB),
    "fhn_k65_66_rm7": _plan("k_fwd_scan", 1, "k_fwd_par", 2, False, True, _COMB, _COMB),
    "sir_k66_67": _plan("KFwd", 1, "KFwd", 1, False, True, _COMB, _COMB),
    # K = [4, 5], 16 row slots: at most 4 blocks per chain take the interval-parallel state evaluation and rebuild the rows on
    # demand, 5 blocks keep the rows of k_rev_wave_ldsrows -- in the same context; the Newton round is the same in both
    "sir16_k4_5": _plan("k_fwd_scan", 1, "k_fwd_scan", 1, False, False,
                        _part("ivl+comb", "ivl+comb,factor_wave,solve", "ivl", "k_jw_pb", True),
                        _part("ldsrows+gram", "ivl+comb,factor_wave,solve", "compact_fwd+ldsrows_bwd", "k_jw_pb", False)),
    # few_long_blocks (K <= 4, longest block >= 1024 steps) with several blocks per chain: the time-parallel scan, one wavefront
    # per block below 2048 steps, two from there; the comparator's one block of T S steps: 3120 and 2048 steps 2 wavefronts, 4096 4
    "sir16_long_k3_4": _plan("k_fwd_par", 1, "k_fwd_par", 2, False, False,
                             *[_part("ivl+comb", "ivl+comb,factor_wave,solve", "ivl", "k_jw_pb", True)] * 2, par_scan=True,
                             fwd_cold="k_fwd_scan"),
    "fhn_long_k2_3": _plan("k_fwd_par", 1, "k_fwd_par", 2, True, True, _FHN, _FHN, par_scan=True, fwd_cold="k_fwd_scan"),
    "fhn_long_w2_k2_3": _plan("k_fwd_par", 2, "k_fwd_par", 4, True, True, _FHN, _FHN, par_scan=True, fwd_cold="k_fwd_scan"),
}

_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
res = {}
for name, v in json.loads(sys.argv[2]).items():
    ins = (ctypes.c_int * 12)(*v)
    out = (ctypes.c_int * 32)()
    n = lib.chmc_plan_probe(ins, out)
    res[name] = list(out[:n])
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def probe():
    srcs = [os.path.join(HERE, "emu", "plan_probe.cpp"), os.path.join(CSRC, "chmc_plan.h")]
    if not os.path.exists(PROBE) or any(os.path.getmtime(PROBE) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", PROBE,
                               "plan_probe.cpp"], cwd=os.path.join(HERE, "emu"))
    return PROBE


def probe_plans(probe, env):
    ins = {name: [L["rmt"], L["npart"], L["K"][0], L["K"][1], L["longest"], L["chain_steps"], int(L["tiles8"]), L["V"],
                  int(L["even"]), int(L["gaussian"]), L["chains"], L["cus"]] for name, L in LAYOUTS.items()}
    clean = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    r = subprocess.run([sys.executable, "-c", _CHILD, probe, json.dumps(ins)], env={**clean, **env}, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plans = {}
    for name, o in json.loads(r.stdout).items():
        parts = [dict(state=STATE[s], newton=NEWTON[n], gld=GLD[g], jp=JP[j], rebuild_rows=bool(rr), retract_waves=rw,
                      traj_waves=tw) for s, n, g, j, rr, rw, tw in zip(*[iter(o[10:])] * 7)]
        plans[name] = dict(rows=ROWS[o[0]], pb_allocated=bool(o[1]), par_scan=bool(o[2]), fwd=FWD[o[3]], fwd_cold=FWD[o[4]],
                           fwd_waves=o[5], nld=FWD[o[6]], nld_waves=o[7], mom_fix_in_jp=bool(o[8]),
                           rev_flow_in_update=bool(o[9]), part=parts)
    return plans


def test_layout_integers():
    assert LAYOUTS["configs1_fhn_noisy_S400"] == dict(rmt=7, npart=2, K=[20, 21], longest=2000, chain_steps=40000,
                                                      tiles8=True, V=2, even=True, gaussian=False, chains=256, cus=256)
    assert LAYOUTS["configs2_fhn_noiseless_S400"]["rmt"] == 6 and LAYOUTS["fhn_notebook"]["rmt"] == 6
    assert LAYOUTS["configs3_sir_S200_shard"] == dict(rmt=16, npart=1, K=[1, 1], longest=2800, chain_steps=2800, tiles8=True,
                                                      V=3, even=False, gaussian=False, chains=256, cus=256)
    assert LAYOUTS["sir_partitioned_8rows"]["K"] == [3, 4] and LAYOUTS["sir_partitioned_8rows"]["rmt"] == 8
    assert LAYOUTS["sir_16rows_7blocks"]["K"] == [6, 7] and LAYOUTS["sir_16rows_4blocks"]["K"] == [3, 4]
    assert LAYOUTS["fhn_varsig"]["rmt"] == 8 and not LAYOUTS["fhn_varsig"]["even"]
    assert LAYOUTS["fhn_k64_65"]["K"] == [64, 65] and LAYOUTS["fhn_k64_65"]["rmt"] == 8
    assert LAYOUTS["fhn_k65_66_rm7"]["K"] == [65, 66] and LAYOUTS["fhn_k65_66_rm7"]["rmt"] == 7
    assert LAYOUTS["sir_k66_67"]["K"] == [66, 67] and LAYOUTS["sir_k66_67"]["rmt"] == 8
    assert LAYOUTS["sir16_k4_5"] == dict(rmt=16, npart=2, K=[4, 5], longest=80, chain_steps=320, tiles8=True, V=3, even=False,
                                         gaussian=False, chains=5, cus=256)
    assert LAYOUTS["sir16_long_k3_4"]["K"] == [3, 4] and LAYOUTS["sir16_long_k3_4"]["longest"] == 1040
    assert LAYOUTS["sir16_long_k3_4"]["rmt"] == 16 and LAYOUTS["sir16_long_k3_4"]["chain_steps"] == 3120
    assert LAYOUTS["fhn_long_k2_3"]["K"] == [2, 3] and (LAYOUTS["fhn_long_k2_3"]["longest"], LAYOUTS["fhn_long_k2_3"]["rmt"]) == (1024, 8)
    assert LAYOUTS["fhn_long_w2_k2_3"]["K"] == [2, 3] and LAYOUTS["fhn_long_w2_k2_3"]["longest"] == 2048


def test_default_plans_by_hand(probe):
    got = probe_plans(probe, {})
    assert set(got) == set(DEFAULT_PLANS)
    for name in LAYOUTS:
        assert got[name] == DEFAULT_PLANS[name], name
    # K = [64, 65]: the wavefront-per-chain round (NewtonIvlFsm) holds one block per lane, so 64 blocks are its last layout
    # and the 65 blocks of the other partition take the unfused round (NewtonIvlComb) -- in the same context
    assert [pp["newton"] for pp in got["fhn_k64_65"]["part"]] == ["ivl+comb,fsm", "ivl+comb,factor,solve"]
    # K = [4, 5] with 16 row slots: both state evaluations in one context
    assert [(pp["state"], pp["rebuild_rows"]) for pp in got["sir16_k4_5"]["part"]] == [("ivl+comb", True), ("ldsrows+gram", False)]
    # the time-parallel scan never pairs retractions and is the only scan with more than one wavefront per block
    for name in ("sir16_long_k3_4", "fhn_long_k2_3", "fhn_long_w2_k2_3"):
        assert got[name]["par_scan"] and got[name]["fwd"] == "k_fwd_par" and got[name]["fwd_cold"] == "k_fwd_scan", name


@pytest.mark.parametrize("env", SWITCHES + [{"CHMC_COMPACT_ROWS": "0", "CHMC_GRAM_MFMA": "1"}, {"CHMC_RETRACT_KERNEL": "0"},
                                            {"CHMC_RETRACT_KERNEL": "1"}, {"CHMC_RETRACT_KERNEL": "2"},
                                            {"CHMC_PAR_WAVES": "3"}],
                         ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()) or "default")
def test_plan_equals_the_parent_predicates(probe, env):
    got = probe_plans(probe, env)
    for name, L in LAYOUTS.items():
        assert got[name] == parent_plan(L, env), (name, env)


def test_switches_select_the_documented_families(probe):
    """A few switch settings spelled out, so that the transcription above is not the only witness."""
    stored = probe_plans(probe, {"CHMC_COMPACT_ROWS": "0"})
    for name, L in LAYOUTS.items():
        p = stored[name]
        assert p["rows"] == "stored" and not p["pb_allocated"] and not p["mom_fix_in_jp"] and not p["rev_flow_in_update"]
        for pp in p["part"]:
            assert pp["jp"] == "k_jw_wave" and pp["gld"] == "stored" and not pp["rebuild_rows"] and pp["retract_waves"] == 0
            assert pp["state"] == ("ldsrows+gram" if L["rmt"] > 8 else "rev_wave")
            assert pp["newton"] == ("ldsrows+gram,factor_wave,solve" if L["rmt"] > 8 else "rev_wave,factor,solve")
    mfma = probe_plans(probe, {"CHMC_GRAM_MFMA": "1"})
    for name, L in LAYOUTS.items():
        p = mfma[name]
        assert p["rows"] == "stored_mfma" and p["pb_allocated"] == (L["rmt"] > 8)
        for pp in p["part"]:
            assert pp["state"] == ("ldsrows+gram_mfma" if L["rmt"] > 8 else "rev_wave_store+gram_mfma")
            assert pp["jp"] == "k_jw_wave" and pp["retract_waves"] == 0
    split1 = probe_plans(probe, {"CHMC_ROW_SPLIT": "1"})["configs3_sir_S200_shard"]["part"][0]
    assert split1 == _part("ldsrows+gram", "ivl+comb_factor", "compact_fwd+ldsrows_bwd", "k_jw_pb", False, 8, 0)
    split4 = probe_plans(probe, {"CHMC_ROW_SPLIT": "4"})["sir_16rows_7blocks"]["part"]
    assert split4 == [_part("ivl+comb", "ivl+comb,factor_wave,solve", "ivl", "k_jw_pb", True)] * 2
    nofwd = probe_plans(probe, {"CHMC_NO_FWD_SCAN": "1"})
    assert nofwd["configs1_fhn_noisy_S400"]["fwd"] == "KFwd" and nofwd["configs3_sir_S200_shard"]["fwd"] == "k_fwd_par"
    assert nofwd["configs3_sir_S200_shard"]["fwd_cold"] == "KFwd" and nofwd["configs3_sir_S200_shard"]["nld"] == "k_fwd_par"
    nofuse = probe_plans(probe, {"CHMC_STEP_FUSIONS": "0"})
    assert not any(p["mom_fix_in_jp"] or p["rev_flow_in_update"] for p in nofuse.values())
    seq = probe_plans(probe, {"CHMC_PAR_SCAN": "0"})["configs3_sir_S200_shard"]
    assert seq["fwd"] == "k_fwd_scan" and seq["nld"] == "k_fwd_scan" and seq["part"][0]["retract_waves"] == 8  # 
    for w in (1, 2, 4):
        p = probe_plans(probe, {"CHMC_PAR_WAVES": str(w)})
        assert p["configs3_sir_S200_shard"]["fwd_waves"] == w and p["configs1_fhn_noisy_S400"]["nld_waves"] == w
