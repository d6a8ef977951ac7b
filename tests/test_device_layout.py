"""The list of per-chain device arrays (csrc/chmc_layout.h), stated on the CPU.

chmc_create allocates, and a half-batch view offsets, by walking that one list.  The list is read through a TEST-ONLY probe
(tests/emu/layout_probe.cpp, plain g++) in a fresh process per switch setting (two switches are latched per process).

`PARENT` is what chmc_create of commit 4d66d32 -- the last one with hand-written allocations -- asked of the device for three
layouts with 7 chains: every allocation as (bytes, zeroed at creation), recorded from a build of THAT commit's emulation
library whose dev_alloc / dev_zero logged their sizes.  The list plus the shared arrays named in chmc_layout.h must reproduce
it allocation for allocation.  The emulation build has no wave kernels, so the arrays that only exist with them (Slots::PB, LF,
work.gcq, gbw) and work.JvW are stated by hand below, for the default switches and for CHMC_GRAM_MFMA=1."""
import collections
import json
import os
import subprocess
import sys
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "manifold_mcmc_for_diffusions_amd", "csrc")
PROBE = os.path.join(HERE, "emu", "liblayout_probe.so")
B = 7
KIND_ZEROED, KIND_LAZY, KIND_ABSENT = 1, 2, 4
SWITCHES = ("CHMC_COMPACT_ROWS", "CHMC_GRAM_MFMA", "CHMC_PAR_SCAN", "CHMC_PAR_WAVES", "CHMC_ROW_SPLIT", "CHMC_HALVES",
            "CHMC_NO_FWD_SCAN", "CHMC_STEP_FUSIONS", "CHMC_RETRACT_KERNEL")

# T, S, noisy, U, X, V, Z, V0, blocks per chain by partition, row slots RM, most observations in a block
LAYOUTS = {
    "fhn_12_16_5_noisy": dict(T=12, S=16, noisy=1, U=4, X=2, V=2, Z=4, V0=2, K=[3, 3], RM=7, NOBS=5),   # blocks 5 5 2 | 2 5 5
    "sir_14_8_14": dict(T=14, S=8, noisy=1, U=4, X=3, V=3, Z=4, V0=1, K=[1], RM=16, NOBS=14),
    "sir_26_24_13": dict(T=26, S=24, noisy=1, U=4, X=3, V=3, Z=4, V0=1, K=[2, 3], RM=16, NOBS=13),      # blocks 13 13 | 6 13 7
}

# commit 4d66d32, emulation build: {(bytes, zeroed): number of such allocations}, allocations, bytes, bytes zeroed
PARENT = {
    "fhn_12_16_5_noisy": ({(28, 0): 5, (28, 1): 1, (40, 0): 2, (48, 0): 3, (52, 0): 2, (56, 0): 4, (56, 1): 3, (84, 0): 2,
                           (96, 0): 1, (112, 0): 1, (144, 0): 3, (168, 0): 2, (224, 0): 1, (512, 1): 1, (672, 0): 2, (896, 0): 4,
                           (1176, 0): 1, (1176, 1): 4, (1344, 1): 1, (2048, 1): 1, (2352, 0): 1, (2688, 0): 1, (4704, 0): 9,
                           (8232, 0): 4, (22512, 0): 5, (22512, 1): 4, (24560, 1): 3, (26880, 0): 3, (150528, 0): 1,
                           (151312, 1): 2}, 77, 907352, 475156),
    "sir_14_8_14": ({(16, 0): 1, (20, 0): 1, (28, 0): 6, (28, 1): 1, (48, 0): 2, (56, 0): 7, (56, 1): 3, (112, 0): 2, (144, 0): 1,
                     (224, 0): 3, (512, 1): 1, (896, 0): 6, (896, 1): 4, (2048, 1): 1, (2352, 1): 1, (2688, 0): 1, (3584, 0): 9,
                     (14336, 0): 4, (19880, 0): 5, (19880, 1): 4, (21504, 0): 3, (21928, 1): 3, (301056, 0): 1, (301952, 1): 3},
                    73, 1624216, 1059852),
    "sir_26_24_13": ({(28, 0): 6, (28, 1): 1, (36, 0): 1, (40, 0): 1, (48, 0): 1, (52, 0): 1, (56, 0): 5, (56, 1): 3, (84, 0): 1,
                      (96, 0): 1, (104, 0): 2, (112, 0): 1, (144, 0): 2, (168, 0): 2, (208, 0): 1, (224, 0): 1, (512, 1): 1,
                      (672, 0): 2, (896, 0): 4, (2048, 1): 1, (2688, 0): 2, (2688, 1): 4, (4368, 1): 1, (8064, 0): 1, (10752, 0): 9,
                      (43008, 0): 4, (106568, 0): 5, (106568, 1): 4, (108616, 1): 3, (112896, 0): 3, (1677312, 0): 1,
                      (1678208, 1): 3}, 78, 8642808, 5804620),
}

# Elements per chain of Slots::PB [T S][X V], Slots::LF [Kmax][NOBS][RM][X], work.gcq [Kmax][NOBS][2 X X + X Z], work.gbw
# [Kmax][NOBS][X + 2 Z] and work.JvW [RM][NV] in the shipped library (wave kernels), by hand; 0: the context has none.
#   default switches: PB / LF everywhere; gcq, gbw and JvW with 16 row slots only
#   CHMC_GRAM_MFMA=1: blocks of at most 8 rows lose PB / LF and get JvW; 16-row blocks keep everything
FIVE = {
    "fhn_12_16_5_noisy": {"": (192 * 4, 3 * 5 * 7 * 2, 0, 0, 0), "CHMC_GRAM_MFMA": (0, 0, 0, 0, 7 * 386)},
    "sir_14_8_14": {"": (112 * 9, 14 * 16 * 3, 14 * 30, 14 * 11, 16 * 337), "CHMC_GRAM_MFMA": (112 * 9, 14 * 16 * 3, 14 * 30, 14 * 11, 16 * 337)},
    "sir_26_24_13": {"": (624 * 9, 39 * 16 * 3, 39 * 30, 39 * 11, 16 * 1873),
                     "CHMC_GRAM_MFMA": (624 * 9, 39 * 16 * 3, 39 * 30, 39 * 11, 16 * 1873)},
}

_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
res = {}
for name, v in json.loads(sys.argv[2]).items():
    ins = (ctypes.c_int * 13)(*v)
    out = (ctypes.c_longlong * 1024)()
    n = lib.chmc_layout_probe(ins, out)
    assert 5 + 4 * n <= 1024
    res[name] = list(out[:5 + 4 * n])
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def probe():
    srcs = [os.path.join(HERE, "emu", "layout_probe.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(PROBE) or any(os.path.getmtime(PROBE) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", PROBE,
                               "layout_probe.cpp"], cwd=os.path.join(HERE, "emu"))
    return PROBE


def probe_lists(probe, env, wave_kernels):
    ins = {}
    for name, L in LAYOUTS.items():
        Q = L["U"] + L["V0"] + L["T"] * L["S"] * L["V"] + (L["T"] if L["noisy"] else 0)
        groups = ((Q + 1) // 2 + 2047) // 2048  # rowsum_groups: 4 096 columns per group of the row sums
        ins[name] = [L["T"], L["S"], L["noisy"], L["U"], L["X"], L["V"], L["Z"], L["V0"], max(L["K"]), L["RM"], L["NOBS"],
                     groups, int(wave_kernels)]
    clean = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-c", _CHILD, probe, json.dumps(ins)], env={**clean, **env}, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {}
    for name, o in json.loads(r.stdout).items():
        out[name] = (tuple(o[:5]), [tuple(o[i:i + 4]) for i in range(5, len(o), 4)])  # (per chain, slack, bytes each, kind)
    return out


def shared_allocations(L):
    """The allocations of chmc_create that are NOT per chain (named in the header comment of chmc_layout.h), by hand."""
    T = L["T"]
    shared = []
    for K in L["K"]:  # per partition: block table (12 ints per block), observation -> block, work orders (batch, halves 3 | 4)
        shared += [(48 * K, 0), (4 * T, 0), (4 * B * K, 0), (4 * ((B // 2) * K + 1), 0), (4 * ((B - B // 2) * K + 1), 0)]
    shared.append((8 * T, 0))                            # d_y
    shared.append((8 * (B + (3 * B * 4 + 7) // 8), 0))   # d_out: [rev (8 B) | status | iters_fwd | iters_bwd] x B
    shared += [(4 * 12, 0), (8 * 256, 1), (4 * 128, 1)]  # work.n_active, work.zeros, work.nfallback
    shared.append((8 * B * 4, 0))                        # d_ham
    return shared


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_allocations_equal_the_hand_written_ones(probe, name):
    _, arrays = probe_lists(probe, {}, wave_kernels=False)[name]
    got = shared_allocations(LAYOUTS[name])
    for per_chain, slack, size, kind in arrays:
        if not kind & (KIND_LAZY | KIND_ABSENT):
            got.append(((B * per_chain + slack) * size, int(bool(kind & KIND_ZEROED))))
    counts, n, total, zeroed = PARENT[name]
    assert sum(counts.values()) == n and sum(b * k for (b, _), k in counts.items()) == total  # (the record is consistent)
    assert len(got) == n and sum(b for b, _ in got) == total and sum(b for b, z in got if z) == zeroed
    assert dict(collections.Counter(got)) == counts


@pytest.mark.parametrize("switch", ["", "CHMC_GRAM_MFMA"])
def test_arrays_that_depend_on_the_kernel_family(probe, switch):
    got = probe_lists(probe, {switch: "1"} if switch else {}, wave_kernels=True)
    for name in LAYOUTS:
        assert got[name][0] == FIVE[name][switch], (name, switch)


def test_lazy_arrays_are_in_the_list(probe):
    """d_q0, d_p0, d_qbak, d_pbak [Q] and d_ncommit, d_nsteps, d_ndone [1]: sized by the list, allocated on first use."""
    for name, L in LAYOUTS.items():
        Q = L["U"] + L["V0"] + L["T"] * L["S"] * L["V"] + L["T"]
        lazy = sorted(a[:3] for a in probe_lists(probe, {}, wave_kernels=True)[name][1] if a[3] & KIND_LAZY)
        assert lazy == sorted([(Q, 0, 8)] * 4 + [(1, 0, 4)] * 3), name
