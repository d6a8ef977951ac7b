"""CPU screening of the cases of tests/test_hip_layout_edges.py, tests/test_hip_multiblock16.py and tests/test_hip_fhn16.py (a
case id is looked up in all three tables): runs the module's run_case on the TEST-ONLY emulation build with every C-oracle step traced, and reports per case
whether
  * every oracle step ended with status 0, and in how many iterations,
  * any retraction residual (|c| against constraint_tol 1e-9, |dq| against position_tol 1e-8) of any iteration of any chain
    lies within 1e-2 relative of its tolerance -- the condition of test_hip_autodiff_parity.reference_side under which
    "equal iteration counts" is a fair demand on the library.
A seed that fails is replaced in the test module and noted there.  The other bodies of the modules that use a case
(partition switches, masked and failing chains, trajectories, the block metric of tests/test_hip_fhn16.py) run after it, traced the same way; their chain at dt = 5.0 fails
by design, so only the steps of run_case must all end with status 0.

    python tools/screen_layout_edges.py [case id | case id:seed to try ...]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ctypes  # noqa: E402
import subprocess  # noqa: E402
import numpy as np  # noqa: E402
from oracle import c_oracle  # noqa: E402
from manifold_mcmc_for_diffusions_amd import _lib  # noqa: E402
import test_hip_layout_edges as le  # noqa: E402
import test_hip_multiblock16 as mb  # noqa: E402
import test_hip_fhn16 as f16  # noqa: E402
from helpers import make_ctx, check_block_metric_against_oracle  # noqa: E402

EDGE = 1e-2


def use_emulation_build():
    emu = os.path.join(ROOT, "tests", "emu")
    so = os.path.join(emu, "libchmc_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I.", "-o", so, "chmc_emu.cpp"], cwd=emu)
    _lib._LIB = _lib._bind(ctypes.CDLL(so))
    assert _lib.lib().chmc_backend() == b"emu:host-TEST-ONLY"


def main(names):
    use_emulation_build()
    log = []
    plain_step = c_oracle.OracleChain.step

    def traced_step(self, dt, **kw):
        out = plain_step(self, dt, **kw)
        near = []
        for d in (0, 1):
            err, ndq = self.trace(d)
            near += [(d, float(e), float(n)) for e, n in zip(err, ndq)
                     if abs(e - 1e-9) <= EDGE * 1e-9 or abs(n - 1e-8) <= EDGE * 1e-8]
        log.append((out[0], out[1], out[2], near))
        return out

    c_oracle.OracleChain.step = traced_step
    bad = []
    for name in names:
        name, _, seed = name.partition(":")
        mod = f16 if name in f16.CASES else mb if name in mb.CASES else le
        cfg = mod.CASES[name][:12] + (int(seed) if seed else mod.CASES[name][12],)
        del log[:]
        t0 = time.time()
        case = le.build_case(cfg)
        ctx = make_ctx(case)
        try:
            mod.run_case(ctx, case, cfg, on_device=False)
            err = None
        except AssertionError as e:  # (the emulation build's own mismatch, if any, is reported and the screening goes on)
            err = str(e)[:300]
        n_case = len(log)
        if err is None and name in ("fhn_128_4_2_k64_65", "fhn_130_4_2_k65_66"):  # the other tests on these two cases
            if name == "fhn_128_4_2_k64_65":
                le.switch_body(ctx, case, cfg, on_device=False)
                assert all(st == 0 for st, _, _, _ in log[n_case:])
            for newton in (True, False):
                le.masked_body(ctx, case, cfg, newton)  # (one chain fails by design)
        if err is None and mod is mb:
            try:
                if name == "sir16_k4_5":
                    mb.switch_16(ctx, case, cfg, on_device=False)
                    assert all(st == 0 for st, _, _, _ in log[n_case:])
                n_switch = len(log)
                if name in ("sir16_k4_5", "sir16_long_k3_4"):
                    mb.trajectories(case, cfg)
                    assert all(st == 0 for st, _, _, _ in log[n_switch:])
                if name in mb.MASKED:
                    for newton in (True, False):
                        mb.masked_16(ctx, case, cfg, name, newton, on_device=False)  # (one chain fails by design)
            except AssertionError as e:
                err = "other bodies: " + str(e)[:300]
        if err is None and mod is f16:
            try:
                if name == "fhn16_k4_5":
                    f16.switch_16(ctx, case, cfg, on_device=False)
                    f16.trajectories(case, cfg)
                    for newton in (True, False):  # (the block metric's own case: same layout, 4 chains from one point)
                        mcase = f16.metric_case()
                        mctx = make_ctx(mcase)
                        check_block_metric_against_oracle(mctx, mcase, newton, le.FHN_DTS[:4])
                        mctx.close()
                    assert all(st == 0 for st, _, _, _ in log[n_case:])
                if name in f16.MASKED:
                    for newton in (True, False):
                        f16.masked_16(ctx, case, cfg, name, newton, on_device=False)  # (one chain fails by design)
            except AssertionError as e:
                err = "other bodies: " + str(e)[:300]
        ctx.close()
        iters = [i for _, f, b, _ in log for i in (f, b)]
        statuses = sorted({st for st, _, _, _ in log[:n_case]})
        near = [n for _, _, _, ns in log for n in ns]
        ok = statuses == [0] and not near and err is None
        print(f"SCREEN {name}: seed {cfg[12]} steps {len(log)} statuses {statuses} iterations {min(iters, default=None)}..{max(iters, default=None)} "
              f"near-edge {near} {'' if err is None else 'ASSERT ' + err} {time.time() - t0:.1f} s {'ok' if ok else 'REPLACE'}",
              flush=True)
        if not ok:
            bad.append(name)
    print("failed:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:] or list(le.CASES) + list(mb.CASES) + list(f16.CASES)))
