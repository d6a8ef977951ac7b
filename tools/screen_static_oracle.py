"""CPU screening of the cases of tests/test_hip_static_oracle.py: the module's bodies on the TEST-ONLY emulation build (no GPU).

    python tools/screen_static_oracle.py [case id ...]            the cases as the test module's table has them, then the
                                                                  live set_metric bodies
    python tools/screen_static_oracle.py --search [--statuses=1,3] case id ...
                                                                  choose (seed, eps0) for a case (at most MAX_SEEDS seeds, from
                                                                  the case's seed or seed0; eps0 from EPS_GRID), optionally
                                                                  one whose replay shows the given failing statuses

For every case it runs static_body (the unmodified sampler, then helpers.oracle_static_transition for every chain and
transition) and prints the worst ratios, the events reached and the failing statuses.  A case is admitted only if every accept
draw of a complete trajectory is at least 1e-6 from its probability, no retraction residual lies within 1e-2 relative of its
tolerance, every reversibility error is at least 0.5 relative from reverse_check_tol, no complete trajectory has a non-finite
dh, and the replay shows every event the test module requires of the case.  A (seed, eps0) that fails is noted in the
module's REPLACED table.  A disagreement of the emulation build itself with the oracle is reported as such and the screening
goes on."""
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import make_ctx  # noqa: E402
from manifold_mcmc_for_diffusions_amd import _lib  # noqa: E402
import test_hip_tree_oracle as to  # noqa: E402
import test_hip_static_oracle as so  # noqa: E402

EPS_GRID = [0.3, 0.2, 0.4, 0.15, 0.6, 0.1, 0.8]
MAX_SEEDS = 20


def use_emulation_build():
    emu = os.path.join(ROOT, "tests", "emu")
    lib = os.path.join(emu, "libchmc_emu.so")
    csrc = os.path.join(ROOT, "manifold_mcmc_for_diffusions_amd", "csrc")
    srcs = [os.path.join(emu, f) for f in ("chmc_emu.cpp", "backend_emu.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(lib) or any(os.path.getmtime(lib) < os.path.getmtime(s) for s in srcs):  # (as the tests' fixture)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I.", "-o", lib, "chmc_emu.cpp"], cwd=emu)
    _lib._LIB = _lib._bind(ctypes.CDLL(lib))
    assert _lib.lib().chmc_backend() == b"emu:host-TEST-ONLY"


def run(cfg, case, seed, eps0):
    """static_body on a fresh context: (ok, statuses, what failed)."""
    for k, v in cfg["env"].items():
        os.environ[k] = v
    ctx = make_ctx(case)
    t0 = time.time()
    try:
        _, _, statuses, problems = so.static_body(ctx, case, cfg, seed=seed, eps0=eps0, screening=True)
    except AssertionError as e:
        return False, set(), [f"the emulation build itself disagrees with the oracle: {str(e)[:300]}"]
    finally:
        ctx.close()
        print(f"  {time.time() - t0:.1f} s", flush=True)
    return not problems, statuses, problems


def screen(name):
    cfg = so.cfg_of(name)
    case = to.build_case(cfg)
    ok, statuses, problems = run(cfg, case, cfg["seed"], cfg["eps0"])
    ok = ok and tuple(sorted(statuses)) == tuple(cfg["statuses"])
    print(f"SCREEN {name}: seed {cfg['seed']} eps0 {cfg['eps0']} statuses {sorted(statuses)} {'ok' if ok else 'REPLACE ' + str(problems)}",
          flush=True)
    return ok


def screen_live(name):
    cfg = so.cfg_of(name)
    case = to.build_case(cfg, seed=so.LIVE_METRIC[name][0])
    ctx = make_ctx(case)
    try:
        _, problems = so.live_metric_body(ctx, case, name, screening=True)
    except AssertionError as e:
        problems = [f"disagreement or failed step: {str(e)[:300]}"]
    ctx.close()
    print(f"SCREEN live set_metric {name}: {'ok' if not problems else 'REPLACE ' + str(problems)}", flush=True)
    return not problems


def search(name, want_statuses=()):
    cfg = so.cfg_of(name)
    failed = {}
    seed0 = cfg.get("seed", cfg.get("seed0", 31))
    for seed in range(seed0, seed0 + 100 * MAX_SEEDS, 100):
        cfg["seed"] = seed
        try:
            case = to.build_case(cfg, seed)
        except AssertionError as e:
            failed[seed] = f"building the chains: {str(e)[:60]}"
            continue
        for eps0 in EPS_GRID:
            print(f"{name}: seed {seed} eps0 {eps0}", flush=True)
            ok, statuses, problems = run(cfg, case, seed, eps0)
            if ok and not set(want_statuses) <= statuses:
                ok, problems = False, [f"statuses {sorted(statuses)}: {sorted(want_statuses)} wanted"]
            if ok:
                print(f'CHOSEN    "{name}": ({seed}, {eps0}, {tuple(sorted(statuses))}),')
                print(f'REPLACED  "{name}": {failed},', flush=True)
                return seed, eps0
            failed[seed, eps0] = "; ".join(p.split(": ", 1)[-1][:110] for p in problems[:2])
            print(f"  no: {failed[seed, eps0]}", flush=True)
    print(f"NONE FOUND for {name} in {MAX_SEEDS} seeds; failures {failed}")
    return None


if __name__ == "__main__":
    use_emulation_build()
    args = sys.argv[1:]
    if args and args[0] == "--search":
        want = ()
        if len(args) > 1 and args[1].startswith("--statuses="):
            want = tuple(int(s) for s in args[1].split("=")[1].split(","))
            args = args[:1] + args[2:]
        for n in args[1:]:
            search(n, want)
        sys.exit(0)
    results = {n: screen(n) for n in (args or list(so.CASES))}
    if not args:
        results.update({f"live:{n}": screen_live(n) for n in so.LIVE_METRIC})
    print("failed:", [n for n, ok in results.items() if not ok])
    sys.exit(0 if all(results.values()) else 1)
