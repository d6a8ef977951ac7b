"""Batched leapfrog-step time against the sub-sequence length R = num_obs_per_subseq (the reference's grid study,
scripts/utils.py:403-409) on the FitzHugh-Nagumo noisy-observation workload: T = 100 observations, 256 chains, the script's
solver settings (FhnWorkload.solver), one shared step size.  R = 2 and 5 run on blocks of 4 and 7 rows (8 and 7 row slots),
R = 10 and 14 on blocks of 12 and 16 rows in 16 row slots.

    python tools/subseq_timing.py [--chains 256] [--steps-per-obs 25 400] [--subseq 2 5 10 14] [--passes 2]
                                  [--step-size 0.1] [--min-seconds 1.0] [--commit TEXT] [--out FILE]

One process.  Per S every R gets its own context; each is warmed up with a few trajectories with a partition switch after
each, so both partitions have run.  Then, per pass, the points are visited one after the other (alternating), and in each
partition of each point the batched step is timed by a host clock around chmc_leapfrog_step calls (every call ends with the
read-back of the statuses, i.e. synchronised) over at least --min-seconds of work; the momentum refresh every 16 steps is not
in the clock.  Every chain takes every step (a failed step leaves its chain where it was).  Printed per point and partition:
ms per batched step, leapfrog steps/s (chains x steps / time), the share of steps that ended with status 0, the mean forward /
reverse Newton iterations of those, K and RM; then per point the mean over the passes and the pass-to-pass spread
(max - min) / mean.  The table goes to --out (default profiles/fhn_subseq_length.txt) with the commit and the SHA-256 of the
library that was timed (CHMC_HIP_LIBRARY selects another build of the library, e.g. the parent commit's for R = 2 and 5)."""
import argparse
import hashlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd import _lib  # noqa: E402
from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload  # noqa: E402

TRAJ = 16  # steps between momentum refreshes (bench.py's trajectory length)


def commit_of(text):
    if text:
        return text
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (not a git checkout; pass --commit)"


def warm_up(wl, dt, trajectories=3):
    B = wl.B
    for _ in range(trajectories):
        wl.refresh_momentum()
        act = np.ones(B, dtype=np.int32)
        for _ in range(TRAJ):
            r = wl.step(dt, active=act)
            act &= (r["status"] == 0).astype(np.int32)
        wl.ctx.switch_partition()


def time_partition(wl, dt, min_seconds):
    """Batched steps in the context's current partition until min_seconds of step calls (and at least one trajectory)."""
    el, n, ok, itf, itb = 0.0, 0, 0, 0, 0
    while el < min_seconds or n < TRAJ:
        if n % TRAJ == 0:
            wl.refresh_momentum()
            wl.ctx.hamiltonian()  # (a read-back: the refresh has finished before the clock starts)
        t0 = time.perf_counter()
        r = wl.step(dt)
        el += time.perf_counter() - t0
        good = r["status"] == 0
        n, ok = n + 1, ok + int(good.sum())
        itf, itb = itf + int(r["iters_fwd"][good].sum()), itb + int(r["iters_bwd"][good].sum())
    return dict(ms=el / n * 1e3, rate=wl.B * n / el, ok=ok / (wl.B * n), itf=itf / max(ok, 1), itb=itb / max(ok, 1), steps=n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--num-obs", type=int, default=100)
    ap.add_argument("--steps-per-obs", type=int, nargs="+", default=[25, 400])
    ap.add_argument("--subseq", type=int, nargs="+", default=[2, 5, 10, 14])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--step-size", type=float, default=0.1)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fhn_subseq_length.txt"))
    a = ap.parse_args()
    if a.passes < 2:
        ap.error("at least two passes: the spread between them is part of the result")
    L = _lib.lib()
    sha = hashlib.sha256(open(_lib._SO, "rb").read()).hexdigest()
    lines = [f"# FitzHugh-Nagumo, noisy observations (sigma_y = 0.1), T = {a.num_obs}, {a.chains} chains, step size {a.step_size}, "
             f"Newton solver with the script tolerances; backend {L.chmc_backend().decode()}",
             f"# commit {commit_of(a.commit)}",
             f"# library {os.path.basename(_lib._SO)} sha256 {sha}",
             f"# per pass and partition at least {a.min_seconds} s of batched steps; warm-up 3 trajectories of {TRAJ} steps with a "
             f"partition switch after each",
             "# S   R  K        RM pass part  ms/step  steps/s  status0  iters fwd  iters bwd  steps timed"]
    print("\n".join(lines), flush=True)
    summary = []
    for S in a.steps_per_obs:
        wls = {}
        for R in a.subseq:
            t0 = time.perf_counter()
            wls[R] = FhnWorkload(a.chains, num_steps_per_obs=S, num_obs=a.num_obs, num_obs_per_subseq=R, device_init=True)
            warm_up(wls[R], a.step_size)
            print(f"# S = {S} R = {R}: K = {wls[R].ctx.K} RM = {wls[R].ctx.RM}, set-up and warm-up {time.perf_counter() - t0:.1f} s",
                  flush=True)
        res = {(R, part): [] for R in a.subseq for part in range(2)}
        for p in range(a.passes):
            for R in a.subseq:  # alternating: every point once per pass
                wl = wls[R]
                for _ in range(wl.ctx.num_partition):
                    part = wl.ctx.partition
                    m = time_partition(wl, a.step_size, a.min_seconds)
                    res[R, part].append(m)
                    row = (f"{S:4d} {R:3d}  {str(wl.ctx.K):8s} {wl.ctx.RM:2d} {p:4d} {part:4d}  {m['ms']:7.3f}  {m['rate']:7.0f}  "
                           f"{m['ok']:7.4f}  {m['itf']:9.2f}  {m['itb']:9.2f}  {m['steps']:6d}")
                    lines.append(row)
                    print(row, flush=True)
                    wl.ctx.switch_partition()
        for R in a.subseq:
            for part in range(2):
                ms = np.array([m["ms"] for m in res[R, part]])
                if ms.size:
                    summary.append(f"{S:4d} {R:3d}  {str(wls[R].ctx.K):8s} {wls[R].ctx.RM:2d} {part:4d}  {ms.mean():7.3f}  "
                                   f"{a.chains / ms.mean() * 1e3:7.0f}  {(ms.max() - ms.min()) / ms.mean():6.4f}")
        for wl in wls.values():
            wl.ctx.close()
    lines += ["# mean over the passes; spread = (max - min) / mean of ms/step over the passes",
              "# S   R  K        RM part  ms/step  steps/s  spread"] + summary
    print("\n".join(lines[-len(summary) - 2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written:", a.out)


if __name__ == "__main__":
    main()
