"""Cost of the latent-path scan and of a path-posterior update on one MI355X, beside the partition switch's time-parallel
scan (k_xobs_par: the yardstick, same context, same process) and a leapfrog step.
usage: python tools/path_posterior_timing.py [fhn|sir] [chains] [output file] [--scans-only]
--scans-only: the leapfrog step and the transition are not timed, so the chains are still where the warm-up left them when the
scans are (the transitions of the timing loop have no accept / reject step and let chains drift).

Kernel times are HIP events on the library's stream around every launch (chmc_profile_enable / chmc_profile_get, summed per
kernel class over ONE call and read back after it): the median over REPS calls after warm-up.  The path scans are the
only launches of class 7 (constr) in their calls, the moment update the only ones of class 8.  The switch's scan shares
class 0 with three one-item-per-chain launches of the state evaluation behind it (KBegin, KStateChain, KGldChain); those are
measured in a call that runs them without the scan (restore of every chain) and subtracted.  Wall-clock times are host
clocks around calls that end in a device synchronise, with the event recording off.
Bytes a call must move: the positions once and its outputs once (scan: 8 B (Q + NP X); update: + 8 B NP (X + 4 (X + 1)) for
the moments' read-modify-write and the path read back); the share of peak is against 8.0 TB/s."""
import ctypes as C
import os
import socket
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload, SirWorkload  # noqa: E402
from manifold_mcmc_for_diffusions_amd.paths import PathPosterior  # noqa: E402

REPS, WARM, PEAK = 25, 3, 8.0e12
scans_only = "--scans-only" in sys.argv
if scans_only:
    sys.argv.remove("--scans-only")
which = sys.argv[1] if len(sys.argv) > 1 else "fhn"
B = int(sys.argv[2]) if len(sys.argv) > 2 else (256 if which == "fhn" else 1024)
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "path_posterior_timing.txt")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


if which == "fhn":
    wl = FhnWorkload(num_chains=B, num_steps_per_obs=400, device=0, device_init=True)  # BASELINE.json configs[1]
    title, dt = f"FitzHugh-Nagumo noisy, T = 100, S = 400, R = 5, {B} chains (configs[1])", 0.1
else:
    wl = SirWorkload(num_chains=B, keyed_init=True, total_chains=B)
    title, dt = f"SIR boarding school, T = 14, S = {wl.S}, one sub-sequence, {B} chains", 0.05
ctx, L = wl.ctx, wl.ctx.L
assert L.chmc_backend() == b"hip:gfx950" and torch.cuda.is_available()
say(f"== {title}" + (f"   [library {os.path.basename(os.environ['CHMC_HIP_LIBRARY'])}]" if os.environ.get("CHMC_HIP_LIBRARY") else ""))
say(f"   {torch.cuda.get_device_name(0)} on {socket.gethostname()}, torch {torch.__version__}; Q = {ctx.Q}, K = {ctx.K}, RM = {ctx.RM}")


def class_ms(call, classes):
    """median (min, max) over REPS calls of the summed event time of `classes` within one call, and the launches counted"""
    ms, n = (C.c_double * 10)(), (C.c_longlong * 10)()
    got, launches = [], 0
    for rep in range(WARM + REPS):
        L.chmc_profile_enable(1)
        call()
        L.chmc_profile_get(ms, n)
        if rep >= WARM:
            got.append(sum(ms[c] for c in classes))
            launches = sum(n[c] for c in classes)
    L.chmc_profile_enable(0)
    return float(np.median(got)) * 1e3, min(got) * 1e3, max(got) * 1e3, int(launches)


def wall_us(call, reps=REPS):
    got = []
    for rep in range(WARM + reps):
        t0 = time.perf_counter()
        call()
        if rep >= WARM:
            got.append(time.perf_counter() - t0)
    return float(np.median(got)) * 1e6


for _ in range(3):  # the sampler's loop: the chains leave their initial states
    wl.refresh_momentum()
    act = np.ones(B, dtype=np.int32)
    for _ in range(4):
        act &= (wl.step(dt, active=act)["status"] == 0).astype(np.int32)
    ctx.switch_partition()
say(f"   warm-up: {int(act.sum())} of {B} chains completed their last trajectory")

t16 = float("nan")
if not scans_only:
    wl.refresh_momentum()
    step = class_ms(lambda: wl.step(dt), range(10))
    say(f"one leapfrog step: kernels {step[0]:8.1f} us ({step[3]} launches), wall {wall_us(lambda: wl.step(dt), 10):8.1f} us")
    wl.refresh_momentum()
    t16 = wall_us(lambda: (wl.refresh_momentum(), ctx.leapfrog_steps(dt, 16, **wl.solver)), 5)
    say(f"one 16-step transition (momentum refresh + chmc_leapfrog_steps), wall: {t16 / 1e3:8.2f} ms")
    ctx.switch_partition()
# from here on the chains stay where they are: the yardstick and the path scans see the same states
ones = np.ones(B, dtype=np.int32)
ctx.snapshot()
small = class_ms(lambda: ctx.restore(ones), (0,))
sw = class_ms(ctx.switch_partition, (0,))
xobs = sw[0] - small[0]
say(f"partition switch, class 0: {sw[0]:8.1f} us ({sw[1]:.1f} .. {sw[2]:.1f}; {sw[3]} launches); the {small[3]} launches of the state "
    f"evaluation alone: {small[0]:.1f} us  ->  k_xobs_par {xobs:8.1f} us")

S = ctx.S
for stride in (1, S // 8, S):
    pp = PathPosterior(ctx, stride)
    n_p = pp.NP
    _, sweeps = ctx.generate_x_seq(stride, return_sweeps=True)
    scan = class_ms(lambda: ctx.generate_x_seq_device(stride, pp._ptr("x")), (7,))
    upd = class_ms(pp.update, (7, 8))
    upd_wall = wall_us(pp.update)
    b_scan = 8.0 * B * (ctx.Q + n_p * ctx.X)
    b_upd = b_scan + 8.0 * B * n_p * (ctx.X + 4 * (ctx.X + 1))
    say(f"stride {stride:4d} (NP = {n_p:6d}; sweeps {np.bincount(sweeps).tolist()}):")
    say(f"   generate_x_seq_device    {scan[0]:8.1f} us ({scan[1]:.1f} .. {scan[2]:.1f}; {scan[3]} launch)  {b_scan / 1e6:8.1f} MB  "
        f"{b_scan / scan[0] / 1e6:6.3f} TB/s = {100 * b_scan / (scan[0] * 1e-6) / PEAK:5.1f} % of HBM peak   {scan[0] / xobs:5.2f} x k_xobs_par")
    say(f"   path_stats_update_device {upd[0]:8.1f} us ({upd[1]:.1f} .. {upd[2]:.1f}; {upd[3]} launches) {b_upd / 1e6:8.1f} MB  "
        f"{b_upd / upd[0] / 1e6:6.3f} TB/s = {100 * b_upd / (upd[0] * 1e-6) / PEAK:5.1f} % of HBM peak   wall {upd_wall:8.1f} us = "
        f"{100 * upd_wall / t16:5.2f} % of a 16-step transition")
    del pp
    torch.cuda.empty_cache()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n\n")
