"""Cost of the path-wise event summaries on one MI355X.
usage: python tools/path_events_timing.py [pairs] [output file] [--parent-lib PATH]

Every measurement is a child process (`--child`) and a time is a host clock around one call that ends in a device
synchronise: the median over REPS calls after WARM; the child also prints the smallest and largest.
  1. FitzHugh-Nagumo configs[1], 256 chains: one paths.PathEvents.update() at stride 1 with two thresholds on the observed
     channel -- scanning the path itself, and with path_posterior= sharing the scratch of a PathPosterior (the events
     kernel alone) -- beside PathPosterior.update() and one 16-step transition timed in the same process.
  2. chmc_predict_events_device against chmc_predict_device at the shapes of profiles/predictive_timing.txt, same process.
  3. With --parent-lib (a libchmc_hip.so built from the parent commit): chmc_predict_device of this build against the
     parent's, `pairs` pairs of processes, alternating which goes first; per shape every process' median in the order run
     and the two ranges (the run-to-run spread)."""
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
REPS, WARM, B = 15, 3, 256


def wall_us(call, reps=REPS, warm=WARM):
    import numpy as np
    got = []
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        call()
        if rep >= warm:
            got.append(time.perf_counter() - t0)
    return float(np.median(got)) * 1e6, min(got) * 1e6, max(got) * 1e6


def child(lib_path, events):
    import numpy as np
    import torch
    from manifold_mcmc_for_diffusions_amd import _lib
    if lib_path:  # another build of the library: bind what it exports
        cdll = ctypes.CDLL(lib_path)
        for name, res, args in _lib.SYMBOLS:
            if hasattr(cdll, name):
                f = getattr(cdll, name)
                f.restype, f.argtypes = res, args
        _lib._LIB = cdll
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload, SirWorkload
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    res = {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0)}
    for which in ("sir", "fhn"):
        if which == "sir":
            wl, dt = SirWorkload(num_chains=B, keyed_init=True, total_chains=B), 0.05
            shapes = [(7, 1, 64), (7, wl.S, 64)]
        else:
            wl, dt = FhnWorkload(num_chains=B, num_steps_per_obs=400, device=0, device_init=True), 0.1
            shapes = [(10, wl.S, 64), (10, wl.S, 256)]
        ctx = wl.ctx
        assert ctx.L.chmc_backend() == b"hip:gfx950"
        for _ in range(3):  # the sampler's loop: the chains leave their initial states
            wl.refresh_momentum()
            act = np.ones(B, dtype=np.int32)
            for _ in range(4):
                act &= (wl.step(dt, active=act)["status"] == 0).astype(np.int32)
            ctx.switch_partition()
        if events:
            res[f"{which}/t16"] = wall_us(lambda: (wl.refresh_momentum(), ctx.leapfrog_steps(dt, 16, **wl.solver)), 5, 1)
            ctx.switch_partition()
        if events and which == "fhn":
            from manifold_mcmc_for_diffusions_amd.paths import PathEvents, PathPosterior
            pp = PathPosterior(ctx, 1)
            own = PathEvents(ctx, ctx.X, (0.0, 1.0), stride=1)
            shared = PathEvents(ctx, ctx.X, (0.0, 1.0), stride=1, path_posterior=pp)
            res["fhn/path_posterior_update"] = wall_us(pp.update)
            d0 = ctx.diagnostics()
            res["fhn/path_events_own_scan"] = wall_us(own.update)
            res["fhn/path_events_shared_scratch"] = wall_us(shared.update)
            d1 = ctx.diagnostics()
            res["fhn/path_events_launches"] = [d1[k] - d0[k] for k in ("path_events_wave_launches", "path_events_seq_launches")]
            assert shared.update().tobytes() == own.update().tobytes()
            res["fhn/path_events_NP"] = own.NP
        levels = np.linspace(0.0, 400.0, 21) if which == "sir" else np.linspace(-2.5, 2.5, 21)
        for H, stride, n_rep in shapes:
            for tag in ("predict", "predict_events") if events else ("predict",):
                ev = dict(channel=ctx.X + 1, thresholds=(300.0, 500.0) if which == "sir" else (0.0, 1.0)) if tag == "predict_events" else None
                pp = PredictivePosterior(ctx, H, stride, n_rep, levels=levels, events=ev) if ev else \
                    PredictivePosterior(ctx, H, stride, n_rep, levels=levels)
                draw = [0]

                def update():
                    draw[0] += 1
                    pp.update(7, draw[0])

                res[f"{which}/H{H}/stride{stride}/n_rep{n_rep}/{tag}"] = wall_us(update)
                assert pp.moments()[0].tolist() == [n_rep * (REPS + WARM)] * B
                del pp
                torch.cuda.empty_cache()
        ctx.close()
    print("CHILD_RESULT " + json.dumps(res), flush=True)


def run_child(extra):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + extra, capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_RESULT ")]
    if r.returncode != 0 or not line:
        sys.exit(f"child {extra} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(line[0][len("CHILD_RESULT "):])


def main():
    import numpy as np
    args = list(sys.argv[1:])
    parent_lib = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent_lib = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    pairs = int(args[0]) if args else 3
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "path_events_timing.txt")
    ev = run_child(["--events"])
    us = lambda t: f"{t[0]:.1f} us ({t[1]:.1f} .. {t[2]:.1f})"  # noqa: E731
    t16 = ev["fhn/t16"][0]
    lines = [f"== path-wise events, {B} chains, {ev['device']} on {ev['host']}; median over {REPS} calls after {WARM} (host clock "
             "around a call that ends in a device synchronise), one process",
             f"FitzHugh-Nagumo configs[1], stride 1 ({ev['fhn/path_events_NP']} points), observed channel, L = 2:",
             f"   PathEvents.update(), scanning the path itself: {us(ev['fhn/path_events_own_scan'])}",
             f"   PathEvents.update() on the scratch of a PathPosterior (path_posterior=): {us(ev['fhn/path_events_shared_scratch'])}"
             f"; launches wave/functor {ev['fhn/path_events_launches']}",
             f"   PathPosterior.update() (scan + moments): {us(ev['fhn/path_posterior_update'])}",
             f"   a 16-step transition of this context: {t16 / 1e3:.2f} ms ({ev['fhn/t16'][1] / 1e3:.2f} .. {ev['fhn/t16'][2] / 1e3:.2f})"
             f"  ->  events with their own scan = {100 * ev['fhn/path_events_own_scan'][0] / t16:.3f} % of it, on shared scratch "
             f"{100 * ev['fhn/path_events_shared_scratch'][0] / t16:.3f} %",
             "chmc_predict_events_device (y_rep, whole horizon, L = 2) against chmc_predict_device, same process:"]
    for key in [k[:-len("/predict")] for k in ev if k.endswith("/predict")]:
        a, b = ev[key + "/predict"], ev[key + "/predict_events"]
        lines.append(f"   {key}: predict {us(a)}, with events {us(b)}, ratio {b[0] / a[0]:.3f}")
    if parent_lib:
        runs = []
        for k in range(pairs):
            for tag in (("this", "parent") if k % 2 == 0 else ("parent", "this")):
                runs.append((tag, run_child(["--lib", parent_lib] if tag == "parent" else [])))
                print(f"child {len(runs)} ({tag}) done", flush=True)
        lines.append(f"chmc_predict_device of this build against the parent commit's: {pairs} pairs of processes, alternating which "
                     "goes first; every process' median in the order run:")
        for key in [k for k in runs[0][1] if k.endswith("/predict")]:
            med = {tag: [r[key][0] for t, r in runs if t == tag] for tag in ("this", "parent")}
            lines.append(f"   {key}: " + ", ".join(f"{tag} {r[key][0]:.1f}" for tag, r in runs))
            lo, hi = min(med["parent"]), max(med["parent"])
            inside = all(lo <= m <= hi for m in med["this"])
            lines.append(f"      this {np.mean(med['this']):.1f} us ({min(med['this']):.1f} .. {max(med['this']):.1f})   parent "
                         f"{np.mean(med['parent']):.1f} us ({lo:.1f} .. {hi:.1f})   this / parent = "
                         f"{np.mean(med['this']) / np.mean(med['parent']):.4f}   this build's medians "
                         f"{'all inside' if inside else 'NOT all inside'} the parent's range")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None, "--events" in sys.argv)
    else:
        main()
