"""Cost of one posterior predictive update (paths.PredictivePosterior.update = chmc_predict_device) on one MI355X with the wave
kernel (k_predict, the default) and with the functor form (KPredict + KPredictFold, CHMC_COMPACT_ROWS=0), beside a 16-step
transition of the same context.
usage: python tools/predictive_timing.py [pairs] [output file]

The switch is latched at the first create, so every measurement is a child process (`--child`): the parent starts `pairs`
pairs of children, alternating which form goes first, and every child times every shape.  A time is a host clock around
one update, which ends in a device synchronise: the median over REPS calls after WARM; the child also prints the smallest
and largest.  Per shape the parent reports every child's median in the order run, the range over the children of each
form (the run-to-run spread) and the ratio of the means.  The 16-step transition (momentum refresh + chmc_leapfrog_steps)
is timed in every child; the fraction is taken against the default build's, since CHMC_COMPACT_ROWS=0 slows the transition
itself.  Shapes:
  boarding-school SIR, 256 chains, H = 7, n_rep = 64, strides 1 and S;
  FitzHugh-Nagumo configs[1], 256 chains, H = 10, n_rep = 64 and 256, stride S."""
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


def child():
    import numpy as np
    import torch
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
        t16 = wall_us(lambda: (wl.refresh_momentum(), ctx.leapfrog_steps(dt, 16, **wl.solver)), 5, 1)
        ctx.switch_partition()
        res[f"{which}/t16"] = t16
        levels = np.linspace(0.0, 400.0, 21) if which == "sir" else np.linspace(-2.5, 2.5, 21)
        for H, stride, n_rep in shapes:
            pp = PredictivePosterior(ctx, H, stride, n_rep, levels=levels)
            draw = [0]

            def update():
                draw[0] += 1
                pp.update(7, draw[0])

            d0 = ctx.diagnostics()
            res[f"{which}/H{H}/stride{stride}/n_rep{n_rep}"] = wall_us(update)
            d1 = ctx.diagnostics()
            res[f"{which}/H{H}/stride{stride}/n_rep{n_rep}/launches"] = [
                d1["predict_wave_launches"] - d0["predict_wave_launches"], d1["predict_seq_launches"] - d0["predict_seq_launches"]]
            n, mean, _ = pp.moments()
            assert n.tolist() == [n_rep * (REPS + WARM)] * B
            res[f"{which}/H{H}/stride{stride}/n_rep{n_rep}/finite"] = float(np.isfinite(mean).mean())
            del pp
            torch.cuda.empty_cache()
        ctx.close()
    print("CHILD_RESULT " + json.dumps(res), flush=True)


def main():
    import numpy as np
    args = [a for a in sys.argv[1:]]
    pairs = int(args[0]) if args else 3
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "predictive_timing.txt")
    runs = []
    for k in range(pairs):
        for tag in (("wave", "seq") if k % 2 == 0 else ("seq", "wave")):
            env = dict(os.environ)
            if tag == "seq":
                env["CHMC_COMPACT_ROWS"] = "0"
            else:
                env.pop("CHMC_COMPACT_ROWS", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                               timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit(f"child {tag} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs.append((tag, json.loads(line[0][len("CHILD_RESULT "):])))
            print(f"child {len(runs)} ({tag}) done", flush=True)
    lines = [f"== one PredictivePosterior.update, {B} chains: wave kernel (default) against the functor form (CHMC_COMPACT_ROWS=0)",
             f"   {runs[0][1]['device']} on {runs[0][1]['host']}; {pairs} pairs of processes, alternating which form runs first; per "
             f"process the median over {REPS} calls after {WARM} (host clock around a call that ends in a device synchronise)"]
    keys = [k for k in runs[0][1] if k.count("/") == 3 and not k.endswith(("launches", "finite"))]
    for key in keys:
        which = key.split("/")[0]
        t16 = [r[f"{which}/t16"][0] for tag, r in runs if tag == "wave"]
        lines.append(f"{key}:")
        lines.append("   in the order run: " + ", ".join(f"{tag} {r[key][0]:.1f} us ({r[key][1]:.1f} .. {r[key][2]:.1f})" for tag, r in runs))
        med = {tag: [r[key][0] for t, r in runs if t == tag] for tag in ("wave", "seq")}
        launches = {tag: [r[key + "/launches"] for t, r in runs if t == tag][0] for tag in ("wave", "seq")}
        w, s = float(np.mean(med["wave"])), float(np.mean(med["seq"]))
        lines.append(f"   wave {w:9.1f} us (processes {min(med['wave']):.1f} .. {max(med['wave']):.1f}; launches wave/functor {launches['wave']})   "
                     f"functor {s:9.1f} us ({min(med['seq']):.1f} .. {max(med['seq']):.1f}; {launches['seq']})   functor / wave = {s / w:.2f}"
                     f"   ranges {'apart' if max(med['wave']) < min(med['seq']) or max(med['seq']) < min(med['wave']) else 'OVERLAP'}")
        lines.append(f"   a 16-step transition of this context (default build): {np.mean(t16) / 1e3:.2f} ms ({min(t16) / 1e3:.2f} .. "
                     f"{max(t16) / 1e3:.2f})  ->  one update = {100 * w / np.mean(t16):.3f} % of it (functor form: {100 * s / np.mean(t16):.3f} %)"
                     f"; finite share of the means {runs[0][1][key + '/finite']:.3f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
