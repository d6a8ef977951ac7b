"""Cost of scoring arrived observations (chmc_score_future_device), of one sequential.extend_state, and of a sequential run
against fresh fits, on one MI355X.
usage: python tools/future_score_timing.py [processes per form] [output file] [--parent-lib PATH] [--skip-calls] [--skip-run]

1. One score call, host clock around a call that ends in a device synchronise (median over REPS calls after WARM), in
   processes run in interleaved order:
     default             the functor form KFutureScore; in the same process and on the same states the wave kernel
                         k_future_score under CHMC_FUTURE_WAVE=1 (read per call), and chmc_predict_device at the same
                         (H, stride = S, n_rep);
     CHMC_COMPACT_ROWS=0 the stored-rows family (latched at the first create): the functor form with that family's path scan;
     --parent-lib        chmc_predict_device of another build of the library (the parent commit's, via CHMC_HIP_LIBRARY):
                         the same recursion with the fold, which the new call should not be slower than.
   Shapes: boarding-school SIR (S = 200, 256 chains, days 1 .. 10 fitted, the counts of days 11 .. 14 arriving), H = 1
   and 4; FitzHugh-Nagumo configs[1] (S = 400, 256 chains), H = 1;
   n_cand = 64 and 256.  A call is also expressed as a share of a 16-step transition of the same context.
2. One extend_state on the same contexts (score with logw and tail, the splice, chmc_set_state_solve_noise_device, the
   constraint read-back), default processes only.
3. Boarding-school SIR at S = 20, 256 chains, days 10 -> 14: sequential_static_chmc (finder and WARM_FIRST warm-up transitions
   once, then per day WARM_NEXT re-tuning transitions and MAIN draws) against four fresh fits of days 1..11, .., 1..14
   (finder, WARM_FIRST warm-up transitions, MAIN draws each; with --parent-lib on that build): wall time, final step size,
   main-phase accept statistic, and per day the log predictive score and the candidates' effective sample size."""
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
REPS, WARM, B = 15, 3, 256
WARM_FIRST, WARM_NEXT, MAIN, N_STEP, K0 = 100, 20, 100, 16, 10


def wall_us(call, reps=REPS, warm=WARM):
    import numpy as np
    got = []
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        call()
        if rep >= warm:
            got.append(time.perf_counter() - t0)
    return float(np.median(got)) * 1e6, min(got) * 1e6, max(got) * 1e6


def load(parent):
    from manifold_mcmc_for_diffusions_amd import _lib
    if parent:  # another build of the library, which need not export the new symbol
        _lib.SYMBOLS = [s for s in _lib.SYMBOLS if s[0] != "chmc_score_future_device"]
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


def child_calls(parent):
    load(parent)
    import numpy as np
    import torch
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload, BOARDING_SCHOOL_COUNTS
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    from manifold_mcmc_for_diffusions_amd.sequential import extend_state
    res = {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0)}
    solver = dict(newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8)
    counts = np.asarray(BOARDING_SCHOOL_COUNTS, dtype=np.float64)
    for which in ("sir", "fhn"):
        # SIR: days 1 .. 10 (one block of at most 16 rows holds 14 days: room for H = 4), the counts of days 11 .. 14 arrive
        if which == "sir":
            ctx, dt, horizons, y_next = sir_fit(counts[:K0], 200), 0.05, (1, 4), counts[K0:]
        else:
            wl = FhnWorkload(num_chains=B, num_steps_per_obs=400, device=0, device_init=True)
            ctx, dt, horizons, y_next = wl.ctx, 0.1, (1,), np.array([float(wl.y[-1, 0])])
        draw = [0]

        def refresh():
            draw[0] += 1
            ctx.sample_momentum(11, draw[0])

        for _ in range(3):  # the sampler's loop: the chains leave their initial states
            refresh()
            act = np.ones(B, dtype=np.int32)
            for _ in range(4):
                act &= (ctx.leapfrog_step(dt, active=act, **solver)["status"] == 0).astype(np.int32)
            ctx.switch_partition()
        res[f"{which}/t16"] = wall_us(lambda: (refresh(), ctx.leapfrog_steps(dt, 16, **solver)), 5, 1)
        ctx.switch_partition()
        for H in horizons:
            y = y_next[:H]
            dst = None if parent else ctx.extended(y)
            for n_cand in (64, 256):
                key = f"{which}/H{H}/n{n_cand}"
                pp = PredictivePosterior(ctx, H, ctx.S, n_cand)

                def predict():
                    draw[0] += 1
                    pp.update(7, draw[0])

                def score():
                    draw[0] += 1
                    ctx.score_future_device(7, draw[0], 0, y, n_cand)

                res[key + "/predict"] = wall_us(predict)
                if parent:
                    continue
                d0 = ctx.diagnostics()
                res[key + "/score"] = wall_us(score)
                d1 = ctx.diagnostics()
                res[key + "/launches"] = [d1["predict_wave_launches"] - d0["predict_wave_launches"],
                                          d1["predict_seq_launches"] - d0["predict_seq_launches"]]
                os.environ["CHMC_FUTURE_WAVE"] = "1"
                try:
                    res[key + "/score_wave"] = wall_us(score)
                finally:
                    del os.environ["CHMC_FUTURE_WAVE"]
                if os.environ.get("CHMC_COMPACT_ROWS") == "0":
                    continue
                ext = [None]

                def extend():
                    draw[0] += 1
                    ext[0] = extend_state(ctx, dst, 7, draw=draw[0], n_cand=n_cand)

                res[key + "/extend"] = wall_us(extend, 5, 1)
                res[key + "/ess_median"] = float(np.median(ext[0]["ess_cand"]))
                res[key + "/max_constr"] = ext[0]["max_constr"]
                del pp
                torch.cuda.empty_cache()
            if dst is not None:
                dst.close()
        ctx.close()
    print("CHILD_RESULT " + json.dumps(res), flush=True)


def sir_fit(y, S=20, log=None):
    import numpy as np
    from manifold_mcmc_for_diffusions_amd import init
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    ctx = ChmcContext("sir", 1.0, S, None, y, sigma=1.0, num_chains=B)
    init.find_initial_states_by_gradient_descent_noisy_system(ctx, np.random.default_rng(20200710), adam_step_size=1e-1,
                                                              max_iters=5000, log=log)
    return ctx


def child_run(parent, fresh):
    load(parent)
    import numpy as np
    from manifold_mcmc_for_diffusions_amd.workload import BOARDING_SCHOOL_COUNTS
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    y = np.asarray(BOARDING_SCHOOL_COUNTS, dtype=np.float64)
    res = {}
    if fresh:
        for T in range(K0 + 1, len(y) + 1):
            t0 = time.perf_counter()
            ctx = sir_fit(y[:T])
            t_init = time.perf_counter() - t0
            out = sample_static_chmc(ctx, WARM_FIRST + MAIN, N_STEP, 0.05, seed=7 + T, n_adapt=WARM_FIRST, n_head=5,
                                     jitter_length=True)
            res[str(T)] = dict(seconds=time.perf_counter() - t0, init_seconds=t_init, step=float(out["final_step_size"]),
                               accept=float(out["accept_stat"][WARM_FIRST:].mean()),
                               fail=float(out["fail_rate"][WARM_FIRST:].mean()))
            ctx.close()
    else:
        from manifold_mcmc_for_diffusions_amd.sequential import sequential_static_chmc
        for n_cand in (64, 1024):
            t0 = time.perf_counter()
            ctx = sir_fit(y[:K0])
            t_init = time.perf_counter() - t0
            out = sequential_static_chmc(ctx, [y[d:d + 1] for d in range(K0, len(y))], WARM_FIRST, WARM_NEXT, MAIN, N_STEP, 0.05,
                                         seed=7, n_cand=n_cand, n_head=5, jitter_length=True)
            res[f"n_cand{n_cand}"] = dict(
                seconds=time.perf_counter() - t0, init_seconds=t_init,
                stages=[dict(T=s["T"], seconds=s["seconds"], step=float(s["final_step_size"]), accept=s["mean_accept_stat"],
                             log_pred=s["log_pred"], ess_median=None if s["ess_cand"] is None else float(np.median(s["ess_cand"])),
                             ess_min=None if s["ess_cand"] is None else float(s["ess_cand"].min()),
                             moved=None if s["moved"] is None else float(s["moved"].max())) for s in out["stages"]])
            out["ctx"].close(), ctx.close()
    print("CHILD_RESULT " + json.dumps(res), flush=True)


def run_child(flag, env_extra, parent_lib=None):
    env = dict(os.environ)
    env.pop("CHMC_COMPACT_ROWS", None)
    env.update(env_extra)
    args = [sys.executable, os.path.abspath(__file__), flag]
    if parent_lib:
        env["CHMC_HIP_LIBRARY"] = parent_lib
        args.append("--parent")
    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=1100)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_RESULT ")]
    if r.returncode != 0 or not line:
        sys.exit(f"child {flag} {env_extra} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(line[0][len("CHILD_RESULT "):])


def spread(v):
    import numpy as np
    return f"{np.mean(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"


def main():
    import numpy as np
    args = [a for a in sys.argv[1:]]
    parent_lib = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent_lib = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    skip_calls, skip_run = "--skip-calls" in args, "--skip-run" in args
    args = [a for a in args if not a.startswith("--")]
    n_proc = int(args[0]) if args else 6
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "future_score_timing.txt")
    lines = []
    if not skip_calls:
        forms = ["default", "rows0"] + (["parent"] if parent_lib else [])
        runs = []
        for k in range(n_proc):
            for tag in (forms if k % 2 == 0 else forms[::-1]):
                runs.append((tag, run_child("--child-calls", {"CHMC_COMPACT_ROWS": "0"} if tag == "rows0" else {},
                                            parent_lib if tag == "parent" else None)))
                print(f"child {len(runs)} ({tag}) done", flush=True)
        first = [r for t, r in runs if t == "default"][0]
        lines += [f"== chmc_score_future_device, {B} chains: {first['device']} on {first['host']}; {n_proc} processes per form in "
                  f"interleaved order ({' '.join(t for t, _ in runs)}); per process the median over {REPS} calls after {WARM} (host "
                  "clock around a call that ends in a device synchronise); mean over the processes (their range)"]
        for key in sorted(k[:-len("/score")] for k in first if k.endswith("/score")):
            which = key.split("/")[0]
            get = lambda tag, what: [r[f"{key}/{what}"][0] for t, r in runs if t == tag and f"{key}/{what}" in r]  # noqa: E731
            t16 = [r[f"{which}/t16"][0] for t, r in runs if t == "default"]
            fun, wave, pred = get("default", "score"), get("default", "score_wave"), get("default", "predict")
            r0, r0p = get("rows0", "score"), get("rows0", "predict")
            lines.append(f"{key}:   launches wave/functor, default {first[key + '/launches']}, CHMC_COMPACT_ROWS=0 "
                         f"{[r for t, r in runs if t == 'rows0'][0][key + '/launches']}")
            lines.append(f"   score, functor form (default)           {spread(fun)}")
            lines.append(f"   score, wave form (CHMC_FUTURE_WAVE=1)   {spread(wave)}   wave / functor = {np.mean(wave) / np.mean(fun):.2f}   "
                         f"ranges {'apart' if max(wave) < min(fun) or max(fun) < min(wave) else 'OVERLAP'}")
            lines.append(f"   score, CHMC_COMPACT_ROWS=0              {spread(r0)}   / default = {np.mean(r0) / np.mean(fun):.2f}")
            lines.append(f"   chmc_predict_device, this build         {spread(pred)}   score / predict = {np.mean(fun) / np.mean(pred):.2f}   "
                         f"(CHMC_COMPACT_ROWS=0: {spread(r0p)})")
            if parent_lib:
                pp = get("parent", "predict")
                lines.append(f"   chmc_predict_device, parent build       {spread(pp)}   score / parent's predict = "
                             f"{np.mean(fun) / np.mean(pp):.2f}   ranges {'apart' if max(fun) < min(pp) or max(pp) < min(fun) else 'OVERLAP'}")
            ext = get("default", "extend")
            lines.append(f"   a 16-step transition of this context: {np.mean(t16) / 1e3:.2f} ms ({min(t16) / 1e3:.2f} .. {max(t16) / 1e3:.2f})"
                         f"  ->  one score call = {100 * np.mean(fun) / np.mean(t16):.3f} % of it")
            lines.append(f"   one extend_state                        {spread(ext)}   = {100 * np.mean(ext) / np.mean(t16):.2f} % of the "
                         f"transition; candidates' ESS median {first[key + '/ess_median']:.1f}, max |constraint| afterwards "
                         f"{first[key + '/max_constr']:.1e}")
    if not skip_run:
        seq = run_child("--child-run-seq", {})
        fresh = run_child("--child-run-fresh", {}, parent_lib)
        lines.append(f"== boarding-school SIR, S = 20, {B} chains, days {K0} -> 14: sequential_static_chmc ({WARM_FIRST} warm-up transitions "
                     f"once, then {WARM_NEXT} re-tuning transitions per day; {MAIN} draws per stage; up to {N_STEP} steps per transition) "
                     f"against fresh fits (finder, {WARM_FIRST} warm-up transitions, {MAIN} draws each"
                     + (", parent build)" if parent_lib else ")"))
        for tag, r in seq.items():
            st = r["stages"]
            lines.append(f"sequential, {tag}: {r['seconds']:.1f} s in all (finder {r['init_seconds']:.1f} s, first fit {st[0]['seconds']:.1f} s, "
                         f"days {K0 + 1}-14 {sum(s['seconds'] for s in st[1:]):.1f} s)")
            lines.append("   day  seconds   step  accept  log_pred  ESS median / min   moved")
            for s in st:
                tail = "" if s["log_pred"] is None else (f" {s['log_pred']:9.2f}  {s['ess_median']:8.1f} / {s['ess_min']:.1f}  "
                                                         f"{s['moved']:.1e}")
                lines.append(f"   {s['T']:3d} {s['seconds']:8.1f} {s['step']:6.3f} {s['accept']:7.2f}{tail}")
        lines.append(f"fresh fits: {sum(r['seconds'] for r in fresh.values()):.1f} s in all")
        lines.append("   day  seconds (finder)   step  accept  failed")
        for T, r in fresh.items():
            lines.append(f"   {int(T):3d} {r['seconds']:8.1f} ({r['init_seconds']:.1f}) {r['step']:6.3f} {r['accept']:7.2f} {r['fail']:7.3f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    par = "--parent" in sys.argv
    if "--child-calls" in sys.argv:
        child_calls(par)
    elif "--child-run-seq" in sys.argv:
        child_run(False, False)
    elif "--child-run-fresh" in sys.argv:
        child_run(par, True)
    else:
        main()
