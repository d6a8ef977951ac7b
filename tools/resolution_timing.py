"""Cost and effect of carrying chains between time resolutions on one MI355X.
usage: python tools/resolution_timing.py [warm-up transitions] [main transitions] [output file]
       python tools/resolution_timing.py --noiseless [warm-up transitions] [main transitions] [output file]

FitzHugh-Nagumo configs[1] (256 chains, T = 100, R = 5, sigma = 0.1, 16-step transitions), two runs in ONE process; the
record is appended per run and the second one is the figure to quote (the first carries the one-off costs of the process).
  (a) one resolution.transfer_state 50 -> 400 and 200 -> 400 (host clock around calls that end in a device synchronise,
      median over REPS), the resample kernel alone from the library's HIP events (chmc_profile_*, class 8) with its store
      bandwidth as a fraction of the 8 TB/s peak, beside one 16-step transition at S = 400;
  (b) the plain warm-up at S = 400 (sample_static_chmc alone) against the warm-up through S = 50 and through
      50 -> 100 -> 400 with the same total number of warm-up transitions: wall times, final step sizes, the main phase's
      accept statistic, moved;
  (c) posterior means and sds of the u components from the routes' main phases, with R-hat over the pooled chains of the
      plain and each coarse route.
--noiseless: the same question at configs[2] (no observation noise, 256 chains), where the carried state is PROJECTED
(chmc_set_state_project_device), one run, appended to profiles/resolution_noiseless_timing.txt:
  (a) one transfer_state 50 -> 400 and 200 -> 400, host clock around the call (it ends in a synchronise), the second of two
      runs; the Newton iterations per chain, defect, moved and tries;
  (b) the warm-up (default 150 transitions) plain at S = 400 against four fifths of it at S = 50 and one fifth at S = 400:
      wall times, final step sizes and the main phase's accept statistic, both routes in this one session."""
import ctypes as C
import os
import socket
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

B, N_STEP, EPS0, REPS = 256, 16, 0.1, 5
PEAK = 8.0e12


def kernel_ms(L, call, cls=8):
    """HIP-event time of the launches of kernel class `cls` inside call(), in ms, and their number."""
    from manifold_mcmc_for_diffusions_amd import _lib
    L.chmc_profile_enable(1 << cls)
    call()
    ms, n = np.zeros(10), np.zeros(10, dtype=np.int64)
    L.chmc_profile_get(ms.ctypes.data_as(_lib.dp), n.ctypes.data_as(C.POINTER(C.c_longlong)))
    L.chmc_profile_enable(0)
    return float(ms[cls]), int(n[cls])


def median_ms(call, reps=REPS):
    got = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        got.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(got)), min(got), max(got)


def rhat_pooled(a, b):
    """R-hat of one scalar over the chains of two runs pooled: a, b [draws, chains]."""
    x = np.concatenate([a, b], 1)
    n = x.shape[0]
    within, between = x.var(0, ddof=1).mean(), x.mean(0).var(ddof=1)
    return float(np.sqrt(((n - 1) / n * within + between) / within))


def one_run(n_warm, n_main, run):
    import torch
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state, coarse_to_fine_static_chmc
    from manifold_mcmc_for_diffusions_amd.devbuf import DeviceBuffers
    lines = [f"== run {run}: carrying {B} FitzHugh-Nagumo chains (configs[1]) between resolutions, "
             f"{torch.cuda.get_device_name(0)} on {socket.gethostname()}"]
    # ---- (a)
    ms = lambda t: f"{t[0]:.2f} ms ({t[1]:.2f} .. {t[2]:.2f})"  # noqa: E731
    fine = FhnWorkload(B, num_steps_per_obs=400, device_init=True)
    L = fine.ctx.L
    for S_src in (50, 200):
        src = FhnWorkload(B, num_steps_per_obs=S_src, device_init=True)
        dst = src.ctx.sibling(400)
        t_all = median_ms(lambda: transfer_state(src.ctx, dst, 7))
        buf_src, buf_dst = DeviceBuffers(src.ctx, dict(q=(B, src.ctx.Q))), DeviceBuffers(dst, dict(q=(B, dst.Q)))
        q_src, q_dst = buf_src.ptr("q"), buf_dst.ptr("q")
        src.ctx.get_state_device(q_src, None)
        t_call = median_ms(lambda: dst.resample_q_device(q_src, src.ctx.S, 7, q_dst))
        k_ms, k_n = kernel_ms(L, lambda: [dst.resample_q_device(q_src, src.ctx.S, 7, q_dst, draw=d) for d in range(REPS)])
        k_ms = k_ms / k_n if k_n and k_ms > 0 else float("nan")
        stored = 8.0 * B * dst.T * dst.S * dst.V
        lines.append(f"(a) transfer_state {S_src} -> 400: {ms(t_all)}; chmc_resample_q_device alone {ms(t_call)}; its kernel by HIP "
                     f"events {k_ms * 1e3:.1f} us per launch ({k_n} launches) = {stored / (k_ms * 1e-3) / 1e12:.2f} TB/s of stores "
                     f"({stored / 1e6:.0f} MB) = {100 * stored / (k_ms * 1e-3) / PEAK:.1f} % of the 8 TB/s peak")
        dst.close(), src.ctx.close()
        del buf_src, buf_dst
    for _ in range(2):
        fine.refresh_momentum()
        fine.ctx.leapfrog_steps(EPS0 / 4, N_STEP, **fine.solver)
        fine.ctx.switch_partition()
    t16 = median_ms(lambda: (fine.refresh_momentum(), fine.ctx.leapfrog_steps(EPS0 / 4, N_STEP, **fine.solver)))
    lines.append(f"    one {N_STEP}-step transition at S = 400: {ms(t16)}")
    fine.ctx.close()
    # ---- (b) and (c)
    routes = {}
    t0 = time.perf_counter()
    plain = FhnWorkload(B, num_steps_per_obs=400, device_init=True)
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = sample_static_chmc(plain.ctx, n_warm, N_STEP, EPS0, seed=plain.seed, n_adapt=n_warm)
    t_warm = time.perf_counter() - t0
    t0 = time.perf_counter()
    main = sample_static_chmc(plain.ctx, n_main, N_STEP, res["final_step_size"], seed=plain.seed + 100)
    routes["plain 400"] = dict(warm_s=t_warm, main_s=time.perf_counter() - t0, eps=[res["final_step_size"]],
                               acc=float(main["accept_stat"].mean()), heads=main["heads"], moved=None, setup_s=t_setup)
    plain.ctx.close()
    n_fine = max(2, n_warm // 5)
    for name, ladder_S in (("50 -> 400", (400,)), ("50 -> 100 -> 400", (100, 400))):
        t0 = time.perf_counter()
        coarse = FhnWorkload(B, num_steps_per_obs=50, device_init=True)
        ladder = [coarse.ctx.sibling(S) for S in ladder_S]
        t_setup = time.perf_counter() - t0
        n_coarse = n_warm - n_fine * len(ladder)
        t0 = time.perf_counter()
        out = coarse_to_fine_static_chmc(coarse.ctx, ladder, n_coarse, n_fine, 0, N_STEP, EPS0, seed=coarse.seed)
        t_warm = time.perf_counter() - t0
        t0 = time.perf_counter()
        main = sample_static_chmc(ladder[-1], n_main, N_STEP, out["final_step_size"], seed=coarse.seed + 100)
        routes[name] = dict(warm_s=t_warm, main_s=time.perf_counter() - t0, eps=[r["final_step_size"] for r in out["rungs"]],
                            acc=float(main["accept_stat"].mean()), heads=main["heads"], setup_s=t_setup,
                            moved=[float(np.max(r["moved"])) for r in out["rungs"][1:]],
                            split=[n_coarse] + [n_fine] * len(ladder),
                            rung_s=[r["seconds"] for r in out["rungs"]])
        for c in ladder + [coarse.ctx]:
            c.close()
    p = routes["plain 400"]
    lines.append(f"(b) warm-up of {n_warm} transitions, then {n_main} main transitions at S = 400 ({N_STEP} steps each):")
    for name, r in routes.items():
        extra = "" if r["moved"] is None else (f"; transitions per rung {r['split']}, seconds per rung "
                                               f"{[round(s, 2) for s in r['rung_s']]}; max moved per transfer "
                                               f"{['%.1e' % m for m in r['moved']]}")
        lines.append(f"    {name:18s} warm-up {r['warm_s']:.2f} s = {r['warm_s'] / p['warm_s']:.3f} x plain (set-up "
                     f"{r['setup_s']:.2f} s apart); final step sizes {[round(float(e), 4) for e in r['eps']]}; main phase "
                     f"{r['main_s']:.2f} s, accept statistic {r['acc']:.3f}{extra}")
    lines.append("(c) u components over the main phase, mean (sd) over draws and chains, R-hat over the route's own chains; "
                 "'pooled': R-hat over the chains of the plain route and the coarse one together:")
    for k, nm in enumerate(("log sigma", "log epsilon", "log gamma", "beta")):
        row = f"    {nm:12s}"
        for name, r in routes.items():
            h = r["heads"][:, :, k]
            half = h.shape[1] // 2
            row += f"  {name}: {h.mean():+.4f} ({h.std():.4f}) R-hat {rhat_pooled(h[:, :half], h[:, half:]):.3f}"
            if name != "plain 400":
                row += f" pooled {rhat_pooled(p['heads'][:, :, k], h):.3f}"
        lines.append(row)
    return lines


def noiseless_run(n_warm, n_main):
    import torch
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state, coarse_to_fine_static_chmc
    lines = [f"== carrying {B} noiseless FitzHugh-Nagumo chains (configs[2]) between resolutions, "
             f"{torch.cuda.get_device_name(0)} on {socket.gethostname()}"]
    for S_src in (50, 200):
        src = FhnWorkload(B, num_steps_per_obs=S_src, sigma=None)
        dst = src.ctx.sibling(400)
        took = []
        for _ in range(2):
            t0 = time.perf_counter()
            tr = transfer_state(src.ctx, dst, 7)
            took.append((time.perf_counter() - t0) * 1e3)
        it, df = tr["iters"], tr["defect"]
        lines.append(f"(a) transfer_state {S_src} -> 400: {took[1]:.1f} ms (first call {took[0]:.1f} ms); Newton iterations per chain "
                     f"min {it.min()} mean {it.mean():.2f} max {it.max()}, chains per count {np.bincount(it).tolist()}; defect min "
                     f"{df.min():.1e} median {np.median(df):.1e} max {df.max():.1e}; moved max {tr['moved'].max():.1e}; tries max "
                     f"{tr['tries'].max()}; max |constraint| afterwards {tr['max_constr']:.1e}")
        dst.close(), src.ctx.close()
    n_fine = max(2, n_warm // 5)
    routes = {}
    t0 = time.perf_counter()
    plain = FhnWorkload(B, num_steps_per_obs=400, sigma=None)
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = sample_static_chmc(plain.ctx, n_warm, N_STEP, EPS0, seed=plain.seed, n_adapt=n_warm)
    t_warm = time.perf_counter() - t0
    t0 = time.perf_counter()
    main = sample_static_chmc(plain.ctx, n_main, N_STEP, res["final_step_size"], seed=plain.seed + 100)
    routes["plain 400"] = dict(warm_s=t_warm, main_s=time.perf_counter() - t0, eps=[res["final_step_size"]], setup_s=t_setup,
                               acc=float(main["accept_stat"].mean()), fail=float(main["fail_rate"].mean()), extra="")
    plain.ctx.close()
    t0 = time.perf_counter()
    coarse = FhnWorkload(B, num_steps_per_obs=50, sigma=None)
    fine = coarse.ctx.sibling(400)
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = coarse_to_fine_static_chmc(coarse.ctx, fine, n_warm - n_fine, n_fine, 0, N_STEP, EPS0, seed=coarse.seed)
    t_warm = time.perf_counter() - t0
    t0 = time.perf_counter()
    main = sample_static_chmc(fine, n_main, N_STEP, out["final_step_size"], seed=coarse.seed + 100)
    r1 = out["rungs"][1]
    routes["50 -> 400"] = dict(
        warm_s=t_warm, main_s=time.perf_counter() - t0, eps=[r["final_step_size"] for r in out["rungs"]], setup_s=t_setup,
        acc=float(main["accept_stat"].mean()), fail=float(main["fail_rate"].mean()),
        extra=f"; transitions per rung {[n_warm - n_fine, n_fine]}, seconds per rung {[round(r['seconds'], 2) for r in out['rungs']]}; "
              f"carried over with {r1['proj_iters'].min()} to {r1['proj_iters'].max()} Newton iterations, defect max "
              f"{r1['defect'].max():.1e}, moved max {r1['moved'].max():.1e}, tries max {r1['tries'].max()}")
    fine.close(), coarse.ctx.close()
    p = routes["plain 400"]
    lines.append(f"(b) warm-up of {n_warm} transitions, then {n_main} main transitions at S = 400 ({N_STEP} steps each):")
    for name, r in routes.items():
        lines.append(f"    {name:10s} warm-up {r['warm_s']:.2f} s = {r['warm_s'] / p['warm_s']:.3f} x plain (set-up {r['setup_s']:.2f} s "
                     f"apart); final step sizes {[round(float(np.mean(e)), 4) for e in r['eps']]}; main phase {r['main_s']:.2f} s, "
                     f"accept statistic {r['acc']:.3f}, failed trajectories {r['fail']:.3f}{r['extra']}")
    return lines


def main():
    if "--noiseless" in sys.argv:
        sys.argv.remove("--noiseless")
        n_warm = int(sys.argv[1]) if len(sys.argv) > 1 else 150
        n_main = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "resolution_noiseless_timing.txt")
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        lines = noiseless_run(n_warm, n_main)
        print("\n".join(lines), flush=True)
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n\n")
        return
    n_warm = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    n_main = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "resolution_timing.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for run in (1, 2):
        lines = one_run(n_warm, n_main, run)
        print("\n".join(lines), flush=True)
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
