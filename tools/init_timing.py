"""Wall time of initial-state generation.
usage: python tools/init_timing.py [chains]                            FitzHugh-Nagumo bench workload: host (NumPy) against device
       python tools/init_timing.py sir [chains] [legacy|keyed] [sigma]  boarding-school SIR (S = 200): the Adam-based finder, device
                                                                       loop, draws from one generator (legacy) or keyed by
                                                                       (seed, chain, try); sigma: a number or "variable"
       python tools/init_timing.py gd [chains] [noiseless|noisy] [S]   FitzHugh-Nagumo bench workload (T = 100, R = 5): the generic
                                                                       gradient-descent finder (keyed, device-resident) with Adam
                                                                       iterations, projection calls and tries per chain, and
                                                                       chmc_init_linear_interpolation on the same context
The SIR and gd modes print one line per run: two runs on fresh contexts in one process, the second is the figure to quote (the first
pays for the process's HIP and torch start-up)."""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from manifold_mcmc_for_diffusions_amd import example_models as em
from manifold_mcmc_for_diffusions_amd.context import ChmcContext
from manifold_mcmc_for_diffusions_amd import init


def sir(B, mode, sigma):
    from manifold_mcmc_for_diffusions_amd.workload import BOARDING_SCHOOL_COUNTS, SEED
    y = np.asarray(BOARDING_SCHOOL_COUNTS, dtype=np.float64)
    for run in range(2):
        ctx = ChmcContext("sir", 1.0, 200, len(y), y, sigma=sigma, num_chains=B)
        t0 = time.perf_counter()
        if mode == "keyed":
            _, _, tries = init.find_initial_states_by_gradient_descent_noisy_system(
                ctx, seed=SEED, adam_step_size=0.1, max_iters=5000, device_resident=True)
        else:
            _, _, tries = init.find_initial_states_by_gradient_descent_noisy_system(
                ctx, np.random.default_rng(SEED), adam_step_size=0.1, max_iters=5000, device_resident=True)
        dt = time.perf_counter() - t0
        print(f"sir {B} chains sigma={sigma} {mode} run {run}: {dt:.3f} s; tries max {int(tries.max())} mean {tries.mean():.3f}",
              flush=True)
        ctx.close()


def gd(B, noisy, S):
    from manifold_mcmc_for_diffusions_amd.workload import SEED
    sigma = 0.1 if noisy else None
    y = em.simulate_fhn_observations(100, 0.2, 10000, seed=SEED, sigma=sigma)
    for run in range(2):
        ctx = ChmcContext("fhn", 0.2, S, 5, y[:, 0], sigma=sigma, num_chains=B)
        t0 = time.perf_counter()
        _, _, tries, st = init.find_initial_states_by_gradient_descent(ctx, init.fhn_x_obs_seq_init(y[:, 0], SEED), SEED,
                                                                        return_status=True)
        t1 = time.perf_counter()
        err = np.abs(ctx.constr()).max()
        t2 = time.perf_counter()
        init.fhn_initial_states_device(ctx, em.fhn, y)
        t3 = time.perf_counter()
        print(f"gd fhn {'noisy' if noisy else 'noiseless'} T=100 S={S} R=5 {B} chains run {run}: gradient descent {t1 - t0:.3f} s, "
              f"{st['adam_iterations']} Adam iterations, {st['projection_calls']} projection calls, tries per chain max "
              f"{int(tries.max())} mean {tries.mean():.3f}, max|constr| {err:.1e}; linear interpolation (draws + solve + evaluate) "
              f"{t3 - t2:.3f} s", flush=True)
        ctx.close()


if len(sys.argv) > 1 and sys.argv[1] == "gd":
    gd(int(sys.argv[2]) if len(sys.argv) > 2 else 256, (sys.argv[3] if len(sys.argv) > 3 else "noiseless") == "noisy",
       int(sys.argv[4]) if len(sys.argv) > 4 else 400)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "sir":
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    mode = sys.argv[3] if len(sys.argv) > 3 else "legacy"
    sigma = sys.argv[4] if len(sys.argv) > 4 else "1.0"
    sir(B, mode, sigma if sigma == "variable" else float(sigma))
    sys.exit(0)

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
y = em.simulate_fhn_observations(100, 0.2, 10000, seed=20200710, sigma=0.1)
ctx = ChmcContext("fhn", 0.2, 400, 5, y[:, 0], sigma=0.1, num_chains=B)
t0 = time.perf_counter()
q, xo, _ = init.fhn_initial_states(em.fhn, 0.2, 400, y, B, True)
t1 = time.perf_counter()
ctx.set_state(q, None, xo, 0)
t2 = time.perf_counter()
init.fhn_initial_states_device(ctx, em.fhn, y)
t3 = time.perf_counter()
qd = ctx.get_state()[0]
print(f"{B} chains: host solve {t1 - t0:.2f} s + upload/evaluate {t2 - t1:.3f} s; device (draws + solve + evaluate) "
      f"{t3 - t2:.3f} s; max |q_dev - q_host| = {np.abs(qd - q).max():.2e}")
