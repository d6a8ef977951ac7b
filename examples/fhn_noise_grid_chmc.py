#!/usr/bin/env python3
"""The reference's noisy FitzHugh-Nagumo sweep (scripts/run_fhn_model_noisy_obs_experiments.sh: observation-noise levels
{0.01, 0.0316, 0.1, 0.316} x data seeds, 4 chains per cell) as ONE context on an MI355X: every chain carries the data and the
noise level of its own grid cell (ChmcContext.set_observations through workload.GridWorkload), every cell adapts its own step
size, and one summary.json per cell is written.

usage: fhn_noise_grid_chmc.py [seeds] [S] [iters] [warm-up] [output dir] [chains per cell] [T] [data steps per obs] [metric]

With the trailing word `metric` every cell also adapts its own block metric M_0 over the dim_u global parameters during the
warm-up (OnlineBlockDiagonalMetricAdapter.finalize_groups, ChmcContext.set_metric(M, groups=...)): the posterior scale of u
differs widely between sigma_y = 0.01 and 0.316.  The adapted diagonal of every cell is printed.

Prints leapfrog steps/s of the batch and, measured in the same process on the same build, of ONE cell run alone (4 chains: how
a sweep runs without per-chain observations, one cell after the other), and their ratio."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd.workload import GridWorkload  # noqa: E402
from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc  # noqa: E402
from manifold_mcmc_for_diffusions_amd.adapters import OnlineBlockDiagonalMetricAdapter  # noqa: E402
from manifold_mcmc_for_diffusions_amd import example_models as em  # noqa: E402

SIGMAS = (0.01, 0.0316, 0.1, 0.316)
n_seed = int(sys.argv[1]) if len(sys.argv) > 1 else 4
S = int(sys.argv[2]) if len(sys.argv) > 2 else 100
n_iter = int(sys.argv[3]) if len(sys.argv) > 3 else 60
n_warm = int(sys.argv[4]) if len(sys.argv) > 4 else 30
out_dir = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
n_chain = int(sys.argv[6]) if len(sys.argv) > 6 else 4
T = int(sys.argv[7]) if len(sys.argv) > 7 else 100
data_steps = int(sys.argv[8]) if len(sys.argv) > 8 else 1000
with_metric = len(sys.argv) > 9 and sys.argv[9] == "metric"
N_STEP = 16
seeds = [20200710 + i for i in range(n_seed)]


def trace_func(head, ham):  # scripts/fhn_model_noisy_obs_chmc_experiment.py:82-99
    z = em.fhn.generate_z(head[:, :4])
    return {"σ": z[:, 0], "ϵ": z[:, 1], "γ": z[:, 2], "β": z[:, 3], "x_0": em.fhn.generate_x_0(z, head[:, 4:6]),
            "hamiltonian": ham}


def run(w, trace_dir):
    t0 = time.time()
    extra = dict(metric_adapter=OnlineBlockDiagonalMetricAdapter(w.ctx.U), metric_per_group=True) if with_metric else {}
    res = sample_static_chmc(w.ctx, n_iter, N_STEP, 0.05, seed=w.seed, n_adapt=n_warm, trace_dir=trace_dir, trace_func=trace_func,
                             groups=w.groups, n_groups=w.n_groups, total_chains=w.total_chains, **extra)
    el = time.time() - t0
    return res, n_iter * N_STEP * w.B / el, el


t0 = time.time()
kw = dict(num_obs=T, num_steps_per_obs_data=data_steps, num_steps_per_obs=S, num_obs_per_subseq=5)
grid = GridWorkload.fhn_noise_grid(SIGMAS, seeds, n_chain, **kw)
print(f"set-up {time.time() - t0:.1f} s: {grid.n_groups} cells x {n_chain} chains = {grid.B} chains in one context, dim_q = "
      f"{grid.ctx.Q}", flush=True)
res, rate_grid, el = run(grid, out_dir)
print(f"grid: {n_iter} transitions x {N_STEP} steps x {grid.B} chains in {el:.1f} s = {rate_grid:.0f} leapfrog steps/s")
for g, (sigma, seed) in enumerate(grid.cell_labels):
    z = em.fhn.generate_z(res["heads"][n_warm:, grid.cell_chains(g), :4])
    print(f"  sigma_y {sigma:<7g} data seed {seed}: step size {res['final_step_size'][g]:.4f}  accept "
          f"{res['group_accept_stat'][n_warm:, g].mean():.2f}  posterior means (sigma, eps, gamma, beta) "
          f"{z.reshape(-1, 4).mean(0).round(3)}")
    if with_metric:
        print(f"    adapted M_0 diagonal {np.diag(res['metric_M_0'][g]).round(2)}")
    if out_dir:
        cell_dir = os.path.join(out_dir, f"sigma_{sigma:g}_seed_{seed}")
        os.makedirs(cell_dir, exist_ok=True)
        cell = dict(res["summary"]["groups"][str(g)], final_integrator_step_size=float(res["final_step_size"][g]),
                    obs_noise_std=sigma, data_seed=seed, num_chains=n_chain,
                    total_sampling_time_of_the_grid=res["summary"]["total_sampling_time"])
        with open(os.path.join(cell_dir, "summary.json"), "w") as f:
            json.dump(cell, f, ensure_ascii=False, indent=2)
grid.ctx.close()

# one cell alone, as a sweep runs today: the same sampler call on a context of that cell's 4 chains
one = GridWorkload.fhn_noise_grid(SIGMAS[2:3], seeds[:1], n_chain, **kw)
_, rate_one, el = run(one, None)
one.ctx.close()
print(f"one cell alone (sigma_y {SIGMAS[2]}): {n_iter} transitions x {N_STEP} steps x {one.B} chains in {el:.1f} s = {rate_one:.0f} "
      f"leapfrog steps/s")
print(f"ratio grid / one cell: {rate_grid / rate_one:.1f} x  (T = {T}, S = {S}, {grid.n_groups} cells)")
