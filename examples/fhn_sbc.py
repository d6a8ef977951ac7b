#!/usr/bin/env python3
"""Simulation-based calibration of the constrained-HMC sampler on a small noisy FitzHugh-Nagumo shape, on an MI355X: one data
set per chain, all chains in one context.

Every chain draws its latent state q = [u | v_0 | v_seq | n] from the prior, simulates its own data from it and starts ON that
draw (ChmcContext.simulate_observations): an exact draw from its own posterior, so no initial-state finder and no burn-in are
needed for the check to be valid.  The dynamic (no-U-turn) sampler then runs; the thinning is chosen from the measured
effective sample size of the run; the rank of the prior draw of each u component among the thinned posterior draws must be
uniform (sbc.py).  Needs neither of the project's oracles.

usage: fhn_sbc.py [data sets] [iters] [warm-up] [T] [S] [sigma] [seed]
Exits non-zero when any parameter has p < 1e-4 (family-wise false-alarm rate about 5e-4 over the four parameters)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd import sbc  # noqa: E402
from manifold_mcmc_for_diffusions_amd.context import ChmcContext  # noqa: E402
from manifold_mcmc_for_diffusions_amd.dynamic import sample_dynamic_chmc  # noqa: E402
from manifold_mcmc_for_diffusions_amd.traces import split_rhat_and_ess  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 512
n_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 400
n_warm = int(sys.argv[3]) if len(sys.argv) > 3 else 100
T = int(sys.argv[4]) if len(sys.argv) > 4 else 10
S = int(sys.argv[5]) if len(sys.argv) > 5 else 10
sigma = float(sys.argv[6]) if len(sys.argv) > 6 else 0.3
seed = int(sys.argv[7]) if len(sys.argv) > 7 else 20200710
P, R = 4, 5
names = ["u[0] (log sigma)", "u[1] (log epsilon)", "u[2] (log gamma)", "u[3] (beta)"]

t0 = time.time()
ctx = ChmcContext("fhn", 0.2, S, R, np.zeros(T), sigma=sigma, num_chains=D)
ctx.simulate_observations(seed)
prior_u = ctx.get_head(P)
print(f"set-up {time.time() - t0:.1f} s: {D} data sets, one chain each, T = {T}, S = {S}, sigma_y = {sigma}, dim_q = {ctx.Q}; "
      f"max |constr| after simulate_observations {np.abs(ctx.constr()).max():.1e}", flush=True)
t0 = time.time()
res = sample_dynamic_chmc(ctx, n_iter, 0.1, seed=seed, n_adapt=n_warm, n_head=P, groups=np.arange(D), n_groups=D,
                          callback=lambda it, h, a, e, st: (it % 50 == 0) and print(
                              f"  iter {it:4d} accept {a:.2f} mean step {e:.3f} steps per tree {st['n_step'].mean():.1f}", flush=True))
el = time.time() - t0
main = res["heads"][n_warm:].transpose(1, 0, 2)  # [D, n_main, P]
n_main = main.shape[1]
print(f"{n_iter} transitions x {D} chains in {el:.1f} s = {float(res['n_step'].sum()) * D / el:.0f} leapfrog steps/s; "
      f"integrator errors {res['integrator_error'][n_warm:].mean():.4f}; chains that never moved in the main phase "
      f"{int((res['chain_outcomes_dynamic'][:, 0] == 0).sum())}")
# thinning from the measured effective sample size: per chain and parameter, then the lower quartile over everything
ess = np.array([[split_rhat_and_ess(main[c:c + 1, :, j])[1] for j in range(P)] for c in range(D)])
ess_q = float(np.nanquantile(ess, 0.25))
thin = max(1, int(np.ceil(n_main / max(ess_q, 1.0))))
L = n_main // thin
draws = main[:, n_main - L * thin::thin][:, :L]
bins = int(min(L + 1, max(2, D // 20)))
print(f"ESS per chain and parameter over {n_main} main draws: median {np.nanmedian(ess):.0f}, lower quartile {ess_q:.0f} -> "
      f"thinning {thin}, L = {L} draws per data set, {bins} bins (expected count {D / bins:.1f})")
ranks = sbc.ranks(prior_u, draws)
stat, p = sbc.uniformity(ranks, L, bins)
for j in range(P):
    print(f"  {names[j]:20s} chi^2({bins - 1}) = {stat[j]:7.2f}  p = {p[j]:.4f}  ranks {np.bincount(ranks[:, j], minlength=L + 1).tolist()}")
ctx.close()
if (p < 1e-4).any():
    print("SBC FAILED: a rank distribution is not uniform (p < 1e-4)")
    sys.exit(1)
print("SBC passed: no parameter with p < 1e-4")
