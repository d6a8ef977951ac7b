#!/usr/bin/env python3
"""Coarse warm-up, fine sampling on an MI355X: the FitzHugh-Nagumo posterior of examples/fhn_noisy_chmc.py (T = 100, R = 5,
sigma_y = 0.1) sampled twice -- warm-up and main phase at S steps per observation interval (the plain run), and warm-up at
S / factor with the chains then carried up a ladder of resolutions to S (resolution.coarse_to_fine_static_chmc).
usage: fhn_coarse_to_fine_chmc.py [chains] [S] [factors] [warm-up] [main]
`factors`: the ladder as comma-separated divisors of S, coarsest first, e.g. 8 (S / 8 -> S) or 8,4 (S / 8 -> S / 4 -> S).
Prints the posterior table of both runs side by side, with both wall times."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload  # noqa: E402
from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc  # noqa: E402
from manifold_mcmc_for_diffusions_amd.resolution import coarse_to_fine_static_chmc  # noqa: E402
from manifold_mcmc_for_diffusions_amd import example_models as em  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 400
factors = [int(f) for f in (sys.argv[3] if len(sys.argv) > 3 else "8").split(",")]
n_warm = int(sys.argv[4]) if len(sys.argv) > 4 else 50
n_main = int(sys.argv[5]) if len(sys.argv) > 5 else 100
if any(S % f or f < 2 for f in factors) or sorted(factors, reverse=True) != factors:
    sys.exit("factors must be decreasing divisors of S, each at least 2")
n_fine = max(2, n_warm // 5)                       # re-tuning transitions per finer rung
n_coarse = max(1, n_warm - n_fine * len(factors))  # the same total number of warm-up transitions as the plain run

t0 = time.time()
wl = FhnWorkload(B, num_steps_per_obs=S, device_init=True)
plain = sample_static_chmc(wl.ctx, n_warm + n_main, 16, 0.1, seed=wl.seed, n_adapt=n_warm)
t_plain = time.time() - t0
wl.ctx.close()

t0 = time.time()
coarse = FhnWorkload(B, num_steps_per_obs=S // factors[0], device_init=True)
ladder = [coarse.ctx.sibling(S // f) for f in factors[1:]] + [coarse.ctx.sibling(S)]
c2f = coarse_to_fine_static_chmc(coarse.ctx, ladder, n_coarse, n_fine, n_main, 16, 0.1, seed=coarse.seed)
t_c2f = time.time() - t0

print(f"{B} chains, T = 100, {n_main} main transitions of 16 steps at S = {S}")
print(f"plain:          {n_warm} warm-up transitions at S = {S}; {t_plain:.1f} s with set-up; final step size "
      f"{plain['final_step_size']:.4f}, accept (main) {plain['accept_stat'][n_warm:].mean():.3f}")
print(f"coarse to fine: {t_c2f:.1f} s with set-up = {t_c2f / t_plain:.2f} x plain; per rung:")
for r in c2f["rungs"]:
    moved = "" if r["moved"] is None else (f", n moved by at most {r['moved'].max():.1e} on arrival "
                                           f"(|constr| {r['max_constr']:.1e})")
    print(f"   S = {r['S']:4d}: {r['seconds']:.2f} s, step size {float(r['first_step_size']):.4f} -> {float(r['final_step_size']):.4f}, "
          f"accept {r['mean_accept_stat']:.3f}{moved}")
names, truth = ["sigma", "epsilon", "gamma", "beta"], [0.3, 0.1, 1.5, 0.8]
zp = em.fhn.generate_z(plain["heads"][n_warm:, :, :4])
zc = em.fhn.generate_z(c2f["heads"][n_fine:, :, :4])
print(f"{'':10s}{'true':>6s}   {'plain: mean (sd)':>22s}   {'coarse to fine: mean (sd)':>26s}   R-hat over both runs' chains")
for k in range(4):
    x = np.concatenate([zp[:, :, k], zc[:, :, k]], 1)
    n = x.shape[0]
    within, between = x.var(0, ddof=1).mean(), x.mean(0).var(ddof=1)
    rhat = np.sqrt(((n - 1) / n * within + between) / within)
    print(f"{names[k]:10s}{truth[k]:6.2f}   {zp[:, :, k].mean():12.4f} ({zp[:, :, k].std():.4f})   "
          f"{zc[:, :, k].mean():16.4f} ({zc[:, :, k].std():.4f})   {rhat:.3f}")
for c in ladder + [coarse.ctx]:
    c.close()
