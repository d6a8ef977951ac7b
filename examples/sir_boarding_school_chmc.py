#!/usr/bin/env python3
"""End-to-end example on an MI355X: the SIR model with a time-varying contact rate on the boarding-school influenza
data, as scripts/sir_model_chmc_experiment.py of the reference sets it up (14 daily counts, 20 steps per observation,
one sub-sequence of 14 observations, sigma_y = 1): batched initial states by the Adam-based finder of the noisy system
(sde/mici_extensions.py:1679-1801), then batched constrained HMC.
usage: sir_boarding_school_chmc.py [chains] [iterations] [warm-up] [steps per trajectory] [output dir]
       [--keyed-init] [--chain-offset N] [--total-chains N] [--path-posterior STRIDE] [--forecast DAYS]
       [--peak] [--exceed COUNT] [--coarse-warmup M] [--sequential K]
--sequential K: the data arrive a day at a time.  The first K days are fitted as usual (finder, warm-up, main phase); every
later day is added by sequential.sequential_static_chmc: the chains are carried into a context with one more observation
(64 keyed forecast candidates per chain, weighed by the count that arrived, one drawn in proportion to its weight), the step
size is re-tuned over a fifth of the warm-up transitions and the main phase runs again.  Per day the table shows the log
predictive score of that day's count given the days before (log-mean-exp over the chains), the candidates' effective sample
size (median and minimum over the chains), `moved` (the change of the observation-noise part on arrival, in units of
sigma_y), the re-tuned step size, the main-phase accept statistic and the seconds; with --forecast also the one-day-ahead
forecast band of that day's count from the fit of the days before.  The other options are ignored.
--coarse-warmup M: the initial states are found and the warm-up runs in a context with 20 / M steps per observation (M = 2, 4
or 5); the chains are then carried into the context with 20 steps (resolution.coarse_to_fine_static_chmc: the driving noise
refined as the same Brownian path, the observation noise solved from the constraint), the step size is re-tuned there over
a fifth of the warm-up transitions and the main phase runs as without the option.  The printed `n moved by at most` is the
change of the observation-noise part on arrival, in units of sigma_y.  With these data (counts near 300, sigma_y = 1) the
Euler-Maruyama path at 10 or 5 steps per day differs from the one at 20 by about 1e2 sigma_y around the peak (measured: 95
for M = 2, 120 for M = 4), so the chains arrive far from equilibrium and the sampling context has to settle them again:
here the option shows the mechanics; it pays where `moved` is small (examples/fhn_coarse_to_fine_chmc.py: below 1e-1).
--peak: the posterior of the infected curve's peak size and the day it falls on: path-wise events of I(t) = obs_func(x) at
every step of every post-warm-up state (paths.PathEvents, evaluated on the device and traced like the parameters).
--exceed COUNT (with --forecast): P(the observed count reaches COUNT on some day of the forecast) and the first-passage day,
from the event summaries of every replicate future (PredictivePosterior(events=...)).
--forecast DAYS: posterior predictive forecast of the observed count for DAYS days after day 14: 64 replicate futures of every
post-warm-up state with fresh driving and observation noise (paths.PredictivePosterior, simulated on the device); the band
(mean, sd and the 5 / 50 / 95 % points of the predictive CDF over levels 0, 2, .. 800) is printed per day and `predictive.npz`
is written next to the traces.
--path-posterior STRIDE: accumulate the posterior moments of the latent path (S, I and the contact rate at every STRIDE-th step,
and the observed count) over the main phase; `path_posterior.npz` is written next to the traces and the infected-curve band
is printed beside the data.
--keyed-init: the finder's start and restart points are keyed by (seed, global chain, try) instead of drawn from one generator
for the batch, and the sampler's streams by the global chain: this process runs chains chain-offset .. chain-offset + chains
- 1 of a job of total-chains chains, and any split of the job into such processes gives every chain the same states."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd import example_models as em, init  # noqa: E402
from manifold_mcmc_for_diffusions_amd.context import ChmcContext  # noqa: E402
from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc  # noqa: E402

a = sys.argv[1:]
opts = {"--keyed-init": False, "--chain-offset": 0, "--total-chains": None, "--path-posterior": None, "--forecast": None,
        "--peak": False, "--exceed": None, "--coarse-warmup": None, "--sequential": None}
FLAGS = ("--keyed-init", "--peak")
for name in list(opts):
    if name in a:
        i = a.index(name)
        opts[name] = True if name in FLAGS else int(a[i + 1])
        del a[i:i + (1 if name in FLAGS else 2)]
keyed, chain_offset, total_chains = opts["--keyed-init"], opts["--chain-offset"], opts["--total-chains"]
path_stride, forecast, peak, exceed = opts["--path-posterior"], opts["--forecast"], opts["--peak"], opts["--exceed"]
coarse_m, sequential = opts["--coarse-warmup"], opts["--sequential"]
if coarse_m is not None and (coarse_m < 2 or 20 % coarse_m):
    sys.exit("--coarse-warmup M needs M >= 2 that divides 20")
if exceed is not None and not forecast:
    sys.exit("--exceed needs --forecast DAYS")
B = int(a[0]) if len(a) > 0 else 256
n_iter = int(a[1]) if len(a) > 1 else 300
n_warm = int(a[2]) if len(a) > 2 else 100
n_step = int(a[3]) if len(a) > 3 else 16
out_dir = a[4] if len(a) > 4 else None
data = np.load(os.path.join(ROOT, "tests", "golden", "reference_data", "sir_model_boarding_school_data.npz"))
y, obs_interval = np.asarray(data["y_seq"], dtype=np.float64).reshape(-1), float(data["obs_interval"])
m = em.sir
if sequential is not None and not 2 <= sequential < len(y):
    sys.exit(f"--sequential K needs 2 <= K < {len(y)}")
if sequential is not None:
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    from manifold_mcmc_for_diffusions_amd.sequential import sequential_static_chmc
    K = sequential
    ctx = ChmcContext("sir", obs_interval, 20, None, y[:K], sigma=1.0, num_chains=B)
    print(f"SIR, sequential: {B} chains, days 1-{K} fitted first (dim_q = {ctx.Q}), then a day at a time to day {len(y)}")
    t0 = time.time()
    q, xo, tries = init.find_initial_states_by_gradient_descent_noisy_system(
        ctx, np.random.default_rng(20200710), adam_step_size=1e-1, max_iters=5000, log=print)
    print(f"initial states in {time.time() - t0:.1f} s, |c|max {np.abs(ctx.constr()).max():.1e}")
    bands = {}

    def stage_kw(i, c):  # the one-day-ahead forecast of the next day's count from this stage's fit
        if not forecast or c.T == len(y):
            return {}
        bands[c.T + 1] = PredictivePosterior(c, 1, n_rep=64, levels=np.arange(0.0, 801.0, 2.0))
        return {"predictive": bands[c.T + 1]}

    t0 = time.time()
    res = sequential_static_chmc(ctx, [y[d:d + 1] for d in range(K, len(y))], n_warm, max(2, n_warm // 5), n_iter - n_warm,
                                 n_step, 0.05, seed=7, n_cand=64, stage_kw=stage_kw, n_head=5, jitter_length=True)
    print(f"days {K + 1}-{len(y)} added in {time.time() - t0:.1f} s including the first fit "
          f"({res['stages'][0]['seconds']:.1f} s, step size {float(res['stages'][0]['final_step_size']):.3f}, accept "
          f"{res['stages'][0]['mean_accept_stat']:.2f})")
    print("   day  count  log_pred  ESS med  min   moved    step  accept  seconds" + ("   forecast E +- sd     5 %    50 %    95 %" if forecast else ""))
    for st in res["stages"][1:]:
        row = (f"  {st['T']:4d} {y[st['T'] - 1]:6.0f} {st['log_pred']:9.2f} {np.median(st['ess_cand']):8.1f} {st['ess_cand'].min():4.1f} "
               f"{st['moved'].max():7.1e} {float(st['final_step_size']):7.3f} {st['mean_accept_stat']:7.2f} {st['seconds']:8.1f}")
        if forecast and st["T"] in bands:
            pool = bands[st["T"]].pooled()
            qs = bands[st["T"]].quantiles([0.05, 0.5, 0.95], cdf=pool["cdf"])
            row += f"   {pool['mean'][0, -1]:7.1f} +- {pool['sd'][0, -1]:5.1f} {qs[0, 0]:7.1f} {qs[0, 1]:7.1f} {qs[0, 2]:7.1f}"
        print(row)
    total = sum(st["log_pred"] for st in res["stages"][1:])
    print(f"log p(y_{K + 1}..{len(y)} | y_1..{K}) = {total:.2f} (sum of the days' scores); final max |constraint| "
          f"{np.abs(res['ctx'].constr()).max():.1e}")
    sys.exit(0)
ctx = ChmcContext("sir", obs_interval, 20 // (coarse_m or 1), 14, y, sigma=1.0, num_chains=B)
print(f"SIR: {B} chains, dim_q = {ctx.Q}, {ctx.num_blocks} sub-sequence of {len(y)} observations, {ctx.RM}-row kernels")
rng = np.random.default_rng(20200710)
t0 = time.time()
if keyed:
    total_chains = chain_offset + B if total_chains is None else total_chains
    q, xo, tries = init.find_initial_states_by_gradient_descent_noisy_system(
        ctx, seed=20200710, chain_offset=chain_offset, total_chains=total_chains, adam_step_size=1e-1, max_iters=5000, log=print)
else:
    q, xo, tries = init.find_initial_states_by_gradient_descent_noisy_system(ctx, rng, adam_step_size=1e-1, max_iters=5000,
                                                                             log=print)
print(f"initial states in {time.time() - t0:.1f} s (restarts per chain: max {tries.max() - 1}), |c|max "
      f"{np.abs(ctx.constr()).max():.1e}")


def trace_func(head, ham):  # scripts/sir_model_chmc_experiment.py:75-94
    z = m.generate_z(head[:, :4])
    return {"α₀": m.generate_x_0(z, head[:, 4:5])[:, -1], "β": z[:, 0], "γ": z[:, 1], "ζ": z[:, 2], "ϵ": z[:, 3],
            "hamiltonian": ham}


coarse = None
if coarse_m:  # everything below belongs to the sampling context; the warm-up context hands its chains over
    coarse, ctx = ctx, ctx.sibling(20)
    print(f"warm-up at {coarse.S} steps per observation (dim_q = {coarse.Q}), sampling at {ctx.S}")
pp = None
if path_stride:
    from manifold_mcmc_for_diffusions_amd.paths import PathPosterior
    pp = PathPosterior(ctx, path_stride)
pred = None
if forecast:
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    events = None if exceed is None else dict(channel=ctx.X + 1, thresholds=[float(exceed)])  # y_rep over the whole horizon
    pred = PredictivePosterior(ctx, forecast, n_rep=64, levels=np.arange(0.0, 801.0, 2.0), events=events)
pe = None
if peak:
    from manifold_mcmc_for_diffusions_amd.paths import PathEvents
    pe = PathEvents(ctx, ctx.X, stride=path_stride or 1, path_posterior=pp)  # with --path-posterior: on its scratch path
t0 = time.time()
if coarse is not None:
    from manifold_mcmc_for_diffusions_amd.resolution import coarse_to_fine_static_chmc

    def sample_static_chmc(ctx, n_iter, n_step, step_size, seed, n_adapt, **kw):  # noqa: F811
        """The call below with the warm-up in the coarse context: a fifth of it re-tunes the step size in `ctx`."""
        n_fine = max(2, n_adapt // 5)
        return coarse_to_fine_static_chmc(coarse, ctx, max(1, n_adapt - n_fine), n_fine, n_iter - n_adapt, n_step, step_size,
                                          seed=seed, **kw)
res = sample_static_chmc(ctx, n_iter, n_step, 0.05, seed=7, n_adapt=n_warm, n_head=5, jitter_length=True, path_posterior=pp,
                         **({} if pred is None else {"predictive": pred}), **({} if pe is None else {"path_events": pe}),
                         chain_offset=chain_offset, total_chains=total_chains if keyed else None,
                         trace_dir=out_dir or os.path.join(ROOT, "gpurun_out", "sir_run"), trace_func=trace_func,
                         callback=lambda it, h, acc, e: (it % 25 == 0) and print(
                             f"  iter {it:4d} accept {acc:.2f} step {e:.3f}", flush=True))
if coarse is not None:
    for r in res["rungs"]:
        print(f"  S = {r['S']:3d}: {r['seconds']:.1f} s, step size {float(r['first_step_size']):.3f} -> "
              f"{float(r['final_step_size']):.3f}, accept {r['mean_accept_stat']:.2f}"
              + ("" if r["moved"] is None else f", n moved by at most {r['moved'].max():.1e} on arrival"))
    n_fine = max(2, n_warm // 5)
    n_iter, n_warm = n_fine + n_iter - n_warm, n_fine  # (the traces below are the sampling context's)
el = time.time() - t0
sm = res["summary"]
print(f"{n_iter} transitions x <= {n_step} steps x {B} chains in {el:.1f} s; final step size "
      f"{res['final_step_size']:.3f}, accept {res['accept_stat'][n_warm:].mean():.2f}, failed trajectories "
      f"{res['fail_rate'][n_warm:].mean():.3f}")
for k in ("α₀", "β", "γ", "ζ", "ϵ"):
    print(f"  {k:3s} mean {sm['mean'][k]:8.4f} sd {sm['sd'][k]:7.4f}  r_hat {sm['r_hat'][k]:.3f} ess {sm['ess_bulk'][k]:7.0f}")
if pp is not None:
    pool, per_obs = res["path_posterior"], ctx.S // pp.stride
    trace_dir = os.path.dirname(next(iter(res["trace_files"].values())))  # next to the traces
    print(f"path posterior: {pool['n']} draws pooled over the chains, {pp.NP} points per path -> {pp.save(trace_dir)}")
    print("   day  count   E[I(t)] +- sd")
    for k, yk in enumerate(y):
        p = (k + 1) * per_obs
        print(f"  {pp.times[p]:5.1f} {yk:6.0f}   {pool['mean'][p, -1]:7.1f} +- {pool['sd'][p, -1]:.1f}")
if pred is not None:
    pool = res["predictive"]
    trace_dir = os.path.dirname(next(iter(res["trace_files"].values())))
    qs = pred.quantiles([0.05, 0.5, 0.95], cdf=pool["cdf"])
    print(f"forecast: {pool['n']} replicate futures pooled over the chains -> {pred.save(trace_dir)}")
    print("   day   E[count] +- sd      5 %    50 %    95 %")
    for p, t in enumerate(pred.times):
        print(f"  {t:5.1f}   {pool['mean'][p, -1]:7.1f} +- {pool['sd'][p, -1]:5.1f}  {qs[p, 0]:7.1f} {qs[p, 1]:7.1f} {qs[p, 2]:7.1f}")
    if exceed is not None:
        ev = pool["events"]
        i = ev["names"].index("t_first_0")
        print(f"P(count >= {exceed} on some day of the {forecast}-day forecast) = {ev['reached'][i]:.3f} "
              f"({ev['n'][i]} of {pool['n']} replicate futures); first passage, given it happens: day {ev['mean'][i]:.1f} "
              f"+- {np.sqrt(ev['var'][i]):.1f}; peak of the forecast count {ev['mean'][0]:.0f} +- {np.sqrt(ev['var'][0]):.0f}")
if pe is not None:
    sm = res["path_events_summary"]
    print(f"peak of the infected curve over {res['path_events'].shape[0]} draws x {B} chains:")
    for k, label in (("max", "size"), ("t_max", "day ")):
        print(f"  {label} mean {sm['mean'][k]:8.2f} sd {sm['sd'][k]:7.2f}  r_hat {sm['r_hat'][k]:.3f} ess {sm['ess_bulk'][k]:7.0f}")
