"""A minimal batched sampler on top of the device step: static-length (optionally jittered) constrained HMC
trajectories with a Metropolis accept step, momentum refresh, partition switching and dual-averaging step-size
adaptation.

The reference drives the same integrator with Mici's dynamic multinomial (NUTS-style) transition
(scripts/utils.py:292-306); the batched counterpart of that transition is dynamic.py.  This static variant targets the
same posterior (it is a valid Markov kernel for it), costs no per-leaf bookkeeping and is what bench-like workloads
use: momentum -> L constrained leapfrog steps -> accept / reject -> SwitchPartitionTransition."""
import numpy as np
from .context import DEFAULT_SOLVER
from .distributed import sum_over_ranks
from .paths import SamplerSummaries
from .traces import SamplerTrace


class DualAveragingStepSize:
    """Hoffman & Gelman dual averaging on the mean accept statistic (cf. mici DualAveragingStepSizeAdapter,
    scripts/utils.py:303-306), one step size shared by all chains."""

    def __init__(self, step_size, target=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        self.mu = np.log(10 * step_size)
        self.target, self.gamma, self.t0, self.kappa = target, gamma, t0, kappa
        self.h_bar, self.log_bar, self.t = 0.0, np.log(step_size), 0
        self.step_size = step_size

    def update(self, accept_stat):
        self.t += 1
        eta = 1.0 / (self.t + self.t0)
        self.h_bar = (1 - eta) * self.h_bar + eta * (self.target - accept_stat)
        log_eps = self.mu - np.sqrt(self.t) / self.gamma * self.h_bar
        w = self.t ** (-self.kappa)
        self.log_bar = w * log_eps + (1 - w) * self.log_bar
        self.step_size = float(np.exp(log_eps))
        return self.step_size

    def final(self):
        return float(np.exp(self.log_bar))


class PerChainDualAveragingStepSize:
    """The same adapter with one state per chain, as Mici runs it: every chain adapts ITS OWN step size on its own accept
    statistic during warm-up (mici DualAveragingStepSizeAdapter keeps one adapter state per chain), and the step size of
    the main phase is the average of the chains' smoothed step sizes (Mici's `finalize` with several chains, as recalled:
    SURVEY.md Appendix D marks the adapter defaults `medium`).  A chain that starts where the shared step size is far too
    long for its retraction (every first step an integrator error, accept statistic 0) thereby shortens its own steps
    until it moves, instead of staying put for the whole run while dragging a shared step size down."""

    def __init__(self, step_size, num_chains, target=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        self.mu = np.full(num_chains, np.log(10 * step_size))
        self.target, self.gamma, self.t0, self.kappa = target, gamma, t0, kappa
        self.h_bar = np.zeros(num_chains)
        self.log_bar = np.full(num_chains, np.log(step_size))
        self.t = 0
        self.step_size = np.full(num_chains, float(step_size))

    def update(self, accept_stat):
        self.t += 1
        eta = 1.0 / (self.t + self.t0)
        self.h_bar = (1 - eta) * self.h_bar + eta * (self.target - np.asarray(accept_stat, dtype=np.float64))
        log_eps = self.mu - np.sqrt(self.t) / self.gamma * self.h_bar
        w = self.t ** (-self.kappa)
        self.log_bar = w * log_eps + (1 - w) * self.log_bar
        self.step_size = np.exp(log_eps)
        return self.step_size

    def final(self):
        """Smoothed step size of every chain [B]; the caller averages over the chains of all ranks."""
        return np.exp(self.log_bar)


def _mean_over_all_chains(local_sum, local_count):
    """Mean of a per-chain statistic over the chains of every rank (one tiny all-reduce; SURVEY.md 8f #3: warm-up
    adaptation combines the chains of all GPUs so that every rank integrates with the same step size)."""
    tot = sum_over_ranks([float(local_sum), float(local_count)])
    return float(tot[0]) / float(tot[1])


def _group_sums_over_all_chains(values, groups, n_groups):
    """(sums [G], counts [G]) of a per-chain statistic by group, over the chains of every rank: ONE all-reduce of a vector of
    2 G numbers (distributed.sum_over_ranks), so that every rank adapts every group's step size on the same numbers."""
    values = np.asarray(values, dtype=np.float64)
    local = np.zeros(2 * n_groups)
    for g in np.unique(groups):
        sel = groups == g
        local[g], local[n_groups + g] = values[sel].sum(), sel.sum()
    local = sum_over_ranks(local)
    return local[:n_groups], local[n_groups:]


def check_groups(groups, n_groups, num_chains):
    """groups [B] (global group id of every chain of this rank) and the number of groups of the whole job."""
    groups = np.asarray(groups)
    if groups.shape != (num_chains,) or not np.issubdtype(groups.dtype, np.integer):
        raise ValueError(f"groups must be an integer array of shape ({num_chains},), got {groups.dtype} {groups.shape}")
    G = int(groups.max()) + 1 if n_groups is None else int(n_groups)
    if groups.min() < 0 or groups.max() >= G:
        raise ValueError(f"groups must lie in [0, {G})")
    return groups.astype(np.int64), G


def sample_static_chmc(ctx, n_iter, n_step, step_size, seed, chain_offset=0, n_adapt=0, solver=None, rng=None,
                       n_head=6, callback=None, trace_dir=None, trace_func=None, total_chains=None,
                       jitter_length=False, metric_adapter=None, metric_window=0.75, metric_skip=0.25,
                       path_posterior=None, groups=None, n_groups=None, metric_per_group=False, predictive=None,
                       path_events=None, future_score=None):
    """Runs n_iter transitions on all chains of `ctx`; returns traces of the first `n_head` position components
    ([n_iter, B, n_head]), accept statistics and the step size used.  Directions are sampled per chain and
    transition (forward / backward in time), failed trajectories are rejected.

    trace_dir: write memory-mapped traces (`trace_<var>.npy`, [chain, draw, ...]) and `summary.json` there;
    trace_func chooses the traced variables (traces.SamplerTrace).  Under torch.distributed the accept statistic that
    drives the step-size adaptation is averaged over the chains of all ranks; with `total_chains` (the number of chains
    of the whole job) the per-chain directions and accept draws are taken from one stream indexed by the global chain
    number, so that any sharding of the chains reproduces the single-process run.
    jitter_length: every chain draws its number of leapfrog steps uniformly from 1..n_step per transition (a mixture
    of reversible kernels, so still a valid sampler); chains in regions where the retraction often fails then still
    move with their short trajectories instead of rejecting every long one (Mici's dynamic transition gets the same
    effect by ending a trajectory at the failing step).
    metric_adapter: an `adapters.OnlineBlockDiagonalMetricAdapter` over the `dim_u` global parameters (standard
    splitting only).  It sees the warm-up draws between the fractions `metric_skip` (the initial transient is left
    out, like the first window of a staged warm-up) and `metric_window` of the warm-up; the block metric it produces
    (per-chain statistics combined over all chains and ranks) is installed with `ctx.set_metric` there, and the
    remaining warm-up transitions re-tune the step size for the new metric.
    groups [B], n_groups: chains that sample different posteriors in one context (per-chain observations,
    ChmcContext.set_observations): groups[c] is the GLOBAL id of the data set chain c belongs to, n_groups their number over
    the whole job (default: max + 1 of this rank's).  Every group then has its own dual-averaging state, driven by the mean
    accept statistic of ITS chains over all ranks (one all-reduce of 2 G numbers per transition), and its own step size:
    out["step_size"] is [n_iter, G], out["group_accept_stat"] likewise, out["final_step_size"] [G].  One group gives the
    numbers of the call without `groups`.  The block metric is one M_0 per context: `metric_adapter` with more than one group
    raises ValueError --
    metric_per_group: unless this is set.  The adapter then produces one M_0 per group from the statistics of that group's
    chains over all ranks (`finalize_groups`), in the same window; they are installed with `ctx.set_metric(M, groups=...)`,
    every group's dual averaging restarts from that group's current step size, and out["metric_M_0"] is [G, U, U].
    path_posterior, predictive, path_events, future_score: summaries of the post-warm-up states and their entries of
    `out` (paths.SamplerSummaries)."""
    if metric_per_group and (groups is None or metric_adapter is None):
        raise ValueError("metric_per_group needs groups and a metric_adapter")
    group_metrics = None
    if groups is not None:
        groups, G = check_groups(groups, n_groups, ctx.B)
        if metric_adapter is not None and G > 1 and not metric_per_group:
            raise ValueError("the block metric is one M_0 per context: no metric_adapter with more than one group")
    solver = dict(DEFAULT_SOLVER) if solver is None else solver
    rng = np.random.default_rng(seed) if rng is None else rng
    adapter = DualAveragingStepSize(step_size) if n_adapt > 0 else None
    B = ctx.B
    if groups is not None:  # one adapter state and one step size per group
        adapter = [DualAveragingStepSize(step_size) for _ in range(G)] if n_adapt > 0 else None
        step_size = np.full(G, float(step_size))

    def draw():  # uniforms of this rank's chains
        if total_chains is None:
            return rng.random(B)
        return rng.random(total_chains)[chain_offset:chain_offset + B]

    n_metric, n_skip, metric_state = 0, 0, None
    if metric_adapter is not None and n_adapt > 0:
        if metric_adapter.dim_param != ctx.U:
            raise ValueError(f"the block metric covers the dim_u = {ctx.U} global parameters")
        n_metric = max(2, int(metric_window * n_adapt))
        n_skip = min(int(metric_skip * n_adapt), n_metric - 2)
        n_head = max(n_head, ctx.U)
    stuck = np.zeros(B, dtype=np.int64)  # consecutive trajectories with zero acceptance probability
    # per chain: how its post-warm-up transitions ended: [accepted, rejected after a complete trajectory, retraction did
    # not converge (status 1), diverged (2), non-reversible step (3)] -- the diagnosis of a chain that does not move
    outcome = np.zeros((B, 5), dtype=np.int64)
    heads = np.empty((n_iter, B, n_head))
    acc_hist, eps_hist, fail_hist = np.empty(n_iter), np.empty(n_iter), np.empty(n_iter)
    if groups is not None:
        eps_hist, group_acc_hist = np.empty((n_iter, G)), np.empty((n_iter, G))
    summaries = SamplerSummaries(path_posterior=path_posterior, predictive=predictive, path_events=path_events,
                                 future_score=future_score)
    trace = SamplerTrace(ctx, trace_dir, trace_func, n_iter)
    for it in range(n_iter):
        ctx.sample_momentum(seed, it + 1, chain_offset)
        h0 = ctx.hamiltonian()[:, 0]
        ctx.snapshot()
        # warm-up only: a chain whose trajectories keep failing (a start far from the typical set, where the shared
        # step size is too long for the retraction) backs its own step size off until it moves again
        scale = 0.5 ** np.minimum(stuck, 8) if it < n_adapt else 1.0
        eps = step_size if groups is None else step_size[groups]  # (per chain)
        dt = np.where(draw() < 0.5, eps, -eps) * scale
        act = np.ones(B, dtype=np.int32)
        # the trajectory as ONE library call (the loop an integration transition runs around integrator.step,
        # scripts/utils.py:284-301: a chain stops at its first failed step): single-block layouts walk it in one launch per
        # chain, the lock-step path folds the kicks of consecutive steps when every chain takes the same number of steps
        length = 1 + np.floor(draw() * n_step).astype(np.int32) if jitter_length else int(n_step)
        r = ctx.leapfrog_steps(dt, length, active=act, **solver)
        end_status = np.where(r["status"] > 0, r["status"], 0).astype(np.int64)
        act &= (r["status"] == 0).astype(np.int32)
        h1 = ctx.hamiltonian()[:, 0]
        dh = h1 - h0
        prob = np.where((act == 1) & np.isfinite(dh), np.exp(np.minimum(0.0, -np.where(np.isfinite(dh), dh, np.inf))), 0.0)
        accept = draw() < prob
        stuck = np.where(prob > 0.0, 0, stuck + 1)
        if it >= n_adapt:
            col = np.where(end_status > 0, 1 + np.clip(end_status, 1, 3), np.where(accept, 0, 1))
            outcome[np.arange(B), col] += 1
        ctx.restore((~accept).astype(np.int32))
        ctx.switch_partition()
        summaries.update(seed, it, chain_offset, n_adapt)
        heads[it] = ctx.get_head(n_head)
        trace.write(it, heads[it])
        if n_metric and n_skip <= it < n_metric:
            if metric_state is None:
                metric_state = metric_adapter.initialize(np.zeros((B, ctx.Q)))
            metric_adapter.update(metric_state, heads[it])
            if it == n_metric - 1 and metric_per_group:
                group_metrics = metric_adapter.finalize_groups(metric_state, groups, G)
                ctx.set_metric(group_metrics, groups=groups)
                adapter = [DualAveragingStepSize(float(e)) for e in step_size]  # re-tuned under the new metrics, per group
            elif it == n_metric - 1:
                metric = metric_adapter.finalize(metric_state)
                ctx.set_metric(metric.blocks[0].array)
                # the step size is re-tuned under the new metric
                adapter = DualAveragingStepSize(step_size) if groups is None else [DualAveragingStepSize(float(step_size[0]))]
        if groups is None:
            acc_all = _mean_over_all_chains(prob.sum(), B)
        else:
            sums, counts = _group_sums_over_all_chains(prob, groups, G)
            acc_all = float(sums.sum()) / float(counts.sum())
            acc_group = sums / np.maximum(counts, 1.0)
            group_acc_hist[it] = acc_group
        acc_hist[it], eps_hist[it], fail_hist[it] = acc_all, step_size, 1.0 - act.mean()
        if adapter is not None and it < n_adapt:
            if groups is None:
                step_size = adapter.update(acc_all)
                if it == n_adapt - 1:
                    step_size = adapter.final()
            else:
                step_size = np.array([a.update(acc_group[g]) for g, a in enumerate(adapter)])
                if it == n_adapt - 1:
                    step_size = np.array([a.final() for a in adapter])
        if callback is not None:
            callback(it, heads[it], prob.mean(), step_size)
    out = dict(heads=heads, accept_stat=acc_hist, step_size=eps_hist, fail_rate=fail_hist, final_step_size=step_size,
               chain_outcomes=outcome)
    if groups is not None:
        out["group_accept_stat"] = group_acc_hist
    summaries.fill(out, groups, G if groups is not None else None)
    if n_metric and metric_per_group:
        out["metric_M_0"] = group_metrics
    elif n_metric:
        out["metric_M_0"] = None if ctx.M_0 is None else ctx.M_0.copy()
    trace.finish(out, n_adapt, step_size, groups)
    return out
