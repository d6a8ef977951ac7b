"""Posterior of the latent path x(t): running moments of generate_from_model's x_seq (FitzHugh-Nagumo_example.ipynb:316-335)
over the draws of every chain, kept on the device.

A full position is T S V doubles per chain and draw, so the draws cannot be stored and the paths rebuilt afterwards; the
samplers instead fold the path of every post-warm-up state into per-chain Welford moments (`PathPosterior.update`, one
library call: path scan + moment update) and the chains are merged at the end (`pooled`).  Channels are the X state
components followed by obs_func(x)."""
import os
import numpy as np
from .devbuf import DeviceBuffers
from .distributed import process_group, all_gather_vectors, all_reduce_array


def merge_moments(a, b):
    """Chan's pairwise merge of two (n, mean, m2) triples (n a number, mean / m2 arrays of one shape)."""
    na, ma, sa = a
    nb, mb, sb = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    d = mb - ma
    return n, ma + d * (nb / n), sa + sb + d * d * (na * nb / n)


def merge_ranks(acc):
    """Under torch.distributed with more than one rank: the ranks' (n, mean, m2) merged in rank order; otherwise `acc`."""
    if process_group() is None:
        return acc
    shape, k = acc[1].shape, acc[1].size
    out = (0, np.zeros(shape), np.zeros(shape))
    for p in all_gather_vectors(np.concatenate(([float(acc[0])], acc[1].ravel(), acc[2].ravel()))):
        out = merge_moments(out, (int(round(p[0])), p[1:1 + k].reshape(shape), p[1 + k:].reshape(shape)))
    return out


def merge_moments_per_entry(a, b):
    """merge_moments with a count per entry: (n, mean, m2) arrays of one shape; entries with n_b == 0 keep a's numbers and
    entries with n_a == 0 take b's."""
    na, ma, sa = a
    nb, mb, sb = b
    n = na + nb
    fa, fb = na.astype(np.float64), nb.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = mb - ma
        mean = ma + d * (fb / n)
        m2 = sa + sb + d * d * (fa * fb / n)
    mean = np.where(nb == 0, ma, np.where(na == 0, mb, mean))
    m2 = np.where(nb == 0, sa, np.where(na == 0, sb, m2))
    return n, mean, m2


def merge_ranks_per_entry(acc):
    """Under torch.distributed with more than one rank: the ranks' per-entry (n, mean, m2) merged in rank order."""
    if process_group() is None:
        return acc
    k = len(acc[0])
    out = (np.zeros(k, dtype=np.int64), np.zeros(k), np.zeros(k))
    for p in all_gather_vectors(np.concatenate([acc[0].astype(np.float64), acc[1], acc[2]])):
        out = merge_moments_per_entry(out, (np.rint(p[:k]).astype(np.int64), p[k:2 * k], p[2 * k:]))
    return out


def event_names(n_thresholds):
    """The labels of the NE = 5 + 3 L entries of an event vector (include/chmc.h)."""
    names = ["max", "t_max", "min", "t_min", "integral"]
    for l in range(n_thresholds):
        names += [f"upcross_{l}", f"t_first_{l}", f"time_above_{l}"]
    return names


def _event_thresholds(thresholds):
    th = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if len(th) > 8 or not (np.diff(th) > 0).all() or np.isnan(th).any():
        raise ValueError("thresholds must be at most 8 increasing numbers")
    return th


class PathEvents:
    """Path-wise events of the latent path of every chain's current state (chmc_path_events_device, include/chmc.h):
    extremes and their times, the trapezoid integral and, per threshold, up-crossings, first passage and time above, of
    one channel (a state component, or X for obs_func(x)) over the inclusive window (p0, p1) of points at `stride` (None:
    the whole path).  `update` returns [B, NE] host doubles, small enough to trace like the head components.
    path_posterior: a `PathPosterior` of the same stride whose scratch path of its LAST update is evaluated instead of
    scanning the path again (call its update first)."""

    def __init__(self, ctx, channel, thresholds=(), stride=1, window=None, path_posterior=None):
        self.ctx, self.channel, self.stride = ctx, int(channel), int(stride)
        self.thresholds = _event_thresholds(thresholds)
        self.NP = ctx.path_points(self.stride)[0]
        self.times = np.arange(self.NP) * (self.stride * (ctx._obs_interval / ctx.S))  # t_p = p h, the library's product
        self.window = (0, self.NP - 1) if window is None else (int(window[0]), int(window[1]))
        if not 0 <= self.channel <= ctx.X:
            raise ValueError("channel must be in [0, X] (X: obs_func(x))")
        if not 0 <= self.window[0] <= self.window[1] < self.NP:
            raise ValueError("window must satisfy 0 <= p0 <= p1 < NP")
        if path_posterior is not None and (path_posterior.ctx is not ctx or path_posterior.stride != self.stride):
            raise ValueError("path_posterior must belong to the same context and have the same stride")
        self.path_posterior = path_posterior
        self.names = event_names(len(self.thresholds))
        self.NE = len(self.names)
        f64 = dict(ev=(ctx.B, self.NE))
        if path_posterior is None:  # a scratch path of its own
            f64["x"] = (ctx.B, self.NP, ctx.X)
        self._buf = DeviceBuffers(ctx, f64)

    def update(self, mask=None):
        """[B, NE]: the events of every chain's current path (rows of chains with mask[c] == 0 keep their last values)."""
        if self.path_posterior is not None:
            x_ptr = self.path_posterior._ptr("x")
        else:
            x_ptr = self._buf.ptr("x")
            self.ctx.generate_x_seq_device(self.stride, x_ptr)
        self.ctx.path_events_device(x_ptr, self.NP, self.stride, self.channel, self.window[0], self.window[1],
                                    self.thresholds, self._buf.ptr("ev"), mask=mask)
        return self._buf.host("ev")

    def sampler_update(self, seed, it, chain_offset):
        return self.update()

    def sampler_out(self, draws, groups, G):
        from .traces import summarize
        ev = np.stack(draws) if draws else np.empty((0, self.ctx.B, self.NE))
        return dict(path_events=ev, path_events_summary=summarize({k: ev[:, :, i].T for i, k in enumerate(self.names)},
                                                                  self.names, groups=groups))


class PathPosterior:
    def __init__(self, ctx, stride=1):
        self.ctx, self.stride = ctx, int(stride)
        self.NP, self.times = ctx.path_points(self.stride)
        self.XC = ctx.X + 1
        B = ctx.B
        self._buf = DeviceBuffers(ctx, dict(x=(B, self.NP, ctx.X), mean=(B, self.NP, self.XC), m2=(B, self.NP, self.XC)),
                                  dict(n=(B,)))
        self._ptr, self._host = self._buf.ptr, self._buf.host

    def sampler_update(self, seed, it, chain_offset):
        self.update()

    def sampler_out(self, draws, groups, G):
        return dict(path_posterior=self.pooled())

    def update(self, mask=None):
        """Fold the path of every chain's current state (chains with mask[c] != 0; None: all) into its moments."""
        self.ctx.path_stats_update_device(self.stride, self._ptr("x"), self._ptr("n"), self._ptr("mean"), self._ptr("m2"),
                                          mask=mask)

    def last_paths(self):
        """x_seq [B, NP, X] of the last update (the scratch buffer)."""
        return self._host("x")

    def moments(self):
        """n [B], mean, m2 [B, NP, X + 1] as they stand on the device."""
        return self._host("n"), self._host("mean"), self._host("m2")

    def per_chain(self):
        """n [B], mean, var [B, NP, X + 1]; var = m2 / (n - 1), NaN for chains with fewer than two draws."""
        n, mean, m2 = self.moments()
        with np.errstate(divide="ignore", invalid="ignore"):
            var = m2 / np.where(n > 1, n - 1, np.nan)[:, None, None]
        return n, mean, var

    def pooled(self):
        """All draws of all chains as one sample: the chains merged pairwise in chain order (Chan et al.), and under
        torch.distributed the ranks' results merged in rank order.  dict(n, mean, var, sd, m2), arrays [NP, X + 1]."""
        n, mean, m2 = self.moments()
        acc = (0, np.zeros_like(mean[0]), np.zeros_like(m2[0]))
        for c in range(len(n)):
            acc = merge_moments(acc, (int(n[c]), mean[c], m2[c]))
        acc = merge_ranks(acc)
        nn = acc[0]
        var = acc[2] / (nn - 1) if nn > 1 else np.full_like(acc[2], np.nan)
        return dict(n=nn, mean=acc[1], var=var, sd=np.sqrt(var), m2=acc[2])

    def save(self, directory):
        """`path_posterior.npz` in `directory`: times, per-chain n and means, pooled n, mean and sd."""
        os.makedirs(directory, exist_ok=True)
        n, mean, _ = self.per_chain()
        pool = self.pooled()
        path = os.path.join(directory, "path_posterior.npz")
        np.savez(path, times=self.times, stride=self.stride, n=n, chain_mean=mean, pooled_n=pool["n"], mean=pool["mean"],
                 sd=pool["sd"])
        return path


def sum_ranks(a):
    """Under torch.distributed with more than one rank: the ranks' integer arrays added up; otherwise `a`."""
    return a if process_group() is None else all_reduce_array(a, np.int64)


class PredictivePosterior:
    """Posterior predictive of the model, simulated on the device (chmc_predict_device, include/chmc.h): every `update` draws
    `n_rep` replicate futures of each chain's current state over `horizon` observation intervals -- origin "end": beyond
    the last observation (a forecast); "start": from x_0 (replicated data; horizon = T and stride = S give data sets for a
    posterior predictive check) -- and folds them into running moments per (chain, point, channel) and, with `levels`, into
    counts of y_rep <= level.  Channels: the X state components, obs_func(x), y_rep = obs_func(x) + sigma eps.
    events = dict(channel=, thresholds=(), window=None): every replicate's path-wise event vector (chmc_predict_events_device:
    extremes, integral, per threshold up-crossings, first passage, time above; of one channel, X + 1 = y_rep, over the
    inclusive window (p0, p1) of emitted points, None: all) folded per chain and entry over its finite values
    (`event_moments`, `pooled()["events"]`); keep_events: also the raw vectors of the last update (`last_events`)."""

    def __init__(self, ctx, horizon, stride=None, n_rep=64, origin="end", levels=None, n_keep=0, events=None,
                 keep_events=False):
        if origin not in ("end", "start"):
            raise ValueError('origin must be "end" (forecast) or "start" (replication)')
        self.ctx, self.horizon, self.n_rep, self.n_keep = ctx, int(horizon), int(n_rep), int(n_keep)
        self.stride = ctx.S if stride is None else int(stride)
        self.origin = 0 if origin == "end" else 1
        if not 1 <= self.n_rep <= 65536 or not 0 <= self.n_keep <= self.n_rep:
            raise ValueError("need 1 <= n_rep <= 65536 and 0 <= n_keep <= n_rep")
        self.levels = None if levels is None else np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        if self.levels is not None and (len(self.levels) == 0 or not (np.diff(self.levels) > 0).all()):
            raise ValueError("levels must be a non-empty increasing sequence")
        self.NPF, self.times = ctx.predict_points(self.horizon, self.stride, self.origin)
        self.XC = ctx.X + 2
        B, nl = ctx.B, 0 if self.levels is None else len(self.levels)
        f64 = dict(mean=(B, self.NPF, self.XC), m2=(B, self.NPF, self.XC))
        i64 = dict(n=(B,))
        if self.n_keep:
            f64["paths"] = (B, self.n_keep, self.NPF, self.XC)
        if nl:
            i64["cdf"] = (B, self.NPF, nl)
        self.events = None
        if events is not None:
            unknown = set(events) - {"channel", "thresholds", "window"}
            if unknown or "channel" not in events:
                raise ValueError("events must be dict(channel=, thresholds=(), window=None)")
            win = events.get("window")
            win = (0, self.NPF - 1) if win is None else (int(win[0]), int(win[1]))
            th = _event_thresholds(events.get("thresholds", ()))
            if not 0 <= int(events["channel"]) < self.XC or not 0 <= win[0] <= win[1] < self.NPF:
                raise ValueError("events: channel must be in [0, X + 1] and the window 0 <= p0 <= p1 < NPF")
            self.events = dict(channel=int(events["channel"]), thresholds=th, window=win)
            self.event_names = event_names(len(th))
            ne = len(self.event_names)
            f64.update(emean=(B, ne), em2=(B, ne))
            i64["en"] = (B, ne)
            if keep_events:
                f64["events"] = (B, self.n_rep, ne)
        elif keep_events:
            raise ValueError("keep_events needs events=")
        self._buf = DeviceBuffers(ctx, f64, i64)
        self._ptr, self._host = self._buf.ptr, self._buf.host  # (_ptr: None for an output that was not asked for)

    def sampler_update(self, seed, it, chain_offset):
        self.update(seed, it, chain_offset)

    def sampler_out(self, draws, groups, G):
        out = dict(predictive=self.pooled())
        if groups is not None:
            out["predictive_groups"] = [self.pooled(np.flatnonzero(groups == g)) for g in range(G)]
        return out

    def update(self, seed, draw, chain_offset=0, mask=None):
        """n_rep replicates of every chain's current state (chains with mask[c] != 0; None: all), keyed by (seed, draw,
        chain_offset + c): a chain's replicates do not depend on how the chains are sharded."""
        kw = dict(mask=mask, levels=self.levels, cdf_dev_ptr=self._ptr("cdf"), paths_dev_ptr=self._ptr("paths"),
                  n_keep=self.n_keep)
        if self.events is None:
            self.ctx.predict_device(seed, draw, chain_offset, self.horizon, self.stride, self.origin, self.n_rep,
                                    self._ptr("n"), self._ptr("mean"), self._ptr("m2"), **kw)
        else:
            ev = self.events
            self.ctx.predict_events_device(seed, draw, chain_offset, self.horizon, self.stride, self.origin, self.n_rep,
                                           self._ptr("n"), self._ptr("mean"), self._ptr("m2"), ev["channel"], ev["window"][0],
                                           ev["window"][1], ev["thresholds"], self._ptr("en"), self._ptr("emean"),
                                           self._ptr("em2"), events_dev_ptr=self._ptr("events"), **kw)

    def _need_events(self):
        if self.events is None:
            raise ValueError("no events were asked for (events=)")

    def event_moments(self):
        """en [B, NE] (finite values per chain and entry), emean, em2 [B, NE] as they stand on the device."""
        self._need_events()
        return self._host("en"), self._host("emean"), self._host("em2")

    def last_events(self):
        """[B, n_rep, NE]: the replicates' event vectors of the last update."""
        self._need_events()
        if "events" not in self._buf:
            raise ValueError("no events are kept (keep_events=False)")
        return self._host("events")

    def _pool_events(self, chains, across_ranks, nn):
        en, emean, em2 = self.event_moments()
        ne = en.shape[1]
        acc = (np.zeros(ne, dtype=np.int64), np.zeros(ne), np.zeros(ne))
        for c in chains:  # in chain order, every entry with its own count
            acc = merge_moments_per_entry(acc, (en[c], emean[c], em2[c]))
        if across_ranks:
            acc = merge_ranks_per_entry(acc)
        with np.errstate(divide="ignore", invalid="ignore"):
            var = np.where(acc[0] > 1, acc[2] / (acc[0] - 1), np.nan)
            mean = np.where(acc[0] > 0, acc[1], np.nan)
            reached = acc[0] / nn if nn else np.full(ne, np.nan)
        return dict(names=list(self.event_names), n=acc[0], mean=mean, var=var, m2=acc[2], reached=reached)

    def last_paths(self):
        """[B, n_keep, NPF, X + 2]: the first n_keep replicates of the last update."""
        if not self.n_keep:
            raise ValueError("no paths are kept (n_keep = 0)")
        return self._host("paths")

    def moments(self):
        """n [B] (replicate paths), mean, m2 [B, NPF, X + 2] as they stand on the device."""
        return self._host("n"), self._host("mean"), self._host("m2")

    def counts(self):
        """[B, NPF, n_levels]: per chain, how many y_rep were at or below each level."""
        if self.levels is None:
            raise ValueError("no CDF levels were given")
        return self._host("cdf")

    def per_chain(self):
        """n [B], mean, var [B, NPF, X + 2]; var = m2 / (n - 1), NaN for chains with fewer than two replicates."""
        n, mean, m2 = self.moments()
        with np.errstate(divide="ignore", invalid="ignore"):
            var = m2 / np.where(n > 1, n - 1, np.nan)[:, None, None]
        return n, mean, var

    def _pool(self, chains):
        n, mean, m2 = self.moments()
        acc = (0, np.zeros_like(mean[0]), np.zeros_like(m2[0]))
        for c in chains:
            acc = merge_moments(acc, (int(n[c]), mean[c], m2[c]))
        return acc

    def pooled(self, chains=None, across_ranks=True):
        """All replicates of the chains (None: all) as one sample: merged pairwise in chain order and, under
        torch.distributed, over the ranks in rank order.  dict(n, mean, var, sd, m2) [NPF, X + 2], and with levels cdf
        [NPF, n_levels] = pooled counts / n."""
        chains = range(self.ctx.B) if chains is None else list(chains)
        acc = self._pool(chains)
        if across_ranks:
            acc = merge_ranks(acc)
        nn = acc[0]
        var = acc[2] / (nn - 1) if nn > 1 else np.full_like(acc[2], np.nan)
        out = dict(n=nn, mean=acc[1], var=var, sd=np.sqrt(var), m2=acc[2])
        if self.levels is not None:
            cnt = self.counts()[list(chains)].sum(0)
            if across_ranks:
                cnt = sum_ranks(cnt)
            out["cdf"] = cnt / nn if nn else np.full(cnt.shape, np.nan)
        if self.events is not None:  # reached: the share of replicate paths whose entry is finite (t_first: P(reached))
            out["events"] = self._pool_events(chains, across_ranks, nn)
        return out

    def cdf(self):
        """[NPF, n_levels]: the pooled predictive CDF of y_rep at the levels."""
        if self.levels is None:
            raise ValueError("no CDF levels were given")
        return self.pooled()["cdf"]

    def quantiles(self, probs, cdf=None):
        """[NPF, len(probs)]: the pooled CDF inverted by linear interpolation over the levels; NaN where a probability lies
        outside the CDF's range over the levels."""
        F = self.cdf() if cdf is None else np.asarray(cdf)
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        out = np.full((F.shape[0], len(probs)), np.nan)
        for p in range(F.shape[0]):
            for i, pr in enumerate(probs):
                k = int(np.searchsorted(F[p], pr, side="left"))  # first level with F >= pr
                if k == 0:
                    out[p, i] = self.levels[0] if F[p, 0] == pr else np.nan
                elif k < len(self.levels):
                    f0, f1 = F[p, k - 1], F[p, k]
                    out[p, i] = self.levels[k - 1] + (pr - f0) / (f1 - f0) * (self.levels[k] - self.levels[k - 1])
        return out

    def save(self, directory):
        """`predictive.npz` in `directory`: times, per-chain n and means, pooled n, mean and sd, and with levels the levels and
        the pooled CDF, and with events their names, per-chain counts and means and the pooled n, mean, var and reached."""
        os.makedirs(directory, exist_ok=True)
        n, mean, _ = self.per_chain()
        pool = self.pooled()
        extra = {} if self.levels is None else dict(levels=self.levels, cdf=pool["cdf"])
        if self.events is not None:
            en, emean, _ = self.event_moments()
            ev = pool["events"]
            extra.update(event_names=np.array(self.event_names), event_channel=self.events["channel"],
                         event_window=np.array(self.events["window"]), event_thresholds=self.events["thresholds"],
                         event_chain_n=en, event_chain_mean=emean, event_n=ev["n"], event_mean=ev["mean"],
                         event_var=ev["var"], event_reached=ev["reached"])
        path = os.path.join(directory, "predictive.npz")
        np.savez(path, times=self.times, horizon=self.horizon, stride=self.stride, origin=self.origin, n_rep=self.n_rep, n=n,
                 chain_mean=mean, pooled_n=pool["n"], mean=pool["mean"], sd=pool["sd"], **extra)
        return path


def log_mean_exp(a, axis=None):
    """log of the mean of exp(a) over `axis` (None: all entries); -inf where every entry is -inf."""
    a = np.asarray(a, dtype=np.float64)
    m = np.max(a, axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        out = m0 + np.log(np.mean(np.exp(a - m0), axis=axis, keepdims=True))
    return float(out.reshape(())) if axis is None else np.squeeze(out, axis)


class FutureScore:
    """Log predictive score of observations that arrived behind the fit (chmc_score_future_device, include/chmc.h):
    log p(y_future | y_1..T) as the log-mean over posterior draws of the per-draw score, which the device estimates from
    `n_cand` keyed forecast candidates of each chain's current state.  y_future [H] or [B, H].  The samplers call
    `update(it, chain_offset)` at every post-warm-up state (`future_score=`); `seed` keys the candidates, independent of
    the sampler's seed.  Pooling is over this process' chains; a chain's values do not depend on the sharding, so ranks can
    gather `log_pred` themselves."""

    def __init__(self, ctx, y_future, n_cand=64, seed=0):
        y = np.asarray(y_future, dtype=np.float64)
        if y.ndim == 1:
            y = np.broadcast_to(y, (ctx.B, y.shape[0]))
        if y.ndim != 2 or y.shape[0] != ctx.B or y.shape[1] < 1 or not np.isfinite(y).all():
            raise ValueError(f"y_future must be finite with shape (H,) or ({ctx.B}, H)")
        if not 1 <= int(n_cand) <= 65536:
            raise ValueError("need 1 <= n_cand <= 65536")
        self.ctx, self.y_future, self.n_cand, self.seed = ctx, np.ascontiguousarray(y), int(n_cand), int(seed)
        self.horizon = y.shape[1]
        self._draws = []

    def update(self, draw, chain_offset=0, mask=None):
        """[B]: the score of every chain's current state, kept as one more row of `log_pred`."""
        lp, _ = self.ctx.score_future_device(self.seed, draw, chain_offset, self.y_future, self.n_cand, mask=mask)
        self._draws.append(lp)
        return lp

    def sampler_update(self, seed, it, chain_offset):
        self.update(it, chain_offset)

    def sampler_out(self, draws, groups, G):
        return dict(future_score=self.pooled(), future_log_pred=self.log_pred)

    @property
    def log_pred(self):
        """[n_main, B]: the per-draw, per-chain scores in the order of the updates."""
        return np.stack(self._draws) if self._draws else np.empty((0, self.ctx.B))

    def pooled(self):
        """dict(log_pred: log-mean-exp over draws and chains; chain_log_pred [B]: over the draws of each chain; mcse: the
        standard error of log_pred from the spread of the chains' values, sd(exp(chain - max)) / sqrt(B) on the log scale
        by the delta method (NaN with one chain); n_draws)."""
        lp = self.log_pred
        if lp.shape[0] == 0:
            nan = float("nan")
            return dict(log_pred=nan, chain_log_pred=np.full(self.ctx.B, nan), mcse=nan, n_draws=0)
        chain = log_mean_exp(lp, axis=0)
        total = log_mean_exp(lp)
        mcse = float("nan")
        if len(chain) > 1 and np.isfinite(total):
            w = np.exp(chain - total)  # the chains' mean densities relative to the pooled one (mean 1)
            mcse = float(np.std(w, ddof=1) / np.sqrt(len(chain)))
        return dict(log_pred=total, chain_log_pred=chain, mcse=mcse, n_draws=lp.shape[0])

    def save(self, directory):
        """`future_score.npz` in `directory`: y_future, n_cand, seed, the [n_main, B] scores and the pooled results."""
        os.makedirs(directory, exist_ok=True)
        pool = self.pooled()
        path = os.path.join(directory, "future_score.npz")
        np.savez(path, y_future=self.y_future, n_cand=self.n_cand, seed=self.seed, log_pred=self.log_pred,
                 pooled_log_pred=pool["log_pred"], chain_log_pred=pool["chain_log_pred"], mcse=pool["mcse"])
        return path


SUMMARY_KEYWORDS = ("path_posterior", "predictive", "path_events", "future_score")


class SamplerSummaries:
    """The samplers' keywords for summaries of the post-warm-up states, each an object of the sampler's `ctx` that sees
    every state after the partition switch:
    path_posterior: a `PathPosterior`; the latent path of every such state is folded into its running moments (`update()`),
    and out["path_posterior"] is its `pooled()` result.
    predictive: a `PredictivePosterior`; every such state gets `predictive.update(seed, it, chain_offset)`,
    out["predictive"] is its `pooled()` result and, with `groups`, out["predictive_groups"] the list of the G groups'
    pooled results.
    path_events: a `PathEvents`; every such state gets `update()`, out["path_events"] is [n_main, B, NE] and
    out["path_events_summary"] `traces.summarize` of it under the object's `names` (per group with `groups`).
    future_score: a `FutureScore`; every such state gets `future_score.update(it, chain_offset)`; out["future_score"] is
    its `pooled()` result and out["future_log_pred"] the [n_main, B] scores.  Scoring reads the state and draws from
    keyed streams of its own: the chain is bitwise what it is without it.
    The summaries run in the order of SUMMARY_KEYWORDS: a PathEvents(path_posterior=pp) reads the scratch path of pp's
    update of the same iteration.  A summary takes part through `sampler_update(seed, it, chain_offset)`, whose return
    values the helper keeps per run, and `sampler_out(kept, groups, G)`, its entries of the sampler's `out`."""

    def __init__(self, **summaries):
        self.items = [(summaries[k], []) for k in SUMMARY_KEYWORDS if summaries.get(k) is not None]

    def update(self, seed, it, chain_offset, n_adapt):
        if it >= n_adapt:
            for s, kept in self.items:
                kept.append(s.sampler_update(seed, it, chain_offset))

    def fill(self, out, groups=None, G=None):
        for s, kept in self.items:
            out.update(s.sampler_out(kept, groups, G))
