"""Carrying chains to a longer data record: fit y_1..T, then add the observations that arrive without starting again.

A context's number of observations is fixed when it is created.  `extend_state` moves the chains of a context that holds
the fit of y_1..T into a context with T + H observations (ChmcContext.extended): from every chain's current state the
library runs `n_cand` keyed forecast candidates over the H new observation intervals, weighs each by the density of the
observations that arrived and draws one in proportion to its weight (chmc_score_future_device, include/chmc.h).  The
candidate's step normals and observation-noise values are spliced behind the chain's own, which gives a position of the
longer record whose new constraint rows hold to rounding; chmc_set_state_solve_noise_device then defines the state by the
destination's own scan (contexts with observation noise only).  The log-mean weight is the log predictive score of the new
observations given the chain's draw.  `sequential_static_chmc` is the driver on top: fit, then per arriving batch extend,
re-tune briefly and sample."""
import time
import numpy as np
from .devbuf import DeviceBuffers
from .resolution import METRIC_KEYWORDS, transfer_metric, without
from .paths import SUMMARY_KEYWORDS, log_mean_exp


def _same_but_T(src, dst):
    keys = ("B", "U", "V", "V0", "X", "S", "noisy", "variable_sigma", "_model", "_obs_interval", "_num_obs_per_subseq",
            "_use_gaussian_splitting", "device")
    return all(getattr(src, k) == getattr(dst, k) for k in keys)


def extend_state(src, dst, seed, draw=0, chain_offset=0, n_cand=64, partition=None):
    """The current states of `src` become states of `dst`, a context that differs from `src` in its number of
    observations alone (src.extended(y_new) makes one): dst.T = src.T + H, the first src.T observations and the noise
    levels those of `src`.  The momentum is not carried: dst gets zero momentum, and the sampler refreshes it.
    partition: of dst (default: the one src is in).
    Returns dict(log_pred [B]: the log predictive score of the H new observations given each chain's draw, picked [B]: the
    candidate taken, ess_cand [B] = (sum w)^2 / sum w^2 of the candidates' weights, moved [B] = max_t |n_t new - n_t
    spliced| as dst's own scan sees it, max_constr = max |constraint| of dst afterwards).
    Raises ValueError naming the chains none of whose candidates has a finite weight."""
    if not _same_but_T(src, dst) or dst.T <= src.T:
        raise ValueError("extend_state needs two contexts that differ in their number of observations alone, dst.T > src.T")
    if not src.noisy:
        raise ValueError("extend_state needs observation noise (without it placing the state is a projection: out of scope)")
    y_src, sg_src = src.observations()
    y_dst, sg_dst = dst.observations()
    if y_dst[:, :src.T].tobytes() != y_src.tobytes() or sg_src.tobytes() != sg_dst.tobytes():
        raise ValueError("extend_state: the first observations and the noise levels of dst must be those of src")
    T, H, B = src.T, dst.T - src.T, src.B
    head, nv = src.U + src.V0 + T * src.S * src.V, H * src.S * src.V
    sbuf = DeviceBuffers(src, dict(q=(B, src.Q), tail=(B, nv + H), logw=(B, int(n_cand))))
    dbuf = DeviceBuffers(dst, dict(q=(B, dst.Q)))
    src.get_state_device(sbuf.ptr("q"), None)
    log_pred, picked = src.score_future_device(seed, draw, chain_offset, y_dst[:, T:], n_cand,
                                               logw_dev_ptr=sbuf.ptr("logw"), tail_dev_ptr=sbuf.ptr("tail"))
    if (picked < 0).any():
        raise ValueError(f"extend_state: no forecast candidate of chains {np.flatnonzero(picked < 0).tolist()} has a finite "
                         "weight for the new observations")
    # [u | v_0 | v_seq | tail v] and [n | tail n]: column copies between device buffers
    q_src, tail, q_dst = sbuf.array("q"), sbuf.array("tail"), dbuf.array("q")
    q_dst[:, :head] = q_src[:, :head]
    q_dst[:, head:head + nv] = tail[:, :nv]
    q_dst[:, head + nv:head + nv + T] = q_src[:, head:]
    q_dst[:, head + nv + T:] = tail[:, nv:]
    dbuf.sync()
    moved = dst.set_state_solve_noise(dbuf.ptr("q"), src.partition if partition is None else partition)
    lw = sbuf.host("logw")
    w = np.exp(lw - lw.max(1, keepdims=True))
    return dict(log_pred=log_pred, picked=picked, ess_cand=w.sum(1) ** 2 / (w * w).sum(1), moved=moved,
                max_constr=float(np.abs(dst.constr()).max()))


def sequential_static_chmc(ctx, y_batches, n_warm_first, n_warm_next, n_main, n_step, step_size, seed, n_cand=64,
                           stage_kw=None, **sampler_kw):
    """Static constrained HMC over a growing data record.  ctx holds the initial states for its own observations;
    y_batches is a list of arrays [H_i] or [B, H_i], the observations that arrive.
      0. sample_static_chmc on ctx: n_warm_first warm-up transitions (with sampler_kw's metric_adapter, if any), n_main draws;
      i. per batch: ctx_i = ctx_{i-1}.extended(batch), the metric and the states are carried (transfer_metric,
         extend_state with draw = i), the stage starts from the previous stage's final step size, re-tunes it over
         n_warm_next transitions and runs n_main draws.
    Stage i samples with seed + i, so that two contexts never use the same keyed momentum rows.  stage_kw(i, ctx_i), if
    given, returns further sample_static_chmc keywords for stage i (summaries that belong to that stage's context, such
    as a paths.PredictivePosterior of it).  The contexts the driver
    made are closed again, except the last one, which is out["ctx"].
    Returns the last stage's sample_static_chmc dict with out["stages"]: per stage dict(T, seconds, first_step_size,
    final_step_size, mean_accept_stat (main phase), log_pred (of the stage's batch, pooled over the chains by
    log-mean-exp), chain_log_pred [B], ess_cand [B], moved [B], max_constr, first_head [B, n_head]: the stage's first
    state); log_pred, chain_log_pred, ess_cand, moved are None for stage 0."""
    from .sampling import sample_static_chmc
    # (summaries that belong to ctx itself, paths.SUMMARY_KEYWORDS, see stage 0 only)
    sampler_kw = dict(sampler_kw)
    trace_dir = sampler_kw.pop("trace_dir", None)
    later_kw = without(sampler_kw, METRIC_KEYWORDS + SUMMARY_KEYWORDS)
    chain_offset = int(sampler_kw.get("chain_offset", 0))
    n_head = int(sampler_kw.get("n_head", 6))
    stages = []
    cur, eps, out = ctx, step_size, None
    for i in range(len(y_batches) + 1):
        t0 = time.perf_counter()
        ext = None
        if i:
            nxt = cur.extended(y_batches[i - 1])
            transfer_metric(cur, nxt)
            ext = extend_state(cur, nxt, seed, draw=i, chain_offset=chain_offset, n_cand=n_cand)
            if cur is not ctx:
                cur.close()
            cur = nxt
        first_head = cur.get_head(n_head)
        n_warm = n_warm_next if i else n_warm_first
        kw = dict(later_kw if i else sampler_kw)
        if stage_kw is not None:
            kw.update(stage_kw(i, cur))
        if trace_dir is not None:  # a directory per stage: trace_dir/stage_<i>
            import os
            kw["trace_dir"] = os.path.join(trace_dir, f"stage_{i}")
        out = sample_static_chmc(cur, n_warm + n_main, n_step, eps, seed + i, n_adapt=n_warm, **kw)
        eps = out["final_step_size"]
        acc = out["accept_stat"][n_warm:]
        stages.append(dict(T=cur.T, seconds=time.perf_counter() - t0,
                           first_step_size=float(np.mean(out["step_size"][0])) if n_warm + n_main else float("nan"),
                           final_step_size=eps, mean_accept_stat=float(np.mean(acc)) if len(acc) else float("nan"),
                           log_pred=None if ext is None else log_mean_exp(ext["log_pred"]),
                           chain_log_pred=None if ext is None else ext["log_pred"],
                           ess_cand=None if ext is None else ext["ess_cand"], moved=None if ext is None else ext["moved"],
                           max_constr=float(np.abs(cur.constr()).max()) if ext is None else ext["max_constr"],
                           first_head=first_head))
    out["stages"] = stages
    out["ctx"] = cur
    return out
