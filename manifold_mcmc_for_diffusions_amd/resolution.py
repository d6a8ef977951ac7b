"""Carrying chains between time resolutions: warm up in a context with few steps per observation interval, sample in one
with many.

A context's num_steps_per_obs is fixed when it is created.  `transfer_state` moves the chains of one context into a sibling
context (ChmcContext.sibling) with another resolution: the position is copied device to device, its driving noise refined
with fresh keyed normals so that the fine sequence drives a refinement of the same Brownian path (or coarsened, or copied:
chmc_resample_q_device, include/chmc.h), and the observation-noise part solved from the constraint so that the new state
lies on the manifold of the chain's data (chmc_set_state_solve_noise_device).  Without observation noise there is no such
part: x_obs_seq of the refined position is pinned to the data and the position projected onto the constraint it defines
(chmc_set_state_project_device), with a fresh refinement for a chain whose projection does not converge.
`coarse_to_fine_static_chmc` and `coarse_to_fine_dynamic_chmc` are the drivers on top: warm-up at the coarse resolution, a
short re-tuning at every finer rung, the main phase at the last one."""
import time
import numpy as np
from .devbuf import DeviceBuffers
from .paths import SUMMARY_KEYWORDS

# keywords of sample_static_chmc that belong to one context (or one directory): only the rung they were made for gets them
ONE_CONTEXT_KEYWORDS = SUMMARY_KEYWORDS + ("trace_dir",)
METRIC_KEYWORDS = ("metric_adapter", "metric_window", "metric_skip")  # (the first warm-up alone adapts the metric)


def without(kw, names):
    return {k: v for k, v in kw.items() if k not in names}


def _src_row_length(src):
    return src.U + src.V0 + src.T * src.S * src.V + (src.T if src.noisy else 0)


def transfer_state(src, dst, seed, draw=0, chain_offset=0, partition=None, max_tries=3, solver=None):
    """The current states of `src` become the states of `dst`, a context of the same model, T, noise kind and B with
    another num_steps_per_obs in an integer ratio (src.sibling(S) makes one).  The momentum is not carried: dst gets zero
    momentum, and the sampler refreshes it.  partition: of dst (default: the one src is in).
    With observation noise the refined position is placed exactly through its noise part.  Without, it is projected
    (ChmcContext.set_state_project with `solver`, default context.DEFAULT_SOLVER); a chain whose status is not 0 is refined
    again with fresh normals, try k under resample draw `draw + (k << 32)` (so draw < 2^32 when max_tries > 1): a chain's
    tries depend on (seed, draw, chain_offset + c) alone.  A chain still unplaced after max_tries raises RuntimeError.
    Returns dict(moved [B], max_constr = max |constraint| of dst afterwards, defect [B], status [B], iters [B], tries [B]);
    moved is max_t |n_t new - n_t old| with noise (defect is the same array, tries 1), max_j |q placed - q refined| without."""
    if (src.B, src.T, src.U, src.V, src.V0, src.noisy) != (dst.B, dst.T, dst.U, dst.V, dst.V0, dst.noisy):
        raise ValueError("transfer_state needs two contexts of the same model, T, noise kind and number of chains")
    if not dst.noisy and max_tries < 1:
        raise ValueError("max_tries must be at least 1")
    if not dst.noisy and max_tries > 1 and int(draw) >= 1 << 32:
        raise ValueError("transfer_state: draw must be below 2^32 when max_tries > 1 (try k resamples with draw + (k << 32))")
    part = src.partition if partition is None else partition
    q_src = DeviceBuffers(src, dict(q=(src.B, _src_row_length(src))))
    q_dst = DeviceBuffers(dst, dict(q=(dst.B, dst.Q)))
    src.get_state_device(q_src.ptr("q"), None)
    if dst.noisy:
        dst.resample_q_device(q_src.ptr("q"), src.S, seed, q_dst.ptr("q"), draw=draw, chain_offset=chain_offset)
        moved = dst.set_state_solve_noise(q_dst.ptr("q"), part)
        return dict(moved=moved, max_constr=float(np.abs(dst.constr()).max()), defect=moved,
                    status=np.zeros(dst.B, dtype=np.int32), iters=np.zeros(dst.B, dtype=np.int32),
                    tries=np.ones(dst.B, dtype=np.int32))
    B = dst.B
    res = dict(moved=np.zeros(B), defect=np.zeros(B), status=np.zeros(B, dtype=np.int32), iters=np.zeros(B, dtype=np.int32))
    tries = np.zeros(B, dtype=np.int32)
    pending = np.ones(B, dtype=bool)
    for k in range(max_tries):
        mask = None if k == 0 else pending.astype(np.int32)
        dst.resample_q_device(q_src.ptr("q"), src.S, seed, q_dst.ptr("q"), draw=int(draw) + (k << 32),
                              chain_offset=chain_offset, mask=mask)
        r = dst.set_state_project(q_dst.ptr("q"), part, mask=mask, **(solver or {}))
        for key in res:
            res[key][pending] = r[key][pending]
        tries[pending] = k + 1
        pending = pending & (r["status"] != 0)
        if not pending.any():
            break
    if pending.any():
        bad = np.flatnonzero(pending)
        err = RuntimeError(f"transfer_state: chains {bad.tolist()} are not on the manifold after {max_tries} tries "
                           f"(status {res['status'][bad].tolist()})")
        err.result = dict(res, tries=tries)  # what the tries left, per chain: dst holds these states
        raise err
    return dict(res, max_constr=float(np.abs(dst.constr()).max()), tries=tries)


def transfer_metric(src, dst):
    """dst gets the block metric of src: the shared M_0, the chains' own matrices, or the identity."""
    dst.set_metric(None if src.M_0 is None else src.M_0)


def _coarse_to_fine(sample, coarse_ctx, fine_ctxs, n_warm_coarse, n_warm_fine, n_main, step_size, seed, sampler_kw):
    """The ladder both drivers run.  sample(ctx, n_iter, step_size, seed, n_adapt, **kw) is one sampler call."""
    ladder = list(fine_ctxs) if isinstance(fine_ctxs, (list, tuple)) else [fine_ctxs]
    if not ladder:
        raise ValueError("fine_ctxs must hold at least one context")
    fine_kw = without(sampler_kw, METRIC_KEYWORDS)
    chain_offset = int(sampler_kw.get("chain_offset", 0))
    rungs = []
    t0 = time.perf_counter()
    out = sample(coarse_ctx, n_warm_coarse, step_size, seed, n_warm_coarse, **without(sampler_kw, ONE_CONTEXT_KEYWORDS))
    eps = out["final_step_size"]
    rungs.append(dict(S=coarse_ctx.S, seconds=time.perf_counter() - t0, first_step_size=step_size, final_step_size=eps,
                      mean_accept_stat=float(np.mean(out["accept_stat"])) if n_warm_coarse else float("nan"), moved=None,
                      max_constr=float(np.abs(coarse_ctx.constr()).max()), defect=None, tries=None, proj_iters=None))
    prev = coarse_ctx
    for i, ctx in enumerate(ladder, start=1):
        last = i == len(ladder)
        t0 = time.perf_counter()
        transfer_metric(prev, ctx)
        tr = transfer_state(prev, ctx, seed, draw=i, chain_offset=chain_offset)
        kw = fine_kw if last else without(fine_kw, ONE_CONTEXT_KEYWORDS)
        out = sample(ctx, n_warm_fine + (n_main if last else 0), eps, seed + i, n_warm_fine, **kw)
        eps = out["final_step_size"]
        acc = out["accept_stat"][n_warm_fine:] if last and n_main else out["accept_stat"]
        rungs.append(dict(S=ctx.S, seconds=time.perf_counter() - t0, first_step_size=float(out["step_size"][0]),
                          final_step_size=eps,
                          mean_accept_stat=float(np.mean(acc)) if len(acc) else float("nan"), moved=tr["moved"],
                          max_constr=tr["max_constr"], defect=tr.get("defect"), tries=tr.get("tries"),
                          proj_iters=tr.get("iters")))
        prev = ctx
    out["rungs"] = rungs
    return out


def coarse_to_fine_static_chmc(coarse_ctx, fine_ctxs, n_warm_coarse, n_warm_fine, n_main, n_step, step_size, seed,
                               **sampler_kw):
    """Static constrained HMC with the warm-up at a coarse time resolution.  coarse_ctx holds the initial states;
    fine_ctxs is one context or a ladder of them (e.g. S = 50 -> 100 -> 400), siblings of coarse_ctx, with or without
    observation noise (transfer_state).
      1. sample_static_chmc on coarse_ctx, n_iter = n_adapt = n_warm_coarse (with sampler_kw's metric_adapter, if any);
      2. per rung: states and metric are transferred, the rung starts from the previous rung's final step size and re-tunes
         it over n_adapt = n_warm_fine transitions;
      3. the last rung runs n_iter = n_warm_fine + n_main.
    Rung i (0 = coarse) samples with seed + i, so that two contexts never use the same keyed momentum rows.
    Returns the last rung's sample_static_chmc dict with out["rungs"]: per rung dict(S, seconds, first_step_size,
    final_step_size, mean_accept_stat, moved, max_constr, defect, tries, proj_iters) -- the last five from transfer_state
    (proj_iters = its iters), None for the coarse rung except max_constr."""
    from .sampling import sample_static_chmc

    def sample(ctx, n_iter, eps, sd, n_adapt, **kw):
        return sample_static_chmc(ctx, n_iter, n_step, eps, sd, n_adapt=n_adapt, **kw)
    return _coarse_to_fine(sample, coarse_ctx, fine_ctxs, n_warm_coarse, n_warm_fine, n_main, step_size, seed, sampler_kw)


def coarse_to_fine_dynamic_chmc(coarse_ctx, fine_ctxs, n_warm_coarse, n_warm_fine, n_main, step_size, seed, **sampler_kw):
    """The same ladder on the no-U-turn sampler (sample_dynamic_chmc): rung i samples with seed + i and starts from the
    previous rung's final_step_size, summaries and trace_dir go to the last rung only.  Returns the last rung's
    sample_dynamic_chmc dict with out["rungs"] as in coarse_to_fine_static_chmc."""
    from .dynamic import sample_dynamic_chmc

    def sample(ctx, n_iter, eps, sd, n_adapt, **kw):
        return sample_dynamic_chmc(ctx, n_iter, eps, sd, n_adapt=n_adapt, **kw)
    return _coarse_to_fine(sample, coarse_ctx, fine_ctxs, n_warm_coarse, n_warm_fine, n_main, step_size, seed, sampler_kw)
