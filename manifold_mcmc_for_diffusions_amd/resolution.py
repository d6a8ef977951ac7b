"""Carrying chains between time resolutions: warm up in a context with few steps per observation interval, sample in one
with many.

A context's num_steps_per_obs is fixed when it is created.  `transfer_state` moves the chains of one context into a sibling
context (ChmcContext.sibling) with another resolution: the position is copied device to device, its driving noise refined
with fresh keyed normals so that the fine sequence drives a refinement of the same Brownian path (or coarsened, or copied:
chmc_resample_q_device, include/chmc.h), and the observation-noise part solved from the constraint so that the new state
lies on the manifold of the chain's data (chmc_set_state_solve_noise_device; contexts with observation noise only).
`coarse_to_fine_static_chmc` is the driver on top: warm-up at the coarse resolution, a short re-tuning at every finer
rung, the main phase at the last one."""
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


def transfer_state(src, dst, seed, draw=0, chain_offset=0, partition=None):
    """The current states of `src` become the states of `dst`, a context of the same model, T, noise kind and B with
    another num_steps_per_obs in an integer ratio (src.sibling(S) makes one).  The momentum is not carried: dst gets zero
    momentum, and the sampler refreshes it.  partition: of dst (default: the one src is in).
    Returns dict(moved [B] = max_t |n_t new - n_t old|, max_constr = max |constraint| of dst afterwards)."""
    if (src.B, src.T, src.U, src.V, src.V0, src.noisy) != (dst.B, dst.T, dst.U, dst.V, dst.V0, dst.noisy):
        raise ValueError("transfer_state needs two contexts of the same model, T, noise kind and number of chains")
    q_src = DeviceBuffers(src, dict(q=(src.B, _src_row_length(src))))
    q_dst = DeviceBuffers(dst, dict(q=(dst.B, dst.Q)))
    src.get_state_device(q_src.ptr("q"), None)
    dst.resample_q_device(q_src.ptr("q"), src.S, seed, q_dst.ptr("q"), draw=draw, chain_offset=chain_offset)
    moved = dst.set_state_solve_noise(q_dst.ptr("q"), src.partition if partition is None else partition)
    return dict(moved=moved, max_constr=float(np.abs(dst.constr()).max()))


def transfer_metric(src, dst):
    """dst gets the block metric of src: the shared M_0, the chains' own matrices, or the identity."""
    dst.set_metric(None if src.M_0 is None else src.M_0)


def coarse_to_fine_static_chmc(coarse_ctx, fine_ctxs, n_warm_coarse, n_warm_fine, n_main, n_step, step_size, seed,
                               **sampler_kw):
    """Static constrained HMC with the warm-up at a coarse time resolution.  coarse_ctx holds the initial states;
    fine_ctxs is one context or a ladder of them (e.g. S = 50 -> 100 -> 400), siblings of coarse_ctx.
      1. sample_static_chmc on coarse_ctx, n_iter = n_adapt = n_warm_coarse (with sampler_kw's metric_adapter, if any);
      2. per rung: states and metric are transferred, the rung starts from the previous rung's final step size and re-tunes
         it over n_adapt = n_warm_fine transitions;
      3. the last rung runs n_iter = n_warm_fine + n_main.
    Rung i (0 = coarse) samples with seed + i, so that two contexts never use the same keyed momentum rows.
    Returns the last rung's sample_static_chmc dict with out["rungs"]: per rung dict(S, seconds, first_step_size,
    final_step_size, mean_accept_stat, moved (None for the coarse rung), max_constr)."""
    from .sampling import sample_static_chmc
    ladder = list(fine_ctxs) if isinstance(fine_ctxs, (list, tuple)) else [fine_ctxs]
    if not ladder:
        raise ValueError("fine_ctxs must hold at least one context")
    fine_kw = without(sampler_kw, METRIC_KEYWORDS)
    chain_offset = int(sampler_kw.get("chain_offset", 0))
    rungs = []
    t0 = time.perf_counter()
    out = sample_static_chmc(coarse_ctx, n_warm_coarse, n_step, step_size, seed, n_adapt=n_warm_coarse,
                             **without(sampler_kw, ONE_CONTEXT_KEYWORDS))
    eps = out["final_step_size"]
    rungs.append(dict(S=coarse_ctx.S, seconds=time.perf_counter() - t0, first_step_size=step_size, final_step_size=eps,
                      mean_accept_stat=float(np.mean(out["accept_stat"])) if n_warm_coarse else float("nan"), moved=None,
                      max_constr=float(np.abs(coarse_ctx.constr()).max())))
    prev = coarse_ctx
    for i, ctx in enumerate(ladder, start=1):
        last = i == len(ladder)
        t0 = time.perf_counter()
        transfer_metric(prev, ctx)
        tr = transfer_state(prev, ctx, seed, draw=i, chain_offset=chain_offset)
        kw = fine_kw if last else without(fine_kw, ONE_CONTEXT_KEYWORDS)
        out = sample_static_chmc(ctx, n_warm_fine + (n_main if last else 0), n_step, eps, seed + i, n_adapt=n_warm_fine, **kw)
        eps = out["final_step_size"]
        acc = out["accept_stat"][n_warm_fine:] if last and n_main else out["accept_stat"]
        rungs.append(dict(S=ctx.S, seconds=time.perf_counter() - t0, first_step_size=float(out["step_size"][0]),
                          final_step_size=eps,
                          mean_accept_stat=float(np.mean(acc)) if len(acc) else float("nan"), moved=tr["moved"],
                          max_constr=tr["max_constr"]))
        prev = ctx
    out["rungs"] = rungs
    return out
