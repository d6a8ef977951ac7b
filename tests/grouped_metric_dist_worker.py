"""Worker of tests/test_grouped_metric.py: one rank of a chain-sharded GridWorkload on CPU (gloo) whose static sampler adapts
one block metric per cell, through the TEST-ONLY emulation build.  argv: out_file n_iter"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd import _lib, distributed as D, example_models as em  # noqa: E402

SIGMAS, CHAINS_PER_CELL = (0.03, 0.1, 0.4), 2  # 3 cells x 2 chains = 6 chains; two ranks of 3: cell 1 straddles the boundary


def cells():
    return [(em.simulate_fhn_observations(6, 0.2, 50, seed=5 + i, sigma=s)[:, 0], s) for i, s in enumerate(SIGMAS)]


def run_sampler(n_iter, rank, world):
    """Static sampler with per-group metric adaptation on this rank's shard of the grid.  Returns per local chain: the last
    head, the G metrics this rank installed and the (same for every chain) step-size histories."""
    from manifold_mcmc_for_diffusions_amd.adapters import OnlineBlockDiagonalMetricAdapter
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.workload import GridWorkload
    _lib._LIB = _lib._bind(ctypes.CDLL(os.path.join(HERE, "emu", "libchmc_emu.so")))
    cs = cells()
    total = len(cs) * CHAINS_PER_CELL
    off, cnt = D.shard_chains(total, rank, world)
    w = GridWorkload(cs, CHAINS_PER_CELL, num_steps_per_obs=4, num_obs_per_subseq=2, chain_offset=off, num_chains=cnt, seed=7)
    res = sample_static_chmc(w.ctx, n_iter, 2, 0.05, seed=3, chain_offset=off, n_adapt=n_iter - 2, total_chains=total,
                             groups=w.groups, n_groups=w.n_groups, metric_per_group=True,
                             metric_adapter=OnlineBlockDiagonalMetricAdapter(w.ctx.U))
    assert res["metric_M_0"].shape == (len(cs), w.ctx.U, w.ctx.U)
    assert np.array_equal(w.ctx.metrics(), res["metric_M_0"][w.groups])  # what the kernels use: this rank's chains' matrices
    w.ctx.close()
    tail = np.concatenate([res["metric_M_0"].ravel(), res["step_size"].ravel(), res["final_step_size"]])
    return np.concatenate([res["heads"][-1], np.tile(tail, (cnt, 1))], 1)


if __name__ == "__main__":
    out, n_iter = sys.argv[1], int(sys.argv[2])
    rank, _, world = D.init_process_group("gloo")
    local = run_sampler(n_iter, rank, world)
    gathered = D.gather_samples(local)
    if rank == 0:
        np.save(out, gathered)
    D.barrier()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
