"""Worker of tests/test_path_events.py: one rank of a chain-sharded run on CPU (gloo) through the TEST-ONLY emulation build;
every rank folds the forecast events of two states of its chains into a PredictivePosterior and pooled() merges the ranks.
argv: out_file total_chains"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd import _lib, distributed as D, example_models as em  # noqa: E402
from manifold_mcmc_for_diffusions_amd.context import ChmcContext  # noqa: E402
from manifold_mcmc_for_diffusions_amd.init import fhn_initial_states  # noqa: E402
from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior  # noqa: E402


def run(total, rank, world):
    _lib._LIB = _lib._bind(ctypes.CDLL(os.path.join(HERE, "emu", "libchmc_emu.so")))
    T, S, R, sigma = 8, 4, 3, 0.1
    y = em.simulate_fhn_observations(T, 0.2, 50, seed=11, sigma=sigma)
    off, cnt = D.shard_chains(total, rank, world)
    q, xo, rngs = fhn_initial_states(em.fhn, 0.2, S, y, cnt, True, seed=13, chain_offset=off, total_chains=total)
    ctx = ChmcContext("fhn", 0.2, S, R, y[:, 0], sigma=sigma, num_chains=cnt)
    ctx.set_state(q, np.stack([r.standard_normal(ctx.Q) for r in rngs]), xo, 0)
    ctx.project_onto_cotangent_space()
    pp = PredictivePosterior(ctx, 2, 2, 70, events=dict(channel=3, thresholds=[-1.0, 1.2], window=(0, 3)))
    dt = np.where((np.arange(cnt) + off) % 2 == 0, 0.03, -0.03)
    for it in range(2):
        ctx.leapfrog_step(dt, constraint_tol=1e-9, position_tol=1e-8)
        ctx.switch_partition()
        pp.update(17, it, off)
    pool = pp.pooled()
    ev = pool["events"]
    ctx.close()
    return np.concatenate(([float(pool["n"])], ev["n"].astype(np.float64), ev["mean"], ev["m2"], ev["reached"]))


if __name__ == "__main__":
    out, total = sys.argv[1], int(sys.argv[2])
    rank, _, world = D.init_process_group("gloo")
    flat = run(total, rank, world)
    if rank == 0:
        np.save(out, flat)
    D.barrier()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
