"""Worker of tests/test_keyed_init.py::test_two_gloo_ranks_equal_one_rank_keyed: one rank of a chain-sharded SIR run on CPU
(gloo) through the TEST-ONLY emulation build -- SirWorkload(keyed_init=True) on this rank's shard, then 3 static-trajectory
transitions with the chain-indexed streams.  argv: out_file total_chains"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
from manifold_mcmc_for_diffusions_amd import _lib, distributed as D  # noqa: E402


def run(total, rank, world):
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    from manifold_mcmc_for_diffusions_amd.workload import SirWorkload
    _lib._LIB = _lib._bind(ctypes.CDLL(os.path.join(HERE, "emu", "libchmc_emu.so")))
    off, cnt = D.shard_chains(total, rank, world)
    wl = SirWorkload(cnt, num_steps_per_obs=4, chain_offset=off, total_chains=total, keyed_init=True)
    q0 = wl.ctx.get_state(want_p=False)[0]
    res = sample_static_chmc(wl.ctx, 3, 2, 0.05, seed=3, chain_offset=off, total_chains=total)
    q, p, xo, _ = wl.ctx.get_state()
    local = np.concatenate([q0, q, p, xo.reshape(cnt, -1), res["heads"].transpose(1, 0, 2).reshape(cnt, -1),
                            wl.init_tries[:, None].astype(np.float64)], 1)
    wl.ctx.close()
    return local


if __name__ == "__main__":
    out, total = sys.argv[1], int(sys.argv[2])
    rank, _, world = D.init_process_group("gloo")
    local = run(total, rank, world)
    gathered = D.gather_samples(local)
    if rank == 0:
        assert gathered.shape[0] == total
        np.save(out, gathered)
    D.barrier()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
