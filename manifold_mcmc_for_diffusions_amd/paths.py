"""Posterior of the latent path x(t): running moments of generate_from_model's x_seq (FitzHugh-Nagumo_example.ipynb:316-335)
over the draws of every chain, kept on the device.

A full position is T S V doubles per chain and draw, so the draws cannot be stored and the paths rebuilt afterwards; the
samplers instead fold the path of every post-warm-up state into per-chain Welford moments (`PathPosterior.update`, one
library call: path scan + moment update) and the chains are merged at the end (`pooled`).  Channels are the X state
components followed by obs_func(x)."""
import os
import numpy as np


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


class PathPosterior:
    def __init__(self, ctx, stride=1):
        self.ctx, self.stride = ctx, int(stride)
        self.NP, self.times = ctx.path_points(self.stride)
        self.XC = ctx.X + 1
        B = ctx.B
        shapes = dict(x=(B, self.NP, ctx.X), mean=(B, self.NP, self.XC), m2=(B, self.NP, self.XC))
        if ctx.L.chmc_backend() == b"hip:gfx950":  # torch-ROCm tensors; the library works on their pointers
            import torch
            dev = torch.device("cuda", ctx.device)
            self._buf = {k: torch.zeros(s, dtype=torch.float64, device=dev) for k, s in shapes.items()}
            self._buf["n"] = torch.zeros(B, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            self._ptr = lambda k: self._buf[k].data_ptr()
            self._host = lambda k: self._buf[k].cpu().numpy()
        else:  # the library's "device" is host memory (the emulation build of the tests)
            self._buf = {k: np.zeros(s) for k, s in shapes.items()}
            self._buf["n"] = np.zeros(B, dtype=np.int64)
            self._ptr = lambda k: self._buf[k].ctypes.data
            self._host = lambda k: self._buf[k].copy()

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
        acc = self._merge_ranks(acc)
        nn = acc[0]
        var = acc[2] / (nn - 1) if nn > 1 else np.full_like(acc[2], np.nan)
        return dict(n=nn, mean=acc[1], var=var, sd=np.sqrt(var), m2=acc[2])

    @staticmethod
    def _merge_ranks(acc):
        try:
            import torch
            import torch.distributed as dist
        except ImportError:
            return acc
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return acc
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        flat = np.concatenate(([float(acc[0])], acc[1].ravel(), acc[2].ravel()))
        t = torch.from_numpy(flat).to(dev)
        parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, t)
        shape, k = acc[1].shape, acc[1].size
        out = (0, np.zeros(shape), np.zeros(shape))
        for p in parts:
            p = p.cpu().numpy()
            out = merge_moments(out, (int(round(p[0])), p[1:1 + k].reshape(shape), p[1 + k:].reshape(shape)))
        return out

    def save(self, directory):
        """`path_posterior.npz` in `directory`: times, per-chain n and means, pooled n, mean and sd."""
        os.makedirs(directory, exist_ok=True)
        n, mean, _ = self.per_chain()
        pool = self.pooled()
        path = os.path.join(directory, "path_posterior.npz")
        np.savez(path, times=self.times, stride=self.stride, n=n, chain_mean=mean, pooled_n=pool["n"], mean=pool["mean"],
                 sd=pool["sd"])
        return path
