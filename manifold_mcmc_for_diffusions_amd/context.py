"""Thin NumPy-facing wrapper of one `chmc_ctx` (include/chmc.h): a batch of B chains resident on one MI355X.

This is the level bench.py and the multi-GPU driver work at; the Mici-style classes in system.py /
integrators.py sit on top of it.
"""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import ChmcConfig, as_c, ptr, iptr, check

MODEL_IDS = {"fhn": 0, "sir": 1, "fhn_nb": 2}
STATUS_NAMES = {0: "ok", 1: "not_converged", 2: "diverged", 3: "non_reversible", -1: "inactive"}
# the reference scripts' Newton solver and tolerances (scripts/utils.py:131-166); users take a copy: dict(DEFAULT_SOLVER)
DEFAULT_SOLVER = dict(newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50,
                      reverse_check_tol=2e-8)


class ChmcContext:
    def __init__(self, model, obs_interval, num_steps_per_obs, num_obs_per_subseq, y_seq, sigma=None,
                 use_gaussian_splitting=False, num_chains=1, device=0):
        L = _lib.lib()
        self.L = L
        # y_seq [T] (or [T, 1]): one data set for every chain; [B, T] (or [B, T, 1]): a row per chain.  sigma likewise: a
        # number for every chain, or an array [B] (set_observations)
        y_all = np.asarray(y_seq, dtype=np.float64)
        if y_all.ndim == 3 and y_all.shape[2] == 1:
            y_all = y_all[:, :, 0]
        per_chain_y = y_all.ndim == 2 and y_all.shape[1] != 1
        if per_chain_y and y_all.shape[0] != int(num_chains):
            raise ValueError(f"y_seq must have shape (T,) or ({int(num_chains)}, T), got {y_all.shape}")
        sigma_all = None
        if sigma is not None and not isinstance(sigma, str) and np.ndim(sigma) > 0:
            sigma_all = as_c(np.asarray(sigma, dtype=np.float64))
            if sigma_all.shape != (int(num_chains),):
                raise ValueError(f"sigma must be a number, \"variable\", None or an array of shape ({int(num_chains)},), "
                                 f"got {sigma_all.shape}")
            sigma = float(sigma_all[0])
        y = as_c((y_all[0] if per_chain_y else y_all).reshape(-1))
        self._y = y
        cfg = ChmcConfig(
            model=MODEL_IDS[model] if isinstance(model, str) else int(model), num_obs=len(y),
            num_steps_per_obs=int(num_steps_per_obs),
            num_obs_per_subseq=0 if num_obs_per_subseq is None else int(num_obs_per_subseq),
            # sigma: None (noiseless observations), a number (fixed noise), or "variable": the model's
            # generate_σ_y(u) = exp(u[dim_z]) (sde/example_models/fhn.py:46-47, sir.py:92-93), dim_u = dim_z + 1
            noisy=2 if isinstance(sigma, str) else int(sigma is not None),
            use_gaussian_splitting=int(bool(use_gaussian_splitting)),
            num_chains=int(num_chains), device=int(device), obs_interval=float(obs_interval),
            sigma=0.0 if sigma is None or isinstance(sigma, str) else float(sigma), y_seq=ptr(y))
        h = C.c_void_p()
        check(L.chmc_create(C.byref(cfg), C.byref(h)), "chmc_create")
        self.h = h
        d = np.zeros(16, dtype=np.int32)
        check(L.chmc_get_dims(h, iptr(d)), "chmc_get_dims")
        (self.B, self.Q, self.NV, self.U, self.X, self.T, self.S, self.num_partition, self.RM, self.Kmax) = map(int, d[:10])
        self.M_0 = None  # block metric (set_metric); None = identity
        self.per_chain_metric = False  # set_metric with [B, U, U] or groups: M_0 is [B, U, U]
        self.C = [int(d[10]), int(d[11])][: self.num_partition]
        self.K = [int(d[12]), int(d[13])][: self.num_partition]
        self.V, self.V0 = int(d[14]), int(d[15])
        self.noisy = sigma is not None
        self.per_chain_observations = False  # set_observations / simulate_observations: the chains have data of their own
        self.variable_sigma = isinstance(sigma, str)
        self.sigma = sigma
        self.device = int(device)
        self.on_gpu = L.chmc_backend() == b"hip:gfx950"  # False: the library's "device" is host memory (emulation build)
        self._obs_interval = float(obs_interval)
        self._model, self._num_obs_per_subseq = model, num_obs_per_subseq  # (sibling)
        self._use_gaussian_splitting = bool(use_gaussian_splitting)
        self.partition = 0
        self.blocks = []
        keys = ("obs0", "nobs", "first", "last", "row0", "nrows", "ny", "col0", "ncols", "step0", "nsteps", "_")
        for p in range(self.num_partition):
            raw = np.zeros(self.K[p] * 12, dtype=np.int32)
            check(L.chmc_get_blocks(h, p, iptr(raw)), "chmc_get_blocks")
            self.blocks.append([dict(zip(keys, map(int, raw[12 * b:12 * b + 12]))) for b in range(self.K[p])])
        if per_chain_y or sigma_all is not None:
            self.set_observations(y_all if per_chain_y else np.broadcast_to(y, (self.B, self.T)), sigma_all)

    # ---- per-chain observations (chmc_set_observations, include/chmc.h)
    def set_observations(self, y, sigma=None):
        """Chain c gets the data y[c] (y [B, T] or [B, T, 1]) and, with `sigma` [B] (fixed-noise contexts only), its own
        noise level.  Invalidates the chain state: set or initialise a state afterwards, as after construction."""
        y = as_c(y)
        if y.ndim == 3 and y.shape[2] == 1:
            y = as_c(y[:, :, 0])
        if y.shape != (self.B, self.T):
            raise ValueError(f"y must have shape ({self.B}, {self.T}), got {y.shape}")
        if sigma is not None:
            sigma = as_c(sigma)
            if sigma.shape != (self.B,):
                raise ValueError(f"sigma must have shape ({self.B},), got {sigma.shape}")
        check(self.L.chmc_set_observations(self.h, ptr(y), ptr(sigma)), "chmc_set_observations")
        self.per_chain_observations = True
        if sigma is not None:
            self.sigma = sigma.copy()

    def simulate_observations(self, seed, chain_offset=0, partition=0):
        """Every chain draws its position from the prior N(0, I) (keyed by (seed, chain_offset + chain): any sharding gives
        the same data), simulates its own data from it and becomes a state on the manifold of those data, momentum 0
        (chmc_simulate_observations_device, include/chmc.h).  observations() returns the data."""
        check(self.L.chmc_simulate_observations_device(self.h, int(seed), int(chain_offset), int(partition)),
              "chmc_simulate_observations_device")
        self.per_chain_observations = True
        self.partition = int(partition)

    def observations(self):
        """(y [B, T], sigma [B]) as the kernels use them; the shared values once per chain in a context without per-chain
        data (sigma 0 where the noise level is not a fixed number)."""
        y, sg = np.empty((self.B, self.T)), np.empty(self.B)
        check(self.L.chmc_get_observations(self.h, ptr(y), ptr(sg)), "chmc_get_observations")
        return y, sg

    # ---- carrying chains between time resolutions (chmc_resample_q_device, chmc_set_state_solve_noise_device,
    # chmc_set_state_project_device; resolution.py)
    def sibling(self, num_steps_per_obs):
        """A new context with `num_steps_per_obs` steps per observation interval and everything else as here: model, T, R,
        obs_interval, noise kind, splitting, B and device, the per-chain observations and the metric (per chain or shared)."""
        sigma = self.sigma
        if sigma is not None and not isinstance(sigma, str) and np.ndim(sigma) > 0:
            sigma = float(np.asarray(sigma)[0])  # (the chains' own levels follow with the observations)
        sib = ChmcContext(self._model, self._obs_interval, int(num_steps_per_obs), self._num_obs_per_subseq, self._y,
                          sigma=sigma, use_gaussian_splitting=self._use_gaussian_splitting, num_chains=self.B,
                          device=self.device)
        if self.per_chain_observations:
            y, sg = self.observations()
            sib.set_observations(y, sg if self.noisy and not self.variable_sigma else None)
        if self.M_0 is not None:
            sib.set_metric(self.M_0)
        return sib

    def resample_q_device(self, q_src_dev_ptr, S_src, seed, q_dst_dev_ptr, draw=0, chain_offset=0, mask=None):
        """Positions q_src [B, U + V0 + T S_src V (+ T)] of a context with S_src steps per interval (device) -> positions
        q_dst [B, Q] of this one (device): refined with fresh keyed normals (S = m S_src), coarsened (S_src = m S) or copied
        (chmc_resample_q_device, include/chmc.h).  Rows of chains with mask[c] == 0 are not touched."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        check(self.L.chmc_resample_q_device(self.h, C.c_void_p(q_src_dev_ptr), int(S_src), int(seed), int(draw),
                                            int(chain_offset), iptr(m), C.c_void_p(q_dst_dev_ptr)),
              "chmc_resample_q_device")

    def set_state_solve_noise(self, q_dev_ptr, partition=0):
        """The rows of q [B, Q] (device) become the chains' states with the observation-noise part n solved from the
        constraint, n_t = (y_t - obs_func(x_t)) / sigma, momentum 0 (chmc_set_state_solve_noise_device, include/chmc.h;
        contexts with observation noise only).  Returns moved [B] = max_t |n_t new - n_t given|."""
        moved = np.empty(self.B)
        check(self.L.chmc_set_state_solve_noise_device(self.h, C.c_void_p(q_dev_ptr), int(partition), ptr(moved)),
              "chmc_set_state_solve_noise_device")
        self.partition = int(partition)
        return moved

    def set_state_project(self, q_dev_ptr, partition=0, mask=None, **solver):
        """The same placement without observation noise: the rows of q [B, Q] (device) of the chains with mask[c] != 0 (None:
        all) are projected onto the manifold of the chains' data from x_obs_seq of their own path, pinned to the data
        (chmc_set_state_project_device, include/chmc.h; noiseless contexts only).  solver: the keywords of DEFAULT_SOLVER.
        Returns dict(status, iters, defect, moved), each [B]; a chain with status != 0 holds the pinned, unprojected state."""
        s = dict(DEFAULT_SOLVER, **solver)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        status, iters = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        defect, moved = np.empty(self.B), np.empty(self.B)
        check(self.L.chmc_set_state_project_device(self.h, C.c_void_p(q_dev_ptr), int(partition), iptr(m), int(s["newton"]),
                                                   float(s["constraint_tol"]), float(s["position_tol"]),
                                                   float(s["divergence_tol"]), int(s["max_iters"]), iptr(status), iptr(iters),
                                                   ptr(defect), ptr(moved)), "chmc_set_state_project_device")
        self.partition = int(partition)
        return dict(status=status, iters=iters, defect=defect, moved=moved)

    def close(self):
        if getattr(self, "h", None):
            self.L.chmc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state
    def _bq(self, a, name):
        a = as_c(a)
        if a.shape != (self.B, self.Q):
            raise ValueError(f"{name} must have shape ({self.B}, {self.Q}), got {a.shape}")
        return a

    def set_state(self, q, p, x_obs_seq, partition=0):
        q = self._bq(q, "q")
        p = None if p is None else self._bq(p, "p")
        xo = as_c(x_obs_seq)
        if xo.shape != (self.B, self.T, self.X):
            raise ValueError(f"x_obs_seq must have shape ({self.B}, {self.T}, {self.X})")
        check(self.L.chmc_set_state(self.h, ptr(q), ptr(p), ptr(xo), int(partition)), "chmc_set_state")
        self.partition = int(partition)

    def init_by_linear_interpolation(self, u, v_0, x_obs_seq_init, partition=0):
        """find_initial_state_by_linear_interpolation (sde/mici_extensions.py:1479-1547) for every chain, on the
        device: u [B, U], v_0 [B, V0], x_obs_seq_init [B, T, X]."""
        u, v_0, xo = as_c(u), as_c(v_0), as_c(x_obs_seq_init)
        if u.shape != (self.B, self.U) or v_0.shape != (self.B, self.V0) or xo.shape != (self.B, self.T, self.X):
            raise ValueError(f"expected u ({self.B}, {self.U}), v_0 ({self.B}, {self.V0}), "
                             f"x_obs_seq_init ({self.B}, {self.T}, {self.X})")
        check(self.L.chmc_init_linear_interpolation(self.h, ptr(u), ptr(v_0), ptr(xo), int(partition)),
              "chmc_init_linear_interpolation")
        self.partition = int(partition)

    def get_state(self, want_p=True, want_x_obs=True):
        q = np.empty((self.B, self.Q))
        p = np.empty((self.B, self.Q)) if want_p else None
        xo = np.empty((self.B, self.T, self.X)) if want_x_obs else None
        part = C.c_int(0)
        check(self.L.chmc_get_state(self.h, ptr(q), ptr(p), ptr(xo), C.byref(part)), "chmc_get_state")
        return q, p, xo, part.value

    def set_metric(self, M_0, groups=None):
        """metric = blockdiag(M_0 [U, U] dense positive definite, identity) (sde/mici_extensions.py:279-315); None = identity.
        M_0 [B, U, U] gives every chain a matrix of its own, M_0 [G, U, U] with `groups` [B] (group index per chain) gives
        chain c the matrix M_0[groups[c]] (chmc_set_metrics, include/chmc.h); self.M_0 is then the [B, U, U] array.
        The cached factors of the current state are refreshed; the momentum is left as it is."""
        if M_0 is None:
            if groups is not None:
                raise ValueError("groups needs M_0 of shape (G, U, U)")
            check(self.L.chmc_set_metric(self.h, None), "chmc_set_metric")
            self.M_0 = None
            self.per_chain_metric = False
            return
        m = np.ascontiguousarray(M_0, dtype=np.float64)
        if groups is not None:
            g = np.asarray(groups)
            if m.ndim != 3 or m.shape[1:] != (self.U, self.U):
                raise ValueError(f"with groups, M_0 must have shape (G, {self.U}, {self.U}), got {m.shape}")
            if g.shape != (self.B,) or not np.issubdtype(g.dtype, np.integer) or g.min() < 0 or g.max() >= m.shape[0]:
                raise ValueError(f"groups must be {self.B} integers in [0, {m.shape[0]})")
            m = np.ascontiguousarray(m[g])
        if m.shape == (self.B, self.U, self.U):
            check(self.L.chmc_set_metrics(self.h, ptr(m)), "chmc_set_metrics")
            self.M_0 = m.copy()
            self.per_chain_metric = True
            return
        if m.shape != (self.U, self.U):
            raise ValueError(f"M_0 must have shape ({self.U}, {self.U}) or ({self.B}, {self.U}, {self.U})")
        check(self.L.chmc_set_metric(self.h, ptr(m)), "chmc_set_metric")
        self.M_0 = m.copy()
        self.per_chain_metric = False

    def metrics(self):
        """M_0 [B, U, U] as the kernels use it: the shared matrix once per chain, or the identity (chmc_get_metric)."""
        m = np.empty((self.B, self.U, self.U))
        check(self.L.chmc_get_metric(self.h, ptr(m)), "chmc_get_metric")
        return m

    def tree_leaf(self, run, take, sub_prop_q_ptr, sub_sum_ptr, ck_p_ptr, ck_sum_ptr, store_slot, check_lo, n_check,
                  ck_end_ptr=None):
        """Fused bookkeeping of one leaf of the batched dynamic-integration trees (chmc_tree_leaf, include/chmc.h):
        returns [B, n_check, 6] = per checked span the two no-U-turn criterion values and, with `ck_end_ptr`, the four
        values of Mici's additional sub-tree checks (zeros where not computed)."""
        out = np.zeros((self.B, n_check, 6))
        r = np.ascontiguousarray(run, dtype=np.int32)
        t = np.ascontiguousarray(take, dtype=np.int32)
        check(self.L.chmc_tree_leaf(self.h, iptr(r), iptr(t), C.c_void_p(sub_prop_q_ptr), C.c_void_p(sub_sum_ptr),
                                    C.c_void_p(ck_p_ptr), C.c_void_p(ck_sum_ptr), C.c_void_p(ck_end_ptr or 0),
                                    int(store_slot), int(check_lo), int(n_check), ptr(out) if n_check else None),
              "chmc_tree_leaf")
        return out

    # ---- per-chain tree decisions on the device (chmc_tree_begin / _subtree / _step / _get, include/chmc.h)
    def tree_begin(self):
        h0 = np.empty(self.B)
        check(self.L.chmc_tree_begin(self.h, ptr(h0)), "chmc_tree_begin")
        return h0

    def tree_set_alive(self, alive):
        a = np.ascontiguousarray(alive, dtype=np.int32)
        check(self.L.chmc_tree_set_alive(self.h, iptr(a)), "chmc_tree_set_alive")

    def tree_subtree(self):
        check(self.L.chmc_tree_subtree(self.h), "chmc_tree_subtree")

    def tree_step(self, dt, u_leaf, max_delta_h, sub_prop_q_ptr, sub_sum_ptr, ck_p_ptr, ck_sum_ptr, ck_end_ptr, store_slot,
                  check_lo, n_check, n_inner_step=1, newton=True, constraint_tol=1e-9, position_tol=1e-8,
                  divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8):
        """One leaf for every chain still running in its sub-tree: integrator step, termination tests, multinomial
        weight / proposal update, momentum sums, checkpoints and no-U-turn checks, all on the device.  Returns the
        number of chains still running."""
        dt = as_c(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.B,)))
        u = as_c(np.asarray(u_leaf, dtype=np.float64))
        n = C.c_int(0)
        check(self.L.chmc_tree_step(self.h, ptr(dt), int(n_inner_step), int(newton), constraint_tol, position_tol,
                                    divergence_tol, int(max_iters), reverse_check_tol, ptr(u), float(max_delta_h),
                                    C.c_void_p(sub_prop_q_ptr), C.c_void_p(sub_sum_ptr), C.c_void_p(ck_p_ptr),
                                    C.c_void_p(ck_sum_ptr), C.c_void_p(ck_end_ptr or 0), int(store_slot), int(check_lo),
                                    int(n_check), C.byref(n)), "chmc_tree_step")
        return n.value

    def tree_get(self):
        B = self.B
        o = {k: np.zeros(B, dtype=np.int32) for k in ("alive", "run", "n_step", "failed", "diverged")}
        o["sub_logw"], o["sum_acc"] = np.zeros(B), np.zeros(B)
        check(self.L.chmc_tree_get(self.h, iptr(o["alive"]), iptr(o["run"]), iptr(o["n_step"]), iptr(o["failed"]),
                                   iptr(o["diverged"]), ptr(o["sub_logw"]), ptr(o["sum_acc"])), "chmc_tree_get")
        return o

    def tree_doubling_begin(self, u_dir, neg_q_ptr, neg_p_ptr, pos_q_ptr, pos_p_ptr, sub_sum_ptr):
        """Direction, edge switch (with cache re-evaluation) and sub-tree start of one doubling, on the device; returns the
        number of chains whose tree can still grow."""
        u = as_c(np.asarray(u_dir, dtype=np.float64))
        n = C.c_int(0)
        check(self.L.chmc_tree_doubling_begin(self.h, ptr(u), C.c_void_p(neg_q_ptr), C.c_void_p(neg_p_ptr), C.c_void_p(pos_q_ptr),
                                              C.c_void_p(pos_p_ptr), C.c_void_p(sub_sum_ptr), C.byref(n)),
              "chmc_tree_doubling_begin")
        return n.value

    def tree_doubling_end(self, u_accept, depth, prop_q_ptr, sub_prop_q_ptr, sum_mom_ptr, sub_sum_ptr, neg_q_ptr, neg_p_ptr,
                          pos_q_ptr, pos_p_ptr):
        """Biased progressive sampling, momentum sum, new tree edge and whole-tree no-U-turn criterion of one doubling, on
        the device; returns the number of chains whose tree can still grow."""
        u = as_c(np.asarray(u_accept, dtype=np.float64))
        n = C.c_int(0)
        check(self.L.chmc_tree_doubling_end(self.h, ptr(u), int(depth), C.c_void_p(prop_q_ptr), C.c_void_p(sub_prop_q_ptr),
                                            C.c_void_p(sum_mom_ptr), C.c_void_p(sub_sum_ptr), C.c_void_p(neg_q_ptr),
                                            C.c_void_p(neg_p_ptr), C.c_void_p(pos_q_ptr), C.c_void_p(pos_p_ptr), C.byref(n)),
              "chmc_tree_doubling_end")
        return n.value

    def tree_get_doubling(self):
        moved, depth = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        logw = np.zeros(self.B)
        check(self.L.chmc_tree_get_doubling(self.h, iptr(moved), iptr(depth), ptr(logw)), "chmc_tree_get_doubling")
        return dict(moved=moved != 0, depth=depth.astype(np.int64), logw=logw)

    def set_momentum(self, p):
        p = self._bq(p, "p")
        check(self.L.chmc_set_momentum(self.h, ptr(p)), "chmc_set_momentum")

    def get_state_device(self, q_dev_ptr, p_dev_ptr):
        check(self.L.chmc_get_state_device(self.h, C.c_void_p(q_dev_ptr or 0), C.c_void_p(p_dev_ptr or 0)),
              "chmc_get_state_device")

    def set_momentum_device(self, p_dev_ptr):
        check(self.L.chmc_set_momentum_device(self.h, C.c_void_p(p_dev_ptr)), "chmc_set_momentum_device")

    def sample_momentum(self, seed, draw, chain_offset=0):
        """Momentum refresh on the device: N(0, I) from a counter-based generator, projected onto the cotangent space."""
        check(self.L.chmc_sample_momentum(self.h, int(seed), int(draw), int(chain_offset)), "chmc_sample_momentum")

    def snapshot(self):
        check(self.L.chmc_snapshot(self.h), "chmc_snapshot")

    def restore(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.int32)
        check(self.L.chmc_restore(self.h, iptr(m)), "chmc_restore")

    def restore_device(self, q_dev_ptr, p_dev_ptr, mask, momentum_is_tangent=True):
        m = np.ascontiguousarray(mask, dtype=np.int32)
        check(self.L.chmc_restore_device(self.h, C.c_void_p(q_dev_ptr), C.c_void_p(p_dev_ptr), iptr(m),
                                         int(bool(momentum_is_tangent))), "chmc_restore_device")

    def get_head(self, n):
        out = np.empty((self.B, n))
        check(self.L.chmc_get_head(self.h, int(n), ptr(out)), "chmc_get_head")
        return out

    def update_x_obs_seq(self):
        check(self.L.chmc_update_x_obs_seq(self.h), "chmc_update_x_obs_seq")

    def switch_partition(self):
        check(self.L.chmc_switch_partition(self.h), "chmc_switch_partition")
        self.partition = (self.partition + 1) % self.num_partition

    # ---- the latent path (chmc_generate_x_seq*, chmc_path_stats_update_device; paths.py keeps the running moments)
    def path_points(self, stride=1):
        """(NP, times): the number of points of a path at `stride` and their times p * stride * delta (time 0: x_0)."""
        stride = int(stride)
        if stride < 1 or self.S % stride:
            raise ValueError(f"stride must be at least 1 and divide num_steps_per_obs = {self.S}")
        n_p = self.T * self.S // stride + 1
        return n_p, np.arange(n_p) * (stride * self._obs_interval / self.S)

    def generate_x_seq(self, stride=1, q=None, return_sweeps=False):
        """x_seq [B, NP, X] of generate_from_model (FitzHugh-Nagumo_example.ipynb:316-335): the latent path of the current
        states, or of the positions `q` [B, Q].  return_sweeps: also the sweeps of the time-parallel pass per chain (0 where
        the sequential recursion ran)."""
        n_p = self.T * self.S // max(int(stride), 1) + 1
        q = None if q is None else self._bq(q, "q")
        out = np.empty((self.B, n_p, self.X))
        sw = np.zeros(self.B, dtype=np.int32)
        check(self.L.chmc_generate_x_seq(self.h, ptr(q), int(stride), ptr(out), iptr(sw)), "chmc_generate_x_seq")
        return (out, sw) if return_sweeps else out

    def generate_x_seq_device(self, stride, x_seq_dev_ptr, return_sweeps=False):
        sw = np.zeros(self.B, dtype=np.int32) if return_sweeps else None
        check(self.L.chmc_generate_x_seq_device(self.h, int(stride), C.c_void_p(x_seq_dev_ptr), iptr(sw)),
              "chmc_generate_x_seq_device")
        return sw

    def path_stats_update_device(self, stride, x_seq_dev_ptr, n_dev_ptr, mean_dev_ptr, m2_dev_ptr, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        check(self.L.chmc_path_stats_update_device(self.h, int(stride), iptr(m), C.c_void_p(x_seq_dev_ptr),
                                                   C.c_void_p(n_dev_ptr), C.c_void_p(mean_dev_ptr), C.c_void_p(m2_dev_ptr)),
              "chmc_path_stats_update_device")

    # ---- posterior predictive simulation (chmc_predict_points, chmc_predict_device; paths.PredictivePosterior keeps the buffers)
    def predict_points(self, horizon, stride, origin=0):
        """(NPF, times): the points of a predictive over `horizon` observation intervals at `stride` and their times
        (origin 0: after the last observation; 1: from time 0)."""
        n = C.c_int(0)
        check(self.L.chmc_predict_points(self.h, int(horizon), int(stride), int(origin), C.byref(n), None),
              "chmc_predict_points")
        times = np.empty(n.value)
        check(self.L.chmc_predict_points(self.h, int(horizon), int(stride), int(origin), C.byref(n), ptr(times)),
              "chmc_predict_points")
        return n.value, times

    def predict_device(self, seed, draw, chain_offset, horizon, stride, origin, n_rep, n_dev_ptr, mean_dev_ptr, m2_dev_ptr,
                       mask=None, levels=None, cdf_dev_ptr=None, paths_dev_ptr=None, n_keep=0):
        """n_rep replicate futures (origin 0) or replicated data sets (origin 1) of every chain's current state, merged into
        the caller's device moments, CDF counts and kept paths (chmc_predict_device, include/chmc.h)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        lv = None if levels is None else as_c(levels).reshape(-1)
        check(self.L.chmc_predict_device(self.h, int(seed), int(draw), int(chain_offset), int(horizon), int(stride),
                                         int(origin), int(n_rep), iptr(m), 0 if lv is None else len(lv), ptr(lv),
                                         C.c_void_p(n_dev_ptr), C.c_void_p(mean_dev_ptr), C.c_void_p(m2_dev_ptr),
                                         C.c_void_p(cdf_dev_ptr), C.c_void_p(paths_dev_ptr), int(n_keep)),
              "chmc_predict_device")

    # ---- scoring arrived observations and carrying chains to a longer record (chmc_score_future_device; sequential.py)
    def score_future_device(self, seed, draw, chain_offset, y_future, n_cand=64, mask=None, logw_dev_ptr=None,
                            tail_dev_ptr=None, log_pred=None, picked=None):
        """n_cand keyed forecast candidates of every chain's current state over the next H observation intervals, weighed by
        the observations y_future [H] or [B, H] that arrived (chmc_score_future_device, include/chmc.h).  Returns
        (log_pred [B], picked [B]); logw_dev_ptr [B, n_cand] and tail_dev_ptr [B, H S V + H] are optional device buffers.
        log_pred / picked: arrays to write into (the entries of chains with mask[c] == 0 are left as they are)."""
        y = as_c(y_future)
        if y.ndim == 1:
            y = as_c(np.broadcast_to(y, (self.B, y.shape[0])))
        if y.ndim != 2 or y.shape[0] != self.B:
            raise ValueError(f"y_future must have shape (H,) or ({self.B}, H), got {y.shape}")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        lp = np.full(self.B, np.nan) if log_pred is None else log_pred
        pk = np.full(self.B, -2, dtype=np.int32) if picked is None else picked
        if lp.dtype != np.float64 or pk.dtype != np.int32 or lp.shape != (self.B,) or pk.shape != (self.B,) or \
                not lp.flags.c_contiguous or not pk.flags.c_contiguous:
            raise ValueError(f"log_pred must be float64 [{self.B}] and picked int32 [{self.B}]")
        check(self.L.chmc_score_future_device(self.h, int(seed), int(draw), int(chain_offset), int(y.shape[1]), ptr(y),
                                              int(n_cand), iptr(m), ptr(lp), iptr(pk), C.c_void_p(logw_dev_ptr),
                                              C.c_void_p(tail_dev_ptr)), "chmc_score_future_device")
        return lp, pk

    def extended(self, y_new):
        """A new context with T + H observations: this context's data, shared or per chain, with y_new [H] or [B, H]
        appended, and everything else as `sibling` carries it: model, S, R, obs_interval, noise kind and the chains' own
        sigma, splitting, B, device and the metric (per chain or shared)."""
        y_new = np.asarray(y_new, dtype=np.float64)
        if y_new.ndim == 3 and y_new.shape[2] == 1:
            y_new = y_new[:, :, 0]
        if y_new.ndim not in (1, 2) or y_new.shape[-1] < 1 or (y_new.ndim == 2 and y_new.shape[0] != self.B):
            raise ValueError(f"y_new must have shape (H,) or ({self.B}, H), got {y_new.shape}")
        sigma = self.sigma
        if sigma is not None and not isinstance(sigma, str) and np.ndim(sigma) > 0:
            sigma = float(np.asarray(sigma)[0])  # (the chains' own levels follow with the observations)
        per_chain = self.per_chain_observations or y_new.ndim == 2
        if per_chain:
            y_old, sg = self.observations()
            y_all = np.concatenate([y_old, np.broadcast_to(y_new, (self.B, y_new.shape[-1]))], 1)
        else:
            y_all = np.concatenate([self._y, y_new])
        ext = ChmcContext(self._model, self._obs_interval, self.S, self._num_obs_per_subseq, y_all[0] if per_chain else y_all,
                          sigma=sigma, use_gaussian_splitting=self._use_gaussian_splitting, num_chains=self.B,
                          device=self.device)
        if per_chain:
            ext.set_observations(y_all, sg if self.per_chain_observations and self.noisy and not self.variable_sigma else None)
        if self.M_0 is not None:
            ext.set_metric(self.M_0)
        return ext

    # ---- path-wise events (chmc_path_events_device, chmc_predict_events_device; paths.PathEvents / PredictivePosterior)
    def path_events_device(self, x_seq_dev_ptr, n_points, stride, channel, p0, p1, thresholds, events_dev_ptr, mask=None):
        """The event vectors [B][5 + 3 L] of one channel of the device path buffer x_seq [B][n_points][X] over the points
        p0 .. p1 (chmc_path_events_device, include/chmc.h)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        th = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        check(self.L.chmc_path_events_device(self.h, C.c_void_p(x_seq_dev_ptr), int(n_points), int(stride), int(channel),
                                             int(p0), int(p1), len(th), ptr(th) if len(th) else None, iptr(m),
                                             C.c_void_p(events_dev_ptr)), "chmc_path_events_device")

    def predict_events_device(self, seed, draw, chain_offset, horizon, stride, origin, n_rep, n_dev_ptr, mean_dev_ptr,
                              m2_dev_ptr, channel, p0, p1, thresholds, en_dev_ptr, emean_dev_ptr, em2_dev_ptr,
                              events_dev_ptr=None, mask=None, levels=None, cdf_dev_ptr=None, paths_dev_ptr=None, n_keep=0):
        """predict_device which also evaluates every replicate's event vector and folds it per chain and entry
        (chmc_predict_events_device, include/chmc.h)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        lv = None if levels is None else as_c(levels).reshape(-1)
        th = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        check(self.L.chmc_predict_events_device(self.h, int(seed), int(draw), int(chain_offset), int(horizon), int(stride),
                                                int(origin), int(n_rep), iptr(m), 0 if lv is None else len(lv), ptr(lv),
                                                C.c_void_p(n_dev_ptr), C.c_void_p(mean_dev_ptr), C.c_void_p(m2_dev_ptr),
                                                C.c_void_p(cdf_dev_ptr), C.c_void_p(paths_dev_ptr), int(n_keep), int(channel),
                                                int(p0), int(p1), len(th), ptr(th) if len(th) else None,
                                                C.c_void_p(events_dev_ptr), C.c_void_p(en_dev_ptr), C.c_void_p(emean_dev_ptr),
                                                C.c_void_p(em2_dev_ptr)), "chmc_predict_events_device")

    # ---- per-op
    @property
    def dim_c(self):
        return self.C[self.partition]

    @property
    def num_blocks(self):
        return self.K[self.partition]

    def constr(self):
        c = np.empty((self.B, self.dim_c))
        check(self.L.chmc_constr(self.h, ptr(c)), "chmc_constr")
        return c

    def jacob_constr_blocks(self, want_dv=True):
        du = np.empty((self.B, self.dim_c, self.U))
        dv = np.empty((self.B, self.RM, self.NV)) if want_dv else None
        check(self.L.chmc_jacob_constr_blocks(self.h, ptr(du), ptr(dv)), "chmc_jacob_constr_blocks")
        return du, dv

    def chol_gram_blocks(self):
        cC = np.empty((self.B, self.U, self.U))
        cD = np.empty((self.B, self.num_blocks, self.RM, self.RM))
        check(self.L.chmc_chol_gram_blocks(self.h, ptr(cC), ptr(cD)), "chmc_chol_gram_blocks")
        return cC, cD

    def log_det_sqrt_gram(self):
        out = np.empty(self.B)
        check(self.L.chmc_log_det_sqrt_gram(self.h, ptr(out)), "chmc_log_det_sqrt_gram")
        return out

    def grad_log_det_sqrt_gram(self):
        g = np.empty((self.B, self.Q))
        check(self.L.chmc_grad_log_det_sqrt_gram(self.h, ptr(g)), "chmc_grad_log_det_sqrt_gram")
        return g

    def lmult_by_jacob_constr(self, vct):
        vct = self._bq(vct, "vct")
        out = np.empty((self.B, self.dim_c))
        check(self.L.chmc_lmult_by_jacob_constr(self.h, ptr(vct), ptr(out)), "chmc_lmult_by_jacob_constr")
        return out

    def _bc(self, a, name):
        a = as_c(a)
        if a.shape != (self.B, self.dim_c):
            raise ValueError(f"{name} must have shape ({self.B}, {self.dim_c}), got {a.shape}")
        return a

    def rmult_by_jacob_constr(self, lam):
        lam = self._bc(lam, "vct")
        out = np.empty((self.B, self.Q))
        check(self.L.chmc_rmult_by_jacob_constr(self.h, ptr(lam), ptr(out)), "chmc_rmult_by_jacob_constr")
        return out

    def lmult_by_inv_gram(self, vct):
        vct = self._bc(vct, "vct")
        out = np.empty((self.B, self.dim_c))
        check(self.L.chmc_lmult_by_inv_gram(self.h, ptr(vct), ptr(out)), "chmc_lmult_by_inv_gram")
        return out

    def normal_space_component(self, vct):
        vct = self._bq(vct, "vct")
        out = np.empty((self.B, self.Q))
        check(self.L.chmc_normal_space_component(self.h, ptr(vct), ptr(out)), "chmc_normal_space_component")
        return out

    def project_onto_cotangent_space(self):
        check(self.L.chmc_project_onto_cotangent_space(self.h), "chmc_project_onto_cotangent_space")

    def hamiltonian(self):
        h = np.empty((self.B, 3))
        check(self.L.chmc_hamiltonian(self.h, ptr(h)), "chmc_hamiltonian")
        return h

    def neg_log_dens_and_grad(self, q, use_gaussian_splitting=False, want_grad=True):
        """conditioned_diffusion_neg_log_dens_and_grad (sde/mici_extensions.py:82-205) at q [B, U + V0 + T S V]."""
        QH = self.U + self.NV
        q = as_c(q)
        if q.shape != (self.B, QH):
            raise ValueError(f"q must have shape ({self.B}, {QH}), got {q.shape}")
        val = np.empty(self.B)
        g = np.empty((self.B, QH)) if want_grad else None
        check(self.L.chmc_neg_log_dens_and_grad(self.h, ptr(q), int(bool(use_gaussian_splitting)), ptr(val), ptr(g)),
              "chmc_neg_log_dens_and_grad")
        return val, g

    def neg_log_dens_and_grad_device(self, q_dev_ptr, grad_dev_ptr=None, use_gaussian_splitting=False):
        """The same on device buffers (q [B, U + V0 + T S V] and, optionally, the gradient): returns the values [B]."""
        val = np.empty(self.B)
        check(self.L.chmc_neg_log_dens_and_grad_device(self.h, C.c_void_p(q_dev_ptr), int(bool(use_gaussian_splitting)),
                                                       ptr(val), C.c_void_p(grad_dev_ptr or 0)),
              "chmc_neg_log_dens_and_grad_device")
        return val

    def adam_objective_device(self, u_v_dev_ptr, grad_dev_ptr):
        """One read-back per Adam iteration of the initial-state finder: [B, 3] = objective, |u_v|^2, gradient finite."""
        out = np.empty((self.B, 3))
        check(self.L.chmc_adam_objective_device(self.h, C.c_void_p(u_v_dev_ptr), C.c_void_p(grad_dev_ptr), ptr(out)),
              "chmc_adam_objective_device")
        return out

    def adam_update_device(self, u_v_dev_ptr, m_dev_ptr, v_dev_ptr, grad_dev_ptr, coef, b1=0.9, b2=0.999, eps=1e-8):
        """Adam step in place on device buffers; coef [B, 2] = 1 / (1 - b2^t), lr / (1 - b1^t) (0: parameters stay)."""
        coef = as_c(np.asarray(coef, dtype=np.float64).reshape(self.B, 2))
        check(self.L.chmc_adam_update_device(self.h, C.c_void_p(u_v_dev_ptr), C.c_void_p(m_dev_ptr), C.c_void_p(v_dev_ptr),
                                             C.c_void_p(grad_dev_ptr), ptr(coef), float(b1), float(b2), float(eps)),
              "chmc_adam_update_device")

    @staticmethod
    def _row_keys(rows, stream, draw):
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        stream = np.ascontiguousarray(np.broadcast_to(np.asarray(stream, dtype=np.int32), rows.shape))
        draw = np.ascontiguousarray(np.broadcast_to(np.asarray(draw, dtype=np.uint64), rows.shape))
        return rows, stream, draw, draw.ctypes.data_as(C.POINTER(C.c_ulonglong))

    def fill_normal_device(self, seed, rows, stream, draw, n_cols, dst_dev_ptr, ld=None):
        """Keyed N(0, 1) draws into the listed rows of a device buffer [B, ld] (chmc_fill_normal_device, include/chmc.h):
        row rows[r] gets n_cols values of the stream (seed, stream[r], draw[r])."""
        rows, stream, draw, dptr = self._row_keys(rows, stream, draw)
        check(self.L.chmc_fill_normal_device(self.h, int(seed), len(rows), iptr(rows), iptr(stream), dptr, int(n_cols),
                                             C.c_void_p(dst_dev_ptr), int(n_cols if ld is None else ld)),
              "chmc_fill_normal_device")

    def fill_normal(self, seed, rows, stream, draw, out):
        """The same into the listed rows of a host array `out` [B, n_cols] (or a [B, ld] array's view [:, :n_cols]), in place;
        the same kernel, hence the same bits as fill_normal_device on this backend."""
        if out.dtype != np.float64 or out.ndim != 2 or out.shape[0] != self.B or out.strides[1] != 8 or out.strides[0] % 8:
            raise ValueError(f"out must be a float64 array [{self.B}, n_cols] with contiguous rows")
        rows, stream, draw, dptr = self._row_keys(rows, stream, draw)
        check(self.L.chmc_fill_normal(self.h, int(seed), len(rows), iptr(rows), iptr(stream), dptr, int(out.shape[1]),
                                      out.ctypes.data_as(_lib.dp), out.strides[0] // 8), "chmc_fill_normal")
        return out

    def adam_begin_tries_device(self, seed, rows, stream, draw, u_v_dev_ptr, m_dev_ptr, v_dev_ptr, grad_dev_ptr):
        """Deal a try into each listed row of the finder's device buffers (chmc_adam_begin_tries_device): keyed start
        point, zero moments and gradient, the row's carried scan guess back to the cold guess."""
        rows, stream, draw, dptr = self._row_keys(rows, stream, draw)
        check(self.L.chmc_adam_begin_tries_device(self.h, int(seed), len(rows), iptr(rows), iptr(stream), dptr,
                                                  C.c_void_p(u_v_dev_ptr), C.c_void_p(m_dev_ptr), C.c_void_p(v_dev_ptr),
                                                  C.c_void_p(grad_dev_ptr)), "chmc_adam_begin_tries_device")

    def gd_objective_device(self, q_dev_ptr, xo_dev_ptr, reg_coeff, grad_dev_ptr):
        """Objective and gradient of the generic gradient-descent finder on device buffers q [B, Q], x_obs_seq_init
        [B, T, X] (chmc_gd_objective_device): returns [B, 3] = objective, max |c|, objective and gradient finite."""
        out = np.empty((self.B, 3))
        check(self.L.chmc_gd_objective_device(self.h, C.c_void_p(q_dev_ptr), C.c_void_p(xo_dev_ptr), float(reg_coeff),
                                              C.c_void_p(grad_dev_ptr), ptr(out)), "chmc_gd_objective_device")
        return out

    def adam_update_cols_device(self, n_cols, x_dev_ptr, m_dev_ptr, v_dev_ptr, grad_dev_ptr, coef, b1=0.9, b2=0.999, eps=1e-8):
        """adam_update_device on buffers of [B, n_cols]."""
        coef = as_c(np.asarray(coef, dtype=np.float64).reshape(self.B, 2))
        check(self.L.chmc_adam_update_cols_device(self.h, int(n_cols), C.c_void_p(x_dev_ptr), C.c_void_p(m_dev_ptr),
                                                  C.c_void_p(v_dev_ptr), C.c_void_p(grad_dev_ptr), ptr(coef), float(b1),
                                                  float(b2), float(eps)), "chmc_adam_update_cols_device")

    def gd_project_device(self, mask, q_dev_ptr, xo_dev_ptr, newton=True, constraint_tol=1e-9, position_tol=1e-8,
                          divergence_tol=1e10, max_iters=50):
        """Masked rows of q [B, Q] / x_obs_seq_init [B, T, X] (device) become the chains' states in partition 0 and are
        projected from there with dt = 1; converged points replace row and state (chmc_gd_project_device)."""
        m = np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        status, iters, err = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32), np.zeros(self.B)
        check(self.L.chmc_gd_project_device(self.h, iptr(m), C.c_void_p(q_dev_ptr), C.c_void_p(xo_dev_ptr), int(newton),
                                            constraint_tol, position_tol, divergence_tol, int(max_iters), iptr(status),
                                            iptr(iters), ptr(err)), "chmc_gd_project_device")
        self.partition = 0
        return dict(status=status, iters=iters, err=err)

    def project(self, q, dt, newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50):
        q = self._bq(q, "q")
        dt = as_c(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.B,)))
        q_out, mu = np.empty((self.B, self.Q)), np.empty((self.B, self.Q))
        iters, status = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        ndq, err = np.empty(self.B), np.empty(self.B)
        check(self.L.chmc_project(self.h, int(newton), ptr(q), ptr(dt), constraint_tol, position_tol, divergence_tol,
                                  int(max_iters), ptr(q_out), ptr(mu), iptr(iters), ptr(ndq), ptr(err), iptr(status)),
              "chmc_project")
        return dict(q=q_out, mu=mu, iters=iters, norm_dq=ndq, err=err, status=status)

    def leapfrog_step(self, dt, active=None, n_inner_step=1, newton=True, constraint_tol=1e-9, position_tol=1e-8,
                      divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8):
        dt = as_c(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.B,)))
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        status = np.zeros(self.B, dtype=np.int32)
        itf, itb = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        rev = np.zeros(self.B)
        check(self.L.chmc_leapfrog_step(self.h, ptr(dt), iptr(act), int(n_inner_step), int(newton), constraint_tol,
                                        position_tol, divergence_tol, int(max_iters), reverse_check_tol, iptr(status),
                                        iptr(itf), iptr(itb), ptr(rev)), "chmc_leapfrog_step")
        return dict(status=status, iters_fwd=itf, iters_bwd=itb, rev_err=rev)

    def leapfrog_steps(self, dt, n_steps, active=None, n_inner_step=1, newton=True, constraint_tol=1e-9, position_tol=1e-8,
                       divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8):
        """Whole trajectories: up to n_steps (an int, or one int per chain) consecutive integrator steps per chain, every
        chain at its own pace; a chain's trajectory ends at its first failed step (include/chmc.h chmc_leapfrog_steps).
        Returns n_done, status (0, or the failing step's code; -1 inactive), summed iters_fwd / iters_bwd, rev_err."""
        dt = as_c(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.B,)))
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        per_chain = None if np.isscalar(n_steps) else np.ascontiguousarray(np.broadcast_to(n_steps, (self.B,)), dtype=np.int32)
        n_all = int(n_steps) if per_chain is None else 0
        ndone, status = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        itf, itb = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        rev = np.zeros(self.B)
        check(self.L.chmc_leapfrog_steps(self.h, ptr(dt), iptr(act), iptr(per_chain), n_all, int(n_inner_step), int(newton),
                                         constraint_tol, position_tol, divergence_tol, int(max_iters), reverse_check_tol,
                                         iptr(ndone), iptr(status), iptr(itf), iptr(itb), ptr(rev)), "chmc_leapfrog_steps")
        return dict(n_done=ndone, status=status, iters_fwd=itf, iters_bwd=itb, rev_err=rev)

    # ---- the one collective of a chain-sharded run, through the library's own RCCL binding (include/chmc.h)
    def comm_init(self, id128, rank, world):
        """Create this context's RCCL communicator (collective: every rank, same 128-byte id from comm_unique_id)."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        check(self.L.chmc_comm_init(self.h, buf, int(rank), int(world)), "chmc_comm_init")
        self.comm_world = int(world)

    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * 128)()
        check(_lib.lib().chmc_comm_unique_id(buf), "chmc_comm_unique_id")
        return bytes(buf)

    def gather_samples_device(self, local_dev_ptr, count, gathered_dev_ptr):
        """All-gather of `count` doubles per rank between device buffers: gathered [world][count], rank-major."""
        check(self.L.chmc_gather_samples(self.h, C.c_void_p(local_dev_ptr), int(count), C.c_void_p(gathered_dev_ptr)),
              "chmc_gather_samples")

    def comm_info(self):
        """(world size, rank) read back from the RCCL communicator."""
        wd, rk = C.c_int(0), C.c_int(0)
        check(self.L.chmc_comm_info(self.h, C.byref(wd), C.byref(rk)), "chmc_comm_info")
        return wd.value, rk.value

    def comm_destroy(self):
        check(self.L.chmc_comm_destroy(self.h), "chmc_comm_destroy")

    def diagnostics(self):
        """Kernel-path diagnostics (include/chmc.h chmc_get_diagnostics): time-parallel scan counters and launches of the
        optional kernel families."""
        out = (C.c_longlong * 80)()
        check(self.L.chmc_get_diagnostics(self.h, out), "chmc_get_diagnostics")
        v = np.array(out[:], dtype=np.int64)
        return dict(par_scan=v[:64], gram_mfma_launches=int(v[64]), gram_valu_launches=int(v[65]),
                    retract_kernel_launches=int(v[66]), traj_kernel_launches=int(v[67]),
                    newton_fsm_launches=int(v[68]), newton_factor8_launches=int(v[69]), pair_scan_rounds=int(v[70]),
                    newton_scan_launches=int(v[71]), newton_rounds=int(v[72]), path_par_launches=int(v[74]),
                    path_seq_launches=int(v[75]), predict_wave_launches=int(v[76]), predict_seq_launches=int(v[77]),
                    path_events_wave_launches=int(v[78]), path_events_seq_launches=int(v[79]),
                    extra=v[68:80])

    def counters(self):
        out = (C.c_longlong * 8)()
        check(self.L.chmc_get_counters(self.h, out), "chmc_get_counters")
        keys = ("constr", "jacob_constr_blocks", "lu_jacob_product_blocks", "chol_gram_blocks",
                "grad_log_det_sqrt_gram", "leapfrog_step", "projection_iterations", "_")
        return dict(zip(keys, (int(v) for v in out)))
