"""Synthetic FitzHugh-Nagumo workloads of BASELINE.json (host-side set-up shared by bench.py, the examples and the
multi-GPU driver): data simulation, contexts, initial states, momentum refresh, static-trajectory transitions."""
import numpy as np
from . import example_models as em
from .context import ChmcContext, DEFAULT_SOLVER
from .init import fhn_initial_states, fhn_initial_states_device

SEED = 20200710  # scripts/utils.py:75-77
# daily counts of the boarding-school influenza outbreak (the reference's scripts/sir_model_boarding_school_data.npz,
# loaded at scripts/sir_model_chmc_experiment.py:62-64; obs_interval 1.0)
BOARDING_SCHOOL_COUNTS = (3, 8, 28, 75, 221, 281, 255, 235, 190, 125, 70, 28, 12, 5)


class FhnWorkload:
    """FHN chains on one device: B chains of the (T, S, R, sigma) configuration, set up the way
    scripts/fhn_model_noisy_obs_chmc_experiment.py does (simulated data, linear-interpolation initial states,
    Newton solver with the script tolerances).  init="gradient_descent": the initial states come from the reference's generic
    finder instead (init.find_initial_states_by_gradient_descent, keyed by (seed, global chain, try), resident on the device)."""

    def __init__(self, num_chains, num_steps_per_obs=400, num_obs=100, num_obs_per_subseq=5, sigma=0.1,
                 obs_interval=0.2, device=0, chain_offset=0, total_chains=None, use_gaussian_splitting=False,
                 num_steps_per_obs_data=10000, seed=SEED, device_init=False, init=None, log=None):
        self.B, self.S, self.T, self.R = num_chains, num_steps_per_obs, num_obs, num_obs_per_subseq
        self.sigma, self.obs_interval = sigma, obs_interval
        self.seed, self.chain_offset = seed, chain_offset
        self.y = em.simulate_fhn_observations(num_obs, obs_interval, num_steps_per_obs_data, seed=seed, sigma=sigma)
        self.ctx = ChmcContext("fhn", obs_interval, num_steps_per_obs, num_obs_per_subseq, self.y[:, 0], sigma=sigma,
                               use_gaussian_splitting=use_gaussian_splitting, num_chains=num_chains, device=device)
        if init not in (None, "linear_interpolation", "gradient_descent"):
            raise ValueError("init must be None, 'linear_interpolation' or 'gradient_descent'")
        if init == "gradient_descent":
            from .init import find_initial_states_by_gradient_descent, fhn_x_obs_seq_init
            _, _, self.init_tries = find_initial_states_by_gradient_descent(
                self.ctx, fhn_x_obs_seq_init(self.y[:, 0], seed), seed, chain_offset=chain_offset, total_chains=total_chains,
                log=log)
            total = num_chains + chain_offset if total_chains is None else total_chains
            self.rngs = [np.random.default_rng(s) for s in
                         np.random.SeedSequence(seed).spawn(total)[chain_offset:chain_offset + num_chains]]
        elif device_init:  # same states, solved on the device (no [B, Q] host array, no 8 B Q byte upload)
            self.rngs = fhn_initial_states_device(self.ctx, em.fhn, self.y, seed=seed, chain_offset=chain_offset,
                                                  total_chains=total_chains)
        else:
            q, xo, self.rngs = fhn_initial_states(em.fhn, obs_interval, num_steps_per_obs, self.y, num_chains,
                                                  sigma is not None, seed=seed, chain_offset=chain_offset,
                                                  total_chains=total_chains)
            self.ctx.set_state(q, None, xo, 0)
        self.solver = dict(DEFAULT_SOLVER)
        self._torch_gen = None

    # momentum refresh: IndependentMomentumTransition -> system.sample_momentum (sde/mici_extensions.py:1256-1259)
    def refresh_momentum_host(self):
        p = np.stack([r.standard_normal(self.ctx.Q) for r in self.rngs])
        self.ctx.set_momentum(p)
        self.ctx.project_onto_cotangent_space()

    def refresh_momentum_device(self, torch, device):
        """N(0, I) drawn on the device (torch is only the RNG / allocator here), then projected by the library."""
        if self._torch_gen is None:
            self._torch_gen = torch.Generator(device=device)
            self._torch_gen.manual_seed(SEED + 17 * int(self.rngs[0].integers(1 << 30)))
            self._pbuf = torch.empty((self.B, self.ctx.Q), dtype=torch.float64, device=device)
        self._pbuf.normal_(generator=self._torch_gen)
        torch.cuda.synchronize(device)
        self.ctx.set_momentum_device(self._pbuf.data_ptr())
        self.ctx.project_onto_cotangent_space()

    def refresh_momentum(self):
        """Device-side refresh (Philox stream keyed by the workload seed; draw counter per call)."""
        self._draw = getattr(self, "_draw", 0) + 1
        self.ctx.sample_momentum(self.seed, self._draw, self.chain_offset)

    def step(self, dt, active=None):
        return self.ctx.leapfrog_step(dt, active=active, **self.solver)

    def bytes_per_chain_step(self, k_iters, partition=None, newton=True):
        """Algorithmic bytes of one chain-step, SURVEY.md section 8(d): 8 [k (4 nnz + 8 Q) + 10 nnz + 25 Q]
        (quasi-Newton: k (nnz + 7 Q) instead of the Newton term)."""
        nnz = self.nnz(partition)
        it = (4 * nnz + 8 * self.ctx.Q) if newton else (nnz + 7 * self.ctx.Q)
        return 8.0 * (k_iters * it + 10 * nnz + 25 * self.ctx.Q)

    def nnz(self, partition=None):
        c = self.ctx
        p = c.partition if partition is None else partition
        return (c.C[p] * c.U + sum(b["nrows"] * b["ncols"] for b in c.blocks[p])
                + (c.T if c.noisy else 0))


class SirWorkload(FhnWorkload):
    """SIR chains on the boarding-school data as scripts/sir_model_chmc_experiment.py sets them up (BASELINE.json
    configs[3]): 14 daily counts, S steps per observation, ONE sub-sequence of R = 14 observations (dense 14 x 14 Gram
    block), sigma_y = 1, initial states by the Adam-based finder of the noisy system (sde/mici_extensions.py:1679-1801)
    with one generator for the whole batch (the finder restarts chains, so draws are not chain-indexed) -- or, with
    keyed_init, from draws keyed by (seed, global chain, try): chain c of `total_chains` then starts from the same state
    whichever shard [chain_offset, chain_offset + num_chains) it runs in."""

    def __init__(self, num_chains, num_steps_per_obs=200, sigma=1.0, device=0, chain_offset=0, total_chains=None,
                 use_gaussian_splitting=False, seed=SEED, adam_step_size=1e-1, log=None, keyed_init=False):
        from . import init
        self.B, self.S, self.T, self.R = num_chains, num_steps_per_obs, len(BOARDING_SCHOOL_COUNTS), len(BOARDING_SCHOOL_COUNTS)
        self.sigma, self.obs_interval = sigma, 1.0
        self.seed, self.chain_offset = seed, chain_offset
        self.y = np.asarray(BOARDING_SCHOOL_COUNTS, dtype=np.float64).reshape(-1, 1)
        self.ctx = ChmcContext("sir", self.obs_interval, num_steps_per_obs, self.R, self.y[:, 0], sigma=sigma,
                               use_gaussian_splitting=use_gaussian_splitting, num_chains=num_chains, device=device)
        rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(chain_offset + 1)[chain_offset])
        if keyed_init:
            _, _, self.init_tries = init.find_initial_states_by_gradient_descent_noisy_system(
                self.ctx, seed=seed, chain_offset=chain_offset, total_chains=total_chains, adam_step_size=adam_step_size,
                max_iters=5000, log=log)
        else:
            _, _, self.init_tries = init.find_initial_states_by_gradient_descent_noisy_system(
                self.ctx, rng, adam_step_size=adam_step_size, max_iters=5000, log=log)
        self.rngs = [rng]
        self.solver = dict(DEFAULT_SOLVER)
        self._torch_gen = None


class GridWorkload:
    """G data sets x n chains each of ONE shape (model, T, S, R) in one context: the cells of a sweep over noise levels and
    data seeds, a replication study or a calibration check, which on their own (the reference runs 4 chains per cell) leave
    the GPU nearly empty.  Chain c of the whole job belongs to cell c // n; a rank holds the contiguous shard
    [chain_offset, chain_offset + num_chains) of the G n chains -- shards may cut through a cell -- with each chain's own
    (y, sigma) installed by ChmcContext.set_observations.

    cells: a list of (y_seq [T] or [T, 1], sigma) pairs; sigma a number for every cell (fixed noise), or None / "variable"
    for every cell.  `groups` [B] is the global cell id of this rank's chains (the `groups` argument of the samplers and of
    traces.summarize), `total_chains` = G n, `n_groups` = G.  init: "linear_interpolation" (FitzHugh-Nagumo: the scripts'
    initial states, every chain from its own cell's data, keyed by the global chain number: any sharding gives the same
    states), or None (the caller sets or finds the states)."""

    def __init__(self, cells, chains_per_cell, model="fhn", num_steps_per_obs=400, num_obs_per_subseq=5, obs_interval=0.2,
                 device=0, chain_offset=0, num_chains=None, use_gaussian_splitting=False, seed=SEED,
                 init="linear_interpolation"):
        if not cells:
            raise ValueError("cells must hold at least one (y_seq, sigma) pair")
        ys = [np.asarray(y, dtype=np.float64).reshape(-1) for y, _ in cells]
        sigmas = [s for _, s in cells]
        if len({len(y) for y in ys}) != 1:
            raise ValueError("every cell must have the same number of observations")
        kinds = {"variable" if isinstance(s, str) else "none" if s is None else "fixed" for s in sigmas}
        if len(kinds) != 1:
            raise ValueError("sigma must be a number for every cell, or None / \"variable\" for every cell")
        fixed = kinds == {"fixed"}
        self.n_groups, self.chains_per_cell = len(cells), int(chains_per_cell)
        self.total_chains = self.n_groups * self.chains_per_cell
        self.chain_offset = int(chain_offset)
        self.B = self.total_chains - self.chain_offset if num_chains is None else int(num_chains)
        if self.chains_per_cell < 1 or self.chain_offset < 0 or self.B < 1 or self.chain_offset + self.B > self.total_chains:
            raise ValueError(f"the shard [{self.chain_offset}, {self.chain_offset + self.B}) does not lie in the "
                             f"{self.total_chains} chains of {self.n_groups} cells x {self.chains_per_cell}")
        self.groups = (np.arange(self.chain_offset, self.chain_offset + self.B) // self.chains_per_cell).astype(np.int64)
        self.cell_y, self.cell_sigma = np.stack(ys), sigmas
        self.y = self.cell_y[self.groups]                                              # [B, T]
        self.sigma = np.asarray(sigmas, dtype=np.float64)[self.groups] if fixed else sigmas[0]
        self.model, self.S, self.T, self.R = model, num_steps_per_obs, self.y.shape[1], num_obs_per_subseq
        self.obs_interval, self.seed = obs_interval, seed
        self.ctx = ChmcContext(model, obs_interval, num_steps_per_obs, num_obs_per_subseq, self.y, sigma=self.sigma,
                               use_gaussian_splitting=use_gaussian_splitting, num_chains=self.B, device=device)
        if init not in (None, "linear_interpolation"):
            raise ValueError("init must be None or 'linear_interpolation'")
        if init == "linear_interpolation":
            if model != "fhn":
                raise ValueError("linear-interpolation initial states are the FitzHugh-Nagumo scripts'")
            self.rngs = fhn_initial_states_device(self.ctx, em.fhn, self.y[:, :, None], seed=seed, chain_offset=self.chain_offset,
                                                  total_chains=self.total_chains)
        self.solver = dict(DEFAULT_SOLVER)

    @classmethod
    def fhn_noise_grid(cls, sigmas, data_seeds, chains_per_cell, num_obs=100, obs_interval=0.2, num_steps_per_obs_data=10000,
                       **kw):
        """The cells of scripts/run_fhn_model_noisy_obs_experiments.sh: every noise level x every data seed, each cell's
        data simulated the way the experiment script does for that (sigma, seed) (example_models.simulate_fhn_observations).
        Cell order: sigma-major, `cell_labels` holds (sigma, seed) per cell."""
        labels = [(float(s), int(d)) for s in sigmas for d in data_seeds]
        cells = [(em.simulate_fhn_observations(num_obs, obs_interval, num_steps_per_obs_data, seed=d, sigma=s)[:, 0], s)
                 for s, d in labels]
        w = cls(cells, chains_per_cell, model="fhn", obs_interval=obs_interval, **kw)
        w.cell_labels = labels
        return w

    def cell_chains(self, g):
        """Local indices of this rank's chains that belong to cell g."""
        return np.flatnonzero(self.groups == g)
