"""Helper (not collected): a torch-fp64 restatement of find_initial_state_by_gradient_descent
(sde/mici_extensions.py:1550-1676), independent of the library: the objective from oracle/py/models.py's forward_func /
generate_z / generate_x_0 with torch.autograd for its gradient, the Adam step of jax.example_libraries.optimizers.adam
written out, and the projection by the C oracle's solver (OracleSystem.project, what helpers judges chmc_project with).
The keyed start points come from the NumPy restatement of the device generator (test_rng.reference_normals).

ChainSearch is the try loop of ONE chain, one iteration per call; find_one_chain drives it alone, find_chains drives
several of them side by side (lanes that never interact) so that the autograd passes, whose cost is per call and not per
element, are shared: the suite uses that one."""
import numpy as np
import torch
from oracle.py import models as om
from test_rng import reference_normals

GD_DRAW_BIT = (1 << 63) | (1 << 62)


def objective(model, q, xo, S, dl, noisy, var_sigma, reg_coeff):
    """init_objective (:1582-1618) at the points q [L, Q] with x_obs_seq_init xo [L, T, X] (L independent lanes):
    (objective [L], c [L, T, X], gradient [L, Q]).  The T intervals of a point are independent as well, so the S-step scan
    runs over all of them at once (states [X, L, T])."""
    m = om.MODELS[model]
    q, xo = np.atleast_2d(np.asarray(q, dtype=np.float64)), np.asarray(xo, dtype=np.float64)
    xo = xo.reshape((q.shape[0],) + xo.shape[-2:])
    L, T, V = q.shape[0], xo.shape[1], m.dim_v
    U = m.dim_z + int(var_sigma)
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    xot = torch.tensor(xo, dtype=torch.float64)
    nv = T * S * V
    assert qt.shape[1] == U + m.dim_v_0 + nv + (T if noisy else 0)
    u, v_0 = qt[:, :U], qt[:, U:U + m.dim_v_0]
    v = qt[:, U + m.dim_v_0:U + m.dim_v_0 + nv].reshape(L, T, S, V)
    z_l = [m.generate_z(u[l]) for l in range(L)]
    x_0 = torch.stack([m.generate_x_0(z_l[l], v_0[l]) for l in range(L)])          # [L, X]
    z = torch.stack(z_l, 1)[:, :, None]                                             # [Z, L, 1]
    x = torch.cat([x_0[:, None], xot[:, :-1]], 1).permute(2, 0, 1)                  # x_inits (:1604) as [X, L, T]
    for s in range(S):
        x = m.forward_func(z, x, v[:, :, s].permute(2, 0, 1), dl)
    c = x.permute(1, 2, 0) - xot
    obj = 0.5 * torch.mean(c ** 2, (1, 2)) + 0.5 * reg_coeff * torch.mean(qt ** 2, 1)
    obj.sum().backward()                                                            # (lanes do not interact)
    return obj.detach().numpy().copy(), c.detach().numpy().copy(), qt.grad.numpy().copy()


class ChainSearch:
    """The try loop (:1643-1676) of global chain `chain`.  x_obs_seq_init(chains, tries) as the library's finder takes it.
    After the search: q, xo (x_obs_seq_init of the winning try), tries, ends = [(iteration, outcome, deciding figures), ...]."""

    def __init__(self, osys, chain, seed, x_obs_seq_init, tol=1e-9, adam_step_size=2e-1, coarse_tol=1e-1, max_iters=1000,
                 max_num_tries=10, use_newton=True):
        self.osys, self.chain, self.seed, self.gen = osys, chain, seed, x_obs_seq_init
        self.tol, self.lr, self.coarse_tol, self.max_iters, self.max_num_tries = tol, adam_step_size, coarse_tol, max_iters, max_num_tries
        self.newton = use_newton
        self.k, self.ends, self.found = -1, [], False
        self._next_try()

    def _next_try(self):
        self.k += 1
        if self.k >= self.max_num_tries:
            raise RuntimeError(f"Did not find valid state in {self.max_num_tries} tries.")
        Q = self.osys.Q
        self.q = reference_normals(Q, self.chain, self.seed, GD_DRAW_BIT | self.k)
        self.xo = np.asarray(self.gen([self.chain], [self.k]))[0]
        self.m, self.v, self.i = np.zeros(Q), np.zeros(Q), 0

    def advance(self, obj, c, g):
        """iteration self.i of the current try, given objective, c and gradient at self.q"""
        b1, b2, eps = 0.9, 0.999, 1e-8
        i = self.i
        if not np.isfinite(obj):
            self.ends.append((i, "diverged", obj))
            return self._next_try()
        mac = np.abs(c).max()
        if mac < self.coarse_tol:
            st, q1, _, it, ndq, err = self.osys.project(self.newton, self.q, self.q, self.xo, 0, 1.0, ctol=self.tol)
            if st != 0:
                self.ends.append((i, "projection failed", (mac, st, err)))
                return self._next_try()
            cmax = np.abs(self.osys.constr(q1, self.xo, 0)).max()
            if cmax < self.tol:
                self.ends.append((i, "projected", (mac, err, cmax)))
                self.q, self.tries, self.found = q1, self.k + 1, True
                return
        if i + 1 >= self.max_iters:
            self.ends.append((i, "budget", None))
            return self._next_try()
        with np.errstate(over="ignore", invalid="ignore"):
            self.m = b1 * self.m + (1 - b1) * g
            self.v = b2 * self.v + (1 - b2) * g * g
            mh, vh = self.m / (1 - b1 ** (i + 1)), self.v / (1 - b2 ** (i + 1))
            self.q = self.q - self.lr * mh / (np.sqrt(vh) + eps)
        self.i = i + 1


def find_chains(model, osys, chains, seed, x_obs_seq_init, S, dl, noisy, var_sigma=False, reg_coeff=2e-2, **kw):
    """ChainSearch for every chain of `chains`, iterated side by side; returns the list of finished searches."""
    ss = [ChainSearch(osys, c, seed, x_obs_seq_init, **kw) for c in chains]
    while True:
        live = [s for s in ss if not s.found]
        if not live:
            return ss
        obj, c, g = objective(model, np.stack([s.q for s in live]), np.stack([s.xo for s in live]), S, dl, noisy, var_sigma,
                              reg_coeff)
        for l, s in enumerate(live):
            s.advance(obj[l], c[l], g[l])


def find_one_chain(model, osys, chain, seed, x_obs_seq_init, S, dl, noisy, var_sigma=False, reg_coeff=2e-2, **kw):
    return find_chains(model, osys, [chain], seed, x_obs_seq_init, S, dl, noisy, var_sigma, reg_coeff, **kw)[0]
