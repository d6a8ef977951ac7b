"""Helpers for the tests of per-chain observations (chmc_set_observations): G groups of chains, every group with its own
data set y_g [T] and noise level sigma_g, in ONE context -- against one context per group that holds (y_g, sigma_g) as shared
data, the way every other test of the suite runs.

Test infrastructure only (may import oracle/)."""
import numpy as np
from oracle import c_oracle
from helpers import make_case
from manifold_mcmc_for_diffusions_amd import example_models as em
from manifold_mcmc_for_diffusions_amd.context import ChmcContext

SIZES = (4, 5, 4)          # unequal groups: B = 13, CHMC_HALVES=2 splits 6 | 7, inside group 1
MIN_Y_GAP = 0.05           # the groups' y rows differ by at least this much in EVERY entry
FHN_SIGMAS = (0.05, 0.1, 0.2)
SIR_SIGMAS = (1.0, 1.5, 2.5)

# name: model, T, S, R, noisy, gaussian, var_sigma, obs_interval
LAYOUTS = {
    "a_fhn_noisy_7rows": ("fhn", 12, 16, 5, True, False, False, None),
    "b_fhn_noiseless_gauss": ("fhn", 12, 16, 5, False, True, False, None),
    "c_fhn_16rows": ("fhn", 20, 8, 10, True, False, False, None),
    "d_fhn_65blocks": ("fhn", 130, 8, 2, True, False, False, None),
    "e_sir_one_block": ("sir", 14, 8, 14, True, False, False, 0.25),
    "f_sir_multiblock16": ("sir", 26, 24, 13, True, False, False, None),
    "g_fhn_var_sigma": ("fhn", 12, 16, 5, True, False, True, None),
}


def on_manifold(model, q, xo, y, sigma, var_sigma):
    """q with the observation-noise part solved for: obs_func(x_obs) + sigma n = y, chain by chain (noisy contexts).  y is
    [T] or [B, T], sigma a number or [B]; with variable noise sigma_c = exp(u_c[dim_z])."""
    m = em.MODELS[model]
    T = xo.shape[1]
    q = q.copy()
    sg = np.exp(q[:, m.dim_z]) if var_sigma else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(q),))
    q[:, -T:] = (np.broadcast_to(y, (len(q), T)) - m.obs_func(xo)[..., 0]) / sg[:, None]
    return q


def make_groups(name, seed, sizes=SIZES):
    """The grouped case of a layout: per group a helpers.make_case (random chain points, its oracle system built from the
    group's own (y, sigma)) whose data differ from every other group's by at least MIN_Y_GAP in every entry and whose sigma
    values are distinct.  Noisy FitzHugh-Nagumo layouts: every chain is an on-manifold point of its group's data (distinct
    chains); noiseless and SIR layouts: the group's chain 0 is, and stands for all chains of the group (make_case generates
    the data from it; the chains part ways with their momenta).

    Returns dict: per-chain arrays q [B, Q], x_obs [B, T, X], y [B, T], sigma ([B], "variable" or None), groups [B],
    slices (one per group), cases (one make_case dict per group, `osys`, `y`, `sigma` the group's own) and the layout."""
    model, T, S, R, noisy, gaussian, var_sigma, dt_obs = LAYOUTS[name]
    m = em.MODELS[model]
    sigmas = (FHN_SIGMAS if model == "fhn" else SIR_SIGMAS) if noisy and not var_sigma else (None,) * len(sizes)
    cases, ys = [], []
    for g, n in enumerate(sizes):
        s = seed + 1000 * g
        while True:
            case = make_case(model, T, S, R, noisy, B=n, seed=s, obs_interval=dt_obs, gaussian=gaussian, var_sigma=var_sigma)
            y = case["y"].copy()
            if noisy:  # move the data away from the earlier groups'; the noise part of q follows below
                for t in range(T):
                    while any(abs(y[t] - yo[t]) < 2 * MIN_Y_GAP for yo in ys):
                        y[t] += 3 * MIN_Y_GAP
                break
            if all(np.abs(y - yo).min() >= MIN_Y_GAP for yo in ys):
                break
            s += 1  # noiseless: the data ARE the path of chain 0; another draw
        sigma = "variable" if var_sigma else sigmas[g]
        if not noisy or model == "sir":  # (random SIR points lie far from each other's data: noise terms of 100 sigma and more)
            case["q"] = np.repeat(case["q"][:1], n, 0)
            case["x_obs"] = np.repeat(case["x_obs"][:1], n, 0)
        if noisy:
            case["q"] = on_manifold(model, case["q"], case["x_obs"], y, sigma, var_sigma)
        case["y"], case["sigma"] = y, sigma
        case["osys"] = c_oracle.OracleSystem(model, case["obs_interval"], S, R, y, sigma=sigma, use_gaussian_splitting=gaussian)
        cases.append(case)
        ys.append(y)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    slices = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    groups = np.repeat(np.arange(len(sizes)), sizes)
    out = dict(name=name, model=model, T=T, S=S, R=R, noisy=noisy, gaussian=gaussian, var_sigma=var_sigma,
               obs_interval=cases[0]["obs_interval"], B=int(edges[-1]), cases=cases, slices=slices, groups=groups,
               q=np.concatenate([c["q"] for c in cases]), x_obs=np.concatenate([c["x_obs"] for c in cases]),
               y=np.stack(ys)[groups],
               sigma="variable" if var_sigma else np.asarray(sigmas, dtype=np.float64)[groups] if noisy else None)
    assert_groups_differ(out)
    return out


def assert_groups_differ(gc):
    """What keeps a broadcast of chain 0's data from passing: the groups' y rows differ in every entry by at least MIN_Y_GAP
    and their sigma values are distinct."""
    first = [sl.start for sl in gc["slices"]]
    for i, a in enumerate(first):
        for b in first[i + 1:]:
            assert np.abs(gc["y"][a] - gc["y"][b]).min() >= MIN_Y_GAP, (a, b)
            if isinstance(gc["sigma"], np.ndarray):
                assert gc["sigma"][a] != gc["sigma"][b], (a, b)


def ctx_sigma(gc):
    """The `sigma` argument of a context for the whole layout before set_observations: a number, "variable" or None."""
    s = gc["sigma"]
    return float(s[0]) if isinstance(s, np.ndarray) else s


def grouped_ctx(gc, via_constructor=False):
    """ONE context of all B chains with per-chain data."""
    kw = dict(use_gaussian_splitting=gc["gaussian"], num_chains=gc["B"])
    sig = gc["sigma"] if isinstance(gc["sigma"], np.ndarray) else None
    if via_constructor:
        return ChmcContext(gc["model"], gc["obs_interval"], gc["S"], gc["R"], gc["y"], sigma=gc["sigma"], **kw)
    ctx = ChmcContext(gc["model"], gc["obs_interval"], gc["S"], gc["R"], gc["y"][0], sigma=ctx_sigma(gc), **kw)
    ctx.set_observations(gc["y"], sig)
    return ctx


def shared_ctx(gc, y, sigma, n):
    """A context of n chains with (y, sigma) as shared data, as before per-chain observations existed."""
    return ChmcContext(gc["model"], gc["obs_interval"], gc["S"], gc["R"], y, sigma=sigma,
                       use_gaussian_splitting=gc["gaussian"], num_chains=n)


def run_sequence(ctx, q, p, xo, dts, active, failing, nld=True):
    """The operations GPU test 1 compares, in one fixed order, on a context whose chains are rows [lo, hi) of the batch arrays
    handed in.  Returns a list of (name, array); every array's first axis is the chain."""
    out = []

    def rec(name, a):
        out.append((name, np.array(a, copy=True)))

    def state(tag):
        q1, p1, xo1, _ = ctx.get_state()
        rec(tag + ".q", q1), rec(tag + ".p", p1), rec(tag + ".x_obs", xo1)
        rec(tag + ".hamiltonian", ctx.hamiltonian())
        rec(tag + ".log_det", ctx.log_det_sqrt_gram()), rec(tag + ".grad_log_det", ctx.grad_log_det_sqrt_gram())

    ctx.set_state(q, p, xo, 0)
    rec("constr", ctx.constr())
    state("set")
    # One step of every chain from the unprojected momenta first (the full projection of the opening half-kick).  The
    # library keeps "every momentum is tangent" as ONE flag per context: a chain that fails or sits out a step that began
    # from unprojected momenta keeps the whole context on the full-projection path, so with such chains in that step a
    # chain's bits would depend on who shares its context.  Every chain must therefore pass it.
    r = ctx.leapfrog_step(dts, max_iters=12)
    assert (r["status"] == 0).all(), r
    for key in ("iters_fwd", "iters_bwd", "rev_err"):
        rec(f"pre.{key}", r[key])
    state("pre")
    d = dts.copy()
    d[failing] = 5.0
    for k in range(3):  # masked and failing chains
        r = ctx.leapfrog_step(d, active=active if k == 0 else None, max_iters=12)
        for key in ("status", "iters_fwd", "iters_bwd", "rev_err"):
            rec(f"step{k}.{key}", r[key])
        state(f"step{k}")
    r = ctx.leapfrog_steps(dts, 2, max_iters=12)
    for key in ("n_done", "status", "iters_fwd", "iters_bwd", "rev_err"):
        rec(f"steps.{key}", r[key])
    state("steps")
    if ctx.num_partition > 1:
        ctx.switch_partition()
        rec("switch.constr", ctx.constr())
        state("switch")
        r = ctx.leapfrog_step(dts, max_iters=12)
        for key in ("status", "iters_fwd", "iters_bwd", "rev_err"):
            rec(f"part1.{key}", r[key])
        state("part1")
    if nld and ctx.noisy:  # the comparator target and its gradient at the start points
        QH = ctx.U + ctx.NV
        v, g = ctx.neg_log_dens_and_grad(q[:, :QH], use_gaussian_splitting=False)
        rec("nld.value", v), rec("nld.grad", g)
    return out


def sequence_inputs(gc, seed=99):
    B = gc["B"]
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(gc["q"].shape)
    dts = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 + 0.04 * rng.random(B)) * (0.5 if gc["model"] == "sir" else 1.0)
    active = np.ones(B, dtype=np.int32)
    active[5] = 0
    failing = np.zeros(B, dtype=bool)
    failing[[2, 7]] = True
    return p, dts, active, failing


def split_equals_whole(whole, parts, slices):
    """Bitwise: every recorded array of the one-context run, cut at the group edges, equals the separate contexts'.  Returns
    the names that differ (with the largest absolute difference)."""
    bad = []
    for sl, part in zip(slices, parts):
        assert [n for n, _ in part] == [n for n, _ in whole]
        for (name, a), (_, b) in zip(whole, part):
            if not np.array_equal(a[sl], b, equal_nan=True):
                with np.errstate(invalid="ignore"):
                    bad.append((name, sl.start, float(np.nanmax(np.abs(a[sl].astype(np.float64) - b)))))
    return bad


def run_grouped_vs_separate(gc, nld=True):
    """GPU test 1 (and its host-logic twin).  Control first: the 13 chains with ONE shared data set as one context and as the
    4 | 5 | 4 split (the shard-independence claim); then one context with per-chain data against one context per group with
    that group's (y, sigma) as shared data.  Returns (control differences, grouped differences, the grouped run, the grouped context's kernel-path diagnostics)."""
    p, dts, active, failing = sequence_inputs(gc)
    c0 = gc["cases"][0]
    # -- control: everybody on group 0's data
    if gc["noisy"] and gc["model"] != "sir":
        q_ctl = on_manifold(gc["model"], gc["q"], gc["x_obs"], c0["y"], c0["sigma"], gc["var_sigma"])
        xo_ctl = gc["x_obs"]
    else:
        q_ctl, xo_ctl = np.repeat(c0["q"][:1], gc["B"], 0), np.repeat(c0["x_obs"][:1], gc["B"], 0)
    ctx = shared_ctx(gc, c0["y"], c0["sigma"], gc["B"])
    whole = run_sequence(ctx, q_ctl, p, xo_ctl, dts, active, failing, nld)
    ctx.close()
    parts = []
    for sl in gc["slices"]:
        ctx = shared_ctx(gc, c0["y"], c0["sigma"], sl.stop - sl.start)
        parts.append(run_sequence(ctx, q_ctl[sl], p[sl], xo_ctl[sl], dts[sl], active[sl], failing[sl], nld))
        ctx.close()
    control_bad = split_equals_whole(whole, parts, gc["slices"])
    # -- per-chain data
    assert_groups_differ(gc)
    ctx = grouped_ctx(gc)
    y_back, s_back = ctx.observations()
    assert np.array_equal(y_back, gc["y"])
    if isinstance(gc["sigma"], np.ndarray):
        assert np.array_equal(s_back, gc["sigma"])
    whole = run_sequence(ctx, gc["q"], p, gc["x_obs"], dts, active, failing, nld)
    diag = ctx.diagnostics()
    ctx.close()
    parts = []
    for sl, case in zip(gc["slices"], gc["cases"]):
        ctx = shared_ctx(gc, case["y"], case["sigma"], sl.stop - sl.start)
        parts.append(run_sequence(ctx, gc["q"][sl], p[sl], gc["x_obs"][sl], dts[sl], active[sl], failing[sl], nld))
        ctx.close()
    return control_bad, split_equals_whole(whole, parts, gc["slices"]), whole, diag


class GroupView:
    """The chains [lo, hi) of a context as helpers._ops_at_point sees a context: per-operator results of that slice, input
    vectors embedded in a batch of zeros."""

    def __init__(self, ctx, sl):
        self.ctx, self.sl, self.B = ctx, sl, sl.stop - sl.start
        for k in ("Q", "U", "RM", "num_partition"):
            setattr(self, k, getattr(ctx, k))

    dim_c = property(lambda self: self.ctx.dim_c)
    num_blocks = property(lambda self: self.ctx.num_blocks)

    def _embed(self, a, width):
        full = np.zeros((self.ctx.B, width))
        full[self.sl] = a
        return full

    def constr(self):
        return self.ctx.constr()[self.sl]

    def jacob_constr_blocks(self):
        du, dv = self.ctx.jacob_constr_blocks()
        return du[self.sl], dv[self.sl]

    def chol_gram_blocks(self):
        cC, cD = self.ctx.chol_gram_blocks()
        return cC[self.sl], cD[self.sl]

    def log_det_sqrt_gram(self):
        return self.ctx.log_det_sqrt_gram()[self.sl]

    def grad_log_det_sqrt_gram(self):
        return self.ctx.grad_log_det_sqrt_gram()[self.sl]

    def lmult_by_jacob_constr(self, w):
        return self.ctx.lmult_by_jacob_constr(self._embed(w, self.Q))[self.sl]

    def rmult_by_jacob_constr(self, lam):
        return self.ctx.rmult_by_jacob_constr(self._embed(lam, self.dim_c))[self.sl]

    def lmult_by_inv_gram(self, lam):
        return self.ctx.lmult_by_inv_gram(self._embed(lam, self.dim_c))[self.sl]

    def normal_space_component(self, w):
        return self.ctx.normal_space_component(self._embed(w, self.Q))[self.sl]


def check_grouped_against_oracle(ctx, gc, tol_ops=1e-10, tol_steps=1e-9):
    """GPU test 2: every operator of chmc.h's operator section at 1e-10 in every partition, then two steps per solver (Newton
    and quasi-Newton) at 1e-9 with equal statuses and iteration counts, every chain against the oracle system of its own
    group's (y, sigma), the way helpers.check_ops_against_oracle / check_steps_against_oracle judge a shared-data case.  No
    chain is dropped."""
    from helpers import _ops_at_point, _count_unjudged
    from autodiff_checks import failures, UNJUDGED
    rng = np.random.default_rng(5)
    B, q, xo = gc["B"], gc["q"], gc["x_obs"]
    worst = {}
    for part in range(ctx.num_partition):
        ctx.set_state(q, rng.standard_normal((B, ctx.Q)), xo, part)
        for sl, case in zip(gc["slices"], gc["cases"]):
            _count_unjudged(worst, _ops_at_point(GroupView(ctx, sl), case["osys"], q[sl], xo[sl], part, rng, worst))
    bad = failures(worst, tol_ops)
    assert not bad, f"op parity failures (rel err): {bad}; all: {worst}"
    assert worst.get(UNJUDGED, 0) == 0, worst
    dts = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 + 0.04 * rng.random(B))
    out = []
    for newton in (True, False):
        ctx.set_state(q, rng.standard_normal((B, ctx.Q)), xo, 0)
        ctx.project_onto_cotangent_space()
        _, p0, _, _ = ctx.get_state()
        chains = []
        for c in range(B):
            ch = c_oracle.OracleChain(gc["cases"][gc["groups"][c]]["osys"])
            ch.set(q[c], p0[c], xo[c], 0)
            chains.append(ch)
        for _ in range(2):
            res = ctx.leapfrog_step(dts, newton=newton)
            q1, p1, _, _ = ctx.get_state()
            h1 = ctx.hamiltonian()
            for c in range(B):
                st, itf, itb, _ = chains[c].step(dts[c], newton=newton)
                qo, po, _, _ = chains[c].get()
                assert res["status"][c] == st, (c, res["status"][c], st)
                assert res["iters_fwd"][c] == itf and (st != 0 or res["iters_bwd"][c] == itb), (c, res, itf, itb)
                eq = np.abs(q1[c] - qo).max() / max(1.0, np.abs(qo).max())
                ep = np.abs(p1[c] - po).max() / max(1.0, np.abs(po).max())
                assert eq <= tol_steps and ep <= tol_steps, (c, eq, ep)
                assert abs(h1[c, 0] - chains[c].hamiltonian()) <= 1e-9 * max(1.0, abs(h1[c, 0]))
                out.append((st, itf, itb))
    worst["steps"] = out
    return worst


SIMULATE_DRAW = 1 << 62  # CHMC_SIMULATE_DRAW (include/chmc.h)


def simulate_ctx(gc, n, sigma):
    """A context of n chains for simulate_observations: placeholder data (zeros), per-chain fixed noise levels `sigma`."""
    ctx = ChmcContext(gc["model"], gc["obs_interval"], gc["S"], gc["R"], np.zeros(gc["T"]), sigma=ctx_sigma(gc),
                      use_gaussian_splitting=gc["gaussian"], num_chains=n)
    if sigma is not None:
        ctx.set_observations(np.zeros((n, gc["T"])), sigma)
    return ctx


def check_simulated_observations(name, seed=20240131, offset=3):
    """GPU test 4 (and its host-logic twin): after simulate_observations every chain sits on the manifold of the data it
    generated.  |constr| <= 1e-12 in both partitions (exactly 0 on the observation rows without observation noise); y from
    observations() against a host restatement -- the draws of fill_normal with the same keys, the path by the loop over
    oracle/py/models.py, y = obs + sigma n -- to 1e-10 with scale max(1, |ref|); 13 chains as 6 + 7 with chain_offset give the
    same y and q bitwise.  Returns the measured figures."""
    from test_paths import path_by_models
    gc = make_groups(name, seed=41)  # (the layout and distinct per-chain noise levels; its data are not used)
    B, T, S = gc["B"], gc["T"], gc["S"]
    m = em.MODELS[gc["model"]]
    fixed = isinstance(gc["sigma"], np.ndarray)
    sig = gc["sigma"] if fixed else None
    ctx = simulate_ctx(gc, B, sig)
    ctx.simulate_observations(seed, chain_offset=offset, partition=0)
    q, p, xo, part = ctx.get_state()
    y, s_back = ctx.observations()
    assert part == 0 and not p.any() and np.isfinite(q).all() and np.isfinite(y).all() and np.isfinite(xo).all()
    if fixed:
        assert np.array_equal(s_back, sig)
    # the draws: the keyed normals of the same keys, bitwise
    ref_q = ctx.fill_normal(seed, np.arange(B), offset + np.arange(B), np.uint64(SIMULATE_DRAW), np.zeros((B, ctx.Q)))
    assert np.array_equal(q, ref_q)
    from test_rng import reference_normals
    np.testing.assert_allclose(q[1], reference_normals(ctx.Q, offset + 1, seed, SIMULATE_DRAW), rtol=1e-12, atol=1e-13)
    # the data: host restatement
    path = path_by_models(gc["model"], q, T, S, gc["obs_interval"], ctx.U)[:, S::S]
    sg = np.exp(q[:, m.dim_z]) if gc["var_sigma"] else sig if fixed else 0.0
    ref_y = m.obs_func(path)[..., 0] + (np.asarray(sg).reshape(-1, 1) * q[:, -T:] if gc["noisy"] else 0.0)
    out = dict(y=float((np.abs(y - ref_y) / np.maximum(1.0, np.abs(ref_y))).max()),
               x_obs=float((np.abs(xo - path) / np.maximum(1.0, np.abs(path))).max()))
    assert out["y"] <= 1e-10 and out["x_obs"] <= 1e-10, out
    # on the manifold, both partitions
    for k in range(ctx.num_partition):
        if k:
            ctx.switch_partition()
        c = ctx.constr()
        out[f"constr{k}"] = float(np.abs(c).max())
        assert out[f"constr{k}"] <= 1e-12, out
        if not gc["noisy"]:
            rows = np.concatenate([np.arange(b["row0"], b["row0"] + b["ny"]) for b in ctx.blocks[k]])
            assert not c[:, rows].any(), (k, np.abs(c[:, rows]).max())
    ctx.close()
    # any sharding, the same data
    for lo, hi in ((0, 6), (6, 13)):
        part_ctx = simulate_ctx(gc, hi - lo, None if sig is None else sig[lo:hi])
        part_ctx.simulate_observations(seed, chain_offset=offset + lo, partition=0)
        assert np.array_equal(part_ctx.get_state()[0], q[lo:hi]) and np.array_equal(part_ctx.observations()[0], y[lo:hi])
        part_ctx.close()
    return out


def check_fhn_finders(seed=20200710):
    """GPU test 5, FitzHugh-Nagumo: the linear-interpolation initial states and the gradient-descent finder on a grouped
    context.  Every chain ends on the manifold of its OWN data (|c| below the finder's tolerance, 1e-9) and equals, bitwise,
    the same global chain found in a context that holds only its group."""
    from manifold_mcmc_for_diffusions_amd.init import (fhn_initial_states_device, find_initial_states_by_gradient_descent,
                                                       fhn_x_obs_seq_init)
    gc = make_groups("a_fhn_noisy_7rows", seed=47)
    assert_groups_differ(gc)
    B, tol = gc["B"], 1e-9
    found = {}
    for kind in ("linear_interpolation", "gradient_descent"):
        def find(ctx, y, offset):
            if kind == "linear_interpolation":
                fhn_initial_states_device(ctx, em.fhn, y, seed=seed, chain_offset=offset, total_chains=B)
            else:  # (the data generator is indexed by GLOBAL chain numbers: the whole job's rows)
                find_initial_states_by_gradient_descent(ctx, fhn_x_obs_seq_init(gc["y"], seed), seed, chain_offset=offset,
                                                        total_chains=B, tol=tol)
            return ctx.get_state()[0], ctx.constr()
        ctx = grouped_ctx(gc)
        q, c = find(ctx, gc["y"][:, :, None], 0)
        ctx.close()
        found[kind] = float(np.abs(c).max())
        assert found[kind] < tol, (kind, found)
        for sl, case in zip(gc["slices"], gc["cases"]):
            ctx = shared_ctx(gc, case["y"], case["sigma"], sl.stop - sl.start)
            q_g, c_g = find(ctx, case["y"][:, None], sl.start)
            ctx.close()
            assert np.array_equal(q_g, q[sl]) and np.array_equal(c_g, c[sl]), (kind, sl)
    return found


def check_sir_keyed_finder(seed=20200710, S=8, **finder):
    """GPU test 5, SIR: the keyed noisy Adam finder on a grouped single-block context (three variants of the boarding-school
    counts, three noise levels).  Every chain ends with mean squared residual below the finder's threshold for its own
    (y, sigma), on its manifold, and equals bitwise the same global chain found in a context that holds only its group."""
    from manifold_mcmc_for_diffusions_amd.init import find_initial_states_by_gradient_descent_noisy_system as find
    from manifold_mcmc_for_diffusions_amd.workload import BOARDING_SCHOOL_COUNTS
    counts = np.asarray(BOARDING_SCHOOL_COUNTS, dtype=np.float64)
    ys, sigmas = [counts, counts + 2.0, np.maximum(counts - 3.0, 0.5)], (1.0, 1.5, 2.0)
    groups = np.repeat(np.arange(3), SIZES)
    edges = np.concatenate([[0], np.cumsum(SIZES)])
    y, sig = np.stack(ys)[groups], np.asarray(sigmas)[groups]
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(ys[a] - ys[b]).min() >= MIN_Y_GAP and sigmas[a] != sigmas[b]
    B, T = len(groups), len(counts)
    threshold = finder.get("threshold", 1.0)
    ctx = ChmcContext("sir", 1.0, S, T, y, sigma=sig, num_chains=B)
    q, xo, tries = find(ctx, seed=seed, total_chains=B, **finder)
    c = ctx.constr()
    ctx.close()
    msq = np.mean(q[:, -T:] ** 2, 1)
    assert (msq < threshold).all() and np.abs(c).max() < 1e-9, (msq, np.abs(c).max())
    for g in range(3):
        lo, hi = int(edges[g]), int(edges[g + 1])
        ctx = ChmcContext("sir", 1.0, S, T, ys[g], sigma=sigmas[g], num_chains=hi - lo)
        q_g, xo_g, tries_g = find(ctx, seed=seed, chain_offset=lo, total_chains=B, **finder)
        ctx.close()
        assert np.array_equal(tries_g, tries[lo:hi]), (g, tries_g, tries[lo:hi])
        assert np.array_equal(q_g, q[lo:hi]) and np.array_equal(xo_g, xo[lo:hi]), g
    return dict(tries=tries.tolist(), msq=float(msq.max()), constr=float(np.abs(c).max()))


TRANSITION_SOLVER = dict(newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50,
                         reverse_check_tol=2e-8)


def check_transitions(name, seed, eps, depth=3, n_step=3, screening=False):
    """GPU test 3: one no-U-turn transition and one static transition of every chain of a grouped context against the
    restatements of helpers.py (oracle_tree_transition, oracle_static_transition) run on the chain's OWN oracle system.  The
    decisions (leaves, doublings, moved, errors, acceptance) are equal with no allowance, accept statistic and log weight to
    1e-9, positions to 1e-9 max(1, |q|) per leaf.  No decision may be a coin toss between library and oracle: the margins the
    oracle itself reports must pass test_hip_tree_oracle.admissible (the seeds were screened for that on the CPU; with
    `screening` the inadmissible margins are returned instead of asserted)."""
    from helpers import oracle_static_transition, oracle_tree_transition
    from test_hip_tree_oracle import admissible
    from manifold_mcmc_for_diffusions_amd.dynamic import DynamicTransition, TreeUniforms
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    gc = make_groups(name, seed=48)
    assert_groups_differ(gc)
    B = gc["B"]
    osys_of = [gc["cases"][g]["osys"] for g in gc["groups"]]
    ctx = grouped_ctx(gc)
    problems, worst = [], dict(position=0.0, accept_stat=0.0, logw=0.0)
    # ---- one dynamic transition
    ctx.set_state(gc["q"], None, gc["x_obs"], 0)
    tr = DynamicTransition(ctx, eps, seed, max_tree_depth=depth, max_delta_h=1000.0, solver=dict(TRANSITION_SOLVER))
    ctx.sample_momentum(seed, 1)
    q0, p0, xo0, part = ctx.get_state()
    st = tr.sample(0)
    logw = ctx.tree_get_doubling()["logw"]
    q1 = ctx.get_state()[0]
    un = TreeUniforms(seed, 0, B, 0, B)
    leaves = []
    for c in range(B):
        r = oracle_tree_transition(osys_of[c], q0[c], p0[c], xo0[c], part, lambda kind, d, k, c=c: un.get(kind, d, k)[c], eps, depth,
                                   1000.0, dict(TRANSITION_SOLVER), None)
        bad = admissible(r["margins"])
        if bad:
            problems.append(("tree", c, bad))
            continue
        got = (st["n_step"][c], st["depth"][c], bool(st["moved"][c]), bool(st["integrator_error"][c]), bool(st["diverged"][c]))
        want = (r["n_step"], r["depth"], r["moved"], r["event"][0] == "error", r["event"][0] == "diverged")
        assert got == want, (c, got, want, r["event"])
        acc = r["sum_acc"] / max(r["n_step"], 1)
        e_acc = abs(st["accept_stat"][c] - acc) / max(1.0, abs(acc))
        e_logw = abs(logw[c] - r["logw"]) / max(1.0, abs(r["logw"]))
        assert e_acc <= 1e-9 and e_logw <= 1e-9, (c, e_acc, e_logw)
        e_q = np.abs(q1[c] - r["q"]).max() / max(1.0, np.abs(r["q"]).max())
        assert e_q <= 1e-9 * abs(r["offset"]) if r["offset"] else np.array_equal(q1[c], q0[c]), (c, e_q, r["offset"])
        worst["accept_stat"], worst["logw"] = max(worst["accept_stat"], e_acc), max(worst["logw"], e_logw)
        worst["position"] = max(worst["position"], e_q / max(abs(r["offset"]), 1))
        leaves.append(r["n_step"])
    # ---- one static transition: the sampler's own draws, restated
    ctx.set_state(gc["q"], None, gc["x_obs"], 0)
    res = sample_static_chmc(ctx, 1, n_step, eps, seed, n_adapt=0, solver=dict(TRANSITION_SOLVER), n_head=ctx.Q)
    rng = np.random.default_rng(seed)
    dt = np.where(rng.random(B) < 0.5, eps, -eps)
    u = rng.random(B)
    accepted = []
    for c in range(B):
        r = oracle_static_transition(osys_of[c], gc["q"][c], gc["x_obs"][c], 0, c, seed, 1, None, dt[c], n_step, u[c],
                                     dict(TRANSITION_SOLVER))
        bad = admissible(r["margins"])
        if bad:
            problems.append(("static", c, bad))
            continue
        outcome = res["chain_outcomes"][c]
        want_col = 1 + min(max(r["status"], 1), 3) if r["status"] > 0 else (0 if r["accepted"] else 1)
        assert outcome[want_col] == 1 and outcome.sum() == 1, (c, outcome, r["status"], r["accepted"])
        if r["accepted"]:
            e_q = np.abs(res["heads"][0, c] - r["q"]).max() / max(1.0, np.abs(r["q"]).max())
            assert e_q <= 1e-9 * n_step, (c, e_q)
            worst["position"] = max(worst["position"], e_q / n_step)
        else:
            assert np.array_equal(res["heads"][0, c], gc["q"][c]), c
        accepted.append(r["accepted"])
    ctx.close()
    if screening:
        return problems, leaves, accepted
    assert not problems, f"the oracle's own decision margins (screening): {problems}"
    assert max(leaves) >= 3 and any(accepted), (leaves, accepted)  # (trees that grew, trajectories that were accepted)
    return dict(worst, leaves=leaves, accepted=accepted)
