"""The library judged by the AUTODIFF oracle (oracle/py: hand-written models, constraint differentiated by torch.func,
dense LAPACK algebra) -- the one checker that shares no generated model code and no adjoint / tangent sweep with the
device code.  Mirrors helpers.check_ops_against_oracle / check_steps_against_oracle.

The oracle is slow, so its jobs run in worker processes: SPAWNED (never forked from a process that has opened the GPU),
at most 12, sharing 16 CPUs through torch.set_num_threads.  A worker imports oracle.py only, never the library: this
module therefore imports nothing of the package at its top level (a spawned worker re-imports it), and jobs are plain
dicts of arrays and settings.  Submit the jobs, run the library, then collect.

Tolerances are those tests/test_golden.py uses for the same comparison (library vs autodiff): operators 1e-9 relative
(inf-norm, scale max(1, |ref|)), after one step q 1e-9, p 1e-8, Hamiltonian 1e-9; statuses and iteration counts equal."""
import atexit
import multiprocessing
import os
import numpy as np

MAX_WORKERS = 12
CPUS = 16
OP_TOL, Q_TOL, P_TOL, H_TOL = 1e-9, 1e-9, 1e-8, 1e-9
TOLS = dict(constraint_tol=1e-9, position_tol=1e-8, max_iters=50)
_POOL = None


# ---------------------------------------------------------------------------------------------------------------------
# worker side (imports oracle.py only)

def _worker_init(n_threads):
    import torch
    torch.set_num_threads(n_threads)


def _system(spec):
    from oracle.py import models as omodels, system as osys
    return osys, osys.make_system(omodels.MODELS[spec["model"]], spec["obs_interval"], spec["S"], spec["R"],
                                  np.asarray(spec["y"], dtype=np.float64).reshape(-1, 1), sigma=spec["sigma"],
                                  use_gaussian_splitting=spec["gaussian"], M_0=spec.get("M_0"))


def rowslot(jac, rmax, nv):
    """The oracle's block tuples in the library's layout: dc_du [dim_c, U], dc_dv one row slot per block row [rmax, NV]."""
    import torch
    du = torch.cat([b.reshape(-1, b.shape[-1]) for b in jac[0]]).numpy()
    dv = np.zeros((rmax, nv))
    col = 0
    for b in jac[1]:
        b = b.numpy()
        if b.ndim == 2:
            b = b[None]
        for m in range(b.shape[0]):
            r, nc = b[m].shape
            dv[:r, col:col + nc] = b[m]
            col += nc
    return du, dv


def chol_d_list(chol):
    """chol_D blocks in block order, each with its own size (batched middle blocks unstacked)."""
    out = []
    for ch in chol[1]:
        ch = ch.numpy()
        out += [ch] if ch.ndim == 2 else list(ch)
    return out


def ops_job(spec, q, p, x_obs, part, w, lam, want=("grad", "products")):
    """Every operator of one chain in one partition.  want: "grad" (log-det gradient, the expensive one), "products"."""
    osys, sysm = _system(spec)
    st = osys.ConditionedDiffusionHamiltonianState(q, x_obs, part, mom=p)
    out = {"c": sysm.constr(st)}
    if "grad" in want:  # one reverse sweep that also fills the Jacobian / Cholesky caches (:1173-1184)
        out["grad"] = sysm.grad_log_det_sqrt_gram(st)
    jac, chol = sysm.jacob_constr_blocks(st), sysm.chol_gram_blocks(st)
    rmax = max(int(b.shape[-2]) for b in jac[1])
    md = sysm.model_dict
    out["dc_du"], out["dc_dv"] = rowslot(jac, rmax, md["dim_v_0"] + md["num_obs"] * md["num_steps_per_obs"] * md["dim_v"])
    out["chol_C"], out["chol_D"] = chol[0].numpy(), chol_d_list(chol)
    out["log_det"] = sysm.log_det_sqrt_gram(st)
    out["Jw"] = sysm._lmult_by_jacob_constr(*jac, osys.T(w)).numpy()
    out["Ginv_lam"] = sysm._lmult_by_inv_gram(*jac, *chol, osys.T(lam)).numpy()
    if "products" in want:
        out["JTlam"] = sysm._rmult_by_jacob_constr(*jac, osys.T(lam)).numpy()
        out["nsc"] = sysm.normal_space_component(st, w)
        out["h"] = sysm.h(st)
    return out


def step_job(spec, q, p, x_obs, part, dt, newton, n_inner, project):
    """One ConstrainedLeapfrogIntegrator.step of one chain.  project: the start momentum is projected onto the cotangent
    space first (by the oracle itself).  Returns status (0 ok, otherwise the exception's name), the summed iteration
    counts of the forward / reverse retractions, the (|c|, |dq|) each solver stopped at, q, p, Hamiltonians."""
    osys, sysm = _system(spec)
    st = osys.ConditionedDiffusionHamiltonianState(q, x_obs, part, mom=p)
    if project:
        st.mom = sysm.project_onto_cotangent_space(st.mom.copy(), st)
    out = {"p0": st.mom.copy(), "h0": sysm.h(st)}
    solver = (osys.jitted_solve_projection_onto_manifold_newton if newton
              else osys.jitted_solve_projection_onto_manifold_quasi_newton)
    integ = osys.ConstrainedLeapfrogIntegrator(sysm, step_size=abs(dt), n_inner_step=n_inner, projection_solver=solver,
                                               projection_solver_kwargs=TOLS)
    st.dir = 1 if dt > 0 else -1
    try:
        s1 = integ.step(st)
    except (osys.ConvergenceError, osys.NonReversibleStepError) as e:
        out.update(status=type(e).__name__, message=str(e))
        return out
    log = integ.inner_log
    out.update(status=0, q1=s1.pos, p1=s1.mom, h1=sysm.h(s1), iters=(sum(e[0][0] for e in log), sum(e[0][1] for e in log)),
               residuals=[(e[1], e[2]) for e in log], rev=[e[3] for e in log])
    return out


def nld_job(spec, q, gaussian):
    """Value and gradient of the unconstrained comparator target (oracle/py/neg_log_dens.py) for one chain at q [U + NV]."""
    from oracle.py.neg_log_dens import neg_log_dens_and_grad
    return neg_log_dens_and_grad(spec["model"], spec["obs_interval"], spec["S"], spec["y"], spec["sigma"], q, bool(gaussian))


# ---------------------------------------------------------------------------------------------------------------------
# submitting side

def pool():
    """The shared pool of spawned oracle workers (created on first use, shut down at exit)."""
    global _POOL
    if _POOL is None:
        from concurrent.futures import ProcessPoolExecutor
        n = min(MAX_WORKERS, CPUS, os.cpu_count() or 1)
        _POOL = ProcessPoolExecutor(n, mp_context=multiprocessing.get_context("spawn"), initializer=_worker_init,
                                    initargs=(max(1, CPUS // n),))
        atexit.register(shutdown)
    return _POOL


def shutdown():
    global _POOL
    if _POOL is not None:
        _POOL.shutdown(wait=True, cancel_futures=True)
        _POOL = None


def spec_of(case, M_0=None):
    """The picklable description of a helpers.make_case case (its ctypes `osys` stays behind)."""
    return dict(model=case["model"], obs_interval=case["obs_interval"], S=case["S"], R=case["R"], y=np.array(case["y"]),
                sigma=case["sigma"], gaussian=case["gaussian"], M_0=None if M_0 is None else np.array(M_0))


def dim_c_of(case, part):
    return case["osys"].dim_c(part)


def submit_ops(case, chains, seed, M_0=None, want=("grad", "products"), parts=None, q=None, x_obs=None):
    """Jobs for every operator of the chosen chains in every partition, each chain at ITS OWN state (case["q"][c],
    off the manifold for c > 0 in a make_case case).  Returns the handle check_ops takes."""
    spec = spec_of(case, M_0)
    q = case["q"] if q is None else q
    x_obs = case["x_obs"] if x_obs is None else x_obs
    B, Q = q.shape
    rng = np.random.default_rng(seed)
    parts = range(case["osys"].num_partition) if parts is None else parts
    h = dict(case=case, chains=list(chains), q=q, x_obs=x_obs, want=tuple(want), parts={})
    for part in parts:
        p, w = rng.standard_normal((B, Q)), rng.standard_normal((B, Q))
        lam = rng.standard_normal((B, dim_c_of(case, part)))
        futs = {c: pool().submit(ops_job, spec, q[c], p[c], x_obs[c], part, w[c], lam[c], tuple(want)) for c in chains}
        h["parts"][part] = dict(p=p, w=w, lam=lam, futs=futs)
    return h


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


UNJUDGED = "unjudged_chains"  # in a `worst` dict: chains whose REFERENCE holds a non-finite entry; a count, not a distance


def distance(a, b):
    """(relative distance of a library value `a` from its reference `b`, whether every entry of `b` is finite).  Entries
    whose reference is not finite are not compared; a library entry that is not finite where the reference is gives inf
    (np.max / the builtin max would drop a NaN: max(0.0, nan) is 0.0)."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    fin = np.isfinite(b)
    if not fin.any():
        return 0.0, False
    af, bf = a[fin], b[fin]
    if not np.isfinite(af).all():
        return np.inf, bool(fin.all())
    return float(np.max(np.abs(af - bf))) / max(1.0, float(np.max(np.abs(bf)))), bool(fin.all())


def failures(worst, tol):
    """The operators of `worst` that miss `tol` (the count of unjudged chains is not a distance and not subject to it)."""
    return {k: v for k, v in worst.items() if k != UNJUDGED and not v < tol}


def largest(worst):
    """The largest operator distance of `worst`."""
    return max(v for k, v in worst.items() if k != UNJUDGED)


def library_ops(ctx, h, part):
    """What the library computes for every chain of the handle's states in one partition."""
    d = h["parts"][part]
    ctx.set_state(h["q"], d["p"], h["x_obs"], part)
    out = {"c": ctx.constr()}
    out["dc_du"], out["dc_dv"] = ctx.jacob_constr_blocks()
    out["chol_C"], out["chol_D"] = ctx.chol_gram_blocks()
    out["log_det"] = ctx.log_det_sqrt_gram()
    out["Jw"], out["Ginv_lam"] = ctx.lmult_by_jacob_constr(d["w"]), ctx.lmult_by_inv_gram(d["lam"])
    if "grad" in h["want"]:
        out["grad"] = ctx.grad_log_det_sqrt_gram()
    if "products" in h["want"]:
        out["JTlam"], out["nsc"] = ctx.rmult_by_jacob_constr(d["lam"]), ctx.normal_space_component(d["w"])
        out["h"] = ctx.hamiltonian()[:, 0]
    return out


def compare_ops(lib, ref, c, nrows, worst, show=False):
    """One chain's library results against one ops_job result; updates `worst` {operator: largest relative distance, inf
    where the library is not finite and the reference is; UNJUDGED: chains whose reference is not finite somewhere}."""
    rm = ref["dc_dv"].shape[0]
    pairs = [(k, lib[k][c], ref[k]) for k in ("c", "dc_du", "chol_C", "Jw", "Ginv_lam", "grad", "JTlam", "nsc") if k in ref]
    pairs.append(("dc_dv", lib["dc_dv"][c][:rm], ref["dc_dv"]))
    if lib["dc_dv"][c].shape[0] > rm:  # padded row slots stay zero
        pairs.append(("dc_dv_pad", lib["dc_dv"][c][rm:], np.zeros_like(lib["dc_dv"][c][rm:])))
    assert len(ref["chol_D"]) == len(nrows)
    for b, (blk, r) in enumerate(zip(ref["chol_D"], nrows)):  # every D block
        assert blk.shape == (r, r), (b, blk.shape, r)
        pairs.append(("chol_D", lib["chol_D"][c][b][:r, :r], blk))
    pairs.append(("log_det", np.array([lib["log_det"][c]]), np.array([ref["log_det"]])))
    if "h" in ref:
        pairs.append(("hamiltonian", np.array([lib["h"][c]]), np.array([ref["h"]])))
    judged = True
    for k, a, b in pairs:
        assert np.shape(a) == np.shape(b), (k, np.shape(a), np.shape(b))
        e, fin = distance(a, b)
        judged &= fin
        worst[k] = max(worst.get(k, 0.0), e)
        if show:
            print(f"    chain {c} {k}: {e:.2e}")
    worst[UNJUDGED] = worst.get(UNJUDGED, 0) + (not judged)


def check_ops(ctx, h, tol=OP_TOL, timeout=600, show=True):
    """Runs the library on the handle's states and compares with the collected oracle results."""
    worst = {}
    for part, d in h["parts"].items():
        lib = library_ops(ctx, h, part)
        nrows = [blk["nrows"] for blk in ctx.blocks[part]]
        for c, fut in d["futs"].items():
            compare_ops(lib, fut.result(timeout=timeout), c, nrows, worst)
    if show:
        print("  library vs autodiff, operators (rel):", {k: f"{v:.1e}" for k, v in worst.items()})
    bad = failures(worst, tol)
    assert not bad, f"library vs autodiff oracle (rel err): {bad}; all: {worst}"
    return worst


def submit_steps(case, q, p, x_obs, part, dts, chains, newton=True, n_inner=1, project=True, M_0=None):
    """Jobs for one integrator step of the chosen chains from (q[c], p[c]); p is the RAW momentum: with project the oracle
    projects it itself, otherwise the step starts from the unprojected momentum."""
    spec = spec_of(case, M_0)
    dts = np.broadcast_to(np.asarray(dts, dtype=np.float64), (len(q),))
    futs = {c: pool().submit(step_job, spec, q[c], p[c], x_obs[c], part, float(dts[c]), bool(newton), int(n_inner),
                             bool(project)) for c in chains}
    return dict(q=q, p=p, x_obs=x_obs, part=part, dts=dts, newton=newton, n_inner=n_inner, project=project, futs=futs)


def library_step(ctx, h):
    ctx.set_state(h["q"], h["p"], h["x_obs"], h["part"])
    if h["project"]:
        ctx.project_onto_cotangent_space()
    _, p0, _, _ = ctx.get_state()
    h0 = ctx.hamiltonian()[:, 0]
    res = ctx.leapfrog_step(h["dts"], newton=h["newton"], n_inner_step=h["n_inner"])
    q1, p1, _, _ = ctx.get_state()
    return dict(p0=p0, h0=h0, res=res, q1=q1, p1=p1, h1=ctx.hamiltonian()[:, 0])


def check_steps(ctx, h, timeout=900, show=True, what=""):
    """Runs the library's step from the handle's states and compares with the collected oracle results: status, both
    iteration counts, q, p, Hamiltonian (and the projected start momentum and its Hamiltonian)."""
    lib = library_step(ctx, h)
    worst = {}
    for c, fut in h["futs"].items():
        ref = fut.result(timeout=timeout)
        assert ref["status"] == 0, (what, c, ref)  # the inputs are chosen so that the reference step succeeds
        got = (int(lib["res"]["status"][c]), int(lib["res"]["iters_fwd"][c]), int(lib["res"]["iters_bwd"][c]))
        assert got == (0,) + tuple(ref["iters"]), (what, c, got, ref["iters"], ref["residuals"])
        for k, a, b, tol in (("p0", lib["p0"][c], ref["p0"], OP_TOL), ("h0", [lib["h0"][c]], [ref["h0"]], H_TOL),
                             ("q1", lib["q1"][c], ref["q1"], Q_TOL), ("p1", lib["p1"][c], ref["p1"], P_TOL),
                             ("h1", [lib["h1"][c]], [ref["h1"]], H_TOL)):
            e = rel(a, b)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < tol, (what, c, k, e, tol)
    if show:
        print(f"  library vs autodiff, step {what} (rel):", {k: f"{v:.1e}" for k, v in worst.items()})
    return lib, worst
