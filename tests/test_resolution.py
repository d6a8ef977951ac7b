"""Carrying chains between time resolutions (chmc_resample_q_device, chmc_set_state_solve_noise_device, resolution.py), on
the CPU through the TEST-ONLY emulation build.  The map is held against a NumPy restatement written here from the formulas
of include/chmc.h (xi is fetched with chmc_fill_normal under the same keys), against its exact identities, against the
scheme's Brownian increments recomputed from the fine normals, and against the prior it must preserve; the placed states
are judged by the constraint, the oracle's path and chmc_set_state.  The check functions are shared with the GPU tests
(test_hip_resolution.py)."""
import ctypes as C
import numpy as np
import pytest
from test_emu_logic import emu_lib  # noqa: F401
from manifold_mcmc_for_diffusions_amd import example_models as em

RESAMPLE_DRAW = 1 << 60  # CHMC_RESAMPLE_DRAW (include/chmc.h)
SEED = 20240607          # every keyed draw of this file; test_prior_is_preserved passes its NumPy restatement with it
TOL = 1e-13
DT = {"fhn": 0.2, "fhn_nb": 0.2, "sir": 0.25}
NPAIR = {"fhn": 1, "fhn_nb": 1, "sir": 0}  # strong-order-1.5 pairs (a, b) = (v[j], v[NPAIR + j]); the rest are singles

# (model, T, S_c, m, sigma): FHN T = 3, S_c = 1, 2, 5 by m = 2, 3, 8, 65 (T S_dst = 6 .. 975, most no multiple of 64; m = 65
# is past a wavefront and prime to it); SIR T = 2, S_c = 3; variable noise; no observation noise; more than one tile per chain
# at small m (150 and 300 coarse steps); m past a workgroup (300)
SHAPES = [("fhn", 3, sc, m, 0.1) for sc in (1, 2, 5) for m in (2, 3, 8, 65)]
SHAPES += [("sir", 2, 3, 2, 1.0), ("sir", 2, 3, 7, 1.0), ("fhn", 3, 2, 3, "variable"), ("fhn", 3, 2, 3, None),
           ("fhn_nb", 3, 2, 5, 0.1), ("fhn", 3, 50, 2, 0.1), ("fhn", 3, 100, 2, 0.1), ("fhn", 2, 1, 300, 0.1),
           ("sir", 2, 1, 300, 1.0)]


def shape_id(s):
    return f"{s[0]}-T{s[1]}-S{s[2]}-m{s[3]}-{'noiseless' if s[4] is None else s[4]}"


def make_ctx(model, T, S, sigma, B, R=None):
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    if R is None and model != "sir":
        R = 2 if T > 3 else None
    return ChmcContext(model, DT[model], S, R, np.zeros(T), sigma=sigma, num_chains=B)


class Dev:
    """A [B, n] array where the library's kernels reach it: a torch-ROCm tensor, or host memory under the emulation."""

    def __init__(self, ctx, arr):
        self.hip = ctx.L.chmc_backend() == b"hip:gfx950"
        arr = np.array(arr, dtype=np.float64, order="C")
        if self.hip:
            import torch
            self.t = torch.from_numpy(arr).to(torch.device("cuda", ctx.device))
            torch.cuda.synchronize()
            self.ptr = self.t.data_ptr()
        else:
            self.t = arr
            self.ptr = arr.ctypes.data

    def get(self):
        return self.t.cpu().numpy() if self.hip else self.t.copy()


def rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


# ---- the NumPy restatement
def a_matrix(model, m):
    """A [V, m, V]: row i (a coarse normal) over the fine normals (k, i') of the coarse step."""
    V, NP = em.MODELS[model].dim_v, NPAIR[model]
    A = np.zeros((V, m, V))
    k = np.arange(m)
    for j in range(NP):
        A[j, :, j] = m ** -0.5
        A[NP + j, :, j] = m ** -1.5 * np.sqrt(3.0) * (m - 1 - 2 * k)
        A[NP + j, :, NP + j] = m ** -1.5
    for i in range(2 * NP, V):
        A[i, :, i] = m ** -0.5
    return A


def split(ctx_like, q, S):
    """(head [B, U + V0], v [B, T S, V], n [B, T or 0]) of positions with S steps per interval."""
    h = ctx_like.U + ctx_like.V0
    nv = ctx_like.T * S * ctx_like.V
    return q[:, :h], q[:, h:h + nv].reshape(len(q), ctx_like.T * S, ctx_like.V), q[:, h + nv:]


def np_coarsen(model, w, m):
    """v = A w for w [B, NS m, V]."""
    B, n, V = w.shape
    return np.einsum("ikj,bskj->bsi", a_matrix(model, m), w.reshape(B, n // m, m, V))


def np_refine(model, v, xi, m):
    """w = xi + A^T (v - A xi) for v [B, NS, V], xi [B, NS m, V]."""
    B, NS, V = v.shape
    r = v - np_coarsen(model, xi, m)
    return xi + np.einsum("ikj,bsi->bskj", a_matrix(model, m), r).reshape(B, NS * m, V)


def xi_rows(ctx, seed, draw, offset):
    """The keyed rows chmc_resample_q_device takes its fresh normals from, [B, Q] of the destination context."""
    return ctx.fill_normal(seed, np.arange(ctx.B), offset + np.arange(ctx.B), np.uint64(RESAMPLE_DRAW | draw),
                           np.zeros((ctx.B, ctx.Q)))


def brownian_increments(model, v, delta):
    """(dW, dZ) [B, n, pairs or singles] of the steps of length delta from their normals v [B, n, V]: dW = sqrt(delta) a for
    every Wiener dimension, dZ = delta^3/2 (a + b / sqrt 3) / 2 for the pairs (tools/gen_models.py)."""
    NP, V = NPAIR[model], v.shape[2]
    a = np.concatenate([v[..., :NP], v[..., 2 * NP:]], -1)
    dW = np.sqrt(delta) * a
    dZ = delta ** 1.5 * (v[..., :NP] + v[..., NP:2 * NP] / np.sqrt(3.0)) / 2
    return dW, dZ


def check_map(shape, B=3, offset=5, draw=3):
    """Cases 1-3 of the issue on one shape: refinement and coarsening against the restatement, the identities, the copy, the
    masked row, and the Brownian increments of the coarse steps recomputed from the fine normals.  Returns the figures."""
    model, T, Sc, m, sigma = shape
    rng = np.random.default_rng(7)
    fine, coarse = make_ctx(model, T, Sc * m, sigma, B), make_ctx(model, T, Sc, sigma, B)
    V, NP = fine.V, NPAIR[model]
    assert fine.Q - coarse.Q == T * Sc * (m - 1) * V
    q_c = rng.standard_normal((B, coarse.Q))
    mask = np.array([1, 0, 1] + [1] * (B - 3), dtype=np.int32)
    on = mask == 1
    out = {}
    # refinement
    xi = split(fine, xi_rows(fine, SEED, draw, offset), fine.S)[1]
    src, dst = Dev(fine, q_c), Dev(fine, np.full((B, fine.Q), 7.5))
    fine.resample_q_device(src.ptr, Sc, SEED, dst.ptr, draw=draw, chain_offset=offset, mask=mask)
    q_f = dst.get()
    assert (q_f[~on] == 7.5).all()  # the masked chain's row is bitwise untouched
    assert np.array_equal(src.get(), q_c)
    head_c, v_c, n_c = split(coarse, q_c, Sc)
    head_f, w, n_f = split(fine, q_f, fine.S)
    assert np.array_equal(head_f[on], head_c[on]) and np.array_equal(n_f[on], n_c[on])  # u, v_0 and n: bit for bit
    out["refine"] = rel(w[on], np_refine(model, v_c, xi, m)[on])
    # the identities: A w = v, w - A^T v = (I - A^T A) xi
    A = a_matrix(model, m)
    out["A_At"] = float(np.abs(np.einsum("ikj,lkj->il", A, A) - np.eye(V)).max())
    out["A_w"] = rel(np_coarsen(model, w[on], m), v_c[on])
    at = lambda r: np.einsum("ikj,bsi->bskj", A, r).reshape(len(r), -1, V)  # noqa: E731
    out["complement"] = rel(w[on] - at(v_c[on]), xi[on] - at(np_coarsen(model, xi[on], m)))
    # the Brownian path is the same one: coarse increments from the sums of the fine ones
    delta, h = DT[model] / Sc, DT[model] / (Sc * m)
    dW_c, dZ_c = brownian_increments(model, v_c[on], delta)
    dW_f, dZ_f = brownian_increments(model, w[on], h)
    dW_f = dW_f.reshape(on.sum(), T * Sc, m, -1)
    out["dW"] = rel(dW_f.sum(2), dW_c) / np.sqrt(delta)
    if NP:
        W_before = np.cumsum(dW_f[..., :NP], 2) - dW_f[..., :NP]  # W(t_k) - W(t_0)
        dZ_sum = (dZ_f.reshape(on.sum(), T * Sc, m, NP) + h * W_before).sum(2)
        out["dZ"] = rel(dZ_sum, dZ_c) / delta ** 1.5
    # coarsening, and coarsen(refine(v)) = v
    q_f[~on] = rng.standard_normal((int((~on).sum()), fine.Q))
    src, dst = Dev(coarse, q_f), Dev(coarse, np.full((B, coarse.Q), 7.5))
    coarse.resample_q_device(src.ptr, fine.S, 0, dst.ptr, mask=mask)
    back = dst.get()
    assert (back[~on] == 7.5).all()
    hb, vb, nb = split(coarse, back, Sc)
    assert np.array_equal(hb[on], head_c[on]) and np.array_equal(nb[on], n_c[on])
    out["coarsen"] = rel(vb[on], np_coarsen(model, split(fine, q_f, fine.S)[1], m)[on])
    out["round_trip"] = rel(vb[on], v_c[on])
    # S_src = S_dst: a bitwise copy of the rows asked for
    src, dst = Dev(fine, q_f), Dev(fine, np.full((B, fine.Q), 7.5))
    fine.resample_q_device(src.ptr, fine.S, SEED, dst.ptr, mask=mask)
    same = dst.get()
    assert np.array_equal(same[on], q_f[on]) and (same[~on] == 7.5).all()
    fine.close(), coarse.close()
    print(shape_id(shape), {k: f"{v:.1e}" for k, v in out.items()})
    assert max(out.values()) <= TOL, out
    return q_f[on], out


def prior_sample(B=64, T=3, Sc=5, m=4):
    """(w [B, T Sc, m V], v_c, xi): B rows of N(0, I) (keyed draws under another key) refined by m."""
    fine, coarse = make_ctx("fhn", T, Sc * m, 0.1, B), make_ctx("fhn", T, Sc, 0.1, B)
    q_c = coarse.fill_normal(SEED, np.arange(B), np.arange(B), np.uint64(1 << 62), np.zeros((B, coarse.Q)))
    src, dst = Dev(fine, q_c), Dev(fine, np.zeros((B, fine.Q)))
    fine.resample_q_device(src.ptr, Sc, SEED, dst.ptr)
    xi = split(fine, xi_rows(fine, SEED, 0, 0), fine.S)[1]
    w = split(fine, dst.get(), fine.S)[1]
    v_c = split(coarse, q_c, Sc)[1]
    fine.close(), coarse.close()
    return w.reshape(B, T * Sc, m * fine.V), v_c, xi


def check_prior(w):
    """Every one of the m V positions within a coarse step: sample variance 1 and pairwise sample correlations 0 over the
    n = B T Sc coarse steps, each within 5 standard errors (of a variance of normals: sqrt(2 / (n - 1)); of a correlation of
    independent normals: 1 / sqrt(n)); the mean within 5 / sqrt(n)."""
    x = w.reshape(-1, w.shape[2])
    n = len(x)
    var, corr = x.var(0, ddof=1), np.corrcoef(x.T)
    off = corr[~np.eye(x.shape[1], dtype=bool)]
    figures = dict(n=n, var=float(np.abs(var - 1).max() / np.sqrt(2.0 / (n - 1))), corr=float(np.abs(off).max() * np.sqrt(n)),
                   mean=float(np.abs(x.mean(0)).max() * np.sqrt(n)))
    print("prior preservation, in standard errors:", figures)
    assert figures["var"] <= 5 and figures["corr"] <= 5 and figures["mean"] <= 5, figures
    return figures


MANIFOLD = [("fhn", 6, 5, 2, 0), ("fhn", 6, 5, 2, 1), ("sir", 4, 4, None, 0)]  # (model, T, S_c, R, partition)


def state_ops(ctx):
    q, p, xo, part = ctx.get_state()
    cC, cD = ctx.chol_gram_blocks()
    return dict(q=q, p=p, xo=xo, part=np.array(part), constr=ctx.constr(), ham=ctx.hamiltonian(), ld=ctx.log_det_sqrt_gram(),
                gld=ctx.grad_log_det_sqrt_gram(), cC=cC, cD=cD)


def check_on_the_manifold(model, T, Sc, R, part, m, B=3):
    """Case 5: a state on the coarse manifold (simulate_observations) carried to m times the resolution."""
    from manifold_mcmc_for_diffusions_amd.resolution import transfer_state
    from test_paths import path_by_models
    sigma = 1.0 if model == "sir" else 0.1
    coarse = make_ctx(model, T, Sc, sigma, B, R=R)
    coarse.simulate_observations(SEED, partition=part)
    fine = coarse.sibling(Sc * m)
    y, sg = coarse.observations()
    yf, sgf = fine.observations()
    assert np.array_equal(y, yf) and np.array_equal(sg, sgf) and y.any()
    q_c = coarse.get_state()[0]
    tr = transfer_state(coarse, fine, SEED, draw=9)
    st = state_ops(fine)
    assert st["part"] == part and not st["p"].any()
    out = dict(max_constr=tr["max_constr"], constr=float(np.abs(st["constr"]).max()))
    assert tr["max_constr"] < 1e-9 and out["constr"] < 1e-9, out
    # v_seq is the refinement of the coarse one, u and v_0 are the coarse ones
    hf, w, n_new = split(fine, st["q"], fine.S)
    hc, v_c, n_old = split(coarse, q_c, Sc)
    assert np.array_equal(hf, hc)
    assert rel(np_coarsen(model, w, m), v_c) <= TOL
    # moved, from the oracle's path of the refined position
    path = path_by_models(model, st["q"], T, fine.S, DT[model], fine.U)[:, fine.S::fine.S]
    n_ref = (y - em.MODELS[model].obs_func(path)[..., 0]) / sg[:, None]
    out["moved"] = float(np.abs(tr["moved"] - np.abs(n_ref - n_old).max(1)).max())
    out["n"] = float(np.abs(n_new - n_ref).max())
    out["moved_max"] = float(tr["moved"].max())
    assert out["moved"] <= 1e-10 and out["n"] <= 1e-10, out
    # bitwise the state chmc_set_state gives for what chmc_get_state returns
    fine.set_state(st["q"], None, st["xo"], part)
    again = state_ops(fine)
    for k in st:
        assert np.array_equal(st[k], again[k]), k
    r = fine.leapfrog_step(0.02)
    assert (r["status"] == 0).all(), r
    fine.close(), coarse.close()
    print(model, T, Sc, R, part, m, {k: f"{v:.1e}" for k, v in out.items()})
    return out


def check_noiseless_is_refused():
    coarse = make_ctx("fhn", 4, 2, None, 2, R=2)
    q = Dev(coarse, np.zeros((2, coarse.Q)))
    with pytest.raises(RuntimeError, match="not supported"):
        coarse.set_state_solve_noise(q.ptr, 0)
    coarse.close()


def check_shards(model="fhn", T=3, Sc=2, m=3, sigma=0.1):
    """Case 6: 6 chains in one context against 2 x 3 with chain_offset."""
    rng = np.random.default_rng(3)
    whole = make_ctx(model, T, Sc * m, sigma, 6)
    q_c = rng.standard_normal((6, whole.Q - T * Sc * (m - 1) * whole.V))
    src, dst = Dev(whole, q_c), Dev(whole, np.zeros((6, whole.Q)))
    whole.resample_q_device(src.ptr, Sc, SEED, dst.ptr, draw=2, chain_offset=10)
    ref = dst.get()
    whole.close()
    for lo in (0, 3):
        part = make_ctx(model, T, Sc * m, sigma, 3)
        src, dst = Dev(part, q_c[lo:lo + 3]), Dev(part, np.zeros((3, part.Q)))
        part.resample_q_device(src.ptr, Sc, SEED, dst.ptr, draw=2, chain_offset=10 + lo)
        assert np.array_equal(dst.get(), ref[lo:lo + 3])
        part.close()
    other = make_ctx(model, T, Sc * m, sigma, 3)
    src, dst = Dev(other, q_c[:3]), Dev(other, np.zeros((3, other.Q)))
    other.resample_q_device(src.ptr, Sc, SEED, dst.ptr, draw=3, chain_offset=10)
    assert not np.array_equal(dst.get(), ref[:3])  # another draw, other normals
    other.close()


def check_errors():
    ctx = make_ctx("fhn", 3, 6, 0.1, 2)
    src, dst = Dev(ctx, np.zeros((2, ctx.Q))), Dev(ctx, np.zeros((2, ctx.Q)))
    for kw, text in ((dict(S_src=0), "S_src"), (dict(S_src=4), "integer ratio"), (dict(S_src=9), "integer ratio"),
                     (dict(S_src=3, draw=1 << 45), "2\\^45"), (dict(S_src=3, chain_offset=-1), "chain_offset")):
        args = dict(S_src=3, draw=0, chain_offset=0)
        args.update(kw)
        with pytest.raises(RuntimeError, match=text):
            ctx.resample_q_device(src.ptr, args["S_src"], SEED, dst.ptr, draw=args["draw"], chain_offset=args["chain_offset"])
    for s, d in ((0, dst.ptr), (src.ptr, 0)):
        with pytest.raises(RuntimeError, match="null"):
            ctx.resample_q_device(s, 3, SEED, d)
    assert ctx.L.chmc_resample_q_device(None, C.c_void_p(src.ptr), 3, SEED, 0, 0, None, C.c_void_p(dst.ptr)) != 0
    with pytest.raises(RuntimeError, match="null"):
        ctx.set_state_solve_noise(0, 0)
    with pytest.raises(RuntimeError, match="partition"):
        ctx.set_state_solve_noise(src.ptr, 5)
    ctx.resample_q_device(src.ptr, 3, SEED, dst.ptr, draw=(1 << 45) - 1)  # the largest draw
    ctx.close()


# ---- the tests
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_map_against_the_numpy_restatement_and_its_identities(emu_lib, shape):  # noqa: F811
    check_map(shape)


def test_prior_is_preserved(emu_lib):  # noqa: F811
    w, v_c, xi = prior_sample()
    check_prior(np_refine("fhn", v_c, xi, 4).reshape(w.shape))  # the restatement itself passes with SEED
    check_prior(w)


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("model,T,Sc,R,part", MANIFOLD)
def test_transferred_state_is_on_the_fine_manifold(emu_lib, model, T, Sc, R, part, m):  # noqa: F811
    check_on_the_manifold(model, T, Sc, R, part, m)


def test_noiseless_context_is_refused(emu_lib):  # noqa: F811
    check_noiseless_is_refused()


def test_shard_independence(emu_lib):  # noqa: F811
    check_shards()
    check_shards("sir", 2, 3, 7, 1.0)


def test_errors(emu_lib):  # noqa: F811
    check_errors()


def test_coarse_to_fine_driver(emu_lib):  # noqa: F811
    """Case 8: S = 2 -> 4 -> 8, FHN T = 4, B = 4, a handful of transitions."""
    from manifold_mcmc_for_diffusions_amd.resolution import coarse_to_fine_static_chmc
    coarse = make_ctx("fhn", 4, 2, 0.1, 4, R=2)
    coarse.simulate_observations(SEED)
    rng = np.random.default_rng(5)
    G = rng.standard_normal((4, coarse.U, coarse.U))
    coarse.set_metric(np.einsum("bij,bkj->bik", G, G) + 2 * np.eye(coarse.U))  # a matrix per chain
    ladder = [coarse.sibling(4), coarse.sibling(8)]
    out = coarse_to_fine_static_chmc(coarse, ladder, n_warm_coarse=4, n_warm_fine=2, n_main=3, n_step=2, step_size=0.05,
                                     seed=SEED)
    rungs = out["rungs"]
    assert [r["S"] for r in rungs] == [2, 4, 8] and len(out["accept_stat"]) == 5 and out["heads"].shape[:2] == (5, 4)
    for prev, r in zip(rungs, rungs[1:]):
        assert r["first_step_size"] == prev["final_step_size"]          # the step sizes are handed on
        assert r["moved"].shape == (4,) and np.isfinite(r["moved"]).all() and r["max_constr"] < 1e-9
    assert rungs[0]["moved"] is None and rungs[0]["first_step_size"] == 0.05
    assert out["final_step_size"] == rungs[-1]["final_step_size"] and out["step_size"][0] == rungs[1]["final_step_size"]
    for r in rungs:
        assert r["seconds"] > 0 and 0 <= r["mean_accept_stat"] <= 1
    for ctx in ladder:
        assert ctx.per_chain_metric and np.array_equal(ctx.metrics(), coarse.metrics())      # the metric arrives
        assert all(np.array_equal(a, b) for a, b in zip(ctx.observations(), coarse.observations()))  # and the data
        assert np.abs(ctx.constr()).max() < 1e-8
    # a shared M_0 and no metric are carried too
    coarse.set_metric(np.diag([1.0, 2.0, 3.0, 4.0]))
    sib = coarse.sibling(6)
    assert not sib.per_chain_metric and np.array_equal(sib.metrics(), coarse.metrics())
    coarse.set_metric(None)
    sib2 = coarse.sibling(6)
    assert sib2.M_0 is None
    for c in ladder + [sib, sib2, coarse]:
        c.close()
