"""GPU: SIR initial states from the seed alone.  The keyed normal fill against the NumPy restatement and against the momentum
stream; objective and Adam step of the device-resident finder independent of row and batch (the scan guess included); the
keyed finder as one context of 12 chains, as 5 + 7 and as 12 x 1; max_parallel_tries 1 against 16; another seed; the legacy
rng= call.  Every comparison between contexts is bitwise.

Window of global chains: streams 0-11 at every shape (the last entry of SHAPES).  The device loop restarts chains of that
window at all three shapes, so it did not have to move.  Observed tries of chains 0-11 on an MI355X, device-resident loop:
    14 counts, S = 8,  sigma = 1                 1 1 1 1 1 1 1 2 1 1 1 1
    14 counts, S = 80, sigma = 1                 1 1 2 1 2 1 1 2 1 1 1 1   (time-parallel scan)
    6 counts,  S = 8,  sigma = generate_σ_y(u)   2 1 2 1 2 1 1 1 1 1 1 2
(the first two equal the CPU host loop's, tabulated in test_keyed_init.py).  In the 12-chain context fresh tries ran in
rows of other chains at every shape, e.g. S = 8: the winning try 1 of chain 7 in row 4; S = 80: try 1 of chain 1 in row 0, tries
2 .. 12 of chain 2 in rows 0, 10, 4, 6, ... (speculative: the winners, tries 1 of chains 2, 4 and 7, got their own rows back);
variable sigma: the winning tries 1 of chains 0, 2, 4, 11 in rows 3, 10, 1, 5.  The test reads that from the returned status maps."""
import numpy as np
import pytest
from test_keyed_init import SEED, HI, COUNTS6, COUNTS14, check_fill, sir_ctx

pytestmark = pytest.mark.gpu
FINDER = dict(adam_step_size=0.1, max_iters=3000, threshold=1.0, device_resident=True)
SOLVER = dict(newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8)
# shape -> (counts, S, sigma, first global chain of the twelve)
SHAPES = {
    "sir14_s8": (COUNTS14, 8, 1.0, 0),
    "sir14_s80": (COUNTS14, 80, 1.0, 0),
    "sir6_s8_varsigma": (COUNTS6, 8, "variable", 0),
}


def dev_buf(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t


def test_fill_normal_device_against_the_restatement_the_host_twin_and_the_momentum_stream():
    """chmc_fill_normal_device as in the CPU test (odd / even n_cols, ld > n_cols, padding and unlisted rows untouched, high
    bit, n_rows = 0, two rows / two contexts with one key: identical bits; 1e-12 absolute against NumPy, see check_fill); the
    host-pointer twin gives the same bits; and filling row c with (stream = c + off, draw = d) is the momentum refresh's
    unprojected draw: the library gives no access to KNormalFill's output before the projection, so the filled rows are set as
    momenta and projected by the same call sequence chmc_sample_momentum runs after its fill -- the projected momenta must be
    bitwise those of sample_momentum(seed, d, off)."""
    import torch

    def fill(ctx, rows, stream, draw, n_cols, ld):
        buf = dev_buf(np.full((ctx.B, ld), 7.5))
        ctx.fill_normal_device(SEED, rows, stream, draw, n_cols, buf.data_ptr(), ld)
        out = buf.cpu().numpy()
        host = np.full((ctx.B, ld), 7.5)
        ctx.fill_normal(SEED, rows, stream, draw, host[:, :n_cols])
        assert np.array_equal(out, host)
        return out
    check_fill(lambda B: sir_ctx(COUNTS6, 2, B), fill)
    from helpers import make_case, make_ctx
    for case in (make_case("fhn", 12, 10, 5, True, B=3, seed=32), make_case("sir", 5, 3, None, True, B=3, seed=33)):  # Q even, odd
        ctx = make_ctx(case)
        d, off = 3, 5
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        ctx.sample_momentum(SEED, d, off)
        p_ref = ctx.get_state()[1]
        pb = torch.zeros((3, ctx.Q), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.fill_normal_device(SEED, [2, 0, 1], [2 + off, off, 1 + off], d, ctx.Q, pb.data_ptr())
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        ctx.set_momentum_device(pb.data_ptr())
        ctx.project_onto_cotangent_space()
        assert np.array_equal(ctx.get_state()[1], p_ref) and np.abs(p_ref).max() > 0.5
        ctx.close()


ROWS = {2: [1, 0], 5: [4, 2, 0, 1, 3], 12: [7, 3, 11, 0, 5, 9, 1, 10, 2, 8, 6, 4]}   # point i of a context sits in row ROWS[B][i]


@pytest.mark.parametrize("S,sigma", [(8, 1.0), (80, 1.0), (5, 1.0), (80, "variable")])
def test_objective_and_adam_step_do_not_depend_on_row_or_batch(S, sigma):
    """The same points at different rows of contexts of 2, 5 and 12 chains (14 boarding-school counts; S = 8: hand-scheduled
    scan, 80: time-parallel scan, 5: functor): out3, gradient and the updated (u_v, m, v) of chmc_adam_objective_device /
    chmc_adam_update_device are bitwise equal, at a first evaluation (cold guess) and at a second one after the Adam step
    (guess: the row's own previous trajectory).  Then the rows are dealt new tries with chmc_adam_begin_tries_device, at
    OTHER rows than in a fresh context of 5, over the content the previous evaluations left there: one evaluation, equal bits
    (S = 80: the carried guess of the time-parallel scan is what is being reset)."""
    rng = np.random.default_rng(17)
    T = len(COUNTS14)
    ctxs = {B: sir_ctx(COUNTS14, S, B, sigma) for B in (2, 5, 12)}
    nuv = ctxs[2].Q - T
    pts = 0.5 * rng.standard_normal((12, nuv))
    m0, v0 = rng.standard_normal((12, nuv)), rng.random((12, nuv))
    tt = rng.integers(1, 40, 12).astype(float)
    coef = np.stack([1.0 / (1 - 0.999 ** tt), 0.1 / (1 - 0.9 ** tt)], 1)
    res = {}
    for B, ctx in ctxs.items():
        rows = np.asarray(ROWS[B])
        def place(a):
            out = np.zeros((B,) + a.shape[1:])
            out[rows] = a[:B]
            return out
        u, m, v = dev_buf(place(pts)), dev_buf(place(m0)), dev_buf(place(v0))
        g = dev_buf(np.zeros((B, nuv)))
        st1 = ctx.adam_objective_device(u.data_ptr(), g.data_ptr())
        g1 = g.cpu().numpy()
        ctx.adam_update_device(u.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), place(coef))
        upd = [t.cpu().numpy() for t in (u, m, v)]
        st2 = ctx.adam_objective_device(u.data_ptr(), g.data_ptr())
        g2 = g.cpu().numpy()
        res[B] = [a[rows] for a in (st1, g1, *upd, st2, g2)]
        # new tries over this content: try i + 1 of global chain 20 + i into the row of point B - 1 - i
        rr = rows[::-1]
        ctx.adam_begin_tries_device(SEED, rr, 20 + np.arange(B), np.uint64(HI) | (1 + np.arange(B)).astype(np.uint64),
                                    u.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr())
        assert not m.any() and not v.any() and not g.any()
        st3 = ctx.adam_objective_device(u.data_ptr(), g.data_ptr())
        res[B] += [a[rr] for a in (u.cpu().numpy(), st3, g.cpu().numpy())]
    ok = np.isfinite(res[12][0][:, 0]) & (res[12][0][:, 2] == 1.0)
    assert ok[:2].all() and ok.sum() >= 9, ok                     # (the comparison is of points the model can integrate)
    for B in (2, 5):
        for k, (a, b) in enumerate(zip(res[B], res[12])):
            assert np.array_equal(a, b[:B], equal_nan=True), (B, k, np.abs(a - b[:B]).max())
    # a context that has evaluated nothing before: the same try in row 0
    fresh = sir_ctx(COUNTS14, S, 5, sigma)
    bufs = [dev_buf(np.full((5, nuv), 3.0)) for _ in range(4)]
    fresh.adam_begin_tries_device(SEED, [0], [20], [HI | 1], *(b.data_ptr() for b in bufs))
    st = fresh.adam_objective_device(bufs[0].data_ptr(), bufs[3].data_ptr())
    assert np.array_equal(st[0], res[12][8][0]) and np.array_equal(bufs[3].cpu().numpy()[0], res[12][9][0])
    assert np.array_equal(bufs[0].cpu().numpy()[0], res[12][7][0]) and (bufs[1].cpu().numpy()[1:] == 3.0).all()
    if S == 80:  # the time-parallel scan did run (histogram of sweeps to convergence)
        assert ctxs[12].diagnostics()["par_scan"][1:64].sum() > 0
    for c in list(ctxs.values()) + [fresh]:
        c.close()


def keyed_run(name, off, cnt, seed=SEED, **kw):
    from manifold_mcmc_for_diffusions_amd import init
    counts, S, sigma, w0 = SHAPES[name]
    ctx = sir_ctx(counts, S, cnt, sigma)
    q, xo, tries, status = init.find_initial_states_by_gradient_descent_noisy_system(
        ctx, seed=seed, chain_offset=w0 + off, total_chains=w0 + 12, return_status=True, **{**FINDER, **kw})
    sig = np.exp(q[:, ctx.U - 1]) if sigma == "variable" else 1.0
    assert (np.mean(q[:, -len(counts):] ** 2, 1) < 1.0).all() and np.abs(ctx.constr()).max() < 1e-9 * max(1.0, np.max(sig))
    return ctx, q, xo, tries, status


def steps_after(ctx, off, w0):
    """sample_momentum(seed, 1, offset) and three leapfrog steps, step sizes and solver settings of
    test_hip_parity.py::test_results_do_not_depend_on_the_shard_size (by global chain)."""
    g = off + np.arange(ctx.B)
    dts = (np.where(np.arange(12) % 2 == 0, 1.0, -1.0) * (0.1 + 0.2 * np.random.default_rng(31).random(12)))[g]
    ctx.sample_momentum(SEED, 1, w0 + off)
    res = [ctx.leapfrog_step(dts, **SOLVER) for _ in range(3)]
    q, p, _, _ = ctx.get_state()
    out = [q, p]
    for r in res:
        out += [r["status"], r["iters_fwd"], r["iters_bwd"]]
    return out


@pytest.fixture(scope="module")
def whole():
    """The 12-chain run of every shape, computed once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            ctx, q, xo, tries, status = keyed_run(name, 0, 12)
            after = steps_after(ctx, 0, SHAPES[name][3])
            ctx.close()
            cache[name] = (q, xo, tries, status, after)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_keyed_finder_does_not_depend_on_the_sharding(whole, name):
    """Chains WINDOW .. WINDOW + 11 through the device-resident keyed finder as one context, as 5 + 7 and as 12 x 1: q,
    x_obs_seq and tries bitwise equal, and so are positions, momenta, statuses and iteration counts after a momentum
    refresh and three leapfrog steps."""
    w0 = SHAPES[name][3]
    q, xo, tries, status, after = whole(name)
    print(name, "tries", tries.tolist(), "rows by try", [dict(s) for s in status])
    assert tries.max() <= 40 and (tries >= 2).any(), tries
    # a fresh try ran in a row other than its chain's own
    assert any(k > 0 and r >= 0 and r != c for c, st in enumerate(status) for k, r in st.items()), status
    assert (after[2] == 0).sum() >= 6                             # the steps compared are of moving chains
    for shards in ([(0, 5), (5, 7)], [(c, 1) for c in range(12)]):
        for off, cnt in shards:
            ctx, q1, xo1, tries1, _ = keyed_run(name, off, cnt)
            sl = slice(off, off + cnt)
            assert np.array_equal(tries1, tries[sl]), (off, cnt, tries1, tries[sl])
            assert np.array_equal(q1, q[sl]) and np.array_equal(xo1, xo[sl]), (off, cnt)
            for k, (a, b) in enumerate(zip(steps_after(ctx, off, w0), after)):
                assert np.array_equal(a, b[sl]), (off, cnt, k)
            ctx.close()


def test_max_parallel_tries_1_equals_16(whole):
    q, xo, tries = whole("sir14_s80")[:3]
    for mpt in (1, 16):
        ctx, q1, xo1, tries1, _ = keyed_run("sir14_s80", 0, 12, max_parallel_tries=mpt)
        ctx.close()
        assert np.array_equal(tries1, tries) and np.array_equal(q1, q) and np.array_equal(xo1, xo), mpt


def test_another_seed_gives_other_states_and_the_legacy_call_still_works(whole):
    from manifold_mcmc_for_diffusions_amd import init
    q = whole("sir14_s8")[0]
    ctx, q1, _, tries1, _ = keyed_run("sir14_s8", 0, 12, seed=SEED + 1)
    assert not (q1[:, :5] == q[:, :5]).any() and tries1.max() <= 40
    T = ctx.T
    for resident in (True, False):   # the assertions of test_adam_finder_objective_gradient_and_device_loop_against_the_oracle
        q2, _, tries2 = init.find_initial_states_by_gradient_descent_noisy_system(
            ctx, np.random.default_rng(11), adam_step_size=0.1, max_iters=3000, device_resident=resident)
        assert (np.mean(q2[:, -T:] ** 2, 1) < 1.0).all() and np.abs(ctx.constr()).max() < 1e-9
        assert (tries2 >= 1).all() and tries2.max() <= 40
    ctx.close()
