"""SIR initial states from the seed alone (keyed mode of init.find_initial_states_by_gradient_descent_noisy_system), on the CPU
through the TEST-ONLY emulation build: the keyed normal fill (chmc_fill_normal) against the NumPy restatement of the device
generator (tests/test_rng.py), the momentum refresh's bits after the generator was factored out, the host loop as one context
against two shards, the slot logic of the device loop with stand-ins, two gloo ranks, and misuse.  Comparisons within the
backend are bitwise.  The GPU tests are in test_hip_keyed_init.py."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace
import numpy as np
import pytest
from test_emu_logic import emu_lib  # noqa: F401
from test_rng import reference_normals
from test_distributed_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20200710
HI = 1 << 63
COUNTS6 = np.array([3.0, 8.0, 28.0, 75.0, 221.0, 281.0])
COUNTS14 = np.array([3.0, 8, 28, 75, 221, 281, 255, 235, 190, 125, 70, 28, 12, 5])
# (counts, S) -> tries of chains 0-11 from the keyed draws (seed 20200710, draw = 2^63 | try, streams 0-11), host loop,
# sigma = 1, adam_step_size = 0.1, max_iters = 3000, threshold = 1
SHAPES = {
    "sir6_s8": (COUNTS6, 8, [1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1]),
    "sir14_s8": (COUNTS14, 8, [1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1]),
    "sir14_s80": (COUNTS14, 80, [1, 1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1]),
}
FINDER = dict(adam_step_size=0.1, max_iters=3000, threshold=1.0)


def sir_ctx(counts, S, B, sigma=1.0):
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    return ChmcContext("sir", 1.0, S, len(counts), counts, sigma=sigma, num_chains=B)


def check_fill(ctx_of, fill):
    """fill(ctx, rows, stream, draw, n_cols, ld) -> [B, ld] array that held the sentinel 7.5 everywhere before the call.
    Shared with the GPU test (device-pointer entry point).  Tolerance 1e-12 absolute: |n| <= 8.7 for 53-bit uniforms, log /
    sqrt / cos / sin are good to a few ulp and the angle 2 pi u2 carries up to one ulp of 2 pi (9e-16), which cos / sin
    pass on scaled by the radius: order 1e-14, the bound leaves two decades."""
    c9, c2 = ctx_of(9), ctx_of(2)
    rows, stream = [7, 0, 3, 4], [5, 11, 5, 1 << 20]
    draw = [HI | 3, 0, HI | 3, (1 << 40) + 9]          # high bit set; rows 7 and 3 share (stream, draw)
    got = {}
    for n_cols, ld in ((6, 6), (7, 7), (6, 9), (7, 10), (1, 1), (0, 4)):
        out = fill(c9, rows, stream, draw, n_cols, ld)
        assert out.shape == (9, ld)
        for r, s, d in zip(rows, stream, draw):
            np.testing.assert_allclose(out[r, :n_cols], reference_normals(n_cols, s, SEED, d), rtol=0, atol=1e-12)
            assert (out[r, n_cols:] == 7.5).all()       # padding untouched
        assert (out[[1, 2, 5, 6, 8]] == 7.5).all()      # unlisted rows untouched
        assert np.array_equal(out[7], out[3])
        got[n_cols, ld] = out
    # a value depends on (seed, stream, draw, component) alone: not on the leading dimension, the row, the other rows
    # listed, the number of chains of the context or the number of columns asked for
    assert np.array_equal(got[6, 6][rows], got[6, 9][rows][:, :6]) and np.array_equal(got[7, 7][rows], got[7, 10][rows][:, :7])
    assert np.array_equal(got[6, 6][rows], got[7, 7][rows][:, :6])
    small = fill(c2, [1], [5], [HI | 3], 7, 8)
    assert np.array_equal(small[1, :7], got[7, 7][7]) and (small[0] == 7.5).all()
    assert (fill(c9, [], [], [], 5, 5) == 7.5).all()    # n_rows = 0
    assert not np.array_equal(fill(c2, [0], [5], [3], 6, 6)[0], fill(c2, [0], [5], [HI | 3], 6, 6)[0])
    c9.close(), c2.close()


def test_fill_normal_against_the_numpy_restatement(emu_lib):  # noqa: F811
    def fill(ctx, rows, stream, draw, n_cols, ld):
        buf = np.full((ctx.B, ld), 7.5)
        ctx.fill_normal(SEED, rows, stream, draw, buf[:, :n_cols])
        return buf
    check_fill(lambda B: sir_ctx(COUNTS6, 2, B), fill)


def test_sample_momentum_bits_are_those_of_the_parent(emu_lib):  # noqa: F811
    """tests/golden/keyed_init/sample_momentum_emu.npz: positions and the momenta chmc_sample_momentum(20200710, 3, chain_offset 5) gave
    in the emulation build of the commit BEFORE the Philox + Box-Muller pair was factored out of KNormalFill (even Q = 60 and
    odd Q = 55): the refactored generator must reproduce them bit for bit."""
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    g = np.load(os.path.join(HERE, "golden", "keyed_init", "sample_momentum_emu.npz"))
    for name, args in (("fhn", ("fhn", 0.2, 4, 2)), ("sir", ("sir", 1.0, 3, None))):
        ctx = ChmcContext(*args, g[name + "_y"], sigma=0.1 if name == "fhn" else 1.0, num_chains=3)
        ctx.set_state(g[name + "_q"], None, g[name + "_x_obs"], 0)
        ctx.sample_momentum(SEED, 3, 5)
        p = ctx.get_state()[1]
        assert p.shape == g[name + "_p"].shape and np.array_equal(p, g[name + "_p"]), name
        ctx.close()


def keyed_host_run(name, off, cnt):
    from manifold_mcmc_for_diffusions_amd import init
    counts, S, _ = SHAPES[name]
    ctx = sir_ctx(counts, S, cnt)
    q, xo, tries = init.find_initial_states_by_gradient_descent_noisy_system(
        ctx, seed=SEED, chain_offset=off, total_chains=12, device_resident=False, **FINDER)
    c = ctx.constr()
    ctx.close()
    return q, xo, tries, c


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_loop_one_context_equals_two_shards(emu_lib, name):  # noqa: F811
    counts, S, want = SHAPES[name]
    T = len(counts)
    q, xo, tries, c = keyed_host_run(name, 0, 12)
    assert tries.tolist() == want
    assert np.abs(c).max() < 1e-9 and (np.mean(q[:, -T:] ** 2, 1) < 1.0).all()
    parts = [keyed_host_run(name, 0, 5), keyed_host_run(name, 5, 7)]
    for k in range(3):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), (q, xo, tries)[k]), k
    # try 0 of a chain that kept it starts from the keyed draw: u[...] moved, but the start is what fill_normal gives
    assert not np.array_equal(q[0], q[1])


def stand_ins(B, T, nuv, record):
    """The landscape of tests/test_sampling.py's slot test: a try whose draw has u[0] > 0 never gets below the threshold
    (stalls, or is NaN at once for u[0] > 1.5); begin_tries deals keyed draws from the NumPy restatement."""
    import torch

    def objective(u_v, g):
        u = u_v.numpy()
        bad = u[:, 0] > 0
        h = 10.0 * np.mean(u[:, 1:] ** 2, 1) + np.where(bad, 2.0, 0.0)
        val = 0.5 * T * h + 0.5 * np.sum(u ** 2, 1)
        val = np.where(u[:, 0] > 1.5, np.nan, val)
        gr = u.copy()
        gr[:, 0] = 0.0
        gr[:, 1:] += 0.5 * T * 20.0 * u[:, 1:] / (nuv - 1)
        g.copy_(torch.from_numpy(gr))
        return np.stack([val, np.sum(u ** 2, 1), np.ones(B)], 1)

    def adam_update(u_v, m, v, g, coef, b1, b2, eps):
        c = torch.from_numpy(coef)
        m.mul_(b1).add_((1 - b1) * g)
        v.mul_(b2).add_((1 - b2) * g * g)
        u_v.sub_(c[:, 1:2] * m / (torch.sqrt(v * c[:, 0:1]) + eps))

    def begin_tries(rows, stream, draw, u_v, m, v, g):
        for r, s, d in zip(np.asarray(rows).tolist(), np.asarray(stream).tolist(), np.asarray(draw).tolist()):
            assert d & HI
            record.append((r, s, d ^ HI))
            u_v[r] = torch.from_numpy(reference_normals(nuv, s, 5, d))
            m[r], v[r], g[r] = 0.0, 0.0, 0.0

    return torch.device("cpu"), (lambda: None), objective, adam_update, begin_tries


def test_device_loop_slot_logic_does_not_depend_on_the_schedule_in_keyed_mode():
    """init._adam_on_device with stand-ins for its library calls: the winners (try numbers) and their points are the same
    for max_parallel_tries = 1, 4 and 16, although the tries run in other rows and start at other iterations."""
    from manifold_mcmc_for_diffusions_amd import init
    B, T, nuv, off = 48, 6, 12, 100
    ctx = SimpleNamespace(B=B, Q=nuv + T, T=T, U=3, sigma=1.0, variable_sigma=False)
    res = {}
    for mpt in (1, 4, 16):
        rec = []
        u_v, tries, status = init._adam_on_device(ctx, None, 0.1, 1000, 100, 1.0, 0.8, 100, 10, None, max_parallel_tries=mpt,
                                                  _calls=stand_ins(B, T, nuv, rec), seed=5, chain_offset=off)
        res[mpt] = (u_v.numpy().copy(), tries.copy(), rec, status)
        assert rec[:B] == [(c, off + c, 0) for c in range(B)]      # try 0 runs in the chain's own row
        assert len(rec) == sum(len(st) for st in status)          # every try handed out was dealt in by one keyed draw
    u1, t1 = res[1][:2]
    first = np.stack([reference_normals(nuv, off + c, 5, HI) for c in range(B)])
    assert (t1[first[:, 0] <= 0] == 1).all() and (t1[first[:, 0] > 0] >= 2).all() and t1.max() >= 3
    for mpt in (4, 16):
        assert np.array_equal(res[mpt][1], t1) and np.array_equal(res[mpt][0], u1), mpt
    # the schedules did differ: with 16 parallel tries more tries were started than the winners needed
    assert len(res[16][2]) > len(res[1][2]) == int(t1.sum())
    # a fresh try ran in a row other than its chain's own
    assert any(r != s - off for r, s, k in res[4][2])


def test_two_gloo_ranks_equal_one_rank_keyed(emu_lib, tmp_path):  # noqa: F811
    """SirWorkload(keyed_init=True) plus 3 static transitions on two ranks (5 = 3 + 2 chains) equals the single-rank run."""
    import keyed_dist_worker
    total = 5
    single = keyed_dist_worker.run(total, 0, 1)
    out = str(tmp_path / "gathered.npy")
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "keyed_dist_worker.py"), out, str(total)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, o.decode()[-2000:]
    gathered = np.load(out)
    assert gathered.shape == single.shape and np.array_equal(gathered, single)
    assert len(np.unique(single[:, 0])) == total


def test_misuse(emu_lib):  # noqa: F811
    from manifold_mcmc_for_diffusions_amd import init
    ctx = sir_ctx(COUNTS6, 2, 3)
    L, nuv = ctx.L, ctx.Q - ctx.T
    with pytest.raises(ValueError, match="exactly one"):
        init.find_initial_states_by_gradient_descent_noisy_system(ctx, np.random.default_rng(1), seed=3)
    with pytest.raises(ValueError, match="exactly one"):
        init.find_initial_states_by_gradient_descent_noisy_system(ctx)
    with pytest.raises(ValueError, match="total_chains"):
        init.find_initial_states_by_gradient_descent_noisy_system(ctx, seed=3, chain_offset=2, total_chains=4)
    buf = np.full((3, nuv), 7.5)
    for rows, match in (([3], "row index out of range"), ([-1], "row index out of range"), ([1, 1], "listed twice"),
                        ([0, 1, 2, 0], "n_rows out of range")):
        with pytest.raises(RuntimeError, match=match):
            ctx.fill_normal(SEED, rows, 0, 0, buf)
        with pytest.raises(RuntimeError, match=match):
            ctx.fill_normal_device(SEED, rows, 0, 0, nuv, buf.ctypes.data)
        with pytest.raises(RuntimeError, match=match):
            ctx.adam_begin_tries_device(SEED, rows, 0, 0, *([buf.ctypes.data] * 4))
    assert (buf == 7.5).all()
    one = (C.c_int * 1)(0)
    d = (C.c_ulonglong * 1)(0)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    bp = buf.ctypes.data_as(dp)
    one_p, d_p = C.cast(one, ip), C.cast(d, C.POINTER(C.c_ulonglong))
    assert L.chmc_fill_normal(None, SEED, 1, one_p, one_p, d_p, 2, bp, 2) != 0
    assert L.chmc_fill_normal(ctx.h, SEED, 1, one_p, one_p, d_p, 2, None, 2) != 0
    assert L.chmc_fill_normal(ctx.h, SEED, 1, None, one_p, d_p, 2, bp, 2) != 0
    assert L.chmc_fill_normal(ctx.h, SEED, 1, one_p, None, d_p, 2, bp, 2) != 0
    assert L.chmc_fill_normal(ctx.h, SEED, 1, one_p, one_p, None, 2, bp, 2) != 0
    assert L.chmc_fill_normal(ctx.h, SEED, 1, one_p, one_p, d_p, 3, bp, 2) != 0      # ld < n_cols
    assert L.chmc_fill_normal_device(ctx.h, SEED, 1, one_p, one_p, d_p, 2, None, 2) != 0
    assert b"null argument" in L.chmc_last_error()
    vp = C.c_void_p(buf.ctypes.data)
    for k in range(4):
        args = [vp] * 4
        args[k] = None
        assert L.chmc_adam_begin_tries_device(ctx.h, SEED, 1, one_p, one_p, d_p, *args) != 0
    assert (buf == 7.5).all()
    ctx.close()
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    noiseless = ChmcContext("fhn", 0.2, 4, 2, np.zeros(6), sigma=None, num_chains=2)
    b2 = np.zeros((2, noiseless.Q))
    with pytest.raises(RuntimeError, match="needs observation noise"):
        noiseless.adam_begin_tries_device(SEED, [0], 0, 0, *([b2.ctypes.data] * 4))
    noiseless.close()
