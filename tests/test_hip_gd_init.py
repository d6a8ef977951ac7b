"""GPU: gradient-descent initial states for any system (init.find_initial_states_by_gradient_descent; forward half KGdFwd,
backward half k_gd_grad_wave, chain level KGdReduce).  Objective, gradient and max|c| against the torch restatement at the
shapes where the wave kernel can go wrong (64-step tile edges, one interval, more than 64 intervals, a clipped SIR
component), a row's bits independent of the batch, chmc_gd_project_device against set_state + project, and the whole
finder: oracle, restatement, any sharding and three leapfrog steps afterwards, bitwise.

The finder's windows, the restatement's tries and try-ending iterations and the margins of the deciding quantities are
tabulated in test_gd_init.py; the MI355X ended every try of every window at the iteration the restatement did."""
import numpy as np
import pytest
from helpers import make_case, make_ctx
from test_gd_init import (OBJ_CASES, REG, WINDOWS, check_found_states, check_non_finite_row, check_objective, objective_points,
                          run_finder, window_case)

pytestmark = pytest.mark.gpu
SOLVER = dict(newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8)


def dev_buf(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t


def dev_eval(ctx, q, xo):
    assert ctx.L.chmc_backend() == b"hip:gfx950"
    qd, xd, gd = dev_buf(q), dev_buf(xo), dev_buf(np.full_like(q, 7.5))
    out3 = ctx.gd_objective_device(qd.data_ptr(), xd.data_ptr(), REG, gd.data_ptr())
    assert np.array_equal(qd.cpu().numpy(), q) and np.array_equal(xd.cpu().numpy(), xo)  # inputs untouched
    return out3, gd.cpu().numpy()


@pytest.mark.parametrize("T,S,Rr", [(3, 5, 2), (1, 1, None)])
@pytest.mark.parametrize("model,noisy,vs", OBJ_CASES)
def test_objective_gradient_and_max_c_against_the_restatement(model, noisy, vs, T, S, Rr):
    check_objective(dev_eval, model, T, S, Rr, noisy, vs)


# S = 70: two tiles, the second holding 6 steps; S = 64: exactly one tile; S = 1; T = 1: only the interval that starts at x_0
# (v_0 / gx0_jac); T = 13 with B = 3: 39 (chain, interval) tasks; T = 70: past 64 intervals per chain
SHAPES = [("fhn", False, 3, 70, 2, 3), ("sir", True, 3, 70, None, 3), ("fhn", True, 3, 64, 2, 3), ("sir", True, 4, 1, 2, 3),
          ("fhn", False, 1, 5, None, 3), ("sir", True, 1, 70, None, 3), ("fhn", False, 13, 4, 5, 3), ("fhn", True, 70, 3, 5, 2)]


@pytest.mark.parametrize("model,noisy,T,S,Rr,B", SHAPES)
def test_objective_at_tile_and_interval_edges(model, noisy, T, S, Rr, B):
    check_objective(dev_eval, model, T, S, Rr, noisy, False, B=B, seed=7)


def test_objective_through_a_clipped_sir_component():
    """x_obs_seq_init with log S = -600 at observation 1 of chain 0: the interval that starts there runs on the clipped
    branch of SirModel::step / jac (the component stays at -500, derivatives through it are zero)."""
    c = check_objective(dev_eval, "sir", 3, 5, None, True, False, spike=(0, 1, 0, -600.0))
    assert c[0, 1, 0] > 590.0 and c[0, 2, 0] < -490.0     # (interval 2 of chain 0 ended at the floor, -500)


def test_a_non_finite_row_is_flagged_and_leaves_the_others_alone():
    check_non_finite_row(dev_eval)


@pytest.mark.parametrize("model,noisy,T,S,Rr", [("fhn", True, 3, 70, 2), ("sir", True, 5, 8, None), ("fhn", False, 70, 3, 5)])
def test_a_rows_bits_do_not_depend_on_the_batch(model, noisy, T, S, Rr):
    """One (q, xo) as a context of B = 1 and as row 2 of a context of B = 5 with unrelated neighbours."""
    case, q, xo = objective_points(model, T, S, Rr, noisy, False, 5, 9)
    c5, c1 = make_ctx(case), make_ctx(dict(case, B=1))
    o5, g5 = dev_eval(c5, q, xo)
    o1, g1 = dev_eval(c1, q[2:3], xo[2:3])
    c5.close(), c1.close()
    assert o1[0, 2] == 1.0 and np.array_equal(o1[0], o5[2]) and np.array_equal(g1[0], g5[2])
    assert not np.array_equal(g5[2], g5[1])


@pytest.mark.parametrize("model,T,S,Rr", [("fhn", 6, 8, 2), ("sir", 5, 8, None)])
def test_gd_project_device_against_set_state_and_project(model, T, S, Rr):
    case = make_case(model, T, S, Rr, True, B=4, seed=21)
    rng = np.random.default_rng(22)
    on = np.repeat(case["q"][:1], 4, 0)                  # chain 0 of a case lies on the manifold
    xo = np.repeat(case["x_obs"][:1], 4, 0) + 0.01 * rng.standard_normal((4, T, case["x_obs"].shape[-1]))
    pts = on + 1e-3 * rng.standard_normal(on.shape)
    mask = np.array([1, 0, 1, 0])
    ctx, ref = make_ctx(case), make_ctx(case)
    ctx.set_state(case["q"], rng.standard_normal(on.shape), case["x_obs"], 0)
    q0, p0, x0, _ = ctx.get_state()
    qd, xd = dev_buf(pts), dev_buf(xo)
    # one iteration is not enough: nothing converges, rows and (for masked chains) the states projected from stay
    r = ctx.gd_project_device(mask, qd.data_ptr(), xd.data_ptr(), max_iters=1)
    assert r["status"].tolist() == [1, -1, 1, -1] and np.array_equal(qd.cpu().numpy(), pts)
    r = ctx.gd_project_device(mask, qd.data_ptr(), xd.data_ptr())
    out = qd.cpu().numpy()
    q1, p1, x1, part = ctx.get_state()
    ref.set_state(pts, None, xo, 0)
    rr = ref.project(pts, 1.0)
    assert part == 0 and r["status"].tolist() == [0, -1, 0, -1] and rr["status"][0] == rr["status"][2] == 0
    for c in (1, 3):                                     # unmasked: row and state bitwise untouched
        assert np.array_equal(out[c], pts[c]) and np.array_equal(q1[c], q0[c]) and np.array_equal(p1[c], p0[c])
        assert np.array_equal(x1[c], x0[c])
    for c in (0, 2):                                     # masked: set_state + project(q, dt = 1), bit for bit
        assert np.array_equal(out[c], rr["q"][c]) and np.array_equal(q1[c], rr["q"][c]) and not p1[c].any()
        assert np.array_equal(x1[c], xo[c]) and r["iters"][c] == rr["iters"][c] and r["err"][c] == rr["err"][c]
        assert np.abs(case["osys"].constr(out[c], xo[c], 0)).max() < 1e-9
    # the adopted states carry evaluated caches: the same as setting them afresh
    ref.set_state(q1, p1, x1, 0)
    assert np.array_equal(ctx.constr(), ref.constr()) and np.array_equal(ctx.log_det_sqrt_gram(), ref.log_det_sqrt_gram())
    ctx.close(), ref.close()


def steps_after(ctx, first, off):
    """a keyed momentum refresh and three leapfrog steps, step sizes by global chain"""
    g = off + np.arange(ctx.B)
    dts = (np.where(np.arange(8) % 2 == 0, 1.0, -1.0) * (0.05 + 0.05 * np.random.default_rng(31).random(8)))[g]
    ctx.sample_momentum(20200710, 1, first + off)
    res = [ctx.leapfrog_step(dts, **SOLVER) for _ in range(3)]
    q, p, _, _ = ctx.get_state()
    out = [q, p]
    for r in res:
        out += [r["status"], r["iters_fwd"], r["iters_bwd"]]
    return out


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_finder_against_oracle_and_restatement_and_any_sharding(name):
    first = window_case(name)[3]
    ctx, q, xo, tries, status = run_finder(name, 0, 8)
    assert ctx.L.chmc_backend() == b"hip:gfx950"
    after = steps_after(ctx, first, 0)
    ctx.close()
    check_found_states(name, q, xo, tries, status)
    assert (after[2] == 0).sum() >= 6                    # the steps compared are of moving chains
    for shards in ([(0, 3), (3, 5)], [(c, 1) for c in range(8)]):
        for off, cnt in shards:
            ctx, q1, xo1, tries1, _ = run_finder(name, off, cnt)
            sl = slice(off, off + cnt)
            assert np.array_equal(tries1, tries[sl]) and np.array_equal(q1, q[sl]) and np.array_equal(xo1, xo[sl]), (off, cnt)
            for k, (a, b) in enumerate(zip(steps_after(ctx, first, off), after)):
                assert np.array_equal(a, b[sl]), (off, cnt, k)
            ctx.close()
