"""Gradient-descent initial states for any system (init.find_initial_states_by_gradient_descent, the reference's
find_initial_state_by_gradient_descent, sde/mici_extensions.py:1550-1676), on the CPU through the TEST-ONLY emulation build
(functor twins KGdFwd / KGdGrad / KGdReduce): objective, gradient and max|c| against the torch restatement
(tests/gd_init_restatement.py), the non-finite flag, the whole finder against the oracle and the restatement's try loop, any
sharding bitwise, and the error paths.  The GPU tests are in test_hip_gd_init.py.

Windows of the finder tests (T = 6, S = 8, R = 2 for FitzHugh-Nagumo; T = 5, S = 8, one sub-sequence for SIR; data y of
helpers.make_case(..., B=8, seed=41); reference defaults).  Seed and first global chain were chosen so that the RESTATEMENT
ALONE finds all eight chains within max_num_tries = 10, that no try runs into the iteration budget (1000 autograd passes of
the restatement) and that some chain needs more than one try; candidates were screened with the emulation build, the
restatement then confirmed the window.  Observed with the restatement, (Adam iteration at which the try ended, how):
    fhn noiseless, seed 1,  chains 13-20   tries 1 3 2 1 1 1 3 2
        chain 14: (28, diverged) (19, diverged) (194, projected); chain 15: (37, diverged) (112, projected);
        chain 19: (26, diverged) (9, diverged) (131, projected); chain 20: (1, diverged) (107, projected);
        chains 13, 16, 17, 18 projected at 187, 138, 48, 133
    fhn noisy,     seed 8,  chains 9-16    tries 1 3 1 1 1 1 2 2
        chain 10: (20, diverged) (13, diverged) (77, projected); chain 15: (0, diverged) (99, projected);
        chain 16: (139, diverged) (63, projected); chains 9, 11, 12, 13, 14 projected at 95, 100, 162, 162, 74
    sir noisy,     seed 10, chains 39-46   tries 1 1 2 1 1 1 1 1
        chain 41: (4, diverged) (31, projected); the others projected at 29, 33, 18, 33, 20, 27, 51
The emulation build and the MI355X ended every try of every window at the same iteration as the restatement.  Margins of
the deciding quantities at the deciding iterations (restatement): max|c| against coarse_tol = 0.1 was 0.0497 .. 0.09984, at
least 1.6e-3 relative; the projection's error against tol = 1e-9 was at most 9.65e-10, 3.5e-2 relative; the constraint of the
projected point at most 1.1e-14.  All far above 1e-6 relative: no window had to move for a margin.
"""
import numpy as np
import pytest
from test_emu_logic import emu_lib  # noqa: F401
from helpers import make_case, make_ctx, random_q
import gd_init_restatement as R

REG = 2e-2
# objective cases: (model, noisy, variable sigma)
OBJ_CASES = [("fhn", False, False), ("fhn", True, False), ("fhn", True, True), ("fhn_nb", False, False), ("sir", True, False)]
# finder windows: name -> (model, T, S, R, noisy, seed, first global chain, tries of the eight chains)
WINDOWS = {
    "fhn_noiseless": ("fhn", 6, 8, 2, False, 1, 13, [1, 3, 2, 1, 1, 1, 3, 2]),
    "fhn_noisy": ("fhn", 6, 8, 2, True, 8, 9, [1, 3, 1, 1, 1, 1, 2, 2]),
    "sir_noisy": ("sir", 5, 8, None, True, 10, 39, [1, 1, 2, 1, 1, 1, 1, 1]),
}


def sir_x_obs_seq_init(y_seq, seed):
    """[log S, log I, log contact rate] = [log(762 - i), log i, 0.5 N(0, 1)] with i = max(y, 0.5): a pure function of
    (global chain, try), as init.fhn_x_obs_seq_init."""
    i = np.maximum(np.asarray(y_seq, dtype=np.float64).reshape(-1), 0.5)

    def gen(chains, tries):
        return np.stack([np.stack([np.log(762.0 - i), np.log(i),
                                   0.5 * np.random.default_rng([int(seed), int(c), int(k)]).standard_normal(len(i))], -1)
                         for c, k in zip(chains, tries)])
    return gen


def window_case(name):
    from manifold_mcmc_for_diffusions_amd import init
    model, T, S, Rr, noisy, seed, first, want = WINDOWS[name]
    case = make_case(model, T, S, Rr, noisy, B=8, seed=41)
    gen = (sir_x_obs_seq_init if model == "sir" else init.fhn_x_obs_seq_init)(case["y"], seed)
    return case, gen, seed, first, want


_RESTATED = {}


def restated(name):
    """The restatement's searches of the window's eight chains, computed once per process and left unchanged."""
    if name not in _RESTATED:
        case, gen, seed, first, _ = window_case(name)
        _RESTATED[name] = R.find_chains(case["model"], case["osys"], range(first, first + 8), seed, gen, case["S"],
                                        case["obs_interval"] / case["S"], case["noisy"])
    return _RESTATED[name]


def objective_points(model, T, S, Rr, noisy, vs, B, seed, spike=None):
    """random_q points and x_obs_seq_init within 0.5 of the points' own states (spike: (chain, observation, component, value))"""
    case = make_case(model, T, S, Rr, noisy, B=B, seed=seed, var_sigma=vs)
    xo = case["x_obs"] + np.random.default_rng(seed + 1).uniform(-0.5, 0.5, case["x_obs"].shape)
    if spike is not None:
        xo[spike[:3]] = spike[3]
    return case, np.ascontiguousarray(case["q"]), np.ascontiguousarray(xo)


def check_objective(evaluate, model, T, S, Rr, noisy, vs, B=3, seed=5, spike=None):
    """evaluate(ctx, q, xo) -> (out3, grad) of chmc_gd_objective_device; 1e-10 (the project's per-operator tolerance)
    relative to max(1, max|reference|) for the gradient, the objective and max|c| alike.  Shared with the GPU test."""
    case, q, xo = objective_points(model, T, S, Rr, noisy, vs, B, seed, spike)
    ctx = make_ctx(case)
    out3, g = evaluate(ctx, q, xo)
    ctx.close()
    obj, c, gr = R.objective(model, q, xo, S, case["obs_interval"] / S, noisy, vs, REG)
    for b in range(B):
        mac = np.abs(c[b]).max()
        print(model, T, S, noisy, vs, b, "obj", abs(out3[b, 0] - obj[b]), "max|c|", abs(out3[b, 1] - mac),
              "grad", np.abs(g[b] - gr[b]).max(), "scale", np.abs(gr[b]).max())
        assert np.isfinite(gr[b]).all() and out3[b, 2] == 1.0
        assert np.abs(g[b] - gr[b]).max() <= 1e-10 * max(1.0, np.abs(gr[b]).max())
        assert abs(out3[b, 0] - obj[b]) <= 1e-10 * max(1.0, abs(obj[b]))
        assert abs(out3[b, 1] - mac) <= 1e-10 * max(1.0, mac)
    return c


def host_eval(ctx, q, xo):
    g = np.full_like(q, 7.5)
    return ctx.gd_objective_device(q.ctypes.data, xo.ctypes.data, REG, g.ctypes.data), g


@pytest.mark.parametrize("T,S,Rr", [(3, 5, 2), (1, 1, None)])
@pytest.mark.parametrize("model,noisy,vs", OBJ_CASES)
def test_objective_gradient_and_max_c_against_the_restatement(emu_lib, model, noisy, vs, T, S, Rr):  # noqa: F811
    check_objective(host_eval, model, T, S, Rr, noisy, vs)


def check_non_finite_row(evaluate):
    case, q, xo = objective_points("fhn", 3, 5, 2, True, False, 3, 6)
    ctx = make_ctx(case)
    ref3, ref_g = evaluate(ctx, q, xo)
    q2 = q.copy()
    q2[1, 1] = 800.0                                     # exp overflows: z = generate_z(u) is not finite
    out3, g = evaluate(ctx, q2, xo)
    ctx.close()
    assert out3[1, 2] == 0.0 and not np.isfinite(out3[1, 0])
    assert np.array_equal(out3[[0, 2]], ref3[[0, 2]]) and np.array_equal(g[[0, 2]], ref_g[[0, 2]]) and (ref3[:, 2] == 1.0).all()


def test_a_non_finite_row_is_flagged_and_leaves_the_others_alone(emu_lib):  # noqa: F811
    check_non_finite_row(host_eval)


def run_finder(name, off, cnt, **kw):
    from manifold_mcmc_for_diffusions_amd import init
    case, gen, seed, first, _ = window_case(name)
    ctx = make_ctx(dict(case, B=cnt))
    q, xo, tries, status = init.find_initial_states_by_gradient_descent(
        ctx, gen, seed, chain_offset=first + off, total_chains=first + 8, return_status=True, **kw)
    return ctx, q, xo, tries, status


def check_found_states(name, q, xo, tries, status):
    """max|constr| < tol by the ORACLE at (q, x_obs_seq, partition 0); tries equal to the restatement's."""
    case, _, _, _, want = window_case(name)
    for c in range(8):
        assert np.abs(case["osys"].constr(q[c], xo[c], 0)).max() < 1e-9, c
    ref = restated(name)
    print(name, "tries", tries.tolist(), "library ends", status["ends"], "restatement ends", [s.ends for s in ref])
    assert [s.tries for s in ref] == want                # (the window's table in the module docstring)
    assert tries.tolist() == want
    for c, s in enumerate(ref):                          # the same winning try: the same x_obs_seq_init, a nearby point
        assert np.array_equal(xo[c], s.xo) and np.abs(q[c] - s.q).max() < 1e-3


@pytest.mark.parametrize("name", ["fhn_noiseless", "fhn_noisy"])
def test_finder_against_oracle_and_restatement_and_any_sharding(emu_lib, name):  # noqa: F811
    ctx, q, xo, tries, status = run_finder(name, 0, 8)
    q_s, _, xo_s, part = ctx.get_state(want_p=True)
    assert part == 0 and np.array_equal(q_s, q) and np.array_equal(xo_s, xo) and not ctx.get_state()[1].any()
    ctx.close()
    check_found_states(name, q, xo, tries, status)
    for shards in ([(0, 3), (3, 5)], [(c, 1) for c in range(8)]):
        for off, cnt in shards:
            ctx, q1, xo1, tries1, _ = run_finder(name, off, cnt)
            ctx.close()
            sl = slice(off, off + cnt)
            assert np.array_equal(tries1, tries[sl]) and np.array_equal(q1, q[sl]) and np.array_equal(xo1, xo[sl]), (off, cnt)


def test_error_paths(emu_lib):  # noqa: F811
    from manifold_mcmc_for_diffusions_amd import init
    case, gen, seed, first, _ = window_case("fhn_noiseless")
    ctx = make_ctx(case)
    with pytest.raises(ValueError, match="shape"):
        init.find_initial_states_by_gradient_descent(ctx, lambda chains, tries: gen(chains, tries)[:, :-1], seed)
    with pytest.raises(ValueError, match="total_chains"):
        init.find_initial_states_by_gradient_descent(ctx, gen, seed, chain_offset=3, total_chains=10)
    with pytest.raises(RuntimeError, match="Did not find valid state in 2 tries."):
        init.find_initial_states_by_gradient_descent(ctx, gen, seed, chain_offset=first, max_iters=3, max_num_tries=2)
    ctx.close()


def test_fhn_workload_with_gradient_descent_initial_states(emu_lib):  # noqa: F811
    """FhnWorkload(init="gradient_descent"): the states lie on the manifold and do not depend on the shard."""
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload
    kw = dict(num_steps_per_obs=8, num_obs=6, num_obs_per_subseq=2, num_steps_per_obs_data=200, init="gradient_descent")
    whole = FhnWorkload(4, total_chains=4, **kw)
    q = whole.ctx.get_state()[0]
    assert np.abs(whole.ctx.constr()).max() < 1e-9 and (whole.init_tries >= 1).all() and len(whole.rngs) == 4
    part = FhnWorkload(3, chain_offset=1, total_chains=4, **kw)
    assert np.array_equal(part.ctx.get_state()[0], q[1:]) and np.array_equal(part.init_tries, whole.init_tries[1:])
    with pytest.raises(ValueError, match="init must be"):
        FhnWorkload(2, **dict(kw, init="adam"))
