"""Per-chain observations (chmc_set_observations / chmc_get_observations) on the host emulation build: the `*_host_logic`
twins of tests/test_hip_grouped_observations.py, to the same bounds.  What is judged is the library's host side -- the
per-chain arrays, the stride, the half-batch views, the invalidated state, the API checks -- over the generic functors; the
wave kernels are judged on the device."""
import threading
import numpy as np
import pytest
from test_emu_logic import emu_lib  # noqa: F401  (fixture)
import grouped_obs as go

HOST_LAYOUTS = ["a_fhn_noisy_7rows", "b_fhn_noiseless_gauss", "c_fhn_16rows", "e_sir_one_block", "g_fhn_var_sigma"]


@pytest.mark.parametrize("halves", ["1", "2"])
@pytest.mark.parametrize("name", HOST_LAYOUTS)
def test_grouped_context_equals_separate_contexts_host_logic(emu_lib, monkeypatch, name, halves):  # noqa: F811
    """One context of 13 chains with per-chain (y, sigma) against three contexts with their group's shared data: bitwise,
    after the same comparison of ONE shared data set as one context and as the 4 | 5 | 4 split has passed (control).  The
    comparator target has no emulation form and is judged on the device only."""
    monkeypatch.setenv("CHMC_HALVES", halves)
    gc = go.make_groups(name, seed=41)
    control_bad, bad, whole, _ = go.run_grouped_vs_separate(gc, nld=False)
    assert not control_bad, f"control (shared data, one context against the split) differs: {control_bad}"
    assert not bad, f"per-chain data against one context per group differs: {bad}"
    status0 = dict(whole)["step0.status"]
    assert status0[5] == -1 and (status0[[2, 7]] > 0).all() and (np.delete(status0, [2, 5, 7]) == 0).all()


def test_grouped_context_against_the_oracle_host_logic(emu_lib):  # noqa: F811
    gc = go.make_groups("a_fhn_noisy_7rows", seed=42)
    ctx = go.grouped_ctx(gc)
    go.check_grouped_against_oracle(ctx, gc)
    ctx.close()


def test_constructor_takes_per_chain_data_host_logic(emu_lib):  # noqa: F811
    """ChmcContext(y_seq [B, T], sigma [B]) is set_observations after creation; observations() hands both back; a context
    that never had per-chain data reports the shared values once per chain."""
    gc = go.make_groups("a_fhn_noisy_7rows", seed=43)
    ctx = go.grouped_ctx(gc, via_constructor=True)
    y, s = ctx.observations()
    assert np.array_equal(y, gc["y"]) and np.array_equal(s, gc["sigma"])
    ctx.set_state(gc["q"], None, gc["x_obs"], 0)
    assert np.abs(ctx.constr()).max() < 1e-12  # every chain sits on the manifold of its OWN data
    ctx.close()
    ctx = go.shared_ctx(gc, gc["y"][0], 0.05, 3)
    y, s = ctx.observations()
    assert np.array_equal(y, np.repeat(gc["y"][:1], 3, 0)) and np.array_equal(s, np.full(3, 0.05))
    # y alone: the context keeps its noise level
    ctx.set_observations(gc["y"][[0, 4, 9]])
    y, s = ctx.observations()
    assert np.array_equal(y, gc["y"][[0, 4, 9]]) and np.array_equal(s, np.full(3, 0.05))
    # replacing the data
    ctx.set_observations(gc["y"][[9, 4, 0]], np.array([0.3, 0.2, 0.1]))
    y, s = ctx.observations()
    assert np.array_equal(y, gc["y"][[9, 4, 0]]) and np.array_equal(s, [0.3, 0.2, 0.1])
    ctx.set_observations(gc["y"][[0, 4, 9]])  # sigma = None keeps the per-chain values
    assert np.array_equal(ctx.observations()[1], [0.3, 0.2, 0.1])
    ctx.close()
    with pytest.raises(ValueError, match="y_seq"):
        go.ChmcContext("fhn", 0.2, 16, 5, gc["y"][:5], sigma=0.1, num_chains=4)
    with pytest.raises(ValueError, match="sigma"):
        go.ChmcContext("fhn", 0.2, 16, 5, gc["y"][:4], sigma=np.array([0.1, 0.2]), num_chains=4)


def check_api_misuse(lib):
    """GPU test 6 and its twin: each misuse returns a negative value with a chmc_last_error text and leaves the context
    usable."""
    import ctypes
    from manifold_mcmc_for_diffusions_amd._lib import ptr
    gc = go.make_groups("a_fhn_noisy_7rows", seed=44)
    B = gc["B"]
    y, sig = np.ascontiguousarray(gc["y"]), np.ascontiguousarray(gc["sigma"])

    def usable(ctx, q, xo):
        ctx.set_state(q, None, xo, 0)
        assert np.isfinite(ctx.constr()).all()
        assert (ctx.leapfrog_step(0.02)["status"] >= 0).all()

    # sigma in a noiseless and in a variable-noise context
    for name in ("b_fhn_noiseless_gauss", "g_fhn_var_sigma"):
        g2 = go.make_groups(name, seed=45)
        ctx = go.grouped_ctx(g2)
        rc = lib.chmc_set_observations(ctx.h, ptr(np.ascontiguousarray(g2["y"])), ptr(sig))
        assert rc < 0 and b"noisy == 1" in lib.chmc_last_error()
        with pytest.raises(RuntimeError, match="noisy == 1"):
            ctx.set_observations(g2["y"], sig)
        assert np.array_equal(ctx.observations()[0], g2["y"])
        usable(ctx, g2["q"], g2["x_obs"])
        ctx.close()
    ctx = go.grouped_ctx(gc)
    # a non-positive (or NaN) sigma: refused before anything is replaced
    for v in (0.0, -0.1, np.nan):
        s2 = sig.copy()
        s2[B - 1] = v
        rc = lib.chmc_set_observations(ctx.h, ptr(y + 1.0), ptr(s2))
        assert rc < 0 and b"sigma must be > 0" in lib.chmc_last_error()
    assert lib.chmc_set_observations(ctx.h, None, ptr(sig)) < 0 and b"y_seq is null" in lib.chmc_last_error()
    y_back, s_back = ctx.observations()
    assert np.array_equal(y_back, y) and np.array_equal(s_back, sig)
    # another thread than the creator's
    res = {}

    def other():
        res["rc"] = lib.chmc_set_observations(ctx.h, ptr(y), ptr(sig))
        res["err"] = lib.chmc_last_error()  # (the text is thread-local)
        res["rc_get"] = lib.chmc_get_observations(ctx.h, ptr(np.empty_like(y)), None)

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert res["rc"] < 0 and res["rc_get"] < 0 and b"thread" in res["err"]
    with pytest.raises(ValueError, match="y must have shape"):
        ctx.set_observations(y[:, :-1])
    with pytest.raises(ValueError, match="sigma must have shape"):
        ctx.set_observations(y, sig[:-1])
    usable(ctx, gc["q"], gc["x_obs"])
    ctx.close()
    del ctypes


def test_api_misuse_host_logic(emu_lib):  # noqa: F811
    check_api_misuse(emu_lib)


def test_set_observations_invalidates_the_state_host_logic(emu_lib):  # noqa: F811
    """After set_observations the context is as after chmc_create: entry points that need a state say so."""
    gc = go.make_groups("a_fhn_noisy_7rows", seed=46)
    ctx = go.grouped_ctx(gc)
    ctx.set_state(gc["q"], None, gc["x_obs"], 0)
    ctx.generate_x_seq(stride=16)
    ctx.set_observations(gc["y"], gc["sigma"])
    with pytest.raises(RuntimeError, match="no state"):
        ctx.generate_x_seq(stride=16)
    ctx.close()


@pytest.mark.parametrize("name", ["a_fhn_noisy_7rows", "b_fhn_noiseless_gauss", "e_sir_one_block", "g_fhn_var_sigma"])
def test_simulate_observations_host_logic(emu_lib, name):  # noqa: F811
    print(name, go.check_simulated_observations(name))


@pytest.mark.parametrize("name,seed,eps", [("a_fhn_noisy_7rows", 1, 0.05), ("e_sir_one_block", 4, 0.02)])
def test_transitions_against_each_chains_own_oracle_host_logic(emu_lib, name, seed, eps):  # noqa: F811
    print(name, go.check_transitions(name, seed, eps))
