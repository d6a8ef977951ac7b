"""Carrying chains between time resolutions on the MI355X: the check functions of test_resolution.py on the HIP library
(the wave kernel k_resample with its three tilings, KSolveNoise behind the path scan), and the device's result beside the
host emulation's."""
import ctypes
import numpy as np
import pytest
import test_resolution as tr
from test_emu_logic import emu_lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", tr.SHAPES, ids=tr.shape_id)
def test_map_against_the_numpy_restatement_and_its_identities(shape):
    tr.check_map(shape)


def test_prior_is_preserved():
    tr.check_prior(tr.prior_sample()[0])


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("model,T,Sc,R,part", tr.MANIFOLD)
def test_transferred_state_is_on_the_fine_manifold(model, T, Sc, R, part, m):
    tr.check_on_the_manifold(model, T, Sc, R, part, m)


def test_noiseless_context_is_refused():
    tr.check_noiseless_is_refused()


def test_shard_independence():
    tr.check_shards()
    tr.check_shards("sir", 2, 3, 7, 1.0)
    tr.check_shards("fhn", 2, 1, 300, 0.1)


def test_errors():
    tr.check_errors()


def test_device_against_emulation(emu_lib):  # noqa: F811
    """Case 7.  Both builds pass the restatement at 1e-13 with their own xi (test_map_... here and in test_resolution.py);
    this test puts the two results side by side.  Measured on the MI355X: the refined rows are NOT bitwise equal on every
    shape, because xi is not -- the device's log / cos / sin of the Box-Muller pair round differently from the host's libm,
    max |xi_hip - xi_emu| = 4.4e-16 -- and the rows then differ by the same order (at most 8.9e-16).  On the shapes where the
    two builds' xi agree bitwise (FHN T = 3, S_c = 1, m = 2 and 3) the rows are bitwise equal: given the same xi the ordering
    contract makes the map itself bit-identical.  So the assertions are: bitwise equality wherever xi is bitwise equal, and
    1e-13 on the difference that is left once the two builds' own xi are taken out through the linear map (measured:
    8.6e-16).  The bitwise comparison is reported per shape either way."""
    from manifold_mcmc_for_diffusions_amd import _lib
    emu = _lib._LIB
    hip = _lib._bind(ctypes.CDLL(_lib._SO))
    worst, bitwise = 0.0, True
    for shape in tr.SHAPES:
        model, T, Sc, m, sigma = shape
        got = {}
        for name, L in (("hip", hip), ("emu", emu)):
            _lib._LIB = L
            try:
                fine = tr.make_ctx(model, T, Sc * m, sigma, 3)
                q_c = np.random.default_rng(7).standard_normal((3, fine.Q - T * Sc * (m - 1) * fine.V))
                src, dst = tr.Dev(fine, q_c), tr.Dev(fine, np.zeros((3, fine.Q)))
                fine.resample_q_device(src.ptr, Sc, tr.SEED, dst.ptr, draw=3, chain_offset=5)
                xi = tr.split(fine, tr.xi_rows(fine, tr.SEED, 3, 5), fine.S)[1]
                got[name] = (tr.split(fine, dst.get(), fine.S)[1], xi)
                fine.close()
            finally:
                _lib._LIB = emu
        (w_h, xi_h), (w_e, xi_e) = got["hip"], got["emu"]
        same = np.array_equal(w_h, w_e)
        if np.array_equal(xi_h, xi_e):
            assert same, shape
        bitwise = bitwise and same
        # w is linear in xi: w_h - w_e = (I - A^T A)(xi_h - xi_e) when the two builds apply the same map
        d_xi = xi_h - xi_e
        expect = tr.np_refine(model, np.zeros_like(tr.np_coarsen(model, d_xi, m)), d_xi, m)
        fig = tr.rel(w_h - w_e, expect)
        worst = max(worst, fig)
        print(tr.shape_id(shape), f"bitwise {same}  max |w_hip - w_emu| {np.abs(w_h - w_e).max():.1e}  "
              f"max |xi_hip - xi_emu| {np.abs(d_xi).max():.1e}  beyond xi {fig:.1e}")
    print("device against emulation: bitwise equal on every shape:", bitwise, " worst difference beyond xi:", worst)
    assert worst <= tr.TOL
