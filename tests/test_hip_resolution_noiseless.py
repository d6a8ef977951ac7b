"""Carrying chains between time resolutions without observation noise on the MI355X: the check functions of
test_resolution_noiseless.py on the HIP library (KPinObs behind the path scan, the projection on the wave kernels of every
layout family the shapes reach), and the device's placement beside the host emulation's."""
import ctypes
import numpy as np
import pytest
import test_resolution_noiseless as tn
from test_emu_logic import emu_lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape_part", tn.PLACED, ids=tn.placed_id)
def test_placed_on_the_manifold(shape_part):
    tn.check_placed(*shape_part)


def test_last_pin_workgroup_is_partial():
    tn.check_placed(tn.FIRST, 1, B=130)


@pytest.mark.parametrize("newton", [True, False])
def test_against_the_oracle(newton):
    tn.check_against_oracle(tn.FIRST, newton=newton)


@pytest.mark.parametrize("shape", [tn.SHAPES[5], tn.SHAPES[7]], ids=tn.shape_id)
def test_against_the_oracle_other_layouts(shape):
    tn.check_against_oracle(shape, B=3)


@pytest.mark.parametrize("metric", [False, True])
def test_the_correction_is_a_projection(metric):
    tn.check_is_a_projection(tn.FIRST, metric=metric)


def test_shard_independence():
    tn.check_shards(tn.FIRST)


def test_retries_depend_on_the_global_chain_alone():
    tn.check_shards(tn.SHAPES[9], want_retry=True, max_iters=2)


def test_failure_contract():
    tn.check_failure_contract()


def test_errors():
    tn.check_errors()


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_coarse_to_fine_drivers(dynamic):
    tn.check_driver(dynamic)


def test_device_against_emulation(emu_lib):  # noqa: F811
    """Assertion (8), on the first shape: the same coarse states placed by the HIP library and by the host emulation.
    status and iters are equal; the placed q agrees within 1e-9.  Bitwise is not expected: xi already differs by the
    device's log / sin / cos rounding (test_hip_resolution.py::test_device_against_emulation, 4.4e-16), and defect is a
    function of the refined row's path, so it is held to the 1e-10 the issue gives defect against the NumPy path, with the
    bitwise comparison reported."""
    from manifold_mcmc_for_diffusions_amd import _lib
    emu = _lib._LIB
    hip = _lib._bind(ctypes.CDLL(_lib._SO))
    model, T, Sc, m, R = tn.FIRST
    got = {}
    for name, L in (("hip", hip), ("emu", emu)):
        _lib._LIB = L
        try:
            coarse, _ = tn.start(tn.FIRST, 8)
            fine = coarse.sibling(Sc * m)
            dst, q_given = tn.refined(coarse, fine)
            r = fine.set_state_project(dst.ptr, 0)
            got[name] = dict(r, q=fine.get_state()[0], q_given=q_given)
            fine.close(), coarse.close()
        finally:
            _lib._LIB = emu
    h, e = got["hip"], got["emu"]
    print("defect bitwise equal:", np.array_equal(h["defect"], e["defect"]), f"max difference {np.abs(h['defect'] - e['defect']).max():.1e}",
          f" q given {np.abs(h['q_given'] - e['q_given']).max():.1e}  q placed {np.abs(h['q'] - e['q']).max():.1e}")
    assert (h["status"] == 0).all() and np.array_equal(h["status"], e["status"]) and np.array_equal(h["iters"], e["iters"])
    assert np.abs(h["defect"] - e["defect"]).max() <= 1e-10
    assert np.abs(h["q"] - e["q"]).max() <= 1e-9 * max(1.0, np.abs(e["q"]).max())
