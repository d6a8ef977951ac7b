"""Every CPU copy of the model code judged by numbers the reference's own programs computed.

tests/golden/reference_runs/*.npz (tests/golden/generate_reference_runs.py) hold, per case, the inputs and the results of the
reference's model files and notebook cells executed under stand-ins for their dependencies (oracle/ref_programs.py) with
50-digit arithmetic, and the distance e_ref64 of the same programs run in double precision.  The four CPU copies of the model
are judged against them at the bounds of tests/reference_runs.py:

  host model        manifold_mcmc_for_diffusions_amd/example_models.py
  py oracle         oracle/py/models.py
  C oracle          oracle/c (generate_x_obs_seq, constr, jacob_products)
  emulation build   tests/emu (generate_x_seq(q=), update_x_obs_seq, constr, lmult_ / rmult_by_jacob_constr)

No entry of any case is left out.  `test_regeneration` re-executes the reference and compares with the committed files bit
for bit; it is skipped where the reference directory, sympy or mpmath is absent.  The measured distances are tabulated in
tests/golden/README.md.

That the checks bite: with the sign of the delta-zeta term of the FitzHugh-Nagumo step flipped in a scratch copy of
csrc/models_gen.h (p14 and p25 of chmc_fhn_precompute), test_emulation_build failed at its first check, x_seq of
generate_x_seq(q=), for all five FitzHugh-Nagumo cases (fhn_varsigma_3x8: 2.3e-1 from the reference, bound 4.2e-15); the four
SIR cases passed."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import reference_runs as rr
from test_emu_logic import emu_lib  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _generator():
    spec = importlib.util.spec_from_file_location("generate_reference_runs", os.path.join(HERE, "golden", "generate_reference_runs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_files():
    """The cases of the generator's table, every file within the size limit, every stored number finite."""
    assert tuple(_generator().CASES) == rr.CASES
    names = sorted(os.listdir(rr.RUNS))
    assert names == sorted(c + ".npz" for c in rr.CASES + ("notebook_data", "device_normals"))
    assert all(("pred_x" in rr.load(c)) == (c in rr.PREDICT_CASES) for c in rr.CASES)
    for n in names:
        assert os.path.getsize(os.path.join(rr.RUNS, n)) <= rr.MAX_FILE_BYTES, n
    for cid in rr.CASES:
        f = rr.load(cid)
        assert len(f["u"]) == 3 and f["x_seq"].shape[1] == int(f["T"]) * int(f["S"]) + 1
        assert ("Jw" in f) == ("JTlam" in f) == rr.single_partition(f)
        for k, v in f.items():
            assert v.dtype.kind == "U" or np.isfinite(v).all(), (cid, k)


def test_absorbed_case_meets_the_cutoff():
    """sir_absorbed: the reference's clip and select, executed: log I below the cutoff once, then on it to the end and over
    more than an observation interval; log S within a unit above it and never on it; nothing within 1e-6 of it otherwise."""
    x = rr.load("sir_absorbed")["x_seq"]
    S = int(rr.load("sir_absorbed")["S"])
    for c in range(len(x)):
        on = np.flatnonzero(x[c, :, 1] == -500.0)
        assert len(on) > S and on[-1] == x.shape[1] - 1 and (np.diff(on) == 1).all() and x[c, on[0] - 1, 1] < -500.0
        assert (x[c, :, 0] > -500.0).all() and x[c, on[0] - 1, 0] < -499.0
        off = np.abs(x[c, :, :2] + 500.0)
        assert ((off == 0) | (off > 1e-6)).all()


def _model_functions(copy, cid, generate_z, generate_x_0, generate_sigma_y, path, obs_func):
    f = rr.load(cid)
    model, T, S, R, sigma, obs_interval = rr.meta(f)
    B = len(f["u"])
    z = np.stack([generate_z(f["u"][c]) for c in range(B)])
    x_0 = np.stack([generate_x_0(z[c], f["v_0"][c]) for c in range(B)])
    rr.judge(copy, cid, "z", z)
    rr.judge(copy, cid, "x_0", x_0)
    if sigma == "variable":
        rr.judge(copy, cid, "sigma_y", np.stack([generate_sigma_y(f["u"][c]) for c in range(B)]))
    x_seq = np.stack([np.concatenate([x_0[c][None], path(z[c], x_0[c], f["v_seq"][c], obs_interval / S)]) for c in range(B)])
    rr.judge(copy, cid, "x_seq", x_seq)
    rr.judge(copy, cid, "x_obs", x_seq[:, S::S])
    rr.judge(copy, cid, "obs", np.stack([obs_func(x_seq[c, S::S]) for c in range(B)]))


@pytest.mark.parametrize("cid", rr.CASES)
def test_host_model(cid):
    from manifold_mcmc_for_diffusions_amd import example_models as em
    m = em.MODELS[rr.meta(rr.load(cid))[0]]
    _model_functions("host_model", cid, m.generate_z, m.generate_x_0, getattr(m, "generate_σ_y", None),
                     lambda z, x_0, v, dl: em.generate_x_seq(m, z, x_0, v, dl), m.obs_func)


@pytest.mark.parametrize("cid", rr.CASES)
def test_py_oracle(cid):
    import torch
    from oracle.py import models as om
    m = om.MODELS[rr.meta(rr.load(cid))[0]]
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))  # noqa: E731

    def path(z, x_0, v, dl):
        x, out = t(x_0), []
        for k in range(len(v)):
            x = m.forward_func(t(z), x, t(v[k]), dl)
            out.append(x.numpy())
        return np.stack(out)

    _model_functions("py_oracle", cid, lambda u: m.generate_z(t(u)).numpy(), lambda z, v_0: m.generate_x_0(t(z), t(v_0)).numpy(),
                     lambda u: m.generate_sigma_y(t(u)).numpy(), path, lambda x: m.obs_func(t(x)).numpy())


@pytest.mark.parametrize("cid", rr.CASES)
def test_c_oracle(cid):
    from oracle import c_oracle
    f = rr.load(cid)
    model, T, S, R, sigma, obs_interval = rr.meta(f)
    osys = c_oracle.OracleSystem(model, obs_interval, S, R, f["y"], sigma=sigma)
    assert (osys.num_partition == 1) == rr.single_partition(f)
    q = rr.q_of(f)
    B = len(q)
    rr.judge("c_oracle", cid, "x_obs", np.stack([osys.generate_x_obs_seq(q[c]) for c in range(B)]))
    if rr.single_partition(f):
        rr.judge("c_oracle", cid, "c", np.stack([osys.constr(q[c], f["x_obs"][c], 0) for c in range(B)]))
        prods = [osys.jacob_products(q[c], f["x_obs"][c], 0, f["w"][c], f["lam"][c]) for c in range(B)]
        rr.judge("c_oracle", cid, "Jw", np.stack([p[0] for p in prods]), tol=rr.OPERATOR_TOL)
        rr.judge("c_oracle", cid, "JTlam", np.stack([p[1] for p in prods]), tol=rr.OPERATOR_TOL)


@pytest.mark.parametrize("cid", rr.CASES)
def test_emulation_build(emu_lib, cid):  # noqa: F811
    ctx = rr.make_ctx(cid)
    rr.judge_context("emulation", cid, ctx)
    ctx.close()


def test_notebook_data_function():
    """examples/fhn_notebook_posterior.py's data against the notebook's own cells at the notebook's T = 100, S = 25: the
    legacy generator's draw exactly; z, x_0 and y_seq_ref against the cells' 50-digit run, the yardstick being the distance
    of the cells' own double-precision run (the stored y_seq_ref) from it."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import fhn_notebook_posterior as ex
    finally:
        sys.path.pop(0)
    with np.load(os.path.join(rr.RUNS, "notebook_data.npz")) as f:
        nb = {k: f[k] for k in f.files}
    d = ex.notebook_data()
    assert (d["T"], d["S"], d["obs_interval"]) == (int(nb["T"]), int(nb["S"]), float(nb["obs_interval"]))
    np.testing.assert_array_equal(d["q_ref"][:16], nb["q_ref_head"])
    assert float(np.sum(d["q_ref"])) == float(nb["q_ref_sum"])
    assert nb["y_seq_ref"].shape == (100, 1)
    for name, mine in (("z", d["z_ref"]), ("x_0", d["x_0_ref"]), ("y_seq_ref", d["y"][:, None])):
        dist, b = rr.distance(mine, nb[name + "_mp"]), rr.bound(nb, name)
        print(f"REFRUN host_model notebook_data {name} {dist:.2e} bound {b:.2e}")
        assert dist <= b, (name, dist, b)


@pytest.mark.parametrize("cid", rr.CASES)
def test_emulation_build_state_after_a_null_step(emu_lib, cid):  # noqa: F811
    """The host-logic twin of the device's time-parallel forms (tests/test_hip_reference_runs.py): the forward scan with a
    guess trajectory and the state evaluation that ends a step, on the fixture point."""
    ctx = rr.make_ctx(cid, per_chain_data=True)
    rr.judge_after_null_step("emulation", cid, ctx)
    ctx.close()


from oracle import ref_programs as _rp  # noqa: E402  (a module of the project: an import error is a failure, not a skip)

_ok, _why = _rp.available()


@pytest.mark.skipif(not _ok, reason=f"the reference's programs cannot be executed here: {_why}")
@pytest.mark.parametrize("cid", rr.CASES + ("notebook_data",))
def test_regeneration(cid):
    """The reference re-executed now: every array of the committed file, inputs and results of both number modes (e_ref64 is
    the double-precision run's distance), equal to the last bit.  The central differences of the largest case (sir_12x8, 610
    50-digit paths per chain) are regenerated by the generator alone."""
    gen = _generator()
    if cid == "notebook_data":
        new = gen.notebook_data()
        with np.load(os.path.join(rr.RUNS, cid + ".npz")) as f:
            old = {k: f[k] for k in f.files}
    else:
        new, old = gen.generate_case(cid, with_derivatives=cid != "sir_12x8"), dict(rr.load(cid))
        if cid == "sir_12x8":
            old.pop("Jw"), old.pop("JTlam")
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k]), (cid, k)
