"""Every device form that produces a path, a constraint or a Jacobian product, judged by numbers the reference's own programs
computed (tests/golden/reference_runs, see tests/test_reference_runs.py for the CPU copies and tests/reference_runs.py for the
bounds).  The tests read the fixtures only.

Forms, per case (FORMS: the environment of the context, read by chmc_create or on entry to every call):
  default            the plan's own choice: k_fwd_scan where S % 8 == 0, the functor scan otherwise
  no_fwd_scan        CHMC_NO_FWD_SCAN: the generic functor instead of k_fwd_scan
                     (no launch counter tells KFwd from k_fwd_scan; that the switch selects the functor is stated by
                     tests/test_kernel_plan.py)
  par_w1 / 2 / 4     CHMC_PAR_SCAN=1, CHMC_PAR_WAVES=W: the time-parallel scan k_fwd_par.  It runs only from a guess
                     trajectory (fwd() in csrc/chmc_passes.inc: a state that is set is scanned by KernelPlan::fwd_cold
                     whatever the switch), so the fixture point is put through the rounds and the final state evaluation
                     of a leapfrog step that moves nothing: every chain on the manifold of data of its own, momentum zero,
                     step size 1e-10 (rr.judge_after_null_step, with the form's own stated factor).  constr() and the
                     current path afterwards; diagnostics()["par_scan"] must show scans settled by sweeps (entries 1 ..)
                     and none handed to the in-launch sequential recursion (entry 0).
and in each of them
  generate_x_seq(q=)              the sequential path pass                                 -> x_seq
  set_state, generate_x_seq()     k_path_par seeded with the form's stored trajectories    -> x_seq; sweeps >= 1 per chain
  update_x_obs_seq                                                                         -> x_obs
  constr()                        the form's own forward scan (one partition)              -> c
  lmult_ / rmult_by_jacob_constr  (one partition)                                          -> J w, J^T lam at 1e-9
On sir_12x8 constr() under CHMC_RETRACT_KERNEL = 0, 1, 2.  predict_device with kept paths on fhn_3x8 and sir_3x8: the
replicates' normals are read back with fill_normal under the documented key and must be the bits the fixture was continued
with (device_normals.npz: read from the library on an MI355X, an input of the generator); state channels and the obs_func
channel.  The stored-rows families (CHMC_COMPACT_ROWS=0, CHMC_GRAM_MFMA=1) are latched per process: one child each, under a
time limit, nothing started after a failure.

No entry of any case is skipped or masked."""
import os
import subprocess
import sys

import numpy as np
import pytest

import reference_runs as rr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FORMS = {"default": {}, "no_fwd_scan": {"CHMC_NO_FWD_SCAN": "1"}}
SWITCHES = ("CHMC_PAR_SCAN", "CHMC_PAR_WAVES", "CHMC_NO_FWD_SCAN", "CHMC_RETRACT_KERNEL")


def set_form(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def device_ctx(cid):
    ctx = rr.make_ctx(cid)
    assert ctx.on_gpu
    return ctx


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cid", rr.CASES)
def test_device_forms(monkeypatch, cid, form):
    set_form(monkeypatch, FORMS[form])
    ctx = device_ctx(cid)
    d0 = ctx.diagnostics()
    rr.judge_context("hip:" + form, cid, ctx)
    # the current states' path: k_path_par, seeded with the trajectories this form's forward scan stored
    x, sw = ctx.generate_x_seq(return_sweeps=True)
    d1 = ctx.diagnostics()
    assert d1["path_par_launches"] == d0["path_par_launches"] + 1, (d0, d1)
    assert (sw >= 1).all(), f"k_path_par handed chains to the sequential recursion: sweeps {sw.tolist()}"
    rr.judge("hip:" + form + ":k_path_par", cid, "x_seq", x)
    ctx.close()


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("cid", rr.CASES)
def test_time_parallel_scan_after_a_null_step(monkeypatch, cid, waves):
    """k_fwd_par<W> on a fixture point (rr.judge_after_null_step).  CHMC_RETRACT_KERNEL=0: the lock-step rounds, whose scans
    count in diagnostics()["par_scan"], also for the one 16-row block per chain of sir_12x8."""
    set_form(monkeypatch, {"CHMC_PAR_SCAN": "1", "CHMC_PAR_WAVES": str(waves), "CHMC_RETRACT_KERNEL": "0"})
    ctx = rr.make_ctx(cid, per_chain_data=True)
    assert ctx.on_gpu
    _, sw = rr.judge_after_null_step(f"hip:par_w{waves}", cid, ctx)
    ps = ctx.diagnostics()["par_scan"]
    print(f"  {cid} W={waves}: par_scan[0] {int(ps[0])}, settled after s + 1 sweeps {ps[1:16].tolist()}, k_path_par sweeps {sw.tolist()}")
    assert int(ps[0]) == 0, f"scans handed to the in-launch sequential recursion: {int(ps[0])}"
    assert int(ps[1:48].sum()) > 0, "no time-parallel scan settled: k_fwd_par did not run"
    assert (sw >= 1).all(), sw
    ctx.close()


@pytest.mark.parametrize("kernel", ["0", "1", "2"])
def test_constr_under_the_per_chain_kernel_layouts(monkeypatch, kernel):
    """sir_12x8: one 16-row block per chain, the layout of the per-chain kernels."""
    set_form(monkeypatch, {"CHMC_RETRACT_KERNEL": kernel})
    ctx = device_ctx("sir_12x8")
    assert ctx.RM == 16 and ctx.K == [1]
    rr.judge_context(f"hip:retract_kernel_{kernel}", "sir_12x8", ctx, paths=False)
    ctx.close()


@pytest.mark.parametrize("cid", rr.PREDICT_CASES)
def test_predict_device_continues_the_path(monkeypatch, cid):
    """n_rep replicate futures over one observation interval beyond the last observation, every step emitted."""
    from manifold_mcmc_for_diffusions_amd.paths import PredictivePosterior
    set_form(monkeypatch, {})
    f, P = rr.load(cid), rr.PREDICT
    ctx = device_ctx(cid)
    ctx.set_state(rr.q_of(f), None, np.ascontiguousarray(f["x_obs"]), 0)
    W = rr.predict_normals(ctx, f["pred_W"].shape[2])
    np.testing.assert_array_equal(W, f["pred_W"], err_msg="fill_normal no longer gives the normals the fixture was continued with")
    pp = PredictivePosterior(ctx, P["horizon"], P["stride"], P["n_rep"], "end", n_keep=P["n_rep"])
    pp.update(P["seed"], P["draw"], P["offset"])
    dev = pp.last_paths()
    X = ctx.X
    assert dev.shape == f["pred_x"].shape[:3] + (X + 2,)
    rr.judge("hip:predict_device", cid, "pred_x", dev[..., :X])
    rr.judge("hip:predict_device", cid, "pred_obs", dev[..., X:X + 1])
    ctx.close()


_FAMILY_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import reference_runs as rr
for cid in rr.CASES:
    if rr.single_partition(rr.load(cid)):
        ctx = rr.make_ctx(cid)
        assert ctx.on_gpu
        rr.judge_context("hip:" + {label!r}, cid, ctx)
        ctx.generate_x_seq()
        d = ctx.diagnostics()
        # the Gram blocks of the state evaluation come from the matrix cores exactly under CHMC_GRAM_MFMA=1; with
        # CHMC_COMPACT_ROWS=0 there are no compact rows and the current path comes from the sequential pass
        assert (d["gram_mfma_launches"] > 0) == {mfma}, ("gram", d["gram_mfma_launches"], d["gram_valu_launches"])
        assert {mfma} or (d["path_par_launches"] == 0 and d["path_seq_launches"] == 2), ("path", d["extra"])
        ctx.close()
print("FAMILY_OK")
"""


def test_stored_rows_families():
    """CHMC_COMPACT_ROWS=0, then CHMC_GRAM_MFMA=1: the cases with one partition, paths, c, J w and J^T lam."""
    for label, env in (("compact_rows_0", {"CHMC_COMPACT_ROWS": "0"}), ("gram_mfma_1", {"CHMC_GRAM_MFMA": "1"})):
        script = _FAMILY_SCRIPT.format(root=ROOT, tests=HERE, label=label, mfma=label == "gram_mfma_1")
        clean = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        r = subprocess.run([sys.executable, "-c", script], env={**clean, **env}, capture_output=True, text=True, timeout=120)
        print(r.stdout[-6000:])
        assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
        assert "FAMILY_OK" in r.stdout
