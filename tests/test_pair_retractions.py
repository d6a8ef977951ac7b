"""Paired retractions (KernelPlan::pair_retractions, csrc/chmc_plan.h): inside chmc_leapfrog_steps with one n_steps for all
chains, the reverse retraction of step i and the forward retraction of step i + 1 advance in ONE lock-step Newton loop whose
forward scan is one launch for both.  Nothing about a chain's arithmetic changes, so every comparison here is BITWISE between
the paired call -- the default at these batch sizes -- and the same call with CHMC_PAIR_RETRACT=0 (the switch is read on entry
to every call).
CPU: the TEST-ONLY emulation build (the sequencing, two functor launches in place of the merged scan); `-m gpu`: the HIP
library (k_fwd_scan<.., PAIR>)."""
import os

import numpy as np
import pytest
from helpers import make_case, make_ctx
from test_emu_logic import emu_lib  # noqa: F401

SOLVER = dict(max_iters=12)
B = 70  # 70 K blocks per problem: each problem ends in a partial scan workgroup, the pair boundary falls inside the grid


def batch_inputs(seed=5, late_failure=False, B=B):
    """Per-chain step sizes of mixed sign and size (iteration counts differ between chains and between the two loops of a
    pair), one inactive chain, one chain whose first step fails."""
    rng = np.random.default_rng(seed)
    dts = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 + 0.1 * rng.random(B))
    dts[4] = 5.0
    if late_failure:
        dts[2] = 0.6  # (its forward retraction fails, if at all, after its first steps)
    active = np.ones(B, dtype=np.int32)
    active[3] = 0
    return dts, active


def run(case, dts, n_steps, active, part, newton, pair, kw):
    """One trajectory call and a second one continued from the resulting state (every chain, the failed ones included, with
    small steps), from identical start states; `pair`: CHMC_PAIR_RETRACT of both calls (None: unset, the default)."""
    B = case["B"]
    rng = np.random.default_rng(17)
    qq = np.repeat(case["q"][:1], B, 0)
    xx = np.repeat(case["x_obs"][:1], B, 0)
    p = rng.standard_normal(qq.shape)
    old = os.environ.get("CHMC_PAIR_RETRACT")
    os.environ.pop("CHMC_PAIR_RETRACT", None)
    if pair is not None:
        os.environ["CHMC_PAIR_RETRACT"] = pair
    try:
        ctx = make_ctx(case)
        ctx.set_state(qq, p, xx, part)
        ctx.project_onto_cotangent_space()
        d0, c0 = ctx.diagnostics(), ctx.counters()["projection_iterations"]
        r = ctx.leapfrog_steps(dts, n_steps, active=active, newton=newton, **kw)
        d1, c1 = ctx.diagnostics(), ctx.counters()["projection_iterations"]
        q1, p1, _, _ = ctx.get_state()
        h1 = ctx.hamiltonian()
        r2 = ctx.leapfrog_steps(np.where(np.arange(B) % 3 == 0, -0.03, 0.04), 2, newton=newton, **kw)
        q2, p2, _, _ = ctx.get_state()
        h2 = ctx.hamiltonian()
        ctx.close()
    finally:
        os.environ.pop("CHMC_PAIR_RETRACT", None)
        if old is not None:
            os.environ["CHMC_PAIR_RETRACT"] = old
    diag = {k: d1[k] - d0[k] for k in ("pair_scan_rounds", "newton_scan_launches", "newton_rounds")}
    diag["projection_iterations"] = c1 - c0
    return dict(r=r, q=q1, p=p1, h=h1, r2=r2, q2=q2, p2=p2, h2=h2, diag=diag)


def assert_bitwise(a, b):
    for res in ("r", "r2"):
        for k in ("n_done", "status", "iters_fwd", "iters_bwd", "rev_err"):
            np.testing.assert_array_equal(a[res][k], b[res][k], err_msg=res + "." + k)
    for k in ("q", "p", "h", "q2", "p2", "h2"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def compare(case, n_steps, part=0, newton=True, late_failure=False, merged_scan=False, most_complete=True,
            rounds_must_match=False, **kw):
    """The paired against the unpaired call; returns the unpaired result.  merged_scan: the forward scans are k_fwd_scan
    launches (HIP library, S % 8 == 0), so the launch counts follow from the rounds.
    A paired problem is enqueued for the rounds a loop of its own would have been (run_lockstep, csrc/chmc_api.inc): the
    call's enqueued and counted rounds equal the unpaired call's unless a chain failed late -- after a completed step or in
    a reverse retraction: it has then taken part in a forward retraction of the next step that the unpaired call never
    runs.  rounds_must_match: the case is known to have no such chain, so it must take the asserting branch."""
    dts, active = batch_inputs(late_failure=late_failure)
    kw = {**SOLVER, **kw}
    a = run(case, dts, n_steps, active, part, newton, None, kw)
    b = run(case, dts, n_steps, active, part, newton, "0", kw)
    assert_bitwise(a, b)
    r = b["r"]
    assert r["status"][3] == -1 and r["n_done"][3] == 0 and r["status"][4] > 0 and r["n_done"][4] == 0
    assert not most_complete or (r["n_done"] == n_steps).sum() > B // 2
    # paired rounds ran exactly when there was a step to pair with; the switch removes them
    assert b["diag"]["pair_scan_rounds"] == 0
    assert (a["diag"]["pair_scan_rounds"] > 0) == (n_steps >= 2)
    if merged_scan:  # one scan launch per enqueued round and problem, a paired round's launch serving two
        for d in (a["diag"], b["diag"]):
            assert d["newton_scan_launches"] == d["newton_rounds"] - d["pair_scan_rounds"]
        if n_steps >= 2:
            assert a["diag"]["newton_scan_launches"] < b["diag"]["newton_scan_launches"]
        # a pair runs as long as its longer loop, at least 2 rounds; n_steps - 1 pairs
        assert a["diag"]["pair_scan_rounds"] >= 2 * (n_steps - 1)
    failed_late = (r["status"] > 0) & ((r["n_done"] > 0) | (r["iters_bwd"] > 0))
    print(f"  rounds enqueued / counted: paired {a['diag']['newton_rounds']} / {a['diag']['projection_iterations']}, unpaired "
          f"{b['diag']['newton_rounds']} / {b['diag']['projection_iterations']}; chains that failed late: {failed_late.sum()}")
    assert not (rounds_must_match and failed_late.any()), np.flatnonzero(failed_late)
    if not failed_late.any():
        for k in ("newton_rounds", "projection_iterations"):
            assert a["diag"][k] == b["diag"][k], k
    return b


SHAPES = [("fhn", 10, 8, 5, True, False), ("fhn", 12, 16, 5, True, False)]
# one case each: FitzHugh-Nagumo noiseless, partitioned SIR with R = 2, Gaussian splitting
OTHERS = [("fhn", 12, 16, 5, False, False), ("sir", 6, 16, 2, True, False), ("fhn", 7, 8, 3, False, True)]
# Nine steps: the loops predict from the fourth step on, and a predicting problem of a pair ends early (when the pair had
# a loop of its own it kept different books there: at the SIR shape, partition 0, its call enqueued 84 rounds against 80)
PREDICTING = [("sir", 6, 16, 2, True, False), ("fhn", 7, 8, 3, False, True)]
# 16 row slots with several blocks per chain, SIR at 0.05 between observations (k_fwd_scan<SirModel, 16, .., PAIR>; pair_alloc sizes a
# second set of 16-row work arrays): K = [4, 5] -- interval-parallel and stored-rows state evaluation -- and K = [5, 6] with 9 rows
# in 16 slots.  On the emulation build 68 of the 70 chains complete (the masked chain has status -1, the failing one status 2).
SIR16 = [("sir", 40, 8, 10, True, False), ("sir", 30, 8, 6, True, False)]
SIR16_INTERVAL = 0.05
# Reversibility tolerance of the discarded-speculation case, chosen with the emulation build at SHAPES[0], 5 steps: the
# reverse-check distances of a step lie between 1.3e-15 and 8.3e-15 there (the retractions converge to rounding), and at 5e-15
# 36 chains fail the check (status 3) after at least one good step -- their forward retraction of the next step has run beside
# the reverse one and is never adopted -- while 29 complete all five (3e-15: 31 and 1; 8e-15: 4 and 64).
REV_TOL = 5e-15


def _cases(n_steps_list, shapes):
    for model, T, S, R, noisy, gaussian in shapes:
        for part in range(2 if R and R < T else 1):
            for n in n_steps_list:
                yield pytest.param(model, T, S, R, noisy, gaussian, part, n, id=f"{model}-T{T}-S{S}-R{R}-"
                                   f"{'noisy' if noisy else 'noiseless'}{'-gauss' if gaussian else ''}-p{part}-n{n}")


def _check_all(model, T, S, R, noisy, gaussian, part, n_steps, merged_scan, obs_interval=None, **kw):
    case = make_case(model, T, S, R, noisy, B=B, seed=21, gaussian=gaussian, obs_interval=obs_interval)
    return compare(case, n_steps, part=part, merged_scan=merged_scan, **kw)


def _discarded_speculation(merged_scan):
    case = make_case(*SHAPES[0][:5], B=B, seed=21)
    b = compare(case, 5, part=0, merged_scan=merged_scan, most_complete=False, reverse_check_tol=REV_TOL)
    r = b["r"]
    rejected = (r["status"] == 3) & (r["n_done"] >= 1)
    assert rejected.any() and ((r["status"] == 0) & (r["n_done"] == 5)).any(), (r["status"], r["n_done"])


def _late_forward_failure(merged_scan):
    case = make_case(*SHAPES[0][:5], B=B, seed=21)
    b = compare(case, 5, part=0, late_failure=True, merged_scan=merged_scan)
    r = b["r"]
    assert r["status"][2] in (1, 2) and 1 <= r["n_done"][2] < 5, (r["status"][2], r["n_done"][2])


# ---------------------------------------------------------------------------------------------------- emulation build
@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((1, 2, 5), SHAPES))
def test_paired_equals_unpaired(emu_lib, model, T, S, R, noisy, gaussian, part, n_steps):  # noqa: F811
    _check_all(model, T, S, R, noisy, gaussian, part, n_steps, False, rounds_must_match=True)


@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((3,), OTHERS))
def test_paired_equals_unpaired_other_models(emu_lib, model, T, S, R, noisy, gaussian, part, n_steps):  # noqa: F811
    _check_all(model, T, S, R, noisy, gaussian, part, n_steps, False, rounds_must_match=True)


@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((9,), PREDICTING))
def test_paired_problem_is_enqueued_as_in_a_loop_of_its_own(emu_lib, model, T, S, R, noisy, gaussian, part, n_steps):  # noqa: F811
    _check_all(model, T, S, R, noisy, gaussian, part, n_steps, False, rounds_must_match=True)


@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((2, 5), SIR16))
def test_paired_equals_unpaired_sixteen_row_blocks(emu_lib, model, T, S, R, noisy, gaussian, part, n_steps):  # noqa: F811
    b = _check_all(model, T, S, R, noisy, gaussian, part, n_steps, False, obs_interval=SIR16_INTERVAL)
    assert (b["r"]["n_done"] == n_steps).sum() == B - 2


def test_paired_equals_unpaired_quasi_newton(emu_lib):  # noqa: F811
    case = make_case(*SHAPES[0][:5], B=B, seed=21)
    compare(case, 3, newton=False)


def test_discarded_speculation(emu_lib):  # noqa: F811
    _discarded_speculation(False)


def test_forward_retraction_fails_at_a_later_step(emu_lib):  # noqa: F811
    _late_forward_failure(False)


# ---------------------------------------------------------------------------------------------------- HIP library
def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


@pytest.mark.gpu
@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((1, 2, 5), SHAPES))
def test_paired_equals_unpaired_hip(model, T, S, R, noisy, gaussian, part, n_steps):
    _hip()
    _check_all(model, T, S, R, noisy, gaussian, part, n_steps, True)


@pytest.mark.gpu
@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((3,), OTHERS))
def test_paired_equals_unpaired_other_models_hip(model, T, S, R, noisy, gaussian, part, n_steps):
    _hip()
    _check_all(model, T, S, R, noisy, gaussian, part, n_steps, True)


@pytest.mark.gpu
@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((9,), PREDICTING))
def test_paired_problem_is_enqueued_as_in_a_loop_of_its_own_hip(model, T, S, R, noisy, gaussian, part, n_steps):
    _hip()
    _check_all(model, T, S, R, noisy, gaussian, part, n_steps, True, rounds_must_match=True)


@pytest.mark.gpu
@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,part,n_steps", _cases((2, 5), SIR16))
def test_paired_equals_unpaired_sixteen_row_blocks_hip(model, T, S, R, noisy, gaussian, part, n_steps):
    _hip()
    b = _check_all(model, T, S, R, noisy, gaussian, part, n_steps, True, obs_interval=SIR16_INTERVAL)
    print(f"  chains that completed all {n_steps} steps: {(b['r']['n_done'] == n_steps).sum()} of {B}")


@pytest.mark.gpu
def test_paired_equals_unpaired_quasi_newton_hip():
    _hip()
    case = make_case(*SHAPES[0][:5], B=B, seed=21)
    compare(case, 3, newton=False, merged_scan=True)


@pytest.mark.gpu
def test_discarded_speculation_hip():
    _hip()
    _discarded_speculation(True)


@pytest.mark.gpu
def test_forward_retraction_fails_at_a_later_step_hip():
    _hip()
    _late_forward_failure(True)


@pytest.mark.gpu
def test_a_batch_whose_merged_scan_does_not_fit_the_chip_hip():
    """The choice per call (pair_this_call, csrc/chmc_plan.h): the merged scan has 2 ceil(B K / 64) workgroups and a call pairs
    by default only while each has a compute unit to itself -- 2 800 chains of 3 blocks are 264 workgroups on at most 256
    compute units.  CHMC_PAIR_RETRACT=1 pairs all the same, with the same bits."""
    _hip()
    Bb = 2800
    case = make_case(*SHAPES[1][:5], B=Bb, seed=21)
    dts, active = batch_inputs(B=Bb)
    res = {pair: run(case, dts, 2, active, 0, True, pair, SOLVER) for pair in (None, "1", "0")}
    assert res[None]["diag"]["pair_scan_rounds"] == 0 and res["0"]["diag"]["pair_scan_rounds"] == 0
    assert res["1"]["diag"]["pair_scan_rounds"] >= 2
    assert_bitwise(res["1"], res["0"])
    assert_bitwise(res[None], res["0"])
    assert (res["0"]["r"]["n_done"] == 2).sum() > Bb // 2
