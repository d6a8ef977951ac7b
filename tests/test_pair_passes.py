"""Paired Newton passes (KernelPlan::pair_passes, csrc/chmc_plan.h): in a round of a paired loop in which both problems still
iterate, the interval sums, the combine, the solve and the J^T lambda update run ONCE for both problems (k_newton_ivl_pair,
k_newton_comb_pair, k_newton_fsm_wave_pair, k_colmax_pair<KUpdatePBPair>) instead of once per problem.  Each problem's
arithmetic and its order are untouched, so every comparison is BITWISE: the default call against CHMC_PAIR_PASSES=0 (paired
loop, one launch per problem and pass) and against CHMC_PAIR_RETRACT=0 (a loop per retraction).  Both switches are read on
entry to every call.  The sequencing cases (a problem that finishes or fails early, so that a round falls back to the single
passes) are test_pair_retractions.py's test_discarded_speculation_hip and test_forward_retraction_fails_at_a_later_step_hip,
which run the merged passes by default."""
import functools
import os

import numpy as np
import pytest
import test_pair_retractions as tpr
from helpers import make_case, make_ctx
from test_pair_retractions import assert_bitwise, batch_inputs, run

pytestmark = pytest.mark.gpu

B = 70
SOLVER = dict(max_iters=12)
CASES = [  # (model, T, S, R, noisy)
    ("fhn", 10, 8, 5, True),     # 7 row slots; S below one tile
    ("fhn", 12, 16, 5, False),   # 6 row slots
    ("fhn", 6, 72, 5, True),     # two tiles, the second partial
    ("fhn", 4, 136, 2, True),    # 8 row slots, K = 2 and 3, three tiles
    ("sir", 6, 16, 2, True),     # the other model on 8 slots
]
MERGED_ROUNDS = 5  # chmc_ctx::diag[9] within `extra` (out80[68 ..]) of ChmcContext.diagnostics()


def _id(case):
    model, T, S, R, noisy = case
    return f"{model}-T{T}-S{S}-R{R}-{'noisy' if noisy else 'noiseless'}"


def _params():
    for case in CASES:
        for part in (0, 1):
            for n_steps in (2, 5):
                yield pytest.param(case, part, n_steps, id=f"{_id(case)}-p{part}-n{n_steps}")


def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


def _run(case, part, n_steps, passes, pair):
    """test_pair_retractions.run with CHMC_PAIR_PASSES set as well; the merged-round counter of its first call is added to the
    result's diagnostics (run reads the diagnostics right before and right after that call)."""
    seen = []

    def recording_ctx(c, **kw):
        ctx = make_ctx(c, **kw)
        read = ctx.diagnostics

        def diagnostics():
            d = read()
            seen.append(d)
            return d

        ctx.diagnostics = diagnostics
        return ctx

    dts, active = batch_inputs()
    old = os.environ.pop("CHMC_PAIR_PASSES", None)
    if passes is not None:
        os.environ["CHMC_PAIR_PASSES"] = passes
    saved = tpr.make_ctx
    tpr.make_ctx = recording_ctx
    try:
        res = run(make_case(*case, B=B, seed=21), dts, n_steps, active, part, True, pair, SOLVER)
    finally:
        tpr.make_ctx = saved
        os.environ.pop("CHMC_PAIR_PASSES", None)
        if old is not None:
            os.environ["CHMC_PAIR_PASSES"] = old
    res["diag"]["merged_rounds"] = int(seen[1]["extra"][MERGED_ROUNDS] - seen[0]["extra"][MERGED_ROUNDS])
    return res


@functools.lru_cache(maxsize=None)
def _three(case, part, n_steps):
    """The three settings of one case, computed once for the tests below (nothing changes them afterwards)."""
    _hip()
    return {"default": _run(case, part, n_steps, None, None), "passes0": _run(case, part, n_steps, "0", None),
            "retract0": _run(case, part, n_steps, None, "0")}


@pytest.mark.parametrize("case,part,n_steps", _params())
def test_merged_passes_are_bitwise_the_single_ones(case, part, n_steps):
    res = _three(case, part, n_steps)
    assert_bitwise(res["default"], res["passes0"])
    assert_bitwise(res["default"], res["retract0"])
    r = res["retract0"]["r"]
    assert r["status"][3] == -1 and r["n_done"][3] == 0 and r["status"][4] > 0 and r["n_done"][4] == 0


@pytest.mark.parametrize("case,part,n_steps", _params())
def test_the_merged_kernels_did_the_work(case, part, n_steps):
    d = {k: v["diag"] for k, v in _three(case, part, n_steps).items()}
    print(f"  merged rounds / paired rounds: default {d['default']['merged_rounds']} / {d['default']['pair_scan_rounds']}, "
          f"CHMC_PAIR_PASSES=0 {d['passes0']['merged_rounds']} / {d['passes0']['pair_scan_rounds']}, "
          f"CHMC_PAIR_RETRACT=0 {d['retract0']['merged_rounds']} / {d['retract0']['pair_scan_rounds']}")
    assert d["default"]["merged_rounds"] == d["default"]["pair_scan_rounds"] > 0
    assert d["passes0"]["merged_rounds"] == 0 and d["passes0"]["pair_scan_rounds"] == d["default"]["pair_scan_rounds"]
    assert d["retract0"]["merged_rounds"] == 0 and d["retract0"]["pair_scan_rounds"] == 0


def test_chains_leave_one_problem_before_the_other():
    """The case the merged kernels can get wrong: a chain still in one problem's loop and already out of the other's.  It is a
    property of the inputs, so it is asserted on the UNPAIRED result: two single-step calls from the same start, the second
    for the chains the first completed, give per chain the iterations of step 1's reverse retraction and of step 2's forward
    one -- the two loops of the pair.  Over the four FitzHugh-Nagumo cases and both partitions at least 3 chains that complete
    both steps need more rounds in the reverse loop and at least 3 more in the forward one (the host emulation: 9 and 13, with
    68 of the 70 chains completing in every run)."""
    _hip()
    more_bwd = more_fwd = 0
    old = os.environ.get("CHMC_PAIR_RETRACT")
    os.environ["CHMC_PAIR_RETRACT"] = "0"
    try:
        for case in CASES[:4]:
            for part in (0, 1):
                c = make_case(*case, B=B, seed=21)
                dts, active = batch_inputs()
                qq, xx = np.repeat(c["q"][:1], B, 0), np.repeat(c["x_obs"][:1], B, 0)
                p = np.random.default_rng(17).standard_normal(qq.shape)
                ctx = make_ctx(c)
                ctx.set_state(qq, p, xx, part)
                ctx.project_onto_cotangent_space()
                r1 = ctx.leapfrog_steps(dts, 1, active=active, newton=True, **SOLVER)
                act2 = (r1["status"] == 0).astype(np.int32)
                r2 = ctx.leapfrog_steps(dts, 1, active=act2, newton=True, **SOLVER)
                ctx.close()
                both = (act2 == 1) & (r2["status"] == 0)
                bwd, fwd = r1["iters_bwd"][both], r2["iters_fwd"][both]
                print(f"  {_id(case)} p{part}: {both.sum()} of {B} chains complete both steps; reverse loop longer "
                      f"{(bwd > fwd).sum()}, forward loop longer {(bwd < fwd).sum()}")
                more_bwd += int((bwd > fwd).sum())
                more_fwd += int((bwd < fwd).sum())
    finally:
        os.environ.pop("CHMC_PAIR_RETRACT", None)
        if old is not None:
            os.environ["CHMC_PAIR_RETRACT"] = old
    assert more_bwd >= 3 and more_fwd >= 3, (more_bwd, more_fwd)
