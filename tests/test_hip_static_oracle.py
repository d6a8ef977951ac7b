"""Whole static-HMC transitions -- sampling.sample_static_chmc, unmodified -- against the C oracle, on every kernel family of
the plan (csrc/chmc_plan.h): momentum refresh, snapshot, a trajectory with per-chain step sizes and lengths, accept / reject,
restore(mask), switch_partition, and once during warm-up set_metric on the live state, repeated N_ITER times.

test_static_sampler_against_the_oracle: the sampler runs with n_head = Q, so heads[it] is every chain's full position after
every transition, and with a recorder around ctx.leapfrog_steps (on the instance, test-only).  The host stream
np.random.default_rng(seed) is restated in the sampler's order (direction; length when jittered; accept) together with the
warm-up back-off, the step size of transition `it` is the library's own step_size[it], and the recorded dt / length must equal
the restated ones bitwise.  Every transition of every chain is then replayed with helpers.oracle_static_transition from
heads[it - 1][c] (x_obs = generate_x_obs_seq(q), partition it % num_partition, the metric in force).  With no chain or
transition excused: status, n_done, iters_fwd (and iters_bwd where status is 0) and the accept decision equal; heads[it][c]
bitwise heads[it - 1][c] for a rejected or failed chain, else within 1e-9 max(1, |q|_inf) n_done of the oracle's end point;
accept_stat[it] within 1e-9 of the mean of the oracle's prob; fail_rate and chain_outcomes equal; step_size bitwise a
DualAveragingStepSize re-run on the library's accept_stat (with the reset at the metric install and final()); metric_M_0
the OnlineBlockDiagonalMetricAdapter re-run on the library's heads to 1e-10 relative, and from the next transition on the
oracle carries the installed M_0; after the run check_ops_at_current_state at 1e-10 with no unjudged chain.

test_set_metric_on_a_live_state: set_state, sample_momentum, one step, switch_partition, then set_metric(M_0) -- every operator
at the reported point against an oracle carrying M_0 (1e-10), one step from the reported (q, p) (the momentum is not tangent
for the new metric: the full projection path) with status and iteration counts equal and (q, p) to 1e-9 -- and the same after
set_metric(None).

test_sampler_does_not_depend_on_the_shard_size: 6 chains as one context against 2 x 3 chains with chain_offset and
total_chains = 6, heads and chain_outcomes bitwise chain for chain.

No decision may be a coin toss between library and oracle, so every case was screened with tools/screen_static_oracle.py (this
module's body on the emulation build): every accept draw of a complete trajectory at least 1e-6 from its probability, no
retraction residual of any iteration within 1e-2 relative of constraint_tol / position_tol, every reversibility error at least
0.5 relative from reverse_check_tol, no complete trajectory with a non-finite dh (OracleChain.trace holds the last inner step of
a step: with n_inner_step = 2 the first inner step's residuals are not screened).  The margins are asserted again at test time
on the oracle's replay, and the test then fails naming the seed.  Every case must show, in the oracle's replay, the events of
REQUIRED_EVENTS (and JITTER_EVENTS / METRIC_EVENTS where they apply) and the failing statuses its CHOSEN entry lists; across the
table statuses 1, 2 and 3 each occur (test_the_table_shows_every_failing_status).  (seed, eps0) that failed the screening:
REPLACED.

The emulation-build tests (not marked gpu) run the same bodies on the CPU: host logic only, generic functors, they say nothing
about the device's kernels.

Worst observed ratio to the bound per case on the MI355X (printed by pytest -s; sampler: accepted position, accept_stat,
operators after the run; the installed M_0 was bitwise the re-run adapter's in every metric case):
  fhn_12_16_5         0.0000 0.0002 0.0008      fhn_12_16_5_jitter         0.0000 0.0001 0.0067
  fhn_12_16_5_metric  0.0000 0.0002 0.0004      fhn_12_16_5_halves         0.0000 0.0002 0.0008
  fhn_12_16_5_inner2  0.0000 0.0001 0.0027      fhn_130_4_2                0.0000 0.0003 0.0044
  sir16_14_8 (unset, 2, 0: the same figures) 0.0001 0.0014 0.2121      fhn_6_8_2_noiseless_gauss  0.0000 0.0001 0.0064
  sir16_12_16_varsigma  0.0000 0.0008 0.0385    sir16_two_blocks           0.0001 0.0005 0.0870
  fhn16_k4_5          0.0000 0.0001 0.0010      fhn16_long_k2_3            0.0000 0.0059 0.0686
  stored rows / MFMA children: fhn_12_16_5_metric 0.0000 0.0001 0.0004 / 0.0007, sir16_14_8 0.0000 0.0016 0.1914 / 0.0004 0.0387
  live set_metric (operators with M_0, operators back at the identity, worst of the three compared steps):
    fhn_12_16_5 0.0047 0.0007 0.0000   fhn_130_4_2 0.0017 0.0011 0.0002   sir16_14_8 0.0544 0.1056 0.0025   fhn16_k4_5 0.0003 0.0006 0.0000
sir16_14_8: out80[67] = 8 (one k_traj_chain launch per transition) unset and with 2, 0 with 0; sir16_12_16_varsigma: 8.
Every status, n_done, iteration count, accept decision, fail_rate, chain_outcomes and step size was equal; no disagreement
was found, so the library is unchanged.

Perturbations tried on a scratch copy (emulation build), and what caught each: chmc_set_metric without its state_eval --
both sampler cases (iteration counts of the first trajectory under M_0, then the operators) and the live set_metric body;
chmc_set_metric keeping the tangency flag -- the live set_metric body (iteration counts of the step after set_metric(None));
restore with the mask inverted, in the sampler and in the kernel -- both sampler cases at transition 0 (accept decision);
no partition switch -- both sampler cases (iteration counts at transition 1, x_obs_seq after the run); back-off applied
outside warm-up -- both sampler cases (recorded dt).  Taking the snapshot before the momentum refresh is NOT caught, and need
not be: the restored momentum is replaced by the next refresh before anything reads it."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_ctx, check_ops_at_current_state, oracle_static_transition
from autodiff_checks import UNJUDGED, largest
from test_hip_autodiff_parity import distinct_on_manifold_chains
from test_emu_logic import emu_lib  # noqa: F401
import test_hip_tree_oracle as to

ROOT = to.ROOT
B, N_ITER, N_STEP, N_ADAPT = 5, 8, 3, 6
N_METRIC, N_SKIP = 4, 1  # sample_static_chmc's window of n_adapt = 6: draws 1..3 feed the adapter, installed after transition 3
REQUIRED_EVENTS = ("accepted", "rejected_complete", "first_step_failure", "later_step_failure", "forward", "backward",
                   "backed_off_chain_moves", "accepted_in_every_partition")
JITTER_EVENTS = ("length_1", f"length_{N_STEP}")
METRIC_EVENTS = ("accepted_2_steps_under_installed_metric",)

FHN12 = ("fhn", 12, 16, 5, True, False, False, None)
# id: layout (model, T, S, R, noisy, gaussian, var_sigma, obs_interval), expected K, jitter_length, metric adapter, environment,
#     n_inner_step
CASES = {
    "fhn_6_4_2": dict(layout=("fhn", 6, 4, 2, True, False, False, None), K=[3, 4], jitter=True, metric=True),  # (emulation only)
    "fhn_12_16_5": dict(layout=FHN12, K=[3, 3]),                       # uniform length: the call that may pair retractions (out80[70] is printed)
    "fhn_12_16_5_jitter": dict(layout=FHN12, K=[3, 3], jitter=True),
    "fhn_12_16_5_metric": dict(layout=FHN12, K=[3, 3], jitter=True, metric=True),
    "fhn_12_16_5_halves": dict(layout=FHN12, K=[3, 3], env={"CHMC_HALVES": "2"}),
    "fhn_12_16_5_inner2": dict(layout=FHN12, K=[3, 3], n_inner=2),
    "fhn_130_4_2": dict(layout=("fhn", 130, 4, 2, True, False, False, None), K=[65, 66], jitter=True),
    "fhn_6_8_2_noiseless_gauss": dict(layout=("fhn", 6, 8, 2, False, True, False, None), K=[3, 4]),
    "sir16_14_8": dict(layout=("sir", 14, 8, 14, True, False, False, None), K=[1], jitter=True, metric=True),
    "sir16_12_16_varsigma": dict(layout=("sir", 12, 16, 12, True, False, True, None), K=[1], metric=True),
    "sir16_two_blocks": dict(layout=("sir", 26, 24, 13, True, False, False, 0.1), K=[2, 3]),
    "fhn16_k4_5": dict(layout=("fhn", 40, 8, 10, True, False, False, None), K=[4, 5], RM=16, metric=True),
    # blocks of 13 x 80 = 1040 steps: the time-parallel scan (seed0: where the search starts, test_hip_fhn16.py's seed of this shape)
    "fhn16_long_k2_3": dict(layout=("fhn", 26, 80, 13, True, False, False, None), K=[2, 3], RM=16, seed0=331),
}
# the screening's choices (tools/screen_static_oracle.py --search): id: (seed, eps0, failing statuses the oracle's replay shows)
CHOSEN = {
    "fhn_6_4_2": (31, 0.3, (1, 2, 3)),
    "fhn_12_16_5": (31, 0.3, (2,)),
    "fhn_12_16_5_jitter": (131, 0.4, (2,)),
    "fhn_12_16_5_metric": (31, 0.3, (2,)),
    "fhn_12_16_5_halves": (31, 0.3, (2,)),
    "fhn_12_16_5_inner2": (31, 0.2, (2,)),
    "fhn_130_4_2": (31, 0.2, (2, 3)),
    "fhn_6_8_2_noiseless_gauss": (131, 0.2, (2,)),
    "sir16_14_8": (31, 0.3, (1, 2)),
    "sir16_12_16_varsigma": (31, 0.3, (2,)),
    "sir16_two_blocks": (31, 0.6, (2,)),
    "fhn16_k4_5": (31, 0.3, (2,)),
    "fhn16_long_k2_3": (331, 0.3, (2,)),
}
_NO_LATER = "no failure after a good step"
REPLACED = {  # id: the (seed, eps0) that failed the screening, and on what (transition, chain: relative distance from the tolerance)
    "fhn_12_16_5_jitter": {(31, 0.3): _NO_LATER, (31, 0.2): "4, 0: position_tol 5.4e-03", (31, 0.4): _NO_LATER,
                           (31, 0.15): "2, 2: position_tol 3.1e-03", (31, 0.6): "4, 3: constraint_tol 4.2e-04",
                           (31, 0.1): "4, 0: position_tol 8.6e-03", (31, 0.8): "4, 2: constraint_tol 7.1e-03",
                           (131, 0.3): "4, 3: constraint_tol 1.3e-03", (131, 0.2): _NO_LATER},
    "fhn_12_16_5_inner2": {(31, 0.3): "no failure at the first step"},
    "fhn_130_4_2": {(31, 0.3): "5, 2: position_tol 2.9e-03"},
    "fhn_6_8_2_noiseless_gauss": {(31, 0.3): _NO_LATER, (31, 0.2): "0, 0: constraint_tol 4.3e-03", (31, 0.4): "0, 3: constraint_tol 6.6e-03",
                                  (31, 0.15): "2, 1: constraint_tol 1.6e-03", (31, 0.6): "no complete rejection; " + _NO_LATER,
                                  (31, 0.1): "no complete rejection; " + _NO_LATER, (31, 0.8): "no complete rejection; " + _NO_LATER,
                                  (131, 0.3): "0, 1: position_tol 4.2e-03"},
    "sir16_two_blocks": {(31, 0.3): _NO_LATER, (31, 0.2): _NO_LATER, (31, 0.4): "4, 2: constraint_tol 5.1e-04", (31, 0.15): _NO_LATER},
}
GPU_CASES = [n for n in CASES if n != "fhn_6_4_2"]
EMU_CASES = ["fhn_6_4_2", "sir16_14_8"]
# test_set_metric_on_a_live_state: id: (seed of the chains, momenta draw, step-size scale), screened like the cases
LIVE_METRIC = {
    "fhn_12_16_5": (31, 1, 0.25),
    "fhn_130_4_2": (131, 1, 0.25),
    "sir16_14_8": (31, 1, 0.25),
    "fhn16_k4_5": (31, 1, 0.25),
}
SHARD = dict(seed=31, eps0=0.3, n_iter=6)  # test_sampler_does_not_depend_on_the_shard_size on fhn_12_16_5's layout
_MEMO = {}  # oracle_static_transition by its exact inputs: contexts that agree bitwise share the oracle's side


def cfg_of(name):
    cfg = dict(metric=False, jitter=False, env={}, n_inner=1, RM=None, name=name)
    cfg.update(CASES[name])
    if name in CHOSEN:
        cfg["seed"], cfg["eps0"], cfg["statuses"] = CHOSEN[name]
    return cfg


def required_events(cfg):
    return REQUIRED_EVENTS + (JITTER_EVENTS if cfg["jitter"] else ()) + (METRIC_EVENTS if cfg["metric"] else ())


def _replay(name, osys, q, part, c, seed, draw, M0, dt, length, u, solver):
    key = (name, q.tobytes(), part, c, seed, draw, None if M0 is None else M0.tobytes(), float(dt), int(length), float(u),
           tuple(sorted(solver.items())))
    if key not in _MEMO:
        _MEMO[key] = oracle_static_transition(osys, q, osys.generate_x_obs_seq(q), part, c, seed, draw, M0, dt, length, u, solver)
    return _MEMO[key]


def recorded(ctx):
    """Wraps ctx.leapfrog_steps ON THE INSTANCE with a recorder of every call's dt, length, active and returned dict (copies:
    the sampler updates `active` in place after the call).  Returns the list the calls are appended to."""
    calls, inner = [], ctx.leapfrog_steps

    def leapfrog_steps(dt, n_steps, active=None, **kw):
        before = dict(dt=np.array(dt, copy=True), length=np.array(n_steps, copy=True), active=np.array(active, copy=True), kw=dict(kw))
        r = inner(dt, n_steps, active=active, **kw)
        calls.append(dict(before, r={k: np.array(v, copy=True) for k, v in r.items()}))
        return r

    ctx.leapfrog_steps = leapfrog_steps
    return calls


def static_body(ctx, case, cfg, seed=None, eps0=None, screening=False):
    """Everything test_static_sampler_against_the_oracle checks on one context.  Returns (worst ratios to the bounds, events,
    failing statuses, problems): `problems` lists the oracle's own near-edge margins and the missing events -- asserted empty
    unless `screening`, where the caller reads them.  A disagreement between library and oracle always raises."""
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc, DualAveragingStepSize
    from manifold_mcmc_for_diffusions_amd.adapters import OnlineBlockDiagonalMetricAdapter
    osys, name = case["osys"], cfg["name"]
    seed = cfg["seed"] if seed is None else seed
    eps0 = cfg["eps0"] if eps0 is None else eps0
    solver = to.solver_of(cfg)
    assert ctx.K == cfg["K"] and ctx.B == B and (cfg["RM"] is None or ctx.RM == cfg["RM"]), (ctx.K, ctx.RM)
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    calls = recorded(ctx)
    try:
        res = sample_static_chmc(ctx, N_ITER, N_STEP, eps0, seed, n_adapt=N_ADAPT, solver=solver, n_head=ctx.Q,
                                 jitter_length=cfg["jitter"],
                                 metric_adapter=OnlineBlockDiagonalMetricAdapter(ctx.U) if cfg["metric"] else None)
    finally:
        del ctx.leapfrog_steps
    heads = res["heads"]
    assert heads.shape == (N_ITER, B, ctx.Q) and len(calls) == N_ITER
    worst = dict(position=0.0, accept_stat=0.0, metric=0.0, ops=0.0)
    events, statuses, problems = set(), set(), []
    rng = np.random.default_rng(seed)
    stuck, outcome = np.zeros(B, dtype=np.int64), np.zeros((B, 5), dtype=np.int64)
    adapter, eps = DualAveragingStepSize(eps0), eps0
    metric_adapter, metric_state, M0 = OnlineBlockDiagonalMetricAdapter(ctx.U), None, None
    accepted_parts, prev, log = set(), case["q"], []
    try:
        for it in range(N_ITER):
            # the host's side of the transition, restated
            assert res["step_size"][it] == eps, (it, res["step_size"][it], eps)
            scale = 0.5 ** np.minimum(stuck, 8) if it < N_ADAPT else np.ones(B)
            dt = np.where(rng.random(B) < 0.5, eps, -eps) * scale
            length = 1 + np.floor(rng.random(B) * N_STEP).astype(np.int32) if cfg["jitter"] else np.full(B, N_STEP, dtype=np.int32)
            u = rng.random(B)
            call = calls[it]
            assert call["dt"].dtype == np.float64 and np.array_equal(call["dt"], dt), (it, call["dt"], dt)
            assert np.array_equal(np.broadcast_to(call["length"], (B,)), length), (it, call["length"], length)
            assert (call["length"].ndim == 1) == cfg["jitter"] and np.array_equal(call["active"], np.ones(B, dtype=np.int32))
            assert {k: call["kw"][k] for k in solver} == solver and set(call["kw"]) == set(solver), call["kw"]
            part = it % osys.num_partition
            # the device's side, chain by chain
            rs = [_replay(name, osys, prev[c], part, c, seed, it + 1, M0, dt[c], length[c], u[c], solver) for c in range(B)]
            got = call["r"]
            for c, r in enumerate(rs):
                bad = to.admissible(r["margins"])
                if bad:
                    problems.append(f"seed {seed} eps0 {eps0}: transition {it} chain {c}: the oracle's own margins {bad} (screening)")
                have = (got["status"][c], got["n_done"][c], got["iters_fwd"][c], got["iters_bwd"][c] if r["status"] == 0 else None)
                want = (r["status"], r["n_done"], r["iters_fwd"], r["iters_bwd"] if r["status"] == 0 else None)
                assert have == want, (it, c, have, want)
                moved = not np.array_equal(heads[it][c], prev[c])
                assert moved == r["accepted"], (it, c, moved, r["accepted"], r["prob"], u[c])
                if r["accepted"]:
                    bound = 1e-9 * max(1.0, np.abs(r["q"]).max()) * r["n_done"]
                    e_q = np.abs(heads[it][c] - r["q"]).max()
                    worst["position"] = max(worst["position"], e_q / bound)
                    assert e_q <= bound, (it, c, e_q, bound)
                # the events this transition shows
                if r["status"] > 0:
                    statuses.add(r["status"])
                    events.add("first_step_failure" if r["n_done"] == 0 else "later_step_failure")
                else:
                    events.add("accepted" if r["accepted"] else "rejected_complete")
                    events.add(f"length_{r['n_done']}")
                events.add("forward" if dt[c] > 0 else "backward")
                if r["accepted"]:
                    accepted_parts.add(part)
                    if scale[c] < 1.0:
                        events.add("backed_off_chain_moves")
                    if M0 is not None and r["n_done"] >= 2:
                        events.add("accepted_2_steps_under_installed_metric")
            log.append("".join("A" if r["accepted"] else "r" if r["status"] == 0 else str(r["status"]) for r in rs))
            prob = np.array([r["prob"] for r in rs])
            act = np.array([r["status"] == 0 for r in rs]).astype(np.int32)
            e_acc = abs(res["accept_stat"][it] - prob.sum() / B)
            worst["accept_stat"] = max(worst["accept_stat"], e_acc / 1e-9)
            assert e_acc <= 1e-9, (it, res["accept_stat"][it], prob)
            assert res["fail_rate"][it] == 1.0 - act.mean(), (it, res["fail_rate"][it], act)
            stuck = np.where(prob > 0.0, 0, stuck + 1)
            if it >= N_ADAPT:
                for c, r in enumerate(rs):
                    outcome[c, 1 + min(max(r["status"], 1), 3) if r["status"] > 0 else 0 if r["accepted"] else 1] += 1
            prev = heads[it]
            # the adapters, re-run on what the library reports
            if cfg["metric"] and N_SKIP <= it < N_METRIC:
                if metric_state is None:
                    metric_state = metric_adapter.initialize(np.zeros((B, ctx.Q)))
                metric_adapter.update(metric_state, heads[it])
                if it == N_METRIC - 1:
                    want = metric_adapter.finalize(metric_state).blocks[0].array
                    M0 = res["metric_M_0"]
                    worst["metric"] = float(np.abs(M0 / want - 1.0).max() / 1e-10)
                    np.testing.assert_allclose(M0, want, rtol=1e-10, atol=0)
                    assert np.array_equal(ctx.M_0, M0)
                    osys.set_metric(M0)  # (the metric the device carries from the next transition on)
                    adapter = DualAveragingStepSize(eps)
            if it < N_ADAPT:
                eps = adapter.update(res["accept_stat"][it])
                if it == N_ADAPT - 1:
                    eps = adapter.final()
        assert res["final_step_size"] == eps, (res["final_step_size"], eps)
        assert np.array_equal(res["chain_outcomes"], outcome), (res["chain_outcomes"], outcome)
        assert ("metric_M_0" in res) == cfg["metric"] and (M0 is not None) == cfg["metric"]
        w = check_ops_at_current_state(ctx, osys)
        assert w[UNJUDGED] == 0, w
        worst["ops"] = largest(w) / 1e-10
    finally:
        osys.set_metric(None)
    if len(accepted_parts) == osys.num_partition:
        events.add("accepted_in_every_partition")
    missing = [e for e in required_events(cfg) if e not in events]
    if missing:
        problems.append(f"seed {seed} eps0 {eps0}: the oracle's replay does not show {missing}")
    if "statuses" in cfg and not screening and tuple(sorted(statuses)) != tuple(cfg["statuses"]):
        problems.append(f"seed {seed} eps0 {eps0}: failing statuses {sorted(statuses)}, the table says {cfg['statuses']}")
    print(f"  static: worst ratio to the bound {({k: round(v, 4) for k, v in worst.items()})}; statuses {sorted(statuses)}; "
          f"per transition (A accepted, r rejected, digit: failing status) {' '.join(log)}; step sizes "
          f"{np.round(res['step_size'], 4).tolist()}; events {sorted(events)}")
    assert screening or not problems, problems
    return worst, events, statuses, problems


def oracle_margins_of_step(osys, q, p, xo, part, dt):
    """The admission margins of one oracle step from (q, p): constraint_tol, position_tol, reverse_check (module docstring)."""
    from oracle import c_oracle
    ch = c_oracle.OracleChain(osys)
    ch.set(q, p, xo, part)
    st, _, _, rev = ch.step(dt)
    m = {"reverse_check": abs(rev - 2e-8) / 2e-8}
    for d in (0, 1):
        err, ndq = ch.trace(d)
        for e, n in zip(err, ndq):
            if e == e and n == n:
                m["constraint_tol"] = min(m.get("constraint_tol", np.inf), abs(e - 1e-9) / 1e-9)
                m["position_tol"] = min(m.get("position_tol", np.inf), abs(n - 1e-8) / 1e-8)
    return st, m


def live_metric_body(ctx, case, name, screening=False):
    """Everything test_set_metric_on_a_live_state checks on one context; returns (worst ratios, problems)."""
    seed, draw, scale = LIVE_METRIC[name]
    osys = case["osys"]
    base = np.array([0.02, -0.02, 0.04, 0.01, -0.03] if CASES[name]["layout"][0] == "sir" else [0.05, -0.05, 0.1, 0.02, -0.08])
    dts = scale * base
    M0 = to.metric_of(dict(metric=True))
    worst, problems = {}, []

    def step(what):
        q, p, xo, part = ctx.get_state()
        for c in range(B):
            st, m = oracle_margins_of_step(osys, q[c], p[c], xo[c], part, dts[c])
            if st != 0 or to.admissible(m):
                problems.append(f"{name} seed {seed}: step {what}, chain {c}: status {st}, margins {to.admissible(m)} (screening)")
        assert screening or not problems, problems
        worst[f"step_{what}"] = to._step_and_compare(ctx, osys, dts, what)

    def ops(what, x_obs_current):
        w = check_ops_at_current_state(ctx, osys, x_obs_current=x_obs_current)
        assert w[UNJUDGED] == 0, w
        worst[f"ops_{what}"] = largest(w) / 1e-10

    try:
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        ctx.sample_momentum(seed, draw)
        step("before")  # (against the oracle too: the context is then known to sit at moved, valid states)
        ctx.switch_partition()
        ctx.set_metric(M0)
        osys.set_metric(M0)
        ops("with_M0", True)
        step("with_M0")
        ctx.set_metric(None)
        osys.set_metric(None)
        ops("identity_again", False)  # (a step since the switch)
        step("identity_again")
    finally:
        osys.set_metric(None)
    print(f"  live set_metric {name}: worst ratio to the bound {({k: round(v, 4) for k, v in worst.items()})}")
    return worst, problems


def shard_body():
    """Everything test_sampler_does_not_depend_on_the_shard_size checks."""
    from manifold_mcmc_for_diffusions_amd.sampling import sample_static_chmc
    model, T, S, R, _, gaussian, var_sigma, oi = FHN12
    case = distinct_on_manifold_chains(model, T, S, R, 6, SHARD["seed"], obs_interval=oi, var_sigma=var_sigma, gaussian=gaussian)

    def run(sl, **kw):
        sub = dict(case, B=sl.stop - sl.start)
        ctx = make_ctx(sub)
        ctx.set_state(case["q"][sl], None, case["x_obs"][sl], 0)
        r = sample_static_chmc(ctx, SHARD["n_iter"], N_STEP, SHARD["eps0"], SHARD["seed"], n_adapt=0, solver=dict(to.SOLVER),
                               n_head=ctx.Q, jitter_length=True, **kw)
        ctx.close()
        return r

    whole = run(slice(0, 6))
    moved = (np.abs(np.diff(whole["heads"], axis=0)).max(2) > 0).sum(0)
    assert whole["chain_outcomes"][:, 0].sum() >= 6 and (moved > 0).sum() >= 4, (whole["chain_outcomes"], moved)
    for h in range(2):
        sl = slice(3 * h, 3 * h + 3)
        part = run(sl, chain_offset=3 * h, total_chains=6)
        assert np.array_equal(whole["heads"][:, sl], part["heads"]), h
        assert np.array_equal(whole["chain_outcomes"][sl], part["chain_outcomes"]), h
    print(f"  shards: outcomes per chain {whole['chain_outcomes'].tolist()}")


def run_static(name, monkeypatch, on_device=True):
    cfg = cfg_of(name)
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    case = to.build_case(cfg)
    for ctx, judge in to._contexts(name, case, monkeypatch, on_device):
        print(f"  seed {cfg['seed']} eps0 {cfg['eps0']}")
        static_body(ctx, case, cfg)
        print(f"  out80[70] = {ctx.diagnostics()['pair_scan_rounds']} (rounds of paired retractions)")
        judge(True, False)  # (every trajectory starts from a refreshed, tangent momentum: whole steps in k_traj_chain)


def run_live_metric(name, monkeypatch, on_device=True):
    cfg = cfg_of(name)
    case = to.build_case(cfg, seed=LIVE_METRIC[name][0])
    ctx = make_ctx(case)
    assert ctx.K == cfg["K"], ctx.K
    live_metric_body(ctx, case, name)
    ctx.close()


def test_the_table_shows_every_failing_status():
    seen = set()
    for name in GPU_CASES:
        seen |= set(CHOSEN[name][2])
    assert seen >= {1, 2, 3}, seen


@pytest.mark.parametrize("name", EMU_CASES)
def test_static_sampler_host_logic(emu_lib, monkeypatch, name):  # noqa: F811
    """Without a GPU (TEST-ONLY emulation build: generic functors only, so this says nothing about the device's kernels): the
    host side of the sampler's loop against the oracle's replay, at the same bounds."""
    run_static(name, monkeypatch, on_device=False)


def test_set_metric_on_a_live_state_host_logic(emu_lib, monkeypatch):  # noqa: F811
    run_live_metric("sir16_14_8", monkeypatch, on_device=False)


def test_sampler_shards_host_logic(emu_lib):  # noqa: F811
    shard_body()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_static_sampler_against_the_oracle(name, monkeypatch):
    to._hip()
    run_static(name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LIVE_METRIC))
def test_set_metric_on_a_live_state(name, monkeypatch):
    to._hip()
    run_live_metric(name, monkeypatch)


@pytest.mark.gpu
def test_sampler_does_not_depend_on_the_shard_size():
    to._hip()
    shard_body()


# The stored-rows and the MFMA family are latched by the first chmc_create of a process: a child process each (as
# tests/test_hip_tree_oracle.py starts its children), which runs the body on the two headline layouts.
_FAMILY_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_ctx
import test_hip_tree_oracle as to
import test_hip_static_oracle as so
for name in ("fhn_12_16_5_metric", "sir16_14_8"):
    cfg = so.cfg_of(name)
    case = to.build_case(cfg)
    ctx = make_ctx(case)
    assert ctx.L.chmc_backend() == b"hip:gfx950"
    print(name)
    so.static_body(ctx, case, cfg)
    d = ctx.diagnostics()
    assert d["newton_fsm_launches"] == 0 and d["traj_kernel_launches"] == 0 and d["retract_kernel_launches"] == 0, d
    assert (d["gram_mfma_launches"] > 0) == {mfma}, d
    ctx.close()
print("FAMILY_OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["stored_rows", "mfma"])
def test_row_families_in_a_child_process(family):
    """CHMC_COMPACT_ROWS=0 / CHMC_GRAM_MFMA=1: the static body on fhn_12_16_5_metric and sir16_14_8.  One child under a time
    limit; nothing is started after a failure."""
    to._hip()
    env = {"stored_rows": {"CHMC_COMPACT_ROWS": "0"}, "mfma": {"CHMC_GRAM_MFMA": "1"}}[family]
    script = _FAMILY_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mfma=family == "mfma")
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    print(env, r.stdout[-3000:])
    assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
    assert "FAMILY_OK" in r.stdout
