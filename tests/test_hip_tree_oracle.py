"""The layer the samplers call -- chmc_tree_begin / _step / _get, chmc_tree_doubling_begin / _end / _get_doubling,
chmc_snapshot / chmc_restore / chmc_restore_device, and the partition switch that follows them -- against the C oracle, on
every kernel family of the plan (csrc/chmc_plan.h).

test_transitions_against_the_oracle: DynamicTransition.sample on 5 distinct on-manifold chains with per-chain step sizes,
max_tree_depth = 3, 3 transitions with a partition switch between them; every chain against helpers.oracle_tree_transition
(every leaf an OracleChain.step) with the same TreeUniforms, started from the state the library reports before the
transition.  n_step, depth, moved, integrator_error and diverged equal with no allowance; accept_stat and the tree's log
weight to 1e-9 max(1, |.|); the position left on the context to 1e-9 max(1, |q|_inf) per leaf between the start and the
selected leaf (a chain that did not move: bitwise).  check_ops_at_current_state after every transition (the context has
just been through restore_device) and after every partition switch.

test_restore_leaves_valid_caches: snapshot, a step with a failing and a masked chain, restore(mask) -- (q, p) bitwise the
expected mix, every operator at the reported point, the next step (the p - h pg shortcut on re-evaluated caches), the
partition switch (k_xobs_par seeded from the restored chains' trajectories) and the step after it against oracle chains
started from the reported states; the same through restore_device with tangent and with raw momenta; get_head.

No decision may be a coin toss between library and oracle (they differ at about 1e-9), so every case was screened with
the oracle alone (tools/screen_tree_oracle.py): every draw is at least 1e-6 from its probability, every criterion value at
least 1e-6 (relative to |dh_dmom(edge)| |rho|) from zero, every delta_h at least 1e-6 from max_delta_h, no retraction
residual of any iteration of any leaf within 1e-2 relative of constraint_tol / position_tol, every reversibility error at
least 0.5 relative from reverse_check_tol.  (OracleChain.trace holds the last inner step of a leaf: with n_inner_step = 2
the first inner step's residuals are not screened.)  No chain, leaf or transition is skipped or excused at test time.  The
step sizes and seeds of the table are the screening's choice; in every case the oracle alone shows a chain whose first leaf
fails, a chain that fails at a later leaf while others run, trees ended by a sub-tree criterion, by the whole-tree criterion
and by the maximum depth, both directions, and a doubling that starts from the edge the context is not sitting on
(KTreeRestoreEdge).  Seeds that failed the screening: REPLACED below.

The emulation-build tests (not marked gpu) run the same two bodies on the CPU: host logic only, generic functors, they say
nothing about the device's kernels.

Additional sub-tree checks: tools/screen_tree_oracle.py --extra looked through 50 seeds each of fhn_12_16_5,
fhn_12_16_5_metric, fhn_6_8_2_noiseless_gauss, fhn_7_5_3_noiseless and sir16_14_8 (5 chains x 15 step sizes x 3 transitions per
seed) for a tree that an additional check ends while every plain span criterion of that leaf passes: none was found, so
no case of the table shows that event.  The values the additional checks read are covered another way: after every
transition the buffer of the last leaves of left halves (ck_end) must hold the momenta of the oracle's leaves.

Worst observed ratio to the bound per case on the MI355X (printed by pytest -s; transitions: selected position,
accept_stat, log weight, operators at the current state, ck_end | restore body: operators, compared steps):
  fhn_12_16_5 (both max_delta_h) 0.0000 0.0002 0.0000 0.004 0.0000 | 0.003 0.0000      fhn_12_16_5_metric   <= 0.0002, ops 0.004 | 0.004 0.0001
  fhn_130_4_2               <= 0.0002, ops 0.004 | 0.002 0.0002      the noiseless cases  <= 0.0002, ops 0.001 | 0.001 0.0000
  sir16_14_8 (unset, 2, 0: the same figures) 0.0001 0.0011 0.0001 0.117 0.0004 | 0.117 0.0032      sir16_12_16_varsigma 0.0001 0.0013 0.0000 0.080 0.0002 | 0.100 0.0022
  fhn_12_16_5_halves  0.0000 0.0001 0.0000 0.003 0.0000 | 0.003 0.0000      fhn_12_16_5_inner2  0.0000 0.0002 0.0000 0.003 0.0000 | 0.003 0.0000
  stored rows / MFMA children: fhn 0.0000 0.0002 0.0000 0.004 0.0000 | 0.004 0.0001, sir16 0.0002 0.0012 0.0001 0.132 0.0005 | 0.132 0.0031
sir16_14_8: out80[67] = 17 (transitions) and out80[67] = 3, out80[66] = 4 (restore body) unset and with 2; both 0 with 0."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx, check_ops_at_current_state, oracle_tree_transition
from autodiff_checks import largest
from test_hip_autodiff_parity import distinct_on_manifold_chains
from test_emu_logic import emu_lib  # noqa: F401
from test_rng import reference_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, DEPTH, N_TRANSITIONS = 5, 3, 3
DECISION_MARGIN, RESIDUAL_MARGIN, REVERSE_MARGIN = 1e-6, 1e-2, 0.5
SOLVER = dict(newton=True, constraint_tol=1e-9, position_tol=1e-8, divergence_tol=1e10, max_iters=50, reverse_check_tol=2e-8)
REQUIRED_EVENTS = ("first_leaf_error", "later_error_while_others_run", "subtree", "tree", "max_depth", "forward", "backward",
                   "edge_switch")

# id: layout (model, T, S, R, noisy, gaussian, var_sigma, obs_interval), block metric, environment, n_inner_step,
#     expected K
CASES = {
    "fhn_6_4_2": dict(layout=("fhn", 6, 4, 2, True, False, False, None), K=[3, 4]),            # (emulation build only)
    "fhn_12_16_5": dict(layout=("fhn", 12, 16, 5, True, False, False, None), K=[3, 3]),
    "fhn_12_16_5_metric": dict(layout=("fhn", 12, 16, 5, True, False, False, None), metric=True, K=[3, 3]),
    "fhn_130_4_2": dict(layout=("fhn", 130, 4, 2, True, False, False, None), K=[65, 66]),
    "fhn_6_8_2_noiseless_gauss": dict(layout=("fhn", 6, 8, 2, False, True, False, None), K=[3, 4]),
    "fhn_7_5_3_noiseless": dict(layout=("fhn", 7, 5, 3, False, False, False, None), K=[3, 3]),
    "sir16_14_8": dict(layout=("sir", 14, 8, 14, True, False, False, None), K=[1]),
    "sir16_12_16_varsigma": dict(layout=("sir", 12, 16, 12, True, False, True, None), K=[1]),
    "sir16_two_blocks": dict(layout=("sir", 26, 24, 13, True, False, False, 0.1), K=[2, 3]),
    "fhn_12_16_5_halves": dict(layout=("fhn", 12, 16, 5, True, False, False, None), env={"CHMC_HALVES": "2"}, K=[3, 3]),
    "fhn_12_16_5_inner2": dict(layout=("fhn", 12, 16, 5, True, False, False, None), n_inner=2, K=[3, 3]),
}
# the screening's choices (tools/screen_tree_oracle.py --search): id: (seed, step size per chain)
CHOSEN = {
    "fhn_6_4_2": (31, [0.03, 0.6, 0.5, 0.6, 0.6]),
    "fhn_12_16_5": (31, [0.06, 1.0, 0.6, 0.5, 0.5]),
    "fhn_12_16_5_metric": (31, [1.3, 0.3, 0.5, 0.6, 0.5]),
    "fhn_130_4_2": (131, [0.03, 0.8, 0.6, 0.5, 0.6]),
    "fhn_6_8_2_noiseless_gauss": (31, [0.5, 0.6, 0.4, 0.6, 0.5]),
    "fhn_7_5_3_noiseless": (31, [0.03, 0.8, 1.0, 0.6, 0.6]),
    "sir16_14_8": (31, [0.8, 0.8, 0.6, 0.8, 0.6]),
    "sir16_12_16_varsigma": (31, [1.0, 0.8, 0.6, 0.8, 0.8]),
    "sir16_two_blocks": (31, [0.6, 0.3, 0.6, 0.6, 0.6]),  # (0.1 between observations, as the parity test of this shape)
    "fhn_12_16_5_halves": (31, [0.06, 1.0, 0.6, 0.5, 0.5]),
    "fhn_12_16_5_inner2": (31, [0.03, 1.6, 1.3, 0.5, 0.5]),
}
# second runs with max_delta_h between two of the oracle's own delta_h values: id: max_delta_h
DIVERGENCE_RUNS = {
    "fhn_12_16_5": 3.0,  # chain 3, transition 0: delta_h = 0.42, 5.02, 7.79, 6.65 -- the second leaf diverges
}
REPLACED = {  # id: the seeds that failed the screening, and on what
    "fhn_130_4_2": {31: "restore body: a retraction's |dq| within 4.7e-03 relative of position_tol"},
}
GPU_CASES = [n for n in CASES if n != "fhn_6_4_2"]
EMU_CASES = ["fhn_6_4_2", "fhn_7_5_3_noiseless"]
RETRACT_KERNEL_RUNS = (None, "2", "0")  # sir16_14_8: 8 wavefronts per chain (k_traj_chain), 4 wavefronts, batched launches


def cfg_of(name):
    cfg = dict(metric=False, env={}, n_inner=1, restore_scale=0.25)
    cfg.update(CASES[name])
    if name in CHOSEN:
        cfg["seed"], cfg["eps"] = CHOSEN[name][0], np.array(CHOSEN[name][1], dtype=np.float64)
    return cfg


def solver_of(cfg):
    return dict(SOLVER, n_inner_step=cfg["n_inner"]) if cfg["n_inner"] > 1 else dict(SOLVER)


def metric_of(cfg):
    if not cfg["metric"]:
        return None
    a = np.random.default_rng(3).standard_normal((4, 4))
    return a @ a.T / 4 + 0.5 * np.eye(4)


def build_case(cfg, seed=None):
    """5 distinct on-manifold chains.  Noisy observations: distinct_on_manifold_chains.  Noiseless: chain 0 of make_case
    lies on the manifold; the others are reached from it with two steps of the ORACLE each (own momenta and step sizes), so
    that the points are an input of both sides that neither side's kernels produced."""
    from oracle import c_oracle
    model, T, S, R, noisy, gaussian, var_sigma, oi = cfg["layout"]
    seed = cfg["seed"] if seed is None else seed
    if noisy:
        return distinct_on_manifold_chains(model, T, S, R, B, seed, obs_interval=oi, var_sigma=var_sigma, gaussian=gaussian)
    case = make_case(model, T, S, R, False, B=B, seed=seed, obs_interval=oi, gaussian=gaussian)
    rng = np.random.default_rng(seed + 1)
    for c in range(1, B):
        ch = c_oracle.OracleChain(case["osys"])
        ch.set(case["q"][0], rng.standard_normal(case["q"].shape[1]), case["x_obs"][0], 0)
        ch.project_mom()
        dt = (1.0 if c % 2 else -1.0) * (0.03 + 0.05 * rng.random())
        assert [ch.step(dt)[0] for _ in range(2)] == [0, 0], (c, dt)
        case["q"][c] = ch.get()[0]
        case["x_obs"][c] = case["osys"].generate_x_obs_seq(case["q"][c])
    assert np.abs(case["q"][1:] - case["q"][:1]).max(1).min() > 1e-3
    return case


def oracle_momentum(osys, q, xo, part, c, seed, draw, M0):
    """chmc_sample_momentum restated: metric.sqrt @ (keyed normals of chain c), projected onto the cotangent space."""
    n = reference_normals(osys.Q, c, seed, draw)
    if M0 is not None:
        n[:osys.U] = np.linalg.cholesky(M0) @ n[:osys.U]
    return n - osys.jacob_products(q, xo, part, n, np.zeros(osys.dim_c(part)))[3]


def uniforms_of(seed, it, c):
    from manifold_mcmc_for_diffusions_amd.dynamic import TreeUniforms
    un = TreeUniforms(seed, it, B, 0, B)
    return lambda kind, d, k: un.get(kind, d, k)[c]


def oracle_chain_history(case, cfg, c, eps, max_delta_h=1000.0, seed=None):
    """What the sampler's loop does to chain c -- momentum refresh, transition, partition switch, N_TRANSITIONS times -- with
    the oracle alone (the screening's view of a case)."""
    osys, M0 = case["osys"], metric_of(cfg)
    seed = cfg["seed"] if seed is None else seed
    W = None if M0 is None else np.linalg.inv(M0)
    osys.set_metric(M0)
    try:
        q, xo, part, out = case["q"][c], case["x_obs"][c], 0, []
        for it in range(N_TRANSITIONS):
            p = oracle_momentum(osys, q, xo, part, c, seed, it + 1, M0)
            r = oracle_tree_transition(osys, q, p, xo, part, uniforms_of(seed, it, c), eps, DEPTH, max_delta_h, solver_of(cfg), W)
            out.append(r)
            q, part = r["q"], (part + 1) % osys.num_partition
            xo = osys.generate_x_obs_seq(q)
    finally:
        osys.set_metric(None)
    return out


def admissible(margins):
    """The admission conditions of the module docstring; returns the kinds that miss them."""
    need = {"constraint_tol": RESIDUAL_MARGIN, "position_tol": RESIDUAL_MARGIN, "reverse_check": REVERSE_MARGIN}
    return {k: v for k, v in margins.items() if not v >= need.get(k, DECISION_MARGIN)}


def events_of(histories):
    """histories[c][it] = oracle_tree_transition's result: the events of section "Cases" the batch shows."""
    ev = set()
    for c, hist in enumerate(histories):
        for it, r in enumerate(hist):
            e = r["event"]
            if e[0] == "error" and r["n_step"] == 0 and not r["moved"]:
                ev.add("first_leaf_error")
            if e[0] == "error" and e[2] > 0:
                ev.add("later_error")
                if any((e[3], e[4]) in o[it]["leaves"] for k, o in enumerate(histories) if k != c):
                    ev.add("later_error_while_others_run")
            if e[0] == "diverged" and e[1] > 0:
                ev.add("later_divergence")
            if e[0] in ("subtree", "extra", "tree", "max_depth", "diverged"):
                ev.add(e[0])
            ev |= {"forward" if f else "backward" for f in r["dirs"]}
            if r["edge_switches"]:
                ev.add("edge_switch")
    return ev


def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"


def _device(ctx):
    import torch
    return torch.device("cuda", 0) if ctx.L.chmc_backend().startswith(b"hip") else torch.device("cpu")


def transitions_body(ctx, case, cfg, max_delta_h=1000.0):
    """Everything test_transitions_against_the_oracle checks on one context; returns the worst ratios to the bounds."""
    from manifold_mcmc_for_diffusions_amd.dynamic import DynamicTransition
    osys, seed, eps, M0 = case["osys"], cfg["seed"], cfg["eps"], metric_of(cfg)
    assert ctx.K == cfg["K"], ctx.K
    W = None if M0 is None else np.linalg.inv(M0)
    worst = dict(position=0.0, accept_stat=0.0, logw=0.0, ops=0.0, ck_end=0.0)
    histories = [[] for _ in range(B)]
    osys.set_metric(M0)
    try:
        ctx.set_metric(M0)
        ctx.set_state(case["q"], None, case["x_obs"], 0)
        tr = DynamicTransition(ctx, eps, seed, max_tree_depth=DEPTH, max_delta_h=max_delta_h, solver=solver_of(cfg))
        for it in range(N_TRANSITIONS):
            ctx.sample_momentum(seed, it + 1)
            q0, p0, xo0, part = ctx.get_state()
            ck_before = tr.ck_end.cpu().numpy().copy()
            st = tr.sample(it)
            ck_after = tr.ck_end.cpu().numpy()
            logw = ctx.tree_get_doubling()["logw"]
            q1, p1, _, _ = ctx.get_state()
            for c in range(B):
                r = oracle_tree_transition(osys, q0[c], p0[c], xo0[c], part, uniforms_of(seed, it, c), eps[c], DEPTH, max_delta_h,
                                           solver_of(cfg), W)
                histories[c].append(r)
                bad = admissible(r["margins"])
                assert not bad, f"transition {it} chain {c}: the oracle's own decision margins {bad} (screening)"
                got = (st["n_step"][c], st["depth"][c], bool(st["moved"][c]), bool(st["integrator_error"][c]), bool(st["diverged"][c]))
                want = (r["n_step"], r["depth"], r["moved"], r["event"][0] == "error", r["event"][0] == "diverged")
                assert got == want, (it, c, got, want, r["event"])
                acc = r["sum_acc"] / max(r["n_step"], 1)
                e_acc = abs(st["accept_stat"][c] - acc) / max(1.0, abs(acc))
                e_logw = abs(logw[c] - r["logw"]) / max(1.0, abs(r["logw"]))
                per_leaf = 1e-9 * max(1.0, np.abs(r["q"]).max())
                e_q = np.abs(q1[c] - r["q"]).max()
                worst["accept_stat"], worst["logw"] = max(worst["accept_stat"], e_acc / 1e-9), max(worst["logw"], e_logw / 1e-9)
                if r["offset"] != 0:
                    worst["position"] = max(worst["position"], e_q / (per_leaf * abs(r["offset"])))
                assert e_acc <= 1e-9 and e_logw <= 1e-9, (it, c, e_acc, e_logw)
                assert e_q <= per_leaf * abs(r["offset"]), (it, c, e_q, per_leaf, r["offset"], r["event"])
                assert np.array_equal(p1[c], p0[c]), (it, c)  # (the transition hands the refreshed momentum back)
                # the additional checks' buffer: the slots the oracle's tree recorded hold its leaves' momenta (the step's bound
                # for momenta, per leaf from the start), every other slot is untouched
                for slot in range(DEPTH):
                    if slot in r["ck_end"]:
                        pm, n = r["ck_end"][slot]
                        e_ck = np.abs(ck_after[slot, c] - pm).max() / (1e-9 * max(1.0, np.abs(pm).max()) * n)
                        worst["ck_end"] = max(worst["ck_end"], e_ck)
                        assert e_ck <= 1.0, (it, c, slot, e_ck)
                    else:
                        assert np.array_equal(ck_after[slot, c], ck_before[slot, c]), (it, c, slot)
            moved = np.array([h[-1]["moved"] for h in histories])
            w = check_ops_at_current_state(ctx, osys, x_obs_current=~moved)
            ctx.switch_partition()
            w2 = check_ops_at_current_state(ctx, osys)
            worst["ops"] = max(worst["ops"], largest(w) / 1e-10, largest(w2) / 1e-10)
        ctx.set_metric(None)
    finally:
        osys.set_metric(None)
    ev = events_of(histories)
    print(f"  transitions: worst ratio to the bound {({k: round(v, 4) for k, v in worst.items()})}; events {sorted(ev)}; "
          f"leaves {[[r['n_step'] for r in h] for h in histories]}")
    return worst, ev


def _step_and_compare(ctx, osys, dts, what):
    """One leapfrog step of all chains against oracle chains started from the state the library reports."""
    from oracle import c_oracle
    q0, p0, xo, part = ctx.get_state()
    res = ctx.leapfrog_step(dts)
    q1, p1, _, _ = ctx.get_state()
    worst = 0.0
    for c in range(ctx.B):
        ch = c_oracle.OracleChain(osys)
        ch.set(q0[c], p0[c], xo[c], part)
        st, itf, itb, _ = ch.step(dts[c])
        qo, po, _, _ = ch.get()
        assert (res["status"][c], res["iters_fwd"][c], res["iters_bwd"][c]) == (st, itf, itb) and st == 0, (what, c, res, st, itf, itb)
        eq, ep = np.abs(q1[c] - qo).max() / max(1.0, np.abs(qo).max()), np.abs(p1[c] - po).max() / max(1.0, np.abs(po).max())
        worst = max(worst, eq / 1e-9, ep / 1e-9)
        assert eq <= 1e-9 and ep <= 1e-9, (what, c, eq, ep)
    return worst


def restore_body(ctx, case, cfg):
    """Everything test_restore_leaves_valid_caches checks on one context (steps 1 to 9 of the issue)."""
    import torch
    from oracle import c_oracle
    osys, seed = case["osys"], cfg["seed"]
    dev = _device(ctx)
    base = np.array([0.02, -0.02, 0.04, 0.01, -0.03] if cfg["layout"][0] == "sir" else [0.05, -0.05, 0.1, 0.02, -0.08])
    dts = cfg["restore_scale"] * base
    worst = {}
    # 1-2: snapshot, then a step in which chain 1 fails and chain 3 is masked out
    ctx.set_state(case["q"], None, case["x_obs"], 0)
    ctx.sample_momentum(seed, 7)
    ctx.snapshot()
    q0, p0, _, _ = ctx.get_state()
    bad_dts, active = dts.copy(), np.ones(B, dtype=np.int32)
    bad_dts[1], active[3] = 5.0, 0
    res = ctx.leapfrog_step(bad_dts, active=active)
    assert res["status"][1] > 0 and res["status"][3] == -1 and (res["status"][[0, 2, 4]] == 0).all(), res["status"]
    q1, p1, _, _ = ctx.get_state()
    assert not np.array_equal(q1[0], q0[0]) and not np.array_equal(q1[2], q0[2])
    # 3-4: restore a chain that moved (0, 4) and the failed one (1), keep a chain that moved (2) and the masked one (3)
    mask = np.array([1, 1, 0, 0, 1], dtype=np.int32)
    ctx.restore(mask)
    q2, p2, _, _ = ctx.get_state()
    keep = (mask == 0)[:, None]
    assert np.array_equal(q2, np.where(keep, q1, q0)) and np.array_equal(p2, np.where(keep, p1, p0))
    assert np.array_equal(q2[[1, 3]], q0[[1, 3]]) and np.array_equal(p2[[1, 3]], p0[[1, 3]])
    # 5-7: caches at the reported point, the next step (tangent momenta: p - h pg), the switch, the step after it
    worst["ops_after_restore"] = largest(check_ops_at_current_state(ctx, osys, x_obs_current=np.arange(B) != 2)) / 1e-10
    worst["step_after_restore"] = _step_and_compare(ctx, osys, dts, "after restore")
    ctx.switch_partition()
    worst["ops_after_switch"] = largest(check_ops_at_current_state(ctx, osys)) / 1e-10
    worst["step_after_switch"] = _step_and_compare(ctx, osys, dts, "after switch")
    # 8: restore_device from buffers that hold the oracle's own stepped states (chain 3 is left as it is)
    rng = np.random.default_rng(seed + 2)
    mask = np.array([1, 1, 1, 0, 1], dtype=np.int32)
    for tangent in (True, False):
        qc, pc, xo, part = ctx.get_state()
        qn, pn = np.empty_like(qc), rng.standard_normal(qc.shape)
        for c in range(B):
            ch = c_oracle.OracleChain(osys)
            ch.set(qc[c], pc[c], xo[c], part)
            assert ch.step(dts[c])[0] == 0, c
            qn[c] = ch.get()[0]
            if tangent:
                ch.set_mom(pn[c])
                ch.project_mom()
                pn[c] = ch.get()[1]
        d_q, d_p = torch.from_numpy(qn.copy()).to(dev), torch.from_numpy(pn.copy()).to(dev)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        ctx.restore_device(d_q.data_ptr(), d_p.data_ptr(), mask, tangent)
        q3, p3, _, _ = ctx.get_state()
        keep = (mask == 0)[:, None]
        assert np.array_equal(q3, np.where(keep, qc, qn)) and np.array_equal(p3, np.where(keep, pc, pn)), tangent
        k = "tangent" if tangent else "raw"
        worst[f"ops_after_restore_device_{k}"] = largest(check_ops_at_current_state(ctx, osys, x_obs_current=False)) / 1e-10
        worst[f"step_after_restore_device_{k}"] = _step_and_compare(ctx, osys, dts, f"after restore_device {k}")
    # 9
    for n in (1, 6, ctx.Q):
        assert np.array_equal(ctx.get_head(n), ctx.get_state()[0][:, :n]), n
    print(f"  restore: worst ratio to the bound {({k: round(v, 4) for k, v in worst.items()})}")
    return worst


def _contexts(name, case, monkeypatch, on_device):
    """The contexts a case runs on: one, or for sir16_14_8 on the device one per CHMC_RETRACT_KERNEL setting (read on entry
    to every call).  After each, the launch counters out80[67] (k_traj_chain) and out80[66] (k_retract_chain) are handed to
    `judge`."""
    runs = RETRACT_KERNEL_RUNS if name == "sir16_14_8" and on_device else (None,)
    for rk in runs:
        if rk is not None:
            monkeypatch.setenv("CHMC_RETRACT_KERNEL", rk)
        ctx = make_ctx(case)
        print(f"\n{name} (CHMC_RETRACT_KERNEL {rk}): Q={ctx.Q} K={ctx.K} RM={ctx.RM}")

        def judge(want_traj, want_retract, ctx=ctx, rk=rk):
            d = ctx.diagnostics()
            traj, retract = d["traj_kernel_launches"], d["retract_kernel_launches"]
            print(f"  out80[67] = {traj}, out80[66] = {retract}")
            if name == "sir16_14_8" and on_device:
                if rk == "0":
                    assert (traj, retract) == (0, 0), (rk, traj, retract)
                else:
                    assert (not want_traj or traj > 0) and (not want_retract or retract > 0), (rk, traj, retract)
        yield ctx, judge
        ctx.close()


def run_transitions(name, monkeypatch, on_device=True):
    cfg = cfg_of(name)
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    case = build_case(cfg)
    for ctx, judge in _contexts(name, case, monkeypatch, on_device):
        print(f"  seed {cfg['seed']} eps {cfg['eps'].tolist()}")
        _, ev = transitions_body(ctx, case, cfg)
        missing = [e for e in REQUIRED_EVENTS if e not in ev]
        assert not missing, missing
        if name in DIVERGENCE_RUNS:
            _, ev = transitions_body(ctx, case, cfg, max_delta_h=DIVERGENCE_RUNS[name])
            assert "later_divergence" in ev, ev
        judge(True, False)  # (every leaf starts from a tangent momentum: whole steps in k_traj_chain)


def run_restore(name, monkeypatch, on_device=True):
    cfg = cfg_of(name)
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    case = build_case(cfg)
    M0 = metric_of(cfg)
    for ctx, judge in _contexts(name, case, monkeypatch, on_device):
        case["osys"].set_metric(M0)
        try:
            ctx.set_metric(M0)
            restore_body(ctx, case, cfg)
        finally:
            case["osys"].set_metric(None)
        # (tangent momenta after restore: k_traj_chain; raw momenta after the switch and after restore_device(.., False): the
        # step's retractions in k_retract_chain)
        judge(True, True)


@pytest.mark.parametrize("name", EMU_CASES)
def test_transitions_host_logic(emu_lib, monkeypatch, name):  # noqa: F811
    """Without a GPU (TEST-ONLY emulation build: generic functors only, so this says nothing about the device's kernels):
    the host side of the tree and doubling calls against the oracle's transition, at the same bounds."""
    run_transitions(name, monkeypatch, on_device=False)


@pytest.mark.parametrize("name", EMU_CASES)
def test_restore_host_logic(emu_lib, monkeypatch, name):  # noqa: F811
    """Likewise snapshot / restore / restore_device / get_head and the masked re-evaluation of the caches."""
    run_restore(name, monkeypatch, on_device=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_transitions_against_the_oracle(name, monkeypatch):
    _hip()
    run_transitions(name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_restore_leaves_valid_caches(name, monkeypatch):
    _hip()
    run_restore(name, monkeypatch)


# The stored-rows and the MFMA family are latched by the first chmc_create of a process: a child process each (as
# tests/test_hip_layout_edges.py starts its children), which runs both bodies on the two headline layouts.
_FAMILY_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_ctx
import test_hip_tree_oracle as to
for name in ("fhn_12_16_5", "sir16_14_8"):
    cfg = to.cfg_of(name)
    case = to.build_case(cfg)
    ctx = make_ctx(case)
    assert ctx.L.chmc_backend() == b"hip:gfx950"
    print(name)
    _, ev = to.transitions_body(ctx, case, cfg)
    assert not [e for e in to.REQUIRED_EVENTS if e not in ev], ev
    to.restore_body(ctx, case, cfg)
    d = ctx.diagnostics()
    assert d["newton_fsm_launches"] == 0 and d["traj_kernel_launches"] == 0 and d["retract_kernel_launches"] == 0, d
    assert (d["gram_mfma_launches"] > 0) == {mfma}, d
    ctx.close()
print("FAMILY_OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["stored_rows", "mfma"])
def test_row_families_in_a_child_process(family):
    """CHMC_COMPACT_ROWS=0 / CHMC_GRAM_MFMA=1: transitions and restores on fhn_12_16_5 and sir16_14_8.  One child under a
    time limit; nothing is started after a failure."""
    _hip()
    env = {"stored_rows": {"CHMC_COMPACT_ROWS": "0"}, "mfma": {"CHMC_GRAM_MFMA": "1"}}[family]
    script = _FAMILY_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mfma=family == "mfma")
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    print(env, r.stdout[-3000:])
    assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
    assert "FAMILY_OK" in r.stdout
