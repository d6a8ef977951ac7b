"""CPU screening of the cases of tests/test_hip_tree_oracle.py, with the C oracle alone (no library, no GPU).

    python tools/screen_tree_oracle.py [case id ...]            the cases as the test module's table has them
    python tools/screen_tree_oracle.py --search case id ...     choose a seed and step sizes for a case (at most 50 seeds)
    python tools/screen_tree_oracle.py --extra case id ...      look (at most 50 seeds) for a transition that an additional
                                                                sub-tree check decides while the plain span criteria pass

For every case, chain and transition it runs helpers.oracle_tree_transition (momentum refresh, transition, partition
switch, as the sampler's loop) and the oracle side of the restore body (restore_steps), and prints the smallest margin of
every kind of decision and the events reached.  A case is admitted only if every decision margin is at least 1e-6, no
retraction residual lies within 1e-2 relative of its tolerance, every reversibility error is at least 0.5 relative from
reverse_check_tol, and the batch shows every event of test_hip_tree_oracle.REQUIRED_EVENTS.  A seed that fails is replaced
in the test module and noted in its REPLACED table."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from oracle import c_oracle  # noqa: E402
import test_hip_tree_oracle as to  # noqa: E402

FHN_GRID = [0.03, 0.06, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.6, 0.8, 1.0, 1.3, 1.6, 2.0, 5.0]
SIR_GRID = [0.01, 0.02, 0.04, 0.06, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6, 0.8, 1.0, 1.5, 2.0, 5.0]
MAX_SEEDS = 50


def fmt(m):
    return {k: f"{v:.1e}" for k, v in sorted(m.items())}


def merged(histories):
    m = {}
    for h in histories:
        for r in h:
            for k, v in r["margins"].items():
                m[k] = min(m.get(k, np.inf), v)
    return m


def restore_steps(case, cfg):
    """The oracle's view of the plain steps of restore_body: from every chain's start point with the refreshed momentum,
    the step sizes of the body, four steps on (the body takes four compared steps and two of the oracle's own; its states
    differ from these by what the restores and switches do, so this screens the neighbourhood, and the body's own
    comparisons are the judge).  Returns (statuses, margins)."""
    osys, M0 = case["osys"], to.metric_of(cfg)
    base = np.array([0.02, -0.02, 0.04, 0.01, -0.03] if cfg["layout"][0] == "sir" else [0.05, -0.05, 0.1, 0.02, -0.08])
    dts = cfg["restore_scale"] * base
    osys.set_metric(M0)
    margins, statuses = {}, []
    try:
        for c in range(to.B):
            ch = c_oracle.OracleChain(osys)
            q, xo = case["q"][c], case["x_obs"][c]
            ch.set(q, to.oracle_momentum(osys, q, xo, 0, c, cfg["seed"], 7, M0), xo, 0)
            for k in range(4):
                if k == 1:
                    ch.switch_partition()
                st, _, _, rev = ch.step(dts[c])
                statuses.append(st)
                for d in (0, 1):
                    err, ndq = ch.trace(d)
                    for e, n in zip(err, ndq):
                        margins["constraint_tol"] = min(margins.get("constraint_tol", np.inf), abs(e - 1e-9) / 1e-9)
                        margins["position_tol"] = min(margins.get("position_tol", np.inf), abs(n - 1e-8) / 1e-8)
                margins["reverse_check"] = min(margins.get("reverse_check", np.inf), abs(rev - 2e-8) / 2e-8)
    finally:
        osys.set_metric(None)
    return statuses, margins


def screen(name):
    cfg = to.cfg_of(name)
    t0 = time.time()
    case = to.build_case(cfg)
    ok = True
    for mdh in [1000.0] + ([to.DIVERGENCE_RUNS[name]] if name in to.DIVERGENCE_RUNS else []):
        hist = [to.oracle_chain_history(case, cfg, c, cfg["eps"][c], mdh) for c in range(to.B)]
        m, ev = merged(hist), to.events_of(hist)
        bad = to.admissible(m)
        missing = [e for e in to.REQUIRED_EVENTS if e not in ev] if mdh == 1000.0 else [e for e in ("later_divergence",) if e not in ev]
        ok = ok and not bad and not missing
        print(f"SCREEN {name} max_delta_h {mdh}: seed {cfg['seed']} eps {cfg['eps'].tolist()}\n  margins {fmt(m)}\n  events {sorted(ev)}\n"
              f"  endings {[[r['event'] for r in h] for h in hist]}\n  leaves {[[r['n_step'] for r in h] for h in hist]}"
              f"{'' if not bad else ' NEAR-EDGE ' + str(fmt(bad))}{'' if not missing else ' MISSING ' + str(missing)}")
    st, rm = restore_steps(case, cfg)
    bad = to.admissible(rm)
    ok = ok and not bad and set(st) == {0}
    print(f"  restore body: statuses {sorted(set(st))} margins {fmt(rm)}{'' if not bad else ' NEAR-EDGE'}; {time.time() - t0:.1f} s "
          f"{'ok' if ok else 'REPLACE'}", flush=True)
    return ok


def chain_table(case, cfg, seed, grid):
    """Every (chain, step size) of the grid: its three-transition history, if admissible."""
    tab = {}
    for c in range(to.B):
        for eps in grid:
            h = to.oracle_chain_history(case, cfg, c, eps, seed=seed)
            why = to.admissible(merged([h]))
            tab[c, eps] = (h, why)
    return tab


def search(name, want_extra=False):
    cfg = to.cfg_of(name)
    grid = SIR_GRID if cfg["layout"][0] == "sir" else FHN_GRID
    failed = {}
    for seed in range(31, 31 + 100 * MAX_SEEDS, 100):
        cfg["seed"] = seed
        try:
            case = to.build_case(cfg, seed)
        except AssertionError as e:
            failed[seed] = f"building the chains: {str(e)[:60]}"
            continue
        st, rm = restore_steps(case, cfg)
        if to.admissible(rm) or set(st) != {0}:
            failed[seed] = f"restore body: statuses {sorted(set(st))}, near-edge {fmt(to.admissible(rm))}"
            continue
        tab = chain_table(case, cfg, seed, grid)
        good = {k: h for k, (h, why) in tab.items() if not why}
        if want_extra:
            hits = [(k, it) for k, h in good.items() for it, r in enumerate(h) if r["event"] == ("extra",)]
            print(f"seed {seed}: extra-check endings at (chain, eps), transition: {hits}", flush=True)
            if not hits:
                continue
        # greedy cover of the required events, one step size per chain
        pick, need = {}, set(to.REQUIRED_EVENTS) - {"later_error_while_others_run"} | {"later_error"}
        if want_extra:
            (c, eps), _ = hits[0]
            pick[c] = eps
            need -= to.events_of([good[c, eps]])
        while need and len(pick) < to.B:
            best = max(((k, to.events_of([h]) & need) for k, h in good.items() if k[0] not in pick), key=lambda t: len(t[1]),
                       default=None)
            if best is None or not best[1]:
                break
            pick[best[0][0]] = best[0][1]
            need -= best[1]
        if need:
            failed[seed] = f"no admissible step sizes show {sorted(need)}"
            print(f"seed {seed}: {failed[seed]}", flush=True)
            continue
        for c in range(to.B):  # the chains left over: a moderate step size
            if c not in pick:
                cands = [eps for eps in grid if (c, eps) in good and 0.1 * grid[-2] <= eps <= 0.5 * grid[-2]] or \
                        [eps for eps in grid if (c, eps) in good]
                pick[c] = cands[len(cands) // 2]
        hist = [good[c, pick[c]] for c in range(to.B)]
        ev = to.events_of(hist)
        missing = [e for e in to.REQUIRED_EVENTS if e not in ev]
        if missing:
            failed[seed] = f"assembled batch misses {missing}"
            print(f"seed {seed}: {failed[seed]}", flush=True)
            continue
        print(f'CHOSEN    "{name}": ({seed}, {[pick[c] for c in range(to.B)]}),')
        print(f'REPLACED  "{name}": {failed},')
        print(f"  events {sorted(ev)}\n  endings {[[r['event'] for r in h] for h in hist]}\n  margins {fmt(merged(hist))}")
        dh = sorted((r["dh"], c, it) for c, h in enumerate(hist) for it, r in enumerate(h) if len(r["dh"]) > 1)
        print("  delta_h per leaf (chain, transition):", [(c, it, np.round(d, 4).tolist()) for d, c, it in dh][:8], flush=True)
        return seed
    print(f"NONE FOUND for {name} in {MAX_SEEDS} seeds; failures {failed}")
    return None


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("--search", "--extra"):
        for n in args[1:]:
            search(n, want_extra=args[0] == "--extra")
        sys.exit(0)
    results = {n: screen(n) for n in (args or list(to.CASES))}
    print("failed:", [n for n, ok in results.items() if not ok])
    sys.exit(0 if all(results.values()) else 1)
