"""CPU screening of the cases of tests/test_hip_nld_paths.py: the autodiff oracle alone (no GPU, no library).

    python tools/screen_nld_paths.py                 every table of the module
    python tools/screen_nld_paths.py long [id ...]   the wild calls of LONG only (the WILD_FINITE table)
    python tools/screen_nld_paths.py --search id     seeds for a LONG case whose wild call has both regimes

Parts 1 - 3 (MATRIX, R_INDEPENDENCE, TILES, SEGMENTS, SEGMENTS_SIR16): every chain of every case must have a finite oracle
value and gradient, or the device test cannot judge it -- a case that has not is reported with its chains.
Part 4 (LONG): the healthy and the warm call must be finite in the two chains the test sends to the oracle; of the six
chains of the wild call at least two must be finite and at least two not (the reversed wild call holds the same points).
Prints the WILD_FINITE table as the module has to hold it, and says where the module's differs.
Part 6 (ADAM): the finite chains of both calls."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import autodiff_checks as ac  # noqa: E402
import test_hip_nld_paths as np_  # noqa: E402


def finite_chains(futs):
    """Chains whose oracle value and gradient are finite; chains whose value alone is."""
    res = {c: f.result() for c, f in futs.items()}
    return ([c for c, (v, g) in res.items() if np_.all_finite(v, g)],
            [c for c, (v, g) in res.items() if np.isfinite(v) and not np.isfinite(g).all()])


def screen_all_finite(what, jobs):
    """jobs: [(label, case, q, gaussian)]: every chain finite?"""
    t0 = time.time()
    futs = [(label, len(q), np_.submit(case, q, gaussian, range(len(q)))) for label, case, q, gaussian in jobs]
    bad = 0
    for label, n, f in futs:
        fin, half = finite_chains(f)
        if len(fin) != n:
            bad += 1
            print(f"  {what} {label}: NOT every chain finite: finite {fin}, value only {half}")
    print(f"{what}: {len(jobs)} cases, {bad} with a chain that is not finite ({time.time() - t0:.0f} s)", flush=True)
    return bad


def parts_1_to_3():
    jobs = []
    for cid, (model, vs, gauss, T, S, R, _) in np_.MATRIX.items():
        case, q = np_.build(model, T, S, R, vs, np_.MATRIX_B, np_.MATRIX_SEED)
        jobs.append((cid, case, q, gauss))
    bad = screen_all_finite("MATRIX", jobs)
    jobs = []
    for model, (vs, T, S, rs) in np_.R_INDEPENDENCE.items():
        case, q = np_.build(model, T, S, rs[0][0], vs, np_.MATRIX_B, np_.MATRIX_SEED + 1)
        jobs += [(f"{model} gaussian={g}", case, q, g) for g in (False, True)]
    bad += screen_all_finite("R_INDEPENDENCE", jobs)
    jobs = []
    for T, S in np_.TILES:
        case, q = np_.build("fhn", T, S, None, False, 5, np_.TILES_SEED)
        jobs.append(((T, S), case, q, False))
    bad += screen_all_finite("TILES", jobs)
    jobs = []
    for model in ("fhn", "sir"):
        for W, shapes in np_.SEGMENTS.items():
            jobs += [((model, W, T, S),) + np_.segment_case(model, T, S) + (False,) for T, S in shapes]
    for W, shapes in np_.SEGMENTS_SIR16.items():
        jobs += [(("sir16", W, T, S),) + np_.segment_case("sir", T, S) + (False,) for T, S in shapes]
    bad += screen_all_finite("SEGMENTS", jobs)
    return bad


def long_wild(cid, seed=None):
    """Oracle jobs of LONG[cid] (optionally with another seed): healthy and warm chains (0, B - 1), the wild call whole."""
    if seed is not None:
        np_.LONG[cid] = np_.LONG[cid][:7] + (seed,)
    case, calls = np_.long_calls(cid)
    g = np_.LONG[cid][5]
    ends = (0, np_.LONG_B - 1)
    return [np_.submit(case, calls[0], g, ends), np_.submit(case, calls[1], g, ends), np_.submit(case, calls[2], g, range(np_.LONG_B))]


def part_4(ids):
    t0 = time.time()
    futs = {cid: long_wild(cid) for cid in ids}
    table, bad = {}, 0
    for cid, (healthy, warm, wild) in futs.items():
        ok = len(finite_chains(healthy)[0]) == 2 and len(finite_chains(warm)[0]) == 2
        fin, half = finite_chains(wild)
        table[cid] = tuple(fin)
        both = len(fin) >= 2 and np_.LONG_B - len(fin) >= 2
        bad += not (ok and both)
        print(f"  {cid}: wild call finite {len(fin)} of {np_.LONG_B} {fin}, value finite but gradient not {half}; healthy and warm "
              f"chains finite: {ok}{'' if ok and both else '   <-- NOT ADMITTED'}", flush=True)
    print("WILD_FINITE = {")
    for cid, fin in table.items():
        print(f"    \"{cid}\": {fin},")
    print("}")
    for cid, fin in table.items():
        if np_.WILD_FINITE.get(cid) != fin:
            print(f"  the module's WILD_FINITE[{cid!r}] is {np_.WILD_FINITE.get(cid)}")
            bad += 1
    print(f"LONG: {len(ids)} cases, {bad} problems ({time.time() - t0:.0f} s)", flush=True)
    return bad


def part_6():
    for table, key in np_.ADAM:
        if table == "long":
            case, calls = np_.long_calls(key)
            calls = [calls[0], calls[2]]
        else:
            _, T, S = key
            case, healthy = np_.segment_case("fhn", T, S, B=np_.LONG_B)
            calls = [healthy, np_.WILD_SCALES * np.random.default_rng(np_.SEGMENTS_SEED).standard_normal(healthy.shape)]
        for i, q in enumerate(calls):
            fin, half = finite_chains(np_.submit(case, q, False, range(len(q))))
            print(f"ADAM {key} call {i}: finite {fin}, value finite but gradient not {half}", flush=True)


def search(cid, n=12):
    seed0 = np_.LONG[cid][7]
    for seed in range(seed0, seed0 + 100 * n, 100):
        healthy, warm, wild = long_wild(cid, seed)
        fin, half = finite_chains(wild)
        ok = len(finite_chains(healthy)[0]) == 2 and len(finite_chains(warm)[0]) == 2
        print(f"  {cid} seed {seed}: wild finite {fin}, value only {half}, healthy and warm finite: {ok}", flush=True)
        if ok and len(fin) >= 2 and np_.LONG_B - len(fin) >= 2:
            return seed
    return None


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--search"]:
        print({cid: search(cid) for cid in args[1:]})
        status = 0
    elif args[:1] == ["long"]:
        status = part_4(args[1:] or list(np_.LONG))
    else:
        status = parts_1_to_3() + part_4(list(np_.LONG))
        part_6()
    ac.shutdown()
    sys.exit(1 if status else 0)
