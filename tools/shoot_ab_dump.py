"""A/B dump of everything the whole-chain multiple shooting writes (k_xobs_par, k_path_par), for comparing two builds of the
library bit for bit.

    CHMC_HIP_LIBRARY=<build A> python tools/shoot_ab_dump.py dump <dir A>
    python tools/shoot_ab_dump.py dump <dir B>                              (a fresh process per build)
    python tools/shoot_ab_dump.py compare <dir A> <dir B> [report file]

dump: every case of tests/test_paths.py::CASES through that file's four states (two steps, a switch, a second switch, off the
manifold), and once the two shapes of tools/path_posterior_timing.py after its warm-up (FitzHugh-Nagumo configs[1] with 256
chains, SIR boarding school with 1 024).  Per state one .npz: x_obs right after a switch, generate_x_seq at strides 1 and S,
and the sweep counts of both.  compare: one line per array, in the style of profiles/pair_passes_dump_compare.txt; exit
status 1 unless all are equal element for element (NaN equal to NaN)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402


def state_arrays(ctx, switched):
    q, _, x_obs, _ = ctx.get_state(want_p=False)
    out = {"q": q}  # (the state both builds must have started from, for the comparison to mean anything)
    if switched:
        out["x_obs"] = x_obs
    for stride in (1, ctx.S):
        out[f"x_seq_stride_{stride}"], out[f"sweeps_stride_{stride}"] = ctx.generate_x_seq(stride, return_sweeps=True)
    return out


def dump_case(name, dest):
    """The states of test_paths.path_body, without its checks."""
    import test_paths as tp
    from helpers import make_ctx
    cfg = tp.CASES[name]
    case = tp.build_case(cfg)
    ctx = make_ctx(case)
    rng = np.random.default_rng(cfg[10] + 1000)
    q_on, xo = tp.on_manifold_points(ctx, case, rng)
    ctx.set_state(q_on, rng.standard_normal((ctx.B, ctx.Q)), xo, 0)
    ctx.project_onto_cotangent_space()
    dt = np.where(np.arange(ctx.B) % 2 == 0, 1.0, -1.0) * (0.02 if case["model"] == "sir" else 0.04)
    for _ in range(2):
        ctx.leapfrog_step(dt)
    np.savez(os.path.join(dest, f"{name}.1_two_steps.npz"), **state_arrays(ctx, False))
    ctx.switch_partition()
    np.savez(os.path.join(dest, f"{name}.2_switch.npz"), **state_arrays(ctx, True))
    ctx.switch_partition()
    np.savez(os.path.join(dest, f"{name}.3_two_switches.npz"), **state_arrays(ctx, True))
    ctx.set_state(q_on + 0.01 * rng.standard_normal(q_on.shape), None, xo, 0)
    np.savez(os.path.join(dest, f"{name}.4_off_manifold.npz"), **state_arrays(ctx, False))
    ctx.close()


def dump_timing_shape(which, B, dest):
    """The state tools/path_posterior_timing.py measures at: its warm-up, whose last call is a partition switch."""
    from manifold_mcmc_for_diffusions_amd.workload import FhnWorkload, SirWorkload
    if which == "fhn":
        wl, dt = FhnWorkload(num_chains=B, num_steps_per_obs=400, device=0, device_init=True), 0.1
    else:
        wl, dt = SirWorkload(num_chains=B, keyed_init=True, total_chains=B), 0.05
    for _ in range(3):
        wl.refresh_momentum()
        act = np.ones(B, dtype=np.int32)
        for _ in range(4):
            act &= (wl.step(dt, active=act)["status"] == 0).astype(np.int32)
        wl.ctx.switch_partition()
    np.savez(os.path.join(dest, f"timing_{which}_{B}.switch.npz"), **state_arrays(wl.ctx, True))
    wl.ctx.close()


def dump(dest):
    import test_paths as tp
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"
    os.makedirs(dest, exist_ok=True)
    for name in tp.CASES:
        dump_case(name, dest)
        print("dumped", name, flush=True)
    for which, B in (("fhn", 256), ("sir", 1024)):
        dump_timing_shape(which, B, dest)
        print("dumped timing shape", which, B, flush=True)


def compare(dir_a, dir_b, report=None):
    lines, all_equal = [], True
    files = sorted(os.listdir(dir_a))
    assert files == sorted(os.listdir(dir_b)), "the two dumps hold different files"
    for f in files:
        a, b = np.load(os.path.join(dir_a, f)), np.load(os.path.join(dir_b, f))
        assert sorted(a.files) == sorted(b.files), f
        for k in sorted(a.files):
            same = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True)
            all_equal &= same
            verdict = "equal element for element" if same else f"DIFFERENT in {int(np.sum(a[k] != b[k]))} elements"
            extra = f"  sweeps {np.bincount(a[k]).tolist()}" if k.startswith("sweeps") else ""
            lines.append(f"{f[:-4]:44s} {k:18s} {str(a[k].shape):16s} {verdict}{extra}")
    lines.append("dumped outputs: all equal" if all_equal else "dumped outputs: NOT all equal")
    print("\n".join(lines))
    if report:
        with open(report, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return all_equal


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(0 if compare(*sys.argv[2:5]) else 1)
    else:
        sys.exit(__doc__)
