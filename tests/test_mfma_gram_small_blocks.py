"""CHMC_GRAM_MFMA=1 on layouts whose blocks have at most 8 rows (FitzHugh-Nagumo): BASELINE.json configs[4] as written.

With the switch set these layouts run on the stored-rows kernel family, the sweeps only store the rows
(k_rev_wave<.., GRAM = false>) and every Gram block -- of a state evaluation and of every Newton iteration -- is formed
by k_gram_rows_mfma<RM> (v_mfma_f64_16x16x4_f64, the block's columns folded into the 16 x 16 tile in two halves).  The
switch is read once per process, so every case runs in a child process of its own with the switch in its environment.

Tolerances are those of tests/test_hip_parity.py: 1e-10 per op, 1e-9 per step at equal statuses and iteration counts
(the helpers assert the counts for every chain); the MFMA path differs from the vector kernels in summation order only.
The library's launch counter must show that the MFMA kernel formed the Gram blocks: on a library without the small-block
kernel the counter stays 0 for these layouts and every child fails there.

Row slots: only R = 5 with noisy observations gives the 7-row layout (5 observation rows + 2 state rows, RM == 7, the
layout of configs[4]); the other small shapes have 4 to 6 rows in 6 or 8 slots, which covers the zero-padded operand rows
RM .. 7 at other values of RM as well.  RM is asserted per case."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import make_case, make_ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_PRELUDE = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_case, make_ctx, check_ops_against_oracle, check_steps_against_oracle, check_block_metric_against_oracle


def counted_state_eval_and_newton_step(ctx, case, dts):
    # the MFMA kernel formed the Gram blocks: one launch per state evaluation, one per Newton iteration of a step
    B = case["B"]
    qq, xx = np.repeat(case["q"][:1], B, 0), np.repeat(case["x_obs"][:1], B, 0)
    d0 = ctx.diagnostics()
    ctx.set_state(qq, case["rng"].standard_normal((B, ctx.Q)), xx, 0)
    ctx.chol_gram_blocks()
    d1 = ctx.diagnostics()
    assert d1["gram_mfma_launches"] - d0["gram_mfma_launches"] >= 1, ("state evaluation", d0, d1)
    ctx.project_onto_cotangent_space()
    d2 = ctx.diagnostics()
    res = ctx.leapfrog_step(np.broadcast_to(np.asarray(dts, dtype=np.float64), (B,)), newton=True)
    d3 = ctx.diagnostics()
    assert (res["status"] == 0).all(), res
    iters = int((res["iters_fwd"] + res["iters_bwd"]).max())
    assert d3["gram_mfma_launches"] - d2["gram_mfma_launches"] >= 1 + iters, ("newton step", iters, d2, d3)
    assert d3["gram_valu_launches"] == 0
    print("MFMA_LAUNCHES", d3["gram_mfma_launches"], "IN_STEP", d3["gram_mfma_launches"] - d2["gram_mfma_launches"],
          "ITERS", iters)
"""

_SMALL_SCRIPT = _PRELUDE + r"""
kw = dict(gaussian={gaussian}, var_sigma={var_sigma})
case = make_case({model!r}, {T}, {S}, {R}, {noisy}, B=3, seed=11, **kw)
ctx = make_ctx(case)
assert ctx.L.chmc_backend() == b"hip:gfx950"
assert ctx.RM == {rm}, ctx.RM
worst = check_ops_against_oracle(ctx, case)
print("OPS_WORST", worst)
ctx.close()
case = make_case({model!r}, {T}, {S}, {R}, {noisy}, B=4, seed=12, **kw)
ctx = make_ctx(case)
dts = np.array([0.05, -0.05, 0.1, 0.02])
for newton in (True, False):
    for part in range(ctx.num_partition):
        print("STEPS", newton, part, check_steps_against_oracle(ctx, case, dts, newton=newton, n_steps=3, part=part))
counted_state_eval_and_newton_step(ctx, case, dts)
ctx.close()
"""

_METRIC_SCRIPT = _PRELUDE + r"""
case = make_case("fhn", 12, 16, 5, True, B=4, seed=41)
ctx = make_ctx(case)
assert ctx.RM == 7, ctx.RM
dts = np.array([0.05, -0.05, 0.08, 0.02])
print("OPS_WORST", check_block_metric_against_oracle(ctx, case, {newton}, dts))
counted_state_eval_and_newton_step(ctx, case, dts)
ctx.close()
"""

_FULL_SCRIPT = _PRELUDE + r"""
case = make_case("fhn", 100, 800, 5, True, B=2, seed=20)
ctx = make_ctx(case)
assert ctx.Q == 160106 and ctx.C == [138, 140] and ctx.RM == 7
print("STEPS", check_steps_against_oracle(ctx, case, np.array([0.05, -0.05]), n_steps=1))
counted_state_eval_and_newton_step(ctx, case, np.array([0.05, -0.05]))
ctx.close()
"""

# (the script of test_hip_parity.py::test_compact_row_kernels_agree_with_the_stored_row_kernels_full_size, FHN case)
_PATH_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from helpers import make_case, make_ctx
B = 6
case = make_case("fhn", 100, 400, 5, True, B=B, seed=77)
ctx = make_ctx(case)
assert ctx.RM == 7
rng = np.random.default_rng(5)
out = {{}}
for part in range(ctx.num_partition):
    ctx.set_state(np.repeat(case["q"][:1], B, 0), rng.standard_normal((B, ctx.Q)), np.repeat(case["x_obs"][:1], B, 0), part)
    ctx.project_onto_cotangent_space()
    dts = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.02 + 0.01 * np.arange(B))
    d0 = ctx.diagnostics()["gram_mfma_launches"]
    res = [ctx.leapfrog_step(dts) for _ in range(2)]
    d1 = ctx.diagnostics()["gram_mfma_launches"]
    q, p, xo, _ = ctx.get_state()
    ctx.switch_partition()
    q2, p2, xo2, _ = ctx.get_state()
    out.update({{f"q{{part}}": q, f"p{{part}}": p, f"xo{{part}}": xo2, f"st{{part}}": np.stack([r["status"] for r in res]),
                f"it{{part}}": np.stack([r["iters_fwd"] + r["iters_bwd"] for r in res]), f"h{{part}}": ctx.hamiltonian(),
                f"mfma{{part}}": np.array([d1 - d0, sum(1 + int((r["iters_fwd"] + r["iters_bwd"])[r["status"] == 0].max())
                                                      for r in res)])}})
out["valu"] = np.array(ctx.diagnostics()["gram_valu_launches"])
np.savez({out!r}, **out)
"""


def _run_child(script, env, timeout):
    """One child process with the GPU open at a time, under a time limit; the caller starts nothing after a failure."""
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _fmt(script, **kw):
    return script.format(root=ROOT, tests=os.path.join(ROOT, "tests"), **kw)


SMALL_FHN = [
    # model, T, S, R, noisy, gaussian, var_sigma, row slots: the FitzHugh-Nagumo rows of test_hip_parity.py::SMALL ...
    ("fhn", 6, 4, 2, True, False, False, 8),
    ("fhn", 7, 5, 3, False, False, False, 8),
    ("fhn", 6, 4, 2, True, True, False, 8),
    ("fhn", 5, 4, None, True, False, False, 8),
    ("fhn", 12, 10, 5, True, False, False, 7),
    ("fhn", 12, 10, 5, False, True, False, 6),
    ("fhn_nb", 7, 5, 3, False, True, False, 8),
    ("fhn_nb", 6, 4, 2, True, False, False, 8),
    # ... and variable observation noise (dim_u = 5: the sigma column of dc/du, sigma_l sigma_r on the Gram diagonal)
    ("fhn", 6, 8, 2, True, False, True, 8),
    # ... and the other model the dispatch reaches with at most 8 rows (X = V = 3: three columns per step)
    ("sir", 6, 8, 2, True, False, False, 8),
]


@pytest.mark.parametrize("model,T,S,R,noisy,gaussian,var_sigma,rm", SMALL_FHN)
def test_small_shapes_ops_and_steps(model, T, S, R, noisy, gaussian, var_sigma, rm):
    """Every per-op entry point (1e-10) and three Newton and three quasi-Newton steps per partition (1e-9, equal statuses
    and iteration counts) against the C oracle: a last block with fewer rows than slots, the first block's v_0 columns,
    blocks far shorter than one tile of 2 x 64 columns, both partitions.  Then the launch counter across a state evaluation
    and across a Newton step."""
    out = _run_child(_fmt(_SMALL_SCRIPT, model=model, T=T, S=S, R=R, noisy=noisy, gaussian=gaussian, var_sigma=var_sigma,
                          rm=rm), {"CHMC_GRAM_MFMA": "1"}, 600)
    assert "MFMA_LAUNCHES" in out, out[-2000:]


@pytest.mark.parametrize("newton", [True, False])
def test_block_metric(newton):
    """M = blockdiag(M_0, I) on the 7-row layout: helpers.check_block_metric_against_oracle as
    test_hip_parity.py::test_block_metric calls it (ops, retraction with its multiplier term, momentum sampling, steps)."""
    out = _run_child(_fmt(_METRIC_SCRIPT, newton=newton), {"CHMC_GRAM_MFMA": "1"}, 600)
    assert "MFMA_LAUNCHES" in out, out[-2000:]


def test_full_size_configs4_shape_against_oracle():
    """BASELINE.json configs[4]'s shape (T = 100, S = 800, R = 5, noisy: Q = 160106, 20 / 21 blocks of 7 rows), one step
    against the oracle at 1e-9 with equal counts.  The block lengths (8 000 + 2 columns, 4 000 for the half blocks of
    the second partition) are not multiples of the tile and the first block's two column halves differ from the others'."""
    out = _run_child(_fmt(_FULL_SCRIPT), {"CHMC_GRAM_MFMA": "1"}, 900)
    assert "MFMA_LAUNCHES" in out, out[-2000:]


def test_mfma_family_agrees_with_the_vector_stored_row_kernels_full_size(tmp_path):
    """The same stored-rows family with its Gram blocks formed by vector FMAs inside the sweeps (CHMC_COMPACT_ROWS=0)
    and by the MFMA kernel from the stored rows (CHMC_GRAM_MFMA=1): FHN, T = 100, S = 400, R = 5, 6 chains, two steps per
    partition and a partition switch.  Statuses and iteration counts equal, positions, momenta, x_obs and Hamiltonians to
    1e-9 relative; the MFMA run's counter covers every state evaluation and Newton round of its steps, the vector run's
    stays 0."""
    outs = []
    for name, env in (("stored", {"CHMC_COMPACT_ROWS": "0"}), ("mfma", {"CHMC_GRAM_MFMA": "1"})):
        out = str(tmp_path / f"{name}.npz")
        _run_child(_fmt(_PATH_SCRIPT, out=out), env, 600)
        outs.append(np.load(out))
    a, b = outs
    for k in a.files:
        if k.startswith("mfma") or k == "valu":
            continue
        if k.startswith(("st", "it")):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        else:
            scale = max(np.abs(a[k]).max(), 1.0)
            assert np.abs(a[k] - b[k]).max() <= 1e-9 * scale, (k, np.abs(a[k] - b[k]).max(), scale)
    for part in (0, 1):
        assert a[f"mfma{part}"][0] == 0, a[f"mfma{part}"]
        assert b[f"mfma{part}"][0] >= b[f"mfma{part}"][1] > 0, b[f"mfma{part}"]
    assert int(b["valu"]) == 0


def test_switch_unset_leaves_the_default_family():
    """Without the switch the 7-row layout runs its default kernels: the MFMA kernel is never launched."""
    assert not os.environ.get("CHMC_GRAM_MFMA")
    case = make_case("fhn", 12, 10, 5, True, B=4, seed=12)
    ctx = make_ctx(case)
    assert ctx.RM == 7
    B = case["B"]
    ctx.set_state(np.repeat(case["q"][:1], B, 0), case["rng"].standard_normal((B, ctx.Q)), np.repeat(case["x_obs"][:1], B, 0), 0)
    ctx.project_onto_cotangent_space()
    res = ctx.leapfrog_step(np.array([0.05, -0.05, 0.1, 0.02]))
    assert (res["status"] == 0).all()
    assert ctx.diagnostics()["gram_mfma_launches"] == 0
    ctx.close()
