"""Per-chain observations on the device (chmc_set_observations): many data sets and noise levels in one context.

Layouts (tests/grouped_obs.py), the smallest that still reach each kernel family:
  a  FHN noisy (12, 16, 5)          7 row slots, 3 blocks, both partitions
  b  FHN noiseless (12, 16, 5), Gaussian splitting: per-chain y only
  c  FHN noisy (20, 8, 10)          16-row blocks, K > 1
  d  FHN noisy (130, 8, 2)          more than 64 blocks per chain
  e  SIR (14, 8, 14), interval 0.25 one 16-row block: k_traj_chain / k_retract_chain by default, the batched path and the
                                    four-wavefront form through CHMC_RETRACT_KERNEL = 0 and 2
  f  SIR (26, 24, 13)               multi-block 16-row
  g  FHN (12, 16, 5), variable noise: per-chain y, sigma from u
Three groups of 4, 5 and 4 chains (B = 13; CHMC_HALVES=2 splits 6 | 7, inside a group) whose data differ in every entry by at
least 0.05 and whose noise levels are distinct -- asserted before anything is compared, so that a broadcast of chain 0's data
cannot pass."""
import os
import subprocess
import sys
import numpy as np
import pytest
import grouped_obs as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B_, C_, D, E, F, G = sorted(go.LAYOUTS)

# (layout, switches pinned for BOTH sides): the default switches everywhere, every other switch where it selects something
CASES = [(name, {}) for name in sorted(go.LAYOUTS)]
CASES += [(name, {"CHMC_HALVES": "2"}) for name in (A, B_, C_, D, F, G)]       # (e: one block per chain is always one batch)
CASES += [(A, {"CHMC_PAR_SCAN": "1"}), (F, {"CHMC_PAR_SCAN": "1"}), (E, {"CHMC_PAR_SCAN": "0"})]
CASES += [(A, {"CHMC_STEP_FUSIONS": "0"}), (B_, {"CHMC_STEP_FUSIONS": "0"})]
CASES += [(E, {"CHMC_RETRACT_KERNEL": k}) for k in "012"]
# the two row families that are latched by the first context of a process: a child process each
CHILD_CASES = [("CHMC_COMPACT_ROWS", "0", (A, C_, E)), ("CHMC_GRAM_MFMA", "1", (A, C_))]


def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"
    return _lib.lib()


def grouped_equals_separate(name, env):
    gc = go.make_groups(name, seed=41)
    control_bad, bad, whole, diag = go.run_grouped_vs_separate(gc)
    # The control runs first; its verdict is reported with the result, and a layout whose control fails would be judged at
    # the per-operator bounds instead -- none does.
    assert not control_bad, f"control (shared data, one context against the 4 | 5 | 4 split) differs: {control_bad}"
    assert not bad, f"per-chain data against one context per group differs: {bad}"
    rec = dict(whole)
    status0 = rec["step0.status"]
    assert status0[5] == -1 and (status0[[2, 7]] > 0).all() and (np.delete(status0, [2, 5, 7]) == 0).all(), status0
    assert (rec["steps.n_done"] == 2).all()
    # the family the case is there for did run
    if name == E:
        per_chain = env.get("CHMC_RETRACT_KERNEL", "1") != "0" and "CHMC_COMPACT_ROWS" not in env
        assert (diag["traj_kernel_launches"] > 0) == per_chain, diag
    if env.get("CHMC_GRAM_MFMA") == "1":
        assert diag["gram_mfma_launches"] > 0, diag
    if name == A and not env.keys() & {"CHMC_COMPACT_ROWS", "CHMC_GRAM_MFMA"}:
        assert diag["newton_fsm_launches"] > 0, diag
    if name == D and not env:
        assert diag["newton_factor8_launches"] > 0, diag
    return diag


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", CASES, ids=[n[:1] + "".join(f"-{k[5:]}={v}" for k, v in e.items()) for n, e in CASES])
def test_grouped_context_equals_separate_contexts(monkeypatch, name, env):
    """GPU test 1: one context of 13 chains with per-chain (y, sigma) equals three contexts with their group's shared data,
    bit for bit -- positions, momenta, statuses, iteration counts, reverse-check distances, Hamiltonians, log_det_sqrt_gram
    and its gradient, the partition switch, the comparator target and its gradient -- over one step from unprojected momenta,
    three leapfrog_step calls with a masked and two failing chains (dt = 5.0) and one leapfrog_steps(.., 2).  The fair-case
    control (ONE shared data set, one context against the same split) is judged first, in the same run."""
    _hip()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    grouped_equals_separate(name, env)


_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_hip_grouped_observations as t
t._hip()
for name in {names!r}:
    print(name, t.grouped_equals_separate(name, {env!r}))
print("GROUPED_OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("switch,value,names", CHILD_CASES, ids=[c[0][5:] for c in CHILD_CASES])
def test_grouped_context_equals_separate_contexts_row_families(switch, value, names):
    """The same with CHMC_COMPACT_ROWS=0 (stored rows) and CHMC_GRAM_MFMA=1 (the MFMA Gram build).  One child under a time
    limit; nothing is started after a failure."""
    _hip()
    env = {switch: value}
    script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), names=names, env=env)
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    print(env, r.stdout[-3000:])
    assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
    assert "GROUPED_OK" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", [A, C_, E, G])
def test_grouped_context_against_the_oracle(name):
    """GPU test 2: every operator at 1e-10, two Newton and two quasi-Newton steps at 1e-9 with equal statuses and iteration
    counts, every chain against the C oracle built from its own group's (y, sigma)."""
    _hip()
    gc = go.make_groups(name, seed=42)
    ctx = go.grouped_ctx(gc)
    worst = go.check_grouped_against_oracle(ctx, gc)
    print(name, worst)
    ctx.close()


@pytest.mark.gpu
def test_api_misuse():
    """GPU test 6: a per-chain sigma with noisy 0 or 2, a non-positive sigma, a call from another thread than the creator's:
    a negative return value, a chmc_last_error text, and the context stays usable."""
    from test_grouped_observations import check_api_misuse
    check_api_misuse(_hip())


@pytest.mark.gpu
@pytest.mark.parametrize("name", [A, B_, E, G])
def test_simulate_observations(name):
    """GPU test 4: a prior draw per chain, the data it generates, the chain on the manifold of its own data."""
    _hip()
    print(name, go.check_simulated_observations(name))


@pytest.mark.gpu
def test_fhn_finders_on_a_grouped_context():
    """GPU test 5: linear-interpolation initial states and the gradient-descent finder, every chain from its own data."""
    _hip()
    print(go.check_fhn_finders())


@pytest.mark.gpu
def test_sir_keyed_finder_on_a_grouped_context():
    """GPU test 5: the keyed noisy Adam finder (device-resident loop) on a grouped single-block SIR context."""
    _hip()
    print(go.check_sir_keyed_finder(adam_step_size=0.1, max_iters=3000, threshold=1.0, device_resident=True))


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,eps", [(A, 1, 0.05), (E, 4, 0.02)])
def test_transitions_against_each_chains_own_oracle(name, seed, eps):
    """GPU test 3: one no-U-turn transition and one static transition per layout family, every chain judged by the
    restatements of helpers.py on the oracle system of its own (y, sigma)."""
    _hip()
    print(name, go.check_transitions(name, seed, eps))
