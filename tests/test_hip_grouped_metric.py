"""Per-chain block metrics on the device (chmc_set_metrics): one M_0 per group of chains in one context.

The layouts of tests/grouped_obs.py without the Gaussian-splitting one (no metric there), three groups of 4, 5 and 4 chains,
every group with its own data (y_g, sigma_g) and its own M_g = random_metric(default_rng(100 + g), U) -- pairwise apart by at
least 1.0 in some entry, asserted before anything is compared, so that a broadcast of chain 0's metric cannot pass."""
import os
import subprocess
import sys
import pytest
import grouped_metric as gm
import grouped_obs as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C_, D, E, F, G = gm.LAYOUTS

# (layout, switches pinned for BOTH sides)
CASES = [(name, {}) for name in gm.LAYOUTS]
CASES += [(name, {"CHMC_HALVES": "2"}) for name in (A, C_, D, F, G)]  # (e: one block per chain is always one batch)
CASES += [(A, {"CHMC_PAR_SCAN": "1"}), (F, {"CHMC_PAR_SCAN": "1"}), (E, {"CHMC_PAR_SCAN": "0"})]
CASES += [(A, {"CHMC_STEP_FUSIONS": "0"})]
CASES += [(E, {"CHMC_RETRACT_KERNEL": k}) for k in "012"]
# the two row families that are latched by the first context of a process: a child process each
CHILD_CASES = [("CHMC_COMPACT_ROWS", "0", (A, C_, E)), ("CHMC_GRAM_MFMA", "1", (A, C_))]


def _hip():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert _lib.lib().chmc_backend() == b"hip:gfx950"
    return _lib.lib()


def grouped_equals_separate(name, env):
    gc = go.make_groups(name, seed=41)
    control_bad, bad, whole, diag = gm.run_grouped_vs_separate(gc)
    assert not control_bad, f"control (shared data and metric, one context against the 4 | 5 | 4 split) differs: {control_bad}"
    assert not bad, f"per-chain metrics against one context per group differ: {bad}"
    gm.assert_status_pattern(whole)
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
def test_grouped_metrics_equal_separate_contexts(monkeypatch, name, env):
    """GPU test 1: one context of 13 chains with per-chain (y, sigma, M_0) equals three contexts with their group's shared
    data and set_metric(M_g), bit for bit, over everything grouped_obs.run_sequence records.  The fair-case control (ONE
    shared data set and metric, one context against the same split) is judged first, in the same run; groups 1 and 2 differ
    from a run with group 0's matrix on every chain."""
    _hip()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    grouped_equals_separate(name, env)


_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_hip_grouped_metric as t
t._hip()
for name in {names!r}:
    print(name, t.grouped_equals_separate(name, {env!r}))
print("GROUPED_OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("switch,value,names", CHILD_CASES, ids=[c[0][5:] for c in CHILD_CASES])
def test_grouped_metrics_equal_separate_contexts_row_families(switch, value, names):
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
def test_grouped_metrics_against_the_oracle(name):
    """GPU test 2: every operator at 1e-10, two Newton and two quasi-Newton steps at 1e-9 with equal statuses and iteration
    counts, every chain against the C oracle built from its own group's (y, sigma) with set_metric(M_g)."""
    _hip()
    print(name, gm.check_against_oracle(name))


@pytest.mark.gpu
def test_momentum_of_a_grouped_context():
    """GPU test 4: the u-part of the momentum is chol(M_g) @ keyed normals, projected with the chain's own J M_g^-1."""
    _hip()
    print(gm.check_momentum())


@pytest.mark.gpu
def test_api_misuse():
    """GPU test 5: non-symmetric / indefinite matrix in one chain (named), Gaussian splitting, another thread; back to one
    shared matrix and to the identity, bitwise."""
    gm.check_api_misuse(_hip())


# Seeds screened on the CPU with the oracle alone (grouped_metric.check_transitions(.., screening=True), seeds 1 .. 8 per
# layout): no inadmissible margin on any chain, every tree reaches 7 leaves, trajectories are accepted.  (e: seeds 3 and 7
# have a position_tol margin of 5e-3 on one chain and are not used.)
TRANSITION_SEEDS = [(A, 1, 0.05), (E, 4, 0.02)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,eps", TRANSITION_SEEDS)
def test_transitions_against_each_chains_own_oracle(name, seed, eps):
    """GPU test 3: one no-U-turn transition and one static transition, every chain judged by the restatements of helpers.py on
    the oracle system of its own (y, sigma) with its own M_g."""
    _hip()
    print(name, gm.check_transitions(name, seed, eps))
