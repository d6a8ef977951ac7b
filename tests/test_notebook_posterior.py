"""Statistical pin against the reference's only known-answer material for this path: the posterior table printed by
FitzHugh-Nagumo_example.ipynb (tests/golden/reference_data/notebook_posterior_table.json).  The notebook's experiment
is re-run on the GPU (same data from the same legacy seed, same model, priors, discretisation, splitting, solver and
tolerances; a static-trajectory sampler instead of Mici's dynamic one, 64 chains instead of 2) and the posterior means
must agree within Monte-Carlo error, the posterior standard deviations within 15 %.  Selection step (not in the
reference, whose two chains were simply two usable prior draws): candidate starts are screened by a short pilot run and
chains that move in fewer than 10 % of their main transitions (unusable starts), or whose parameter means over the first
fifth and the second half of the main phase differ by more than 4 within-chain standard deviations (released late: still
in their transient), are left out of the summary and counted."""
import os
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_data_regenerated_from_the_notebook_seed():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import fhn_notebook_posterior as nb
    d = nb.notebook_data()
    np.testing.assert_allclose(d["q_ref"][:3], [1.62073967, 1.08346121, 0.67204724], atol=5e-9)
    assert d["y"].shape == (100,) and np.isfinite(d["y"]).all()
    # data-generating parameters of the notebook's corner plot truths: generate_z(q_ref[:4])
    np.testing.assert_allclose(d["z_ref"], [np.exp(0.5 * d["q_ref"][0] - 1), np.exp(0.5 * d["q_ref"][1] - 2),
                                            0.5 * d["q_ref"][2] + 1, 0.5 * d["q_ref"][3] + 1])


@pytest.mark.timeout(900)
def test_posterior_matches_the_notebook_table(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import fhn_notebook_posterior as nb
    rows, res, n_moving = nb.run(64, 700, 200, 24, out_dir=str(tmp_path / "run"), verbose=False)
    assert n_moving >= 56                               # at most a few stuck starts
    assert 0.6 < res["accept_stat"][200:].mean() < 0.95
    for r in rows:
        assert abs(r["z"]) < 3.5, r                     # means agree within Monte-Carlo error
        assert 0.85 < r["sd"] / r["ref_sd"] < 1.15, r   # posterior spread agrees
        assert r["r_hat"] < 1.1, r


@pytest.mark.timeout(900)
def test_posterior_and_sampler_statistics_with_the_dynamic_transition(tmp_path):
    """The same experiment with the batched dynamic (no-U-turn, multinomial) transition, the counterpart of the
    notebook's own MultinomialDynamicIntegrationTransition: besides the posterior table, the statistics the notebook's
    progress bar reports after adaptation (accept_stat 0.83, n_step 28.3, convergence_error 0.15) are of the same
    size."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import fhn_notebook_posterior as nb
    rows, res, n_moving = nb.run(64, 450, 150, 0, out_dir=str(tmp_path / "run"), verbose=False, transition="dynamic")
    # every chain adapts its own step size during warm-up (as Mici's adapter does), so no start is left behind ...
    assert n_moving >= 60
    # ... and the main phase runs with the MEAN of the chains' adapted step sizes (Mici's finalize): with 64 prior draws as
    # starts, a few of them in stiff regions with tiny adapted steps, that mean is shorter than what a healthy chain would
    # pick, hence an accept statistic above the 0.8 target (the notebook's two chains: 0.83)
    assert 0.7 < res["accept_stat"][150:].mean() < 0.97
    #  the step size itself, not only its consequence: the main phase's step size is the arithmetic mean of the
    # chains' adapted ones, and it must be of the size the bulk of the chains picked -- a mean dragged far below the
    # median by tiny steps (or a main phase that simply runs too small a step) would pass an accept window alone
    assert "adapted_step_sizes" in res
    eps = res["adapted_step_sizes"]
    qs = np.quantile(eps, [0.0, 0.1, 0.5, 0.9, 1.0])
    print("per-chain adapted step sizes: min / 10 % / median / 90 % / max =", np.round(qs, 4), "mean", round(float(eps.mean()), 4),
          "main phase", round(res["final_step_size"], 4), "accept", round(float(res["accept_stat"][150:].mean()), 3),
          "n_step", round(float(res["n_step"][150:].mean()), 1))
    assert abs(res["final_step_size"] - eps.mean()) <= 1e-12 * eps.mean()
    assert 0.6 * qs[2] < res["final_step_size"] < 1.5 * qs[2], (qs, res["final_step_size"])
    assert 15.0 < res["n_step"][150:].mean() < 45.0
    assert res["integrator_error"][150:].mean() < 0.4
    for r in rows:
        assert abs(r["z"]) < 3.5, r
        assert 0.85 < r["sd"] / r["ref_sd"] < 1.15, r
        assert r["r_hat"] < 1.1, r
