"""Simulation-based calibration (Talts, Betancourt, Simpson, Vehtari & Gelman 2018), host side.

Draw a latent from the prior, simulate data from it, sample the posterior given those data: the rank of the prior draw
among L posterior draws is uniform on {0, ..., L} when the sampler targets the right posterior.  The check needs no second
implementation to compare with -- only that data and latent come from the same joint distribution, which
ChmcContext.simulate_observations does for every chain of a context at once (one data set per chain)."""
import math
import numpy as np


def ranks(prior_draw, posterior_draws):
    """prior_draw [D, P] (D data sets, P parameters), posterior_draws [D, L, P] (L thinned draws each): the rank statistic
    [D, P] = number of posterior draws strictly below the prior draw, in {0, ..., L}."""
    prior_draw, posterior_draws = np.asarray(prior_draw, dtype=np.float64), np.asarray(posterior_draws, dtype=np.float64)
    if posterior_draws.ndim != 3 or prior_draw.shape != (posterior_draws.shape[0], posterior_draws.shape[2]):
        raise ValueError(f"expected prior_draw [D, P] and posterior_draws [D, L, P], got {prior_draw.shape} and "
                         f"{posterior_draws.shape}")
    return (posterior_draws < prior_draw[:, None, :]).sum(1).astype(np.int64)


def _gammaincc(a, x):
    """Regularised upper incomplete gamma function Q(a, x) (series for x < a + 1, Lentz's continued fraction otherwise)."""
    if x <= 0.0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return max(0.0, 1.0 - total * lead)
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return min(1.0, h * lead)


def chi2_sf(statistic, dof):
    """P(chi^2(dof) >= statistic)."""
    return _gammaincc(0.5 * dof, 0.5 * float(statistic))


def uniformity(ranks, L, bins):
    """Per parameter, Pearson's chi^2 test of the ranks [D, P] (values in {0, ..., L}) against the uniform distribution:
    the L + 1 rank values are cut into `bins` contiguous bins of (as nearly as possible) equal probability.  Returns
    (statistic [P], p_value [P]); under uniformity the statistic is chi^2(bins - 1).  The expected count per bin, D / bins,
    should be at least 5 or so."""
    r = np.asarray(ranks)
    if r.ndim != 2:
        raise ValueError(f"ranks must be [D, P], got {r.shape}")
    if r.min(initial=0) < 0 or r.max(initial=0) > L:
        raise ValueError(f"ranks must lie in [0, {L}]")
    if not 2 <= bins <= L + 1:
        raise ValueError(f"need 2 <= bins <= L + 1 = {L + 1}")
    D = r.shape[0]
    edges = np.floor(np.arange(bins + 1) * (L + 1) / bins).astype(np.int64)  # bin b holds the rank values edges[b] .. edges[b + 1] - 1
    expected = D * np.diff(edges) / (L + 1.0)
    which = np.searchsorted(edges, r, side="right") - 1
    stat = np.empty(r.shape[1])
    for j in range(r.shape[1]):
        counts = np.bincount(which[:, j], minlength=bins)
        stat[j] = ((counts - expected) ** 2 / expected).sum()
    return stat, np.array([chi2_sf(s, bins - 1) for s in stat])
