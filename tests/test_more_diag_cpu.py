"""Pins tests/more_diag_ref.py, the fp64 restatement of the diagonal MORE estimate, without a GPU:
against the full-covariance oracle where the two coincide (D = 1), against the closed form for a Gaussian target, and the
unregularised bias entry."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import gmm as ogmm, more as omore, philox
import more_diag_ref as ref


def _one_dim_case(rng, k, n):
    means = rng.normal(size=(k, 1)) * 2.0
    var = rng.random((k, 1)) + 0.4
    w = rng.random(k) + 0.1
    w = w / w.sum()
    diag = ogmm.DiagonalGMM(w, means, var)
    full = ogmm.FullCovGMM(w, means, var[:, :, None])
    n_k = rng.multinomial(n, np.ones(k) / k)
    x, mapping = diag.sample_from_components_no_shuffle(n_k, philox.normals(3, 0, n, 1))
    tlp = -0.5 * np.square(x[:, 0] - 0.7) / 1.3 + 0.2 * np.sin(x[:, 0])      # not a quadratic: the fit is a true regression
    cnt = np.maximum(n_k, 1e-9)
    bg = logsumexp(diag.component_log_densities(x) + np.log(cnt / cnt.sum())[:, None], axis=0)
    return diag, full, x, mapping, tlp, bg


@pytest.mark.parametrize("own,snis", [(False, True), (False, False), (True, True)])
def test_one_dimension_equals_the_full_covariance_oracle(rng, own, snis):
    """D = 1: phi = [z^2, z, 1] is upstream's feature vector, so the restatement must equal oracle.more to fp64 rounding."""
    k, n = 3, 90
    diag, full, x, mapping, tlp, bg = _one_dim_case(rng, k, n)
    mp = mapping + (5 if own else 0)
    l2 = np.full(k, 1e-6)
    h, g = ref.get_expected_hessian_and_grad(diag, l2, x, mp, bg, tlp, own, snis)
    rh, rg = omore.get_expected_hessian_and_grad(full, l2, x, mp, bg, tlp, own, snis)
    assert h.shape == (k, 1) and g.shape == (k, 1)
    np.testing.assert_allclose(h[:, 0], rh[:, 0, 0], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(g[:, 0], rg[:, 0], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("snis", [True, False])
def test_gaussian_target_closed_form(rng, snis):
    """K = 1, model N(mu, diag sigma^2), target N(m, diag s^2): the reward log p - log q is exactly the diagonal quadratic
    -1/2 sum_i (1/s_i^2 - 1/sigma_i^2) x_i^2 + sum_i (m_i / s_i^2 - mu_i / sigma_i^2) x_i + c, so whatever the weights
    G_i = 1/s_i^2 - 1/sigma_i^2 and g_i = G_i mu_i - lin_i = (mu_i - m_i) / s_i^2."""
    d = 7
    n = 3 * (2 * d + 1)
    mu, sigma = rng.normal(size=d), rng.random(d) + 0.5
    m, s = rng.normal(size=d), rng.random(d) + 0.5
    model = ogmm.DiagonalGMM([1.0], mu[None], np.square(sigma)[None])
    x, mapping = model.sample_from_components_no_shuffle([n], philox.normals(4, 0, n, d))
    tlp = ogmm.DiagonalGMM.diagonal_gaussian_log_pdf(d, m, s, x)
    bg = rng.normal(size=n) - 5.0                                              # any weights
    h, g = ref.get_expected_hessian_and_grad(model, np.array([1e-10]), x, mapping, bg, tlp, False, snis)
    np.testing.assert_allclose(h[0], 1 / s ** 2 - 1 / sigma ** 2, rtol=0, atol=1e-6)
    np.testing.assert_allclose(g[0], (mu - m) / s ** 2, rtol=0, atol=1e-6)


def test_bias_entry_is_not_regularised(rng):
    """A constant added to every reward lands in the bias parameter alone when the bias carries no ridge
    (least_squares.py:71-73): G and g do not move for lambda > 0."""
    k, d, n = 2, 4, 60
    means, var = rng.normal(size=(k, d)), rng.random((k, d)) + 0.5
    model = ogmm.DiagonalGMM([0.4, 0.6], means, var)
    n_k = [25, 35]
    x, mapping = model.sample_from_components_no_shuffle(n_k, philox.normals(6, 0, n, d))
    tlp = -0.25 * np.sum(np.abs(x) ** 3, axis=1)
    bg = logsumexp(model.component_log_densities(x) + np.log(np.array(n_k) / n)[:, None], axis=0)
    l2 = np.full(k, 0.3)
    h0, g0 = ref.get_expected_hessian_and_grad(model, l2, x, mapping, bg, tlp)
    h1, g1 = ref.get_expected_hessian_and_grad(model, l2, x, mapping, bg, tlp + 123.0)
    np.testing.assert_allclose(h1, h0, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(g1, g0, rtol=1e-9, atol=1e-9)
    # ... and it would move them if the bias were regularised too: the check above is not vacuous
    assert np.abs(h0).max() > 1e-3


def test_a_component_without_samples_is_nan(rng):
    """own samples only, ridge 0, a component that drew nothing: its ridge system is singular -> NaN for it alone."""
    k, d = 2, 3
    model = ogmm.DiagonalGMM([0.5, 0.5], rng.normal(size=(k, d)), rng.random((k, d)) + 0.5)
    n = 40
    x, mapping = model.sample_from_components_no_shuffle([0, n], philox.normals(8, 0, n, d))
    tlp = -0.5 * np.sum(x * x, axis=1)
    h, g = ref.get_expected_hessian_and_grad(model, np.zeros(k), x, mapping, np.zeros(n), tlp, True, True)
    assert np.all(np.isnan(h[0])) and np.all(np.isnan(g[0]))
    assert np.all(np.isfinite(h[1])) and np.all(np.isfinite(g[1]))
