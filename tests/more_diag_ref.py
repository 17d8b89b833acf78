"""fp64 NumPy reference of the MORE estimate for DIAGONAL-covariance mixtures (csrc/more_diag.hip).

Upstream's MoreNgEstimator (gmmvi_modules/ng_estimator.py:296-376) whitens with a dense factor and regresses on every
product z_i z_j; it has no diagonal branch.  The project's definition restricts ``fit_quadratic`` / ``RegressionFunc.fit``
(optimization/least_squares.py:34-76, :126-191) to a diagonal quadratic: the features are the sufficient statistics of a
diagonal Gaussian, phi(z) = [z_1^2 .. z_D^2, z_1 .. z_D, 1] with z = (x - mu) / sigma, F = 2 D + 1.  The importance weights are
formed exactly as ``oracle.more.get_expected_hessian_and_grad`` forms them (the double normalisation included)."""
import numpy as np
from scipy.special import logsumexp


def diag_features(z):
    """[z^2, z, 1] -> [n, 2 d + 1]."""
    return np.concatenate([z * z, z, np.ones((z.shape[0], 1), z.dtype)], axis=1)


def fit_diag_quadratic(regularizer, inputs, outputs, weights, mean, sigma):
    """least_squares.py:126-191 for a diagonal quadratic -> (R [d], lin [d], theta [2 d + 1]); raises LinAlgError when the
    ridge system is not positive definite."""
    d = inputs.shape[1]
    z = (inputs - mean) / sigma                                                 # :172-173, elementwise
    phi = diag_features(z)
    f = phi.shape[1]
    wphi_t = (weights[:, None] * phi).T                                         # :65
    reg = np.eye(f) * regularizer
    reg[-1, -1] = 0.0                                                           # :71-73 (bias unregularised)
    a = wphi_t @ phi + reg
    c = np.linalg.cholesky(a)                                                   # :74-75
    theta = np.linalg.solve(c.T, np.linalg.solve(c, wphi_t @ outputs))
    quad = -2.0 * theta[:d] / (sigma * sigma)                                   # :177-179, :185 (diagonal of -Qt - Qt^T, un-whitened)
    lin = theta[d:2 * d] / sigma + quad * mean                                  # :186-188
    return quad, lin, theta


def importance_weights(log_w, self_normalized):
    """ng_estimator.py:353-358."""
    if self_normalized:
        log_w = log_w - logsumexp(log_w)
        w = np.exp(log_w)
        return w / np.sum(w)
    return np.exp(log_w)


def get_expected_hessian_and_grad(model, l2_regularizers, samples, mapping, background_densities, target_lnpdfs,
                                  only_use_own_samples=False, use_self_normalized_importance_weights=True):
    """-> (expected_hessian_neg [K, D] (diagonals), expected_gradient_neg [K, D]); NaN rows for a component whose ridge
    system is not positive definite.  ``model``: oracle.gmm.DiagonalGMM (chol_cov [K, D] = standard deviations)."""
    samples = np.asarray(samples, np.float64)
    k, d = model.num_components, model.num_dimensions
    mapping = np.asarray(mapping)
    relative_mapping = mapping - (np.max(mapping) if mapping.size else 0) + k - 1            # ng_estimator.py:342
    model_densities, cld = model.log_densities_also_individual(samples)                      # :344
    log_ratios = np.asarray(target_lnpdfs, np.float64) - model_densities                     # :347
    hs, gs = np.full((k, d), np.nan), np.full((k, d), np.nan)
    for i in range(k):
        if only_use_own_samples:                                                             # :110-118
            own = relative_mapping == i
            xs, rewards, lw = samples[own], log_ratios[own], np.zeros(int(own.sum()))
        else:
            xs, rewards, lw = samples, log_ratios, cld[i] - np.asarray(background_densities, np.float64)
        iw = importance_weights(lw, use_self_normalized_importance_weights) if xs.shape[0] else np.zeros(0)
        try:
            quad, lin, _ = fit_diag_quadratic(l2_regularizers[i], xs, rewards, iw, model.means[i], model.chol_cov[i])
        except np.linalg.LinAlgError:
            continue
        hs[i] = quad                                                                         # :369-370
        gs[i] = quad * model.means[i] - lin                                                  # :371-373
    return hs, gs
