"""fp64 NumPy reference of the logistic-regression targets (reference: target_distributions/logistic_regression.py:20-67)
and the fixture tables.  ``LogRegRef`` has the oracle's target interface (oracle/targets.py), so ``oracle.train.OracleGMMVI``
runs on it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logreg_datasets.npz")
FILES = {"breast_cancer": "breast_cancer.data", "german_credit": "german.data-numeric"}
LOG_2PI = np.log(2 * np.pi)


def load_tables():
    """{"breast_cancer": [569, 32], "german_credit": [1000, 25]} fp64, as np.loadtxt reads upstream's files."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def write_dataset_dir(path):
    """Upstream's two files under ``path`` (text that np.loadtxt reads back bit-exactly)."""
    for key, t in load_tables().items():
        np.savetxt(os.path.join(path, FILES[key]), t, fmt="%.17g")
    return str(path)


def log_sigmoid(t):
    return np.minimum(t, 0.0) - np.log1p(np.exp(-np.abs(t)))


def sigmoid(t):
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def literal_preprocess(data, dataset_id):
    """The reference's steps, restated line by line (:26-40): -> (X~ [M, D] as f32 values in fp64, labels [M])."""
    if dataset_id == "breast_cancer":
        X = data[:, 2:].copy()
        labels = data[:, 1]
    else:
        X = data[:, :-1].copy()
        labels = data[:, -1] - 1
    X /= np.std(X, 0)[np.newaxis, :]
    X = np.hstack((np.ones((len(X), 1)), X))
    return X.astype(np.float32).astype(np.float64), labels


def literal_log_density(X, labels, w, prior_mean=0.0, prior_std=10.0):
    """log_density (:61-67) in NumPy fp64: features = -X w^T, tf.where(labels == 1, ...), normal prior."""
    w = np.atleast_2d(np.asarray(w, np.float64))
    features = -(X @ w.T)                                   # [M, N]
    lab = labels[:, None]
    ll = np.where(lab == 1, log_sigmoid(features), log_sigmoid(features) - features).sum(0)
    prior = np.sum(-np.log(prior_std) - 0.5 * LOG_2PI - 0.5 * ((w - prior_mean) / prior_std) ** 2, axis=1)
    return ll + prior


class LogRegRef:
    """sum_m log sigma(a_m . w) + isotropic normal prior, with its gradient, in fp64 on the signed matrix A."""

    def __init__(self, A, prior_mean=0.0, prior_std=10.0):
        self.A = np.asarray(A, np.float64)
        self.prior_mean, self.prior_std = float(prior_mean), float(prior_std)

    def get_num_dimensions(self):
        return self.A.shape[1]

    def _prior(self, w):
        z = (w - self.prior_mean) / self.prior_std
        return np.sum(-np.log(self.prior_std) - 0.5 * LOG_2PI - 0.5 * z * z, axis=1)

    def log_density(self, w):
        w = np.atleast_2d(np.asarray(w, np.float64))
        return log_sigmoid(w @ self.A.T).sum(1) + self._prior(w)

    def log_density_and_grad(self, w):
        w = np.atleast_2d(np.asarray(w, np.float64))
        t = w @ self.A.T                                    # [N, M]
        lp = log_sigmoid(t).sum(1) + self._prior(w)
        grad = sigmoid(-t) @ self.A - (w - self.prior_mean) / self.prior_std ** 2
        return lp, grad

    def abs_terms(self, w):
        """sum_m |log sigma(a_m . w)| per sample: the scale of the f32 rounding of lp."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        return np.abs(log_sigmoid(w @ self.A.T)).sum(1)

    def hessian(self, w):
        """Hessian at one point w [D] (Newton / Laplace in the tests)."""
        t = self.A @ w
        s = sigmoid(t) * sigmoid(-t)
        return -(self.A.T * s) @ self.A - np.eye(self.A.shape[1]) / self.prior_std ** 2
