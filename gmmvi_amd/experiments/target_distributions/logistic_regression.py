"""Bayesian logistic regression on Breast Cancer / German Credit (reference:
src/gmmvi/experiments/target_distributions/logistic_regression.py:11-67).

The reference's posterior, for every w,
    log p(w) = sum_m where(label_m == 1, log sigmoid(-x~_m w), log sigmoid(-x~_m w) + x~_m w) + sum_d log N(w_d; 0, 10^2)
is sum_m log sigmoid(a_m . w) with a_m = s_m x~_m, s_m = -1 where the label is 1 and +1 otherwise (x~ the features divided
by their ddof-0 standard deviation in fp64, behind a bias column of ones, cast to f32).  The sign convention is upstream's
and is kept: it is the posterior the reference benchmarks report.  The device evaluates it with its analytic gradient in
one launch (csrc/logreg.hip) on the signed matrix A = diag(s) X~.

``LogisticRegressionMinibatch`` is upstream's minibatch variant (logistic_regression.py:70-174): the last
``size_test_set`` rows are held out, and the likelihood of every sample is T times the mean over a batch of ``batch_size``
training rows.  Upstream reshuffles with TensorFlow's stateful RNG on every call; this build defines the batches instead
(DESIGN.md 6): call c (the target's call counter) permutes the T training rows by rho_c, the Feistel/Philox permutation of
minibatch_stream.py with key ``seed`` and counter (R | i << 24, 0, c, 4), and sample n takes batch n mod nb, with
nb = floor(T / B) with ``use_own_batch_per_sample`` (upstream's advancing ``start``) and 1 without.  ``minibatch_rows``
restates the map in NumPy; the device evaluates it in csrc/logreg_mb.hip.

The datasets do not ship with the package: ``dataset_dir`` (``environment_config["dataset_dir"]``), else the
``GMMVI_DATASET_DIR`` environment variable, names a directory with upstream's files ``breast_cancer.data`` and
``german.data-numeric``.
"""
import os

import numpy as np

from ... import _lib, hip_ops
from ...device import get_context
from .lnpdf import LNPDF
from .minibatch_stream import STREAM_LOGREG_MINIBATCH as STREAM_MINIBATCH
from .minibatch_stream import MinibatchLNPDF, permute_rows

DATASET_FILES = {"breast_cancer": "breast_cancer.data", "german_credit": "german.data-numeric"}
DATASET_DIR_ENV = "GMMVI_DATASET_DIR"
PRIOR_MEAN, PRIOR_STD = 0.0, 10.0                   # logistic_regression.py:33-34, :43-44
MAX_DIM_MINIBATCH = 128                             # what csrc/logreg_mb.hip supports


def split_table(data, dataset_id):
    """Raw table as np.loadtxt reads it -> (features [M, F] fp64, labels [M] fp64) (logistic_regression.py:27-30, :37-40)."""
    data = np.asarray(data, np.float64)
    if dataset_id == "breast_cancer":
        return data[:, 2:], data[:, 1]
    if dataset_id == "german_credit":
        return data[:, :-1], data[:, -1] - 1
    raise ValueError(f"unknown logistic-regression dataset {dataset_id!r} (expected one of {sorted(DATASET_FILES)})")


def signed_data_matrix(X, labels):
    """A = diag(s) X, s_m = -1 where labels_m == 1 and +1 otherwise (fp64): then sum_m log sigmoid(a_m . w) is the
    reference's tf.where(labels == 1, log_sigmoid(-X w), log_sigmoid(-X w) + X w)."""
    X = np.asarray(X, np.float64)
    s = np.where(np.asarray(labels) == 1, -1.0, 1.0)
    return s[:, None] * X


def preprocess(data, dataset_id):
    """Raw table -> (A [M, D] f32, D): divide by the ddof-0 standard deviation (fp64), prepend the bias column, sign the rows,
    cast to f32.  The sign flip is exact, so A == diag(s) f32(X~)."""
    X, labels = split_table(data, dataset_id)
    X = X / np.std(X, 0)[np.newaxis, :]
    X = np.hstack((np.ones((len(X), 1)), X))
    A = signed_data_matrix(X.astype(np.float32).astype(np.float64), labels).astype(np.float32)
    return A, int(A.shape[1])


def resolve_dataset_dir(dataset_dir=None):
    d = dataset_dir if dataset_dir is not None else os.environ.get(DATASET_DIR_ENV)
    if not d:
        raise FileNotFoundError(
            f"no dataset directory for the logistic-regression targets: set environment_config['dataset_dir'] or the "
            f"{DATASET_DIR_ENV} environment variable to a directory holding {DATASET_FILES['breast_cancer']} and "
            f"{DATASET_FILES['german_credit']}")
    return d


def load_table(dataset_id, dataset_dir=None):
    if dataset_id not in DATASET_FILES:
        raise ValueError(f"unknown logistic-regression dataset {dataset_id!r} (expected one of {sorted(DATASET_FILES)})")
    path = os.path.join(resolve_dataset_dir(dataset_dir), DATASET_FILES[dataset_id])
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} does not exist: the dataset directory (environment_config['dataset_dir'] or "
                                f"{DATASET_DIR_ENV}) must hold {DATASET_FILES[dataset_id]}")
    return np.loadtxt(path)


def build_data_matrix(dataset_id=None, data=None, dataset_dir=None, X=None, labels=None):
    """The signed f32 matrix A [M, D] of a dataset id (with ``data`` or ``dataset_dir``) or of user arrays X, labels."""
    if X is not None or labels is not None:
        if X is None or labels is None or dataset_id is not None or data is not None:
            raise ValueError("pass either a dataset id (with data or dataset_dir) or both X and labels")
        X = np.asarray(X, np.float64)
        if X.ndim != 2 or np.asarray(labels).shape != (X.shape[0],):
            raise ValueError(f"X must be [M, D] and labels [M], got {X.shape} and {np.asarray(labels).shape}")
        A = signed_data_matrix(X, labels).astype(np.float32)
    else:
        if dataset_id is None:
            raise ValueError("pass a dataset id ('breast_cancer' or 'german_credit') or X and labels")
        if data is None:
            data = load_table(dataset_id, dataset_dir)
        A, _ = preprocess(data, dataset_id)
    if A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("the data matrix is empty")
    return A


class LogisticRegression(LNPDF):
    """Logistic-regression posterior with an isotropic normal prior.

    ``LogisticRegression("breast_cancer")`` / ``("german_credit")`` reads the table from ``dataset_dir`` (or
    GMMVI_DATASET_DIR); ``data=`` passes the raw table instead.  ``X=``, ``labels=`` (labels in {0, 1}) make it a general
    logistic-regression posterior on the design matrix X exactly as given (no standardisation, no bias column added)."""

    def __init__(self, dataset_id=None, data=None, dataset_dir=None, X=None, labels=None, prior_mean=PRIOR_MEAN,
                 prior_std=PRIOR_STD):
        super().__init__(use_log_density_and_grad=True)
        self.A = build_data_matrix(dataset_id, data, dataset_dir, X, labels)
        if not prior_std > 0:
            raise ValueError("prior_std must be positive")
        self.dataset_id = dataset_id
        self.prior_mean, self.prior_std = float(prior_mean), float(prior_std)
        self.ctx = get_context()
        self._A_dev = self.ctx.asarray(self.A)

    @property
    def num_data(self):
        return int(self.A.shape[0])

    def get_num_dimensions(self):
        return int(self.A.shape[1])

    def _fast_path_target(self):
        """Descriptor for the single-call iteration (optimization/fused.py) and the phased sharded one (sharded.py)."""
        return _lib.TargetSpec(kind=2, logreg_A=self._A_dev.ptr, logreg_M=self.num_data, logreg_prior_mean=self.prior_mean,
                               logreg_prior_std=self.prior_std)

    def log_density(self, x):
        return hip_ops.target_logreg(self.ctx, self._A_dev, self.prior_mean, self.prior_std, self.ctx.asarray(x),
                                     want_grad=False)[0]

    def log_density_and_grad(self, x):
        return hip_ops.target_logreg(self.ctx, self._A_dev, self.prior_mean, self.prior_std, self.ctx.asarray(x),
                                     want_grad=True)


def make_breast_cancer(dataset_dir=None):
    return LogisticRegression("breast_cancer", dataset_dir=dataset_dir)


def make_german_credit(dataset_dir=None):
    return LogisticRegression("german_credit", dataset_dir=dataset_dir)


def num_batches(num_data, batch_size, use_own_batch_per_sample):
    """nb: floor(T / B) batches per call when every sample takes its own, else 1."""
    return int(num_data) // int(batch_size) if use_own_batch_per_sample else 1


def minibatch_rows(seed, call, n, batch_size, num_data, num_batches):
    """The training rows of the n samples of call ``call``: int64 [n, batch_size], row j of sample i being
    rho_{seed,call}((i mod num_batches) * batch_size + j)."""
    b = np.arange(int(n), dtype=np.int64) % int(num_batches)
    p = b[:, None] * int(batch_size) + np.arange(int(batch_size), dtype=np.int64)[None, :]
    return permute_rows(seed, call, np.zeros_like(p), p, num_data, stream=STREAM_MINIBATCH)


class LogisticRegressionMinibatch(MinibatchLNPDF):
    """Minibatch logistic-regression posterior (logistic_regression.py:70-174).

    The data matrix is built as for ``LogisticRegression`` (a dataset id with ``data`` or ``dataset_dir``, or ``X`` and
    ``labels``); its last ``size_test_set`` rows are held out (``A_test``) and the first T = ``num_data`` rows are the
    training rows ``A``.  ``log_density`` / ``log_density_and_grad`` evaluate T / B times the sum of log sigma over the
    sample's batch plus the prior, on the batches of the stream (``seed``, ``call_count``), and advance the call counter
    when they receive at least one sample; ``log_density_fb`` is the full-data posterior on the training rows.

    A sibling of ``LogisticRegression``, not a subclass: it has no single-call-iteration descriptor, so the iteration takes
    the module-by-module path."""

    def __init__(self, dataset_id=None, batch_size=64, size_test_set=0, use_own_batch_per_sample=True, data=None,
                 dataset_dir=None, X=None, labels=None, seed=0, prior_mean=PRIOR_MEAN, prior_std=PRIOR_STD):
        super().__init__(seed)
        A = build_data_matrix(dataset_id, data, dataset_dir, X, labels)
        size_test_set = int(size_test_set)
        if not 0 <= size_test_set < A.shape[0]:
            raise ValueError(f"size_test_set must lie in [0, {A.shape[0]}) (the number of rows), got {size_test_set}")
        self.A = np.ascontiguousarray(A[:A.shape[0] - size_test_set])
        self.A_test = np.ascontiguousarray(A[A.shape[0] - size_test_set:])
        if not 1 <= int(batch_size) <= self.A.shape[0]:
            raise ValueError(f"batch_size must lie in [1, {self.A.shape[0]}] (the number of training rows), got "
                             f"{batch_size}")
        if self.A.shape[1] > MAX_DIM_MINIBATCH:
            raise ValueError(f"the minibatch target supports at most {MAX_DIM_MINIBATCH} dimensions, got {self.A.shape[1]}")
        if not prior_std > 0:
            raise ValueError("prior_std must be positive")
        self.dataset_id = dataset_id
        self.batch_size, self.size_test_set = int(batch_size), size_test_set
        self.use_own_batch_per_sample = bool(use_own_batch_per_sample)
        self.num_batches = num_batches(self.num_data, self.batch_size, self.use_own_batch_per_sample)
        self.prior_mean, self.prior_std = float(prior_mean), float(prior_std)
        self.ctx = get_context()
        self._A_dev = self.ctx.asarray(self.A)

    @property
    def num_data(self):
        return int(self.A.shape[0])

    def get_num_dimensions(self):
        return int(self.A.shape[1])

    def _launch(self, x, call, want_grad):
        return hip_ops.target_logreg_mb(self.ctx, self._A_dev, self.batch_size, self.num_batches, self.seed, call,
                                        self.prior_mean, self.prior_std, x, want_grad=want_grad)

    def log_density_fb(self, x):
        """The full-batch posterior on the training rows (csrc/logreg.hip); leaves the call counter alone."""
        return hip_ops.target_logreg(self.ctx, self._A_dev, self.prior_mean, self.prior_std, self.ctx.asarray(x),
                                     want_grad=False)[0]

    def expensive_metrics(self, model, samples) -> dict:
        """logistic_regression.py:144-161: the full-batch ELBO, under upstream's key (with its trailing colon)."""
        reward = _host_mean(self.log_density_fb(samples))
        entropy = -_host_mean(model.log_density(samples))
        return {"elbo_fb:": reward + entropy}


def _host_mean(v):
    return float(np.mean(np.asarray(v.numpy() if hasattr(v, "numpy") else v, np.float64)))


def make_breast_cancer_mb(batch_size, size_test_set, use_own_batch_per_sample, dataset_dir=None, seed=0):
    return LogisticRegressionMinibatch("breast_cancer", batch_size, size_test_set, use_own_batch_per_sample,
                                       dataset_dir=dataset_dir, seed=seed)


def make_german_credit_mb(batch_size, size_test_set, use_own_batch_per_sample, dataset_dir=None, seed=0):
    return LogisticRegressionMinibatch("german_credit", batch_size, size_test_set, use_own_batch_per_sample,
                                       dataset_dir=dataset_dir, seed=seed)
