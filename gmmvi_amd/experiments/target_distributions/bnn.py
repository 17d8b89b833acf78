"""Bayesian neural network for regression on the wine-quality data (reference:
src/gmmvi/experiments/target_distributions/bnn.py:59-311,385-448; configs/experiment_configs/wine.yml).

The posterior is a small MLP, features -> H1 -> H2 -> 1 with sigmoid, sigmoid and linear layers, under an MSE likelihood
on a minibatch per sample and a zero-mean isotropic normal prior without its constant (bnn.py:205-240):
    log p(w) = s (-T mean_m (y_m - f(x_m; w))^2 - 0.5 sum_d w_d^2 / sd^2)
with T the size of the training set and s the likelihood scaling.  The parameter vector is the reference's layout
(bnn.py:110-128,151-166): per layer the weights [in, out] row-major, then the biases; D = 177 for WINE.  The device
evaluates it with the analytic gradient (csrc/bnn.hip); the reference uses GradientTape.

Minibatches.  Upstream draws sample i's batch from a freshly reshuffled tf.data stream on every call; TensorFlow's RNG
cannot be reproduced, so this build defines its own stream, keyed by the target's ``seed`` and a call
counter c (+1 after every ``log_density`` / ``log_density_and_grad`` call with at least one sample): row j of sample n's
batch has stream position p = n B + j, epoch e = p div T, rank r = p mod T, and its data row is pi_{seed,c,e}(r), a
balanced 4-round Feistel network on 2h bits (h = ceil(ceil(log2 T) / 2)) with cycle walking, round i mapping
(L, R) -> (R, L xor (F_i(R) & (2^h - 1))), F_i(R) = word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter
(R | i << 24, e, c, 3).  Every epoch visits every row once.  ``minibatch_rows`` restates it in NumPy.

Three classes evaluate the posterior: ``BNNRegression`` (two sigmoid hidden layers, csrc/bnn.hip: WINE),
``BNNClassification`` (one ReLU hidden layer, csrc/bnn_classifier.hip: MNIST) and the generic ``BNN_LNPDF`` (one to three
hidden layers, any of linear / sigmoid / ReLU / tanh per layer, MSE or sparse cross-entropy, csrc/bnn_mlp.hip), which
stands where upstream's base class of the same name does.  All three share the minibatch stream below.

The datasets do not ship with the package: ``dataset_dir`` (``environment_config["dataset_dir"]``), else the
``GMMVI_DATASET_DIR`` environment variable, names a directory laid out like upstream's ``datasets/`` folder:
``wine/wine_seed_{0..9}.npz``.
"""
import os

import numpy as np

from ... import hip_ops
from ...device import get_context
from .lnpdf import LNPDF

DATASET_DIR_ENV = "GMMVI_DATASET_DIR"
STREAM_MINIBATCH = 3                 # stream ids 0-2: component normals, categorical draws, mixture normals
MAX_FEATURES, MAX_HIDDEN = 32, 16    # what csrc/bnn.hip supports
WINE_FILE = os.path.join("wine", "wine_seed_{}.npz")
WINE_ARRAYS = ("features_train", "labels_train", "features_test", "labels_test", "features_vali", "labels_vali")

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def _philox_word0(c0, c1, c2, c3, seed):
    """Word 0 of Philox4x32-10 (csrc/philox.h) for uint64 arrays holding 32-bit counter words."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK32)
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0


def feistel_half_bits(num_data):
    """h = ceil(ceil(log2 T) / 2): the network permutes [0, 2^(2h)) >= [0, T)."""
    bits = int(num_data - 1).bit_length() if num_data > 1 else 0
    return (bits + 1) // 2


def permute_rows(seed, call, epoch, rank, num_data, stream=STREAM_MINIBATCH):
    """pi_{seed,call,epoch}(rank) for int arrays epoch, rank (rank < num_data) -> int64 rows.  ``stream`` is the counter's
    last word: 3 (the default) for these minibatches, 4 for the minibatch logistic regressions."""
    h = feistel_half_bits(num_data)
    mask = np.uint64((1 << h) - 1)
    x = np.asarray(rank, np.uint64).copy()
    e = np.broadcast_to(np.asarray(epoch, np.uint64), x.shape).copy()
    c = np.uint64(int(call) & 0xFFFFFFFF)
    todo = np.arange(x.size)
    x, e = x.reshape(-1), e.reshape(-1)
    xt, et = x, e
    while todo.size:
        L, R = xt >> np.uint64(h), xt & mask
        for i in range(4):
            f = _philox_word0(R | np.uint64(i << 24), et, np.full_like(R, c), np.full_like(R, int(stream)), seed)
            L, R = R, L ^ (f & mask)
        xt = (L << np.uint64(h)) | R
        x[todo] = xt
        walk = xt >= np.uint64(num_data)                       # cycle walking: apply the whole network again
        todo, xt, et = todo[walk], xt[walk], et[walk]
    return x.reshape(np.shape(rank)).astype(np.int64)


def minibatch_rows(seed, call, n, batch_size, num_data):
    """The data rows of the n minibatches of call ``call``: int64 [n, batch_size] (row j of sample i: stream position
    i * batch_size + j)."""
    p = np.arange(int(n) * int(batch_size), dtype=np.int64)
    return permute_rows(seed, call, p // num_data, p % num_data, num_data).reshape(int(n), int(batch_size))


def num_parameters(num_features, hidden_units, num_outputs=1):
    """Per layer W [in, out], then b [out]; ``num_outputs`` is the width of the last layer (1 for a regressor, the number
    of classes for a classifier)."""
    d, last = 0, int(num_features)
    for width in list(hidden_units) + [num_outputs]:
        d += last * int(width) + int(width)
        last = int(width)
    return d


class BNNRegression(LNPDF):
    """Posterior of a features -> H1 -> H2 -> 1 sigmoid network with an MSE likelihood on minibatches of
    ``batch_size`` rows and a zero-mean normal prior of standard deviation ``prior_std`` (bnn.py:59-240).

    ``features`` [T, F] and ``labels`` [T] are the training set; ``eval_sets`` maps "test" / "vali" to (features, labels)
    pairs for ``expensive_metrics``.  ``seed`` keys the minibatch stream; ``call_count`` is the number of evaluations so
    far (the stream's call counter)."""

    def __init__(self, features, labels, hidden_units=(8, 8), likelihood_scaling=1., prior_std=1., batch_size=128,
                 seed=0, eval_sets=None):
        super().__init__(use_log_density_and_grad=True)
        X = np.asarray(features, np.float32)
        y = np.asarray(labels, np.float32)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError(f"features must be [T, F] and labels [T], got {X.shape} and {y.shape}")
        hidden_units = tuple(int(h) for h in hidden_units)
        if len(hidden_units) != 2:
            raise ValueError(f"hidden_units must name two hidden layers, got {hidden_units}")
        if not 1 <= X.shape[1] <= MAX_FEATURES:
            raise ValueError(f"the network takes 1 to {MAX_FEATURES} features, got {X.shape[1]}")
        if not all(1 <= h <= MAX_HIDDEN for h in hidden_units):
            raise ValueError(f"hidden layers must have 1 to {MAX_HIDDEN} units, got {hidden_units}")
        if not 1 <= int(batch_size) <= X.shape[0]:
            raise ValueError(f"batch_size must lie in [1, {X.shape[0]}] (the training-set size), got {batch_size}")
        if not prior_std > 0:
            raise ValueError("prior_std must be positive")
        self.features, self.labels = X, y
        self.hidden_units = hidden_units
        self.likelihood_scaling, self.prior_std = float(likelihood_scaling), float(prior_std)
        self.batch_size, self.seed = int(batch_size), int(seed)
        self.eval_sets = {k: (np.asarray(f, np.float32), np.asarray(l, np.float32))
                          for k, (f, l) in (eval_sets or {}).items()}
        self._call = 0
        self.ctx = get_context()
        self._X_dev, self._y_dev = self.ctx.asarray(X), self.ctx.asarray(y)

    @property
    def call_count(self):
        return self._call

    @property
    def train_size(self):
        return int(self.features.shape[0])

    def get_num_dimensions(self):
        return num_parameters(self.features.shape[1], self.hidden_units)

    def _evaluate(self, x, want_grad):
        x = self.ctx.asarray(x)
        lp, grad = hip_ops.target_bnn(self.ctx, self._X_dev, self._y_dev, self.hidden_units, self.seed, self._call,
                                      self.batch_size, self.likelihood_scaling, self.prior_std, x, want_grad=want_grad)
        if x.shape[0] >= 1:
            self._call += 1
        return lp, grad

    def log_density(self, x):
        return self._evaluate(x, False)[0]

    def log_density_and_grad(self, x):
        return self._evaluate(x, True)

    def predict(self, samples, features):
        """Network outputs [S, M] of the weight vectors ``samples`` [S, D] on the rows ``features`` [M, F]."""
        return hip_ops.bnn_predict(self.ctx, self.hidden_units, self.ctx.asarray(samples),
                                   self.ctx.asarray(np.asarray(features, np.float32)))

    def bayesian_inference_loss(self, samples, dataset):
        """bnn.py:290-310: the outputs averaged over the samples, then the MSE and the RMSE of every batch of
        ``batch_size`` rows (stored order, the last batch partial), averaged over the batches -> (loss, rmse)."""
        features, labels = self.eval_sets[dataset]
        out = self.predict(samples, features)
        mean_out = (out.numpy() if hasattr(out, "numpy") else np.asarray(out)).astype(np.float64).mean(0)
        losses = []
        for b0 in range(0, len(labels), self.batch_size):
            r = labels[b0:b0 + self.batch_size].astype(np.float64) - mean_out[b0:b0 + self.batch_size]
            losses.append(np.mean(r * r))
        losses = np.asarray(losses)
        return float(losses.mean()), float(np.sqrt(losses).mean())

    def expensive_metrics(self, model, samples) -> dict:
        """bnn.py:417-444, keys as upstream names them (``bi_test_accuracy`` is an RMSE)."""
        metrics = dict()
        if "test" in self.eval_sets:
            loss, rmse = self.bayesian_inference_loss(samples, "test")
            metrics.update({"bi_test_loss": loss, "bi_test_accuracy": rmse})
        if "vali" in self.eval_sets:
            loss, rmse = self.bayesian_inference_loss(samples, "vali")
            metrics.update({"bi_vali_loss": loss, "bi_vali_rmse": rmse})
        return metrics


def resolve_dataset_dir(dataset_dir=None):
    d = dataset_dir if dataset_dir is not None else os.environ.get(DATASET_DIR_ENV)
    if not d:
        raise FileNotFoundError(
            f"no dataset directory for the WINE target: set environment_config['dataset_dir'] or the {DATASET_DIR_ENV} "
            f"environment variable to a directory holding {WINE_FILE.format('<dataset_seed % 10>')}")
    return d


def load_wine(dataset_seed, dataset_dir=None):
    """The six arrays of ``wine/wine_seed_{dataset_seed % 10}.npz`` (bnn.py:395-404)."""
    path = os.path.join(resolve_dataset_dir(dataset_dir), WINE_FILE.format(int(dataset_seed) % 10))
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} does not exist: the dataset directory (environment_config['dataset_dir'] or "
                                f"{DATASET_DIR_ENV}) must hold {WINE_FILE.format(int(dataset_seed) % 10)}")
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in WINE_ARRAYS}


class BNN_WINE(BNNRegression):
    """bnn.py:385-444: 11 -> 8 -> 8 -> 1 on the wine-quality split ``dataset_seed % 10``; ``seed`` keys the minibatch
    stream (default: the dataset seed, which is the run seed when built by name)."""

    def __init__(self, dataset_seed, likelihood_scaling, prior_std, batch_size, dataset_dir=None, seed=None):
        data = load_wine(dataset_seed, dataset_dir)
        self.dataset_seed = int(dataset_seed)
        super().__init__(data["features_train"], data["labels_train"], hidden_units=(8, 8),
                         likelihood_scaling=likelihood_scaling, prior_std=prior_std, batch_size=batch_size,
                         seed=self.dataset_seed if seed is None else seed,
                         eval_sets={"test": (data["features_test"], data["labels_test"]),
                                    "vali": (data["features_vali"], data["labels_vali"])})


def make_WINE_target(likelihood_scaling, dataset_seed, prior_std, batch_size, dataset_dir=None, seed=None):
    return BNN_WINE(dataset_seed=dataset_seed, likelihood_scaling=likelihood_scaling, prior_std=prior_std,
                    batch_size=batch_size, dataset_dir=dataset_dir, seed=seed)


# ---- classification: features -> H (ReLU) -> C logits under a cross-entropy likelihood (BNN_MNIST) -----------------------
MAX_CLASSIFIER_FEATURES, MAX_CLASSIFIER_HIDDEN = 1024, 128     # what csrc/bnn_classifier.hip supports
MIN_CLASSES, MAX_CLASSES, MAX_CLASSIFIER_BATCH = 2, 16, 1024
MNIST_FILE = os.path.join("mnist", "mnist.npz")
MNIST_ARRAYS = ("x_train", "y_train", "x_test", "y_test")
MNIST_TEST_ROWS = 5000                                         # bnn.py:336: ds_test.take(5000) / ds_test.skip(5000)


def classifier_num_parameters(num_features, hidden, num_classes):
    """W1 [F, H], b1 [H], W2 [H, C], b2 [C]: 101 770 for MNIST's (784, 128, 10)."""
    return hip_ops.bnn_classifier_num_parameters(num_features, hidden, num_classes)


class BNNClassification(LNPDF):
    """Posterior of a features -> H (ReLU) -> C (logits) network with the sparse categorical cross-entropy from logits on
    minibatches of ``batch_size`` rows and a zero-mean normal prior of standard deviation ``prior_std`` (bnn.py:59-240
    with the network and loss of BNN_MNIST, bnn.py:312-351):
        log p(w) = s (-T mean_m (logsumexp(l_m) - l_m[y_m]) - 0.5 sum_d w_d^2 / sd^2).

    ``features`` [T, F] and integer ``labels`` [T] in [0, num_classes) are the training set; ``eval_sets`` maps "test" /
    "vali" to (features, labels) pairs for ``expensive_metrics``.  The minibatch stream, its ``seed`` and ``call_count``
    are BNNRegression's."""

    def __init__(self, features, labels, num_classes, hidden_units=(128,), likelihood_scaling=1., prior_std=1.,
                 batch_size=128, seed=0, eval_sets=None):
        super().__init__(use_log_density_and_grad=True)
        X = np.asarray(features, np.float32)
        y = np.asarray(labels)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError(f"features must be [T, F] and labels [T], got {X.shape} and {y.shape}")
        hidden_units = tuple(int(h) for h in hidden_units)
        if len(hidden_units) != 1:
            raise ValueError(f"hidden_units must name one hidden layer, got {hidden_units}")
        if not 1 <= X.shape[1] <= MAX_CLASSIFIER_FEATURES:
            raise ValueError(f"the network takes 1 to {MAX_CLASSIFIER_FEATURES} features, got {X.shape[1]}")
        if not 1 <= hidden_units[0] <= MAX_CLASSIFIER_HIDDEN:
            raise ValueError(f"the hidden layer must have 1 to {MAX_CLASSIFIER_HIDDEN} units, got {hidden_units[0]}")
        if not MIN_CLASSES <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must lie in [{MIN_CLASSES}, {MAX_CLASSES}], got {num_classes}")
        if not 1 <= int(batch_size) <= min(X.shape[0], MAX_CLASSIFIER_BATCH):
            raise ValueError(f"batch_size must lie in [1, {min(X.shape[0], MAX_CLASSIFIER_BATCH)}] (the training-set size, "
                             f"at most {MAX_CLASSIFIER_BATCH}), got {batch_size}")
        if not prior_std > 0:
            raise ValueError("prior_std must be positive")
        if y.size and (not np.all(y == np.floor(y)) or y.min() < 0 or y.max() >= int(num_classes)):
            raise ValueError(f"labels must be integers in [0, {int(num_classes)}) (num_classes), got values in "
                             f"[{y.min()}, {y.max()}]")
        self.features, self.labels = X, y.astype(np.int32)
        self.num_classes, self.hidden_units = int(num_classes), hidden_units
        self.likelihood_scaling, self.prior_std = float(likelihood_scaling), float(prior_std)
        self.batch_size, self.seed = int(batch_size), int(seed)
        self.eval_sets = {k: (np.asarray(f, np.float32), np.asarray(l).astype(np.int32))
                          for k, (f, l) in (eval_sets or {}).items()}
        self._call = 0
        self.ctx = get_context()
        self._X_dev, self._y_dev = self.ctx.asarray(X), self.ctx.asarray(self.labels, np.int32)

    @property
    def call_count(self):
        return self._call

    @property
    def train_size(self):
        return int(self.features.shape[0])

    def get_num_dimensions(self):
        return classifier_num_parameters(self.features.shape[1], self.hidden_units[0], self.num_classes)

    def _evaluate(self, x, want_grad):
        x = self.ctx.asarray(x)
        lp, grad = hip_ops.target_bnn_classifier(self.ctx, self._X_dev, self._y_dev, self.hidden_units[0], self.num_classes,
                                                 self.seed, self._call, self.batch_size, self.likelihood_scaling,
                                                 self.prior_std, x, want_grad=want_grad)
        if x.shape[0] >= 1:
            self._call += 1
        return lp, grad

    def log_density(self, x):
        return self._evaluate(x, False)[0]

    def log_density_and_grad(self, x):
        return self._evaluate(x, True)

    def predict(self, samples, features):
        """Logits [S, M, C] of the weight vectors ``samples`` [S, D] on the rows ``features`` [M, F]."""
        return hip_ops.bnn_classifier_predict(self.ctx, self.hidden_units[0], self.num_classes, self.ctx.asarray(samples),
                                              self.ctx.asarray(np.asarray(features, np.float32)))

    def bayesian_inference_loss(self, samples, dataset):
        """bnn.py:290-310: the logits averaged over the samples, then the cross-entropy from logits and the sparse
        categorical accuracy of every batch of ``batch_size`` rows (stored order, the last batch partial), averaged over
        the batches in fp64 -> (loss, accuracy)."""
        features, labels = self.eval_sets[dataset]
        out = self.predict(samples, features)
        logits = (out.numpy() if hasattr(out, "numpy") else np.asarray(out)).astype(np.float64).mean(0)
        losses, accuracies = [], []
        for b0 in range(0, len(labels), self.batch_size):
            l, y = logits[b0:b0 + self.batch_size], labels[b0:b0 + self.batch_size]
            mx = l.max(1)
            lse = mx + np.log(np.exp(l - mx[:, None]).sum(1))
            losses.append(np.mean(lse - l[np.arange(len(y)), y]))
            accuracies.append(np.mean(l.argmax(1) == y))
        return float(np.mean(losses)), float(np.mean(accuracies))

    def expensive_metrics(self, model, samples) -> dict:
        """bnn.py:353-380, keys as BNN_MNIST names them."""
        metrics = dict()
        if "test" in self.eval_sets:
            loss, accuracy = self.bayesian_inference_loss(samples, "test")
            metrics.update({"bi_test_loss": loss, "bi_test_accuracy": accuracy})
        if "vali" in self.eval_sets:
            loss, accuracy = self.bayesian_inference_loss(samples, "vali")
            metrics.update({"bi_vali_loss": loss, "bi_vali_accuracy": accuracy})
        return metrics


def load_mnist(dataset_dir=None):
    """MNIST from ``mnist/mnist.npz`` below the dataset directory, in the widely mirrored array layout: ``x_train`` uint8
    [60000, 28, 28], ``y_train`` [60000], ``x_test`` [10000, 28, 28], ``y_test``.  Features are uint8 / 255 in f32
    (bnn.py:329-331), flattened to 784; "test" is the first 5 000 test rows and "vali" the rest (bnn.py:336).  A file of
    the same layout with at most 5 000 test rows is split in halves.  Upstream reads the TFDS copy with shuffled files,
    so its row order is not reproducible; the rows here keep the file's order."""
    d = dataset_dir if dataset_dir is not None else os.environ.get(DATASET_DIR_ENV)
    if not d:
        raise FileNotFoundError(
            f"no dataset directory for the MNIST target: pass dataset_dir or set the {DATASET_DIR_ENV} environment "
            f"variable to a directory holding {MNIST_FILE}")
    path = os.path.join(d, MNIST_FILE)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} does not exist: the dataset directory (dataset_dir or {DATASET_DIR_ENV}) must "
                                f"hold {MNIST_FILE} with the arrays {', '.join(MNIST_ARRAYS)}")
    with np.load(path, allow_pickle=False) as z:
        raw = {k: z[k] for k in MNIST_ARRAYS}

    def images(a):
        return (a.reshape(a.shape[0], -1).astype(np.float32) / np.float32(255.)).astype(np.float32)

    x_test, y_test = images(raw["x_test"]), raw["y_test"].astype(np.int32)
    cut = MNIST_TEST_ROWS if x_test.shape[0] > MNIST_TEST_ROWS else x_test.shape[0] // 2
    return {"features_train": images(raw["x_train"]), "labels_train": raw["y_train"].astype(np.int32),
            "features_test": x_test[:cut], "labels_test": y_test[:cut],
            "features_vali": x_test[cut:], "labels_vali": y_test[cut:]}


class BNN_MNIST(BNNClassification):
    """bnn.py:312-380: 784 -> 128 (ReLU) -> 10 on MNIST, D = 101 770; ``seed`` keys the minibatch stream."""

    def __init__(self, likelihood_scaling, prior_std, batch_size, dataset_dir=None, seed=0):
        data = load_mnist(dataset_dir)
        super().__init__(data["features_train"], data["labels_train"], num_classes=10, hidden_units=(128,),
                         likelihood_scaling=likelihood_scaling, prior_std=prior_std, batch_size=batch_size, seed=seed,
                         eval_sets={"test": (data["features_test"], data["labels_test"]),
                                    "vali": (data["features_vali"], data["labels_vali"])})


def make_MNIST_target(likelihood_scaling, prior_std, batch_size, dataset_dir=None, seed=0):
    return BNN_MNIST(likelihood_scaling=likelihood_scaling, prior_std=prior_std, batch_size=batch_size,
                     dataset_dir=dataset_dir, seed=seed)


# ---- the generic network: any depth, activation and loss (BNN_LNPDF) -----------------------------------------------------
MLP_LOSSES = ("mse", "sparse_categorical_crossentropy")


class BNN_LNPDF(LNPDF):
    """bnn.py:59-311: the posterior of a dense network features -> hidden_units ... -> outputs on minibatches of
    ``batch_size`` rows under a zero-mean normal prior of standard deviation ``prior_std``:
        log p(w) = s (-T mean_m loss_m - 0.5 sum_d w_d^2 / sd^2)
    evaluated with its analytic gradient by csrc/bnn_mlp.hip.  In place of upstream's Keras objects:

    ``hidden_units``: 1 to 3 hidden widths, each at most 128; at most 1024 features.
    ``activations``: one name per layer, the output layer included, among "linear", "sigmoid", "relu", "tanh"; the output
    layer's must be "linear".
    ``loss``: "mse" (one output, float labels) or "sparse_categorical_crossentropy" (logits over ``num_classes`` classes,
    2 to 16, integer labels in [0, num_classes)).
    ``features`` [T, F], ``labels`` [T]: the training set; ``eval_sets`` maps "test" / "vali" to (features, labels) pairs
    for ``expensive_metrics``.  A subclass may leave ``features`` out and override ``prepare_data`` instead, as upstream's
    subclasses do; it returns (features, labels, eval_sets).
    ``seed`` keys the minibatch stream (BNNRegression's: stream id 3); ``call_count`` is the number of evaluations so far.
    ``dataset_seed`` is kept for ``prepare_data``."""

    def __init__(self, likelihood_scaling=1., prior_std=1., batch_size=128, hidden_units=(8, 8), loss="mse",
                 activations=("sigmoid", "sigmoid", "linear"), features=None, labels=None, num_classes=None,
                 dataset_seed=-1, seed=0, eval_sets=None):
        super().__init__(use_log_density_and_grad=True)
        self.dataset_seed = int(dataset_seed)
        if features is None:
            features, labels, eval_sets = self.prepare_data()
        if loss not in MLP_LOSSES:
            raise ValueError(f"loss must be one of {MLP_LOSSES}, got {loss!r}")
        if loss != "mse" and num_classes is None:
            raise ValueError("num_classes is required for the sparse_categorical_crossentropy loss")
        X = np.asarray(features, np.float32)
        y = np.asarray(labels)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError(f"features must be [T, F] and labels [T], got {X.shape} and {y.shape}")
        self.loss = loss
        self.num_outputs = 1 if loss == "mse" else int(num_classes)
        self.hidden_units = tuple(int(h) for h in hidden_units)
        self.activations = tuple(activations)
        hip_ops.mlp_desc(X.shape[1], self.hidden_units, self.activations, loss, self.num_outputs)    # raises on a limit
        if not 1 <= int(batch_size) <= min(X.shape[0], hip_ops.MLP_MAX_BATCH):
            raise ValueError(f"batch_size must lie in [1, {min(X.shape[0], hip_ops.MLP_MAX_BATCH)}] (the training-set "
                             f"size, at most {hip_ops.MLP_MAX_BATCH}), got {batch_size}")
        if not prior_std > 0:
            raise ValueError("prior_std must be positive")
        if loss != "mse" and y.size and (not np.all(y == np.floor(y)) or y.min() < 0 or y.max() >= self.num_outputs):
            raise ValueError(f"labels must be integers in [0, {self.num_outputs}) (num_classes), got values in "
                             f"[{y.min()}, {y.max()}]")
        self._label_dtype = np.float32 if loss == "mse" else np.int32
        self.features, self.labels = X, y.astype(self._label_dtype)
        self.num_classes = None if loss == "mse" else self.num_outputs
        self.likelihood_scaling, self.prior_std = float(likelihood_scaling), float(prior_std)
        self.batch_size, self.seed = int(batch_size), int(seed)
        self.eval_sets = {k: (np.asarray(f, np.float32), np.asarray(l).astype(self._label_dtype))
                          for k, (f, l) in (eval_sets or {}).items()}
        self._call = 0
        self.ctx = get_context()
        self._X_dev, self._y_dev = self.ctx.asarray(X), self.ctx.asarray(self.labels, self._label_dtype)

    def prepare_data(self):
        """-> (features [T, F], labels [T], eval_sets or None); called when the constructor gets no ``features``."""
        raise NotImplementedError

    @property
    def call_count(self):
        return self._call

    @property
    def train_size(self):
        return int(self.features.shape[0])

    def get_num_dimensions(self):
        return num_parameters(self.features.shape[1], self.hidden_units, self.num_outputs)

    def _evaluate(self, x, want_grad):
        x = self.ctx.asarray(x)
        lp, grad = hip_ops.target_mlp(self.ctx, self._X_dev, self._y_dev, self.hidden_units, self.activations, self.loss,
                                      self.num_outputs, self.seed, self._call, self.batch_size, self.likelihood_scaling,
                                      self.prior_std, x, want_grad=want_grad)
        if x.shape[0] >= 1:
            self._call += 1
        return lp, grad

    def log_density(self, x):
        return self._evaluate(x, False)[0]

    def log_density_and_grad(self, x):
        return self._evaluate(x, True)

    def predict(self, samples, features):
        """Network outputs [S, M] ("mse") or logits [S, M, C] of the weight vectors ``samples`` [S, D] on the rows
        ``features`` [M, F]."""
        return hip_ops.mlp_predict(self.ctx, self.hidden_units, self.activations, self.loss, self.num_outputs,
                                   self.ctx.asarray(samples), self.ctx.asarray(np.asarray(features, np.float32)))

    def bayesian_inference_loss(self, samples, dataset):
        """bnn.py:290-310: the outputs averaged over the samples, then the loss and the second metric of every batch of
        ``batch_size`` rows (stored order, the last batch partial), averaged over the batches in fp64 -> (loss, metric):
        the MSE and the RMSE, or the cross-entropy from logits and the sparse categorical accuracy."""
        features, labels = self.eval_sets[dataset]
        out = self.predict(samples, features)
        mean_out = (out.numpy() if hasattr(out, "numpy") else np.asarray(out)).astype(np.float64).mean(0)
        losses, metrics = [], []
        for b0 in range(0, len(labels), self.batch_size):
            o, y = mean_out[b0:b0 + self.batch_size], labels[b0:b0 + self.batch_size]
            if self.loss == "mse":
                r = y.astype(np.float64) - o
                losses.append(np.mean(r * r))
                metrics.append(np.sqrt(losses[-1]))
            else:
                mx = o.max(1)
                lse = mx + np.log(np.exp(o - mx[:, None]).sum(1))
                losses.append(np.mean(lse - o[np.arange(len(y)), y]))
                metrics.append(np.mean(o.argmax(1) == y))
        return float(np.mean(losses)), float(np.mean(metrics))

    def expensive_metrics(self, model, samples) -> dict:
        """Keys as upstream's subclasses name them; for the "mse" loss the ``accuracy`` entries hold the RMSE, as
        ``bi_test_accuracy`` does upstream (bnn.py:417-444)."""
        metrics = dict()
        if "test" in self.eval_sets:
            loss, second = self.bayesian_inference_loss(samples, "test")
            metrics.update({"bi_test_loss": loss, "bi_test_accuracy": second})
        if "vali" in self.eval_sets:
            loss, second = self.bayesian_inference_loss(samples, "vali")
            metrics.update({"bi_vali_loss": loss, "bi_vali_accuracy": second})
        return metrics
