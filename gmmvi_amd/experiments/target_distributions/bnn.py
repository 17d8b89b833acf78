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
(R | i << 24, e, c, 3).  Every epoch visits every row once.  ``minibatch_stream.minibatch_rows`` restates it in NumPy.

Three classes evaluate the posterior: ``BNNRegression`` (two sigmoid hidden layers, csrc/bnn.hip: WINE),
``BNNClassification`` (one ReLU hidden layer, csrc/bnn_classifier.hip: MNIST) and the generic ``BNN_LNPDF`` (one to three
hidden layers, any of linear / sigmoid / ReLU / tanh per layer, MSE or sparse cross-entropy, csrc/bnn_mlp.hip), which
stands where upstream's base class of the same name does.  All three derive from ``_MinibatchBNN``, which holds what
does not depend on the network: the constructor's checks, the stream's call counter and the metrics.

The datasets do not ship with the package: ``dataset_dir`` (``environment_config["dataset_dir"]``), else the
``GMMVI_DATASET_DIR`` environment variable, names a directory laid out like upstream's ``datasets/`` folder:
``wine/wine_seed_{0..9}.npz`` and ``mnist/mnist.npz``.
"""
import os

import numpy as np

from ... import hip_ops
from ...device import get_context
from .minibatch_stream import STREAM_BNN_MINIBATCH as STREAM_MINIBATCH      # the names tests and tools import from here
from .minibatch_stream import MinibatchLNPDF, feistel_half_bits, minibatch_rows, permute_rows  # noqa: F401

DATASET_DIR_ENV = "GMMVI_DATASET_DIR"
MSE, CROSS_ENTROPY = "mse", "sparse_categorical_crossentropy"
MLP_LOSSES = (MSE, CROSS_ENTROPY)
num_parameters = hip_ops.mlp_num_parameters          # (num_features, hidden_units, num_outputs=1)


def classifier_num_parameters(num_features, hidden, num_classes):
    """W1 [F, H], b1 [H], W2 [H, C], b2 [C]: 101 770 for MNIST's (784, 128, 10)."""
    return num_parameters(num_features, (hidden,), num_classes)


def _host(a):
    return a.numpy() if hasattr(a, "numpy") else np.asarray(a)


class _MinibatchBNN(MinibatchLNPDF):
    """What the three networks share (bnn.py:59-311): the training set and its checks, the minibatch stream's seed and call
    counter, and the metrics.  ``loss`` is "mse" (float labels, one output) or "sparse_categorical_crossentropy" (integer
    labels in [0, ``num_outputs``)).  A subclass sets its network's attributes, then calls this constructor, which hands
    the number of features to ``_check_network`` (ValueError on a limit of the kernel); it implements ``_launch``,
    ``predict`` and ``get_num_dimensions``."""

    MAX_BATCH = None                       # the kernel's cap on batch_size, if it has one
    VALI_METRIC_KEY = "bi_vali_accuracy"

    def __init__(self, features, labels, loss, num_outputs, likelihood_scaling, prior_std, batch_size, seed, eval_sets):
        super().__init__(seed)
        X = np.asarray(features, np.float32)
        y = np.asarray(labels)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError(f"features must be [T, F] and labels [T], got {X.shape} and {y.shape}")
        self.loss, self.num_outputs = loss, int(num_outputs)
        self._check_network(X.shape[1])
        if self.MAX_BATCH is None:
            top, what = X.shape[0], "the training-set size"
        else:
            top, what = min(X.shape[0], self.MAX_BATCH), f"the training-set size, at most {self.MAX_BATCH}"
        if not 1 <= int(batch_size) <= top:
            raise ValueError(f"batch_size must lie in [1, {top}] ({what}), got {batch_size}")
        if not prior_std > 0:
            raise ValueError("prior_std must be positive")
        if loss != MSE and y.size and (not np.all(y == np.floor(y)) or y.min() < 0 or y.max() >= self.num_outputs):
            raise ValueError(f"labels must be integers in [0, {self.num_outputs}) (num_classes), got values in "
                             f"[{y.min()}, {y.max()}]")
        self._label_dtype = np.float32 if loss == MSE else np.int32
        self.features, self.labels = X, y.astype(self._label_dtype)
        self.likelihood_scaling, self.prior_std = float(likelihood_scaling), float(prior_std)
        self.batch_size = int(batch_size)
        self.eval_sets = {k: (np.asarray(f, np.float32), np.asarray(l).astype(self._label_dtype))
                          for k, (f, l) in (eval_sets or {}).items()}
        self.ctx = get_context()
        self._X_dev, self._y_dev = self.ctx.asarray(X), self.ctx.asarray(self.labels, self._label_dtype)

    def _check_network(self, num_features):
        raise NotImplementedError

    def predict(self, samples, features):
        raise NotImplementedError

    @property
    def train_size(self):
        return int(self.features.shape[0])

    def _predict_operands(self, samples, features):
        return self.ctx.asarray(samples), self.ctx.asarray(np.asarray(features, np.float32))

    def bayesian_inference_loss(self, samples, dataset):
        """bnn.py:290-310: the outputs averaged over the samples, then the loss and the second metric of every batch of
        ``batch_size`` rows (stored order, the last batch partial), averaged over the batches in fp64 -> (loss, metric):
        the MSE and the RMSE, or the cross-entropy from logits and the sparse categorical accuracy."""
        features, labels = self.eval_sets[dataset]
        mean_out = _host(self.predict(samples, features)).astype(np.float64).mean(0)
        losses, metrics = [], []
        for b0 in range(0, len(labels), self.batch_size):
            o, y = mean_out[b0:b0 + self.batch_size], labels[b0:b0 + self.batch_size]
            if self.loss == MSE:
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
        """bnn.py:353-380,417-444, keys as upstream's subclasses name them: for the "mse" loss ``bi_test_accuracy`` holds
        the RMSE, as it does upstream."""
        metrics = dict()
        for dataset, key in (("test", "bi_test_accuracy"), ("vali", self.VALI_METRIC_KEY)):
            if dataset in self.eval_sets:
                metrics[f"bi_{dataset}_loss"], metrics[key] = self.bayesian_inference_loss(samples, dataset)
        return metrics


def resolve_dataset_dir(dataset_dir, what):
    """``dataset_dir``, else the GMMVI_DATASET_DIR environment variable; ``what`` names the target and its file."""
    d = dataset_dir if dataset_dir is not None else os.environ.get(DATASET_DIR_ENV)
    if not d:
        raise FileNotFoundError(f"no dataset directory for {what}: pass dataset_dir (environment_config['dataset_dir']) or "
                                f"set the {DATASET_DIR_ENV} environment variable to the directory that holds it")
    return d


# ---- regression: features -> H1 -> H2 -> 1, sigmoid hidden layers, under an MSE likelihood (BNN_WINE) ---------------------
MAX_FEATURES, MAX_HIDDEN = 32, 16    # what csrc/bnn.hip supports
WINE_FILE = os.path.join("wine", "wine_seed_{}.npz")
WINE_ARRAYS = ("features_train", "labels_train", "features_test", "labels_test", "features_vali", "labels_vali")


class BNNRegression(_MinibatchBNN):
    """Posterior of a features -> H1 -> H2 -> 1 sigmoid network with an MSE likelihood on minibatches of
    ``batch_size`` rows and a zero-mean normal prior of standard deviation ``prior_std`` (bnn.py:59-240).

    ``features`` [T, F] and ``labels`` [T] are the training set; ``eval_sets`` maps "test" / "vali" to (features, labels)
    pairs for ``expensive_metrics``.  ``seed`` keys the minibatch stream; ``call_count`` is the number of evaluations so
    far (the stream's call counter)."""

    VALI_METRIC_KEY = "bi_vali_rmse"

    def __init__(self, features, labels, hidden_units=(8, 8), likelihood_scaling=1., prior_std=1., batch_size=128,
                 seed=0, eval_sets=None):
        self.hidden_units = tuple(int(h) for h in hidden_units)
        super().__init__(features, labels, MSE, 1, likelihood_scaling, prior_std, batch_size, seed, eval_sets)

    def _check_network(self, num_features):
        if len(self.hidden_units) != 2:
            raise ValueError(f"hidden_units must name two hidden layers, got {self.hidden_units}")
        if not 1 <= num_features <= MAX_FEATURES:
            raise ValueError(f"the network takes 1 to {MAX_FEATURES} features, got {num_features}")
        if not all(1 <= h <= MAX_HIDDEN for h in self.hidden_units):
            raise ValueError(f"hidden layers must have 1 to {MAX_HIDDEN} units, got {self.hidden_units}")

    def get_num_dimensions(self):
        return num_parameters(self.features.shape[1], self.hidden_units)

    def _launch(self, x, call, want_grad):
        return hip_ops.target_bnn(self.ctx, self._X_dev, self._y_dev, self.hidden_units, self.seed, call, self.batch_size,
                                  self.likelihood_scaling, self.prior_std, x, want_grad=want_grad)

    def predict(self, samples, features):
        """Network outputs [S, M] of the weight vectors ``samples`` [S, D] on the rows ``features`` [M, F]."""
        return hip_ops.bnn_predict(self.ctx, self.hidden_units, *self._predict_operands(samples, features))


def load_wine(dataset_seed, dataset_dir=None):
    """The six arrays of ``wine/wine_seed_{dataset_seed % 10}.npz`` (bnn.py:395-404)."""
    name = WINE_FILE.format(int(dataset_seed) % 10)
    path = os.path.join(resolve_dataset_dir(dataset_dir, f"the WINE target ({name})"), name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} does not exist: the dataset directory (environment_config['dataset_dir'] or "
                                f"{DATASET_DIR_ENV}) must hold {name}")
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in WINE_ARRAYS}


def _eval_sets(data):
    return {"test": (data["features_test"], data["labels_test"]), "vali": (data["features_vali"], data["labels_vali"])}


class BNN_WINE(BNNRegression):
    """bnn.py:385-444: 11 -> 8 -> 8 -> 1 on the wine-quality split ``dataset_seed % 10``; ``seed`` keys the minibatch
    stream (default: the dataset seed, which is the run seed when built by name)."""

    def __init__(self, dataset_seed, likelihood_scaling, prior_std, batch_size, dataset_dir=None, seed=None):
        data = load_wine(dataset_seed, dataset_dir)
        self.dataset_seed = int(dataset_seed)
        super().__init__(data["features_train"], data["labels_train"], hidden_units=(8, 8),
                         likelihood_scaling=likelihood_scaling, prior_std=prior_std, batch_size=batch_size,
                         seed=self.dataset_seed if seed is None else seed, eval_sets=_eval_sets(data))


def make_WINE_target(likelihood_scaling, dataset_seed, prior_std, batch_size, dataset_dir=None, seed=None):
    return BNN_WINE(dataset_seed=dataset_seed, likelihood_scaling=likelihood_scaling, prior_std=prior_std,
                    batch_size=batch_size, dataset_dir=dataset_dir, seed=seed)


# ---- classification: features -> H (ReLU) -> C logits under a cross-entropy likelihood (BNN_MNIST) -----------------------
MAX_CLASSIFIER_FEATURES, MAX_CLASSIFIER_HIDDEN = 1024, 128     # what csrc/bnn_classifier.hip supports
MIN_CLASSES, MAX_CLASSES, MAX_CLASSIFIER_BATCH = 2, 16, 1024
MNIST_FILE = os.path.join("mnist", "mnist.npz")
MNIST_ARRAYS = ("x_train", "y_train", "x_test", "y_test")
MNIST_TEST_ROWS = 5000                                         # bnn.py:336: ds_test.take(5000) / ds_test.skip(5000)


class BNNClassification(_MinibatchBNN):
    """Posterior of a features -> H (ReLU) -> C (logits) network with the sparse categorical cross-entropy from logits on
    minibatches of ``batch_size`` rows and a zero-mean normal prior of standard deviation ``prior_std`` (bnn.py:59-240
    with the network and loss of BNN_MNIST, bnn.py:312-351):
        log p(w) = s (-T mean_m (logsumexp(l_m) - l_m[y_m]) - 0.5 sum_d w_d^2 / sd^2).

    ``features`` [T, F] and integer ``labels`` [T] in [0, num_classes) are the training set; ``eval_sets`` maps "test" /
    "vali" to (features, labels) pairs for ``expensive_metrics``.  The minibatch stream, its ``seed`` and ``call_count``
    are BNNRegression's."""

    MAX_BATCH = MAX_CLASSIFIER_BATCH

    def __init__(self, features, labels, num_classes, hidden_units=(128,), likelihood_scaling=1., prior_std=1.,
                 batch_size=128, seed=0, eval_sets=None):
        self.num_classes, self.hidden_units = int(num_classes), tuple(int(h) for h in hidden_units)
        super().__init__(features, labels, CROSS_ENTROPY, num_classes, likelihood_scaling, prior_std, batch_size, seed,
                         eval_sets)

    def _check_network(self, num_features):
        if len(self.hidden_units) != 1:
            raise ValueError(f"hidden_units must name one hidden layer, got {self.hidden_units}")
        if not 1 <= num_features <= MAX_CLASSIFIER_FEATURES:
            raise ValueError(f"the network takes 1 to {MAX_CLASSIFIER_FEATURES} features, got {num_features}")
        if not 1 <= self.hidden_units[0] <= MAX_CLASSIFIER_HIDDEN:
            raise ValueError(f"the hidden layer must have 1 to {MAX_CLASSIFIER_HIDDEN} units, got {self.hidden_units[0]}")
        if not MIN_CLASSES <= self.num_classes <= MAX_CLASSES:
            raise ValueError(f"num_classes must lie in [{MIN_CLASSES}, {MAX_CLASSES}], got {self.num_classes}")

    def get_num_dimensions(self):
        return classifier_num_parameters(self.features.shape[1], self.hidden_units[0], self.num_classes)

    def _launch(self, x, call, want_grad):
        return hip_ops.target_bnn_classifier(self.ctx, self._X_dev, self._y_dev, self.hidden_units[0], self.num_classes,
                                             self.seed, call, self.batch_size, self.likelihood_scaling, self.prior_std, x,
                                             want_grad=want_grad)

    def predict(self, samples, features):
        """Logits [S, M, C] of the weight vectors ``samples`` [S, D] on the rows ``features`` [M, F]."""
        return hip_ops.bnn_classifier_predict(self.ctx, self.hidden_units[0], self.num_classes,
                                              *self._predict_operands(samples, features))


def load_mnist(dataset_dir=None):
    """MNIST from ``mnist/mnist.npz`` below the dataset directory, in the widely mirrored array layout: ``x_train`` uint8
    [60000, 28, 28], ``y_train`` [60000], ``x_test`` [10000, 28, 28], ``y_test``.  Features are uint8 / 255 in f32
    (bnn.py:329-331), flattened to 784; "test" is the first 5 000 test rows and "vali" the rest (bnn.py:336).  A file of
    the same layout with at most 5 000 test rows is split in halves.  Upstream reads the TFDS copy with shuffled files,
    so its row order is not reproducible; the rows here keep the file's order."""
    path = os.path.join(resolve_dataset_dir(dataset_dir, f"the MNIST target ({MNIST_FILE})"), MNIST_FILE)
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
                         eval_sets=_eval_sets(data))


def make_MNIST_target(likelihood_scaling, prior_std, batch_size, dataset_dir=None, seed=0):
    return BNN_MNIST(likelihood_scaling=likelihood_scaling, prior_std=prior_std, batch_size=batch_size,
                     dataset_dir=dataset_dir, seed=seed)


# ---- the generic network: any depth, activation and loss (BNN_LNPDF) -----------------------------------------------------
class BNN_LNPDF(_MinibatchBNN):
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

    MAX_BATCH = hip_ops.MLP_MAX_BATCH

    def __init__(self, likelihood_scaling=1., prior_std=1., batch_size=128, hidden_units=(8, 8), loss="mse",
                 activations=("sigmoid", "sigmoid", "linear"), features=None, labels=None, num_classes=None,
                 dataset_seed=-1, seed=0, eval_sets=None):
        self.dataset_seed = int(dataset_seed)
        if features is None:
            features, labels, eval_sets = self.prepare_data()
        if loss not in MLP_LOSSES:
            raise ValueError(f"loss must be one of {MLP_LOSSES}, got {loss!r}")
        if loss != MSE and num_classes is None:
            raise ValueError("num_classes is required for the sparse_categorical_crossentropy loss")
        self.hidden_units, self.activations = tuple(int(h) for h in hidden_units), tuple(activations)
        self.num_classes = None if loss == MSE else int(num_classes)
        super().__init__(features, labels, loss, 1 if loss == MSE else num_classes, likelihood_scaling, prior_std,
                         batch_size, seed, eval_sets)

    def prepare_data(self):
        """-> (features [T, F], labels [T], eval_sets or None); called when the constructor gets no ``features``."""
        raise NotImplementedError

    def _check_network(self, num_features):
        hip_ops.mlp_desc(num_features, self.hidden_units, self.activations, self.loss, self.num_outputs)

    def get_num_dimensions(self):
        return num_parameters(self.features.shape[1], self.hidden_units, self.num_outputs)

    def _launch(self, x, call, want_grad):
        return hip_ops.target_mlp(self.ctx, self._X_dev, self._y_dev, self.hidden_units, self.activations, self.loss,
                                  self.num_outputs, self.seed, call, self.batch_size, self.likelihood_scaling,
                                  self.prior_std, x, want_grad=want_grad)

    def predict(self, samples, features):
        """Network outputs [S, M] ("mse") or logits [S, M, C] of the weight vectors ``samples`` [S, D] on the rows
        ``features`` [M, F]."""
        return hip_ops.mlp_predict(self.ctx, self.hidden_units, self.activations, self.loss, self.num_outputs,
                                   *self._predict_operands(samples, features))
