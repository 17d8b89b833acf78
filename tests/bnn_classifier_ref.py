"""NumPy reference of the Bayesian-neural-network classification target (reference: target_distributions/bnn.py,
BNN_LNPDF with the network and loss of BNN_MNIST) and synthetic data for its tests.  ``BNNClassifierRef`` has the interface
of ``bnn_ref.BNNRef`` (the oracle's target interface), takes its minibatches from the same stream and keeps its own call
counter; ``dtype=np.float32`` evaluates the same formulas in single precision (the yardstick of the kernel's error bound)."""
import os

import numpy as np

from bnn_ref import stream_rows


def num_parameters(num_features, hidden, num_classes):
    return num_features * hidden + hidden + hidden * num_classes + num_classes


def offsets(num_features, hidden, num_classes):
    """Start of W1, b1, W2, b2 in the parameter vector, and its length."""
    o_b1 = num_features * hidden
    o_w2 = o_b1 + hidden
    o_b2 = o_w2 + hidden * num_classes
    return 0, o_b1, o_w2, o_b2, o_b2 + num_classes


def unpack(w, num_features, hidden, num_classes):
    o_w1, o_b1, o_w2, o_b2, d = offsets(num_features, hidden, num_classes)
    assert w.shape[-1] == d
    return (w[o_w1:o_b1].reshape(num_features, hidden), w[o_b1:o_w2], w[o_w2:o_b2].reshape(hidden, num_classes),
            w[o_b2:d])


def log_softmax(l):
    mx = l.max(-1, keepdims=True)
    return l - (mx + np.log(np.exp(l - mx).sum(-1, keepdims=True)))


def literal_forward(features, w, hidden, num_classes):
    """forward_from_weight_vector (bnn.py:151-166) line by line in fp64 with BNN_MNIST's layers: hidden_units [hidden],
    activations [relu, linear]."""
    input_dim = features.shape[-1]
    layer_shape = [[input_dim, hidden], [hidden], [hidden, num_classes], [num_classes]]
    layer_size = [input_dim * hidden, hidden, hidden * num_classes, num_classes]
    activations = [lambda a: np.maximum(a, 0.0), lambda a: a]
    output = np.reshape(features, [-1, input_dim]).astype(np.float64)
    start = i = j = 0
    while i < len(layer_shape):
        W = np.reshape(w[start:start + layer_size[i]], layer_shape[i])
        start += layer_size[i]
        i += 1
        b = np.reshape(w[start:start + layer_size[i]], layer_shape[i])
        start += layer_size[i]
        i += 1
        output = activations[j](output @ W + b)
        j += 1
    return output


def literal_cross_entropy(labels, logits):
    """tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True)(labels [B], logits [B, C]): the mean over the
    batch of -log_softmax(logits)[label]."""
    ls = log_softmax(np.asarray(logits, np.float64))
    return np.mean(-ls[np.arange(len(labels)), np.asarray(labels, np.int64)])


class BNNClassifierRef:
    """s (-T mean_m CE_m - 0.5 |w|^2 / sd^2) with its gradient, minibatches from the stream."""

    def __init__(self, features, labels, num_classes, hidden=128, likelihood_scaling=1.0, prior_std=1.0, batch_size=128,
                 seed=0, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.X = np.asarray(features, self.dtype)
        self.y = np.asarray(labels, np.int64)
        self.H, self.C = int(hidden), int(num_classes)
        self.s, self.prior_std, self.B, self.seed = float(likelihood_scaling), float(prior_std), int(batch_size), seed
        self.T, self.F = self.X.shape
        self.D = num_parameters(self.F, self.H, self.C)
        self.call_count = 0

    def get_num_dimensions(self):
        return self.D

    def next_rows(self, n):
        rows = stream_rows(self.seed, self.call_count, n, self.B, self.T)
        if n >= 1:
            self.call_count += 1
        return rows

    def evaluate_rows(self, w, rows, want_grad=True):
        """lp [N], grad [N, D] (or None) of the weight vectors w [N, D] on the given batch rows [N, B]."""
        t = self.dtype.type
        w = np.atleast_2d(np.asarray(w, self.dtype))
        n = w.shape[0]
        lp = np.empty(n, self.dtype)
        grad = np.empty((n, self.D), self.dtype) if want_grad else None
        c, s, inv_var = t(self.T / self.B), t(self.s), t(1.0 / self.prior_std ** 2)
        for i in range(n):
            W1, b1, W2, b2 = unpack(w[i], self.F, self.H, self.C)
            x, y = self.X[rows[i]], self.y[rows[i]]
            z1 = x @ W1 + b1
            h = np.maximum(z1, t(0))
            ls = log_softmax(h @ W2 + b2)
            ce = -ls[np.arange(len(y)), y]
            lp[i] = s * (-c * np.sum(ce) - t(0.5) * np.sum(w[i] ** 2) * inv_var)
            if want_grad:
                dl = np.exp(ls)
                dl[np.arange(len(y)), y] -= t(1)
                dl *= -c                                                 # d(-c sum CE) / d logits
                dz = (dl @ W2.T) * (z1 > 0)
                g = np.concatenate([(x.T @ dz).ravel(), dz.sum(0), (h.T @ dl).ravel(), dl.sum(0)])
                grad[i] = s * (g - w[i] * inv_var)
        return lp, grad

    def min_abs_preactivation(self, w, rows):
        """Smallest |z1| over the samples and their batch rows: the distance from the ReLU kink."""
        w = np.atleast_2d(np.asarray(w, self.dtype))
        return min(np.abs(self.X[rows[i]] @ unpack(w[i], self.F, self.H, self.C)[0] +
                          unpack(w[i], self.F, self.H, self.C)[1]).min() for i in range(w.shape[0]))

    def log_density(self, w):
        w = np.atleast_2d(np.asarray(w, self.dtype))
        return self.evaluate_rows(w, self.next_rows(w.shape[0]), want_grad=False)[0]

    def log_density_and_grad(self, w):
        w = np.atleast_2d(np.asarray(w, self.dtype))
        return self.evaluate_rows(w, self.next_rows(w.shape[0]), want_grad=True)

    def predict(self, w, features):
        """[S, M, C] logits."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        return np.stack([literal_forward(np.asarray(features, np.float64), wi, self.H, self.C) for wi in w])


def separable_data(num_rows, num_features, num_classes, rng, spread=2.0, noise=0.7):
    """Gaussian blobs around ``num_classes`` random centres: features f32 [rows, F], labels int32 [rows]."""
    centres = rng.normal(size=(num_classes, num_features)) * spread
    y = rng.integers(0, num_classes, size=num_rows)
    X = centres[y] + rng.normal(size=(num_rows, num_features)) * noise
    return X.astype(np.float32), y.astype(np.int32)


def write_mnist_dir(path, num_train, num_test, seed=0):
    """A dataset directory holding mnist/mnist.npz in the widely mirrored layout (x_train uint8 [n, 28, 28], y_train,
    x_test, y_test) with random images and labels.  Returns (directory, the arrays)."""
    rng = np.random.default_rng(seed)
    arrays = {"x_train": rng.integers(0, 256, size=(num_train, 28, 28), dtype=np.uint8),
              "y_train": rng.integers(0, 10, size=num_train).astype(np.uint8),
              "x_test": rng.integers(0, 256, size=(num_test, 28, 28), dtype=np.uint8),
              "y_test": rng.integers(0, 10, size=num_test).astype(np.uint8)}
    os.makedirs(os.path.join(str(path), "mnist"), exist_ok=True)
    np.savez(os.path.join(str(path), "mnist", "mnist.npz"), **arrays)
    return str(path), arrays
