"""fp64 NumPy reference of the Bayesian-neural-network regression target (reference: target_distributions/bnn.py:59-311,
385-448) and the WINE fixture.  ``BNNRef`` has the oracle's target interface (oracle/targets.py), so
``oracle.train.OracleGMMVI`` runs on it; it keeps its own call counter and restates the minibatch stream (the Feistel
network of DESIGN.md 6) on its own, with ``oracle.philox.philox4x32_10`` for the round function."""
import os

import numpy as np

from oracle.philox import philox4x32_10

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wine_seed_0.npz")
ARRAYS = ("features_train", "labels_train", "features_test", "labels_test", "features_vali", "labels_vali")
STREAM_MINIBATCH = 3


def load_wine():
    """The six arrays of upstream's wine_seed_0.npz (features f32, labels int32)."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in ARRAYS}


def write_dataset_dir(path, seeds=(0,)):
    """A dataset directory laid out like upstream's datasets/ folder: wine/wine_seed_{i}.npz, each the fixture."""
    os.makedirs(os.path.join(str(path), "wine"), exist_ok=True)
    data = load_wine()
    for i in seeds:
        np.savez(os.path.join(str(path), "wine", f"wine_seed_{i}.npz"), **data)
    return str(path)


def stream_rows(seed, call, n, batch_size, num_data):
    """int64 [n, batch_size]: row pi_{seed,call,e}(r) for stream position p = i B + j, e = p // T, r = p % T."""
    T = int(num_data)
    bits = 0
    while (1 << bits) < T:
        bits += 1
    h = -(-bits // 2)
    mask = (1 << h) - 1
    p = np.arange(int(n) * int(batch_size), dtype=np.int64)
    epoch, x = (p // T).astype(np.uint32), (p % T).astype(np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
    done = np.zeros(x.shape, bool)
    out = x.copy()
    while not done.all():
        left, right = out >> np.uint32(h), out & np.uint32(mask)
        for i in range(4):
            ctr = np.stack([right | np.uint32(i << 24), epoch, np.full_like(epoch, int(call) & 0xFFFFFFFF),
                            np.full_like(epoch, STREAM_MINIBATCH)], axis=-1)
            f = philox4x32_10(ctr, key)[..., 0] & np.uint32(mask)
            left, right = right, left ^ f
        nxt = (left << np.uint32(h)) | right
        out = np.where(done, out, nxt)                         # cycle walking until the value lies below T
        done = out < T
    return out.astype(np.int64).reshape(int(n), int(batch_size))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def unpack(w, num_features, hidden_units=(8, 8)):
    """[D] -> [(W [in, out], b [out])] in the reference's layout."""
    layers, start, last = [], 0, num_features
    for width in list(hidden_units) + [1]:
        W = w[start:start + last * width].reshape(last, width)
        start += last * width
        b = w[start:start + width]
        start += width
        layers.append((W, b))
        last = width
    assert start == len(w)
    return layers


def literal_forward(features, w, hidden_units=(8, 8)):
    """forward_from_weight_vector (bnn.py:151-166) line by line in fp64: reshape slices of w, output @ W + b, activation."""
    input_dim = features.shape[-1]
    layer_shape, layer_size, last = [], [], input_dim
    for width in hidden_units:
        layer_shape += [[last, width], [width]]
        layer_size += [last * width, width]
        last = width
    layer_shape += [[last, 1], [1]]
    layer_size += [last, 1]
    activations = [sigmoid, sigmoid, lambda a: a]
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


def literal_mse(labels, output):
    """tf.keras.losses.MeanSquaredError()(labels [B], output [B, 1]): the (B, 1) prediction is squeezed to (B,)."""
    return np.mean((np.asarray(labels, np.float64) - np.squeeze(output, -1)) ** 2)


class BNNRef:
    """s (-T mean_m (y_m - f(x_m; w))^2 - 0.5 |w|^2 / sd^2) with its gradient in fp64, minibatches from the stream."""

    def __init__(self, features, labels, hidden_units=(8, 8), likelihood_scaling=1.0, prior_std=1.0, batch_size=128,
                 seed=0):
        self.X = np.asarray(features, np.float64)
        self.y = np.asarray(labels, np.float64)
        self.hidden_units = tuple(hidden_units)
        self.s, self.prior_std, self.B, self.seed = float(likelihood_scaling), float(prior_std), int(batch_size), seed
        self.T, self.F = self.X.shape
        h1, h2 = self.hidden_units
        self.D = self.F * h1 + h1 + h1 * h2 + h2 + h2 + 1
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
        w = np.atleast_2d(np.asarray(w, np.float64))
        n = w.shape[0]
        lp = np.empty(n)
        grad = np.empty((n, self.D)) if want_grad else None
        c = self.T / self.B
        for i in range(n):
            (W1, b1), (W2, b2), (W3, b3) = unpack(w[i], self.F, self.hidden_units)
            x, y = self.X[rows[i]], self.y[rows[i]]
            h1 = sigmoid(x @ W1 + b1)
            h2 = sigmoid(h1 @ W2 + b2)
            r = y - (h2 @ W3 + b3)[:, 0]
            lp[i] = self.s * (-c * np.sum(r * r) - 0.5 * np.sum(w[i] ** 2) / self.prior_std ** 2)
            if want_grad:
                d3 = 2.0 * c * r                                         # d ll / d f
                d2 = d3[:, None] * W3[:, 0][None, :] * h2 * (1 - h2)
                d1 = (d2 @ W2.T) * h1 * (1 - h1)
                g = np.concatenate([(x.T @ d1).ravel(), d1.sum(0), (h1.T @ d2).ravel(), d2.sum(0), h2.T @ d3, [d3.sum()]])
                grad[i] = self.s * (g - w[i] / self.prior_std ** 2)
        return lp, grad

    def abs_terms(self, w, rows):
        """Scale of the f32 rounding of lp: T/B sum r^2 + 0.5 |w|^2 / sd^2 (both terms are negative)."""
        return -self.evaluate_rows(w, rows, want_grad=False)[0] / self.s

    def log_density(self, w):
        w = np.atleast_2d(np.asarray(w, np.float64))
        return self.evaluate_rows(w, self.next_rows(w.shape[0]), want_grad=False)[0]

    def log_density_and_grad(self, w):
        w = np.atleast_2d(np.asarray(w, np.float64))
        return self.evaluate_rows(w, self.next_rows(w.shape[0]), want_grad=True)

    def predict(self, w, features):
        """[S, M] network outputs."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        return np.stack([literal_forward(features, wi, self.hidden_units)[:, 0] for wi in w])
