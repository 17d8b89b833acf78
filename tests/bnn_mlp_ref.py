"""NumPy reference of the generic Bayesian-neural-network target (reference: target_distributions/bnn.py, BNN_LNPDF with any
hidden_units list, one activation per layer and an MSE or sparse categorical cross-entropy loss): forward pass, loss,
prior, gradient and predict.  ``BNNMlpRef`` has the oracle's target interface (oracle/targets.py), takes its minibatch rows
from ``bnn.minibatch_rows`` and keeps its own call counter; ``dtype=np.float32`` evaluates the same formulas in single
precision (the yardstick of the kernel's error bound)."""
import numpy as np

from gmmvi_amd.experiments.target_distributions.bnn import minibatch_rows

ACTIVATIONS = ("linear", "sigmoid", "relu", "tanh")
LOSSES = ("mse", "sparse_categorical_crossentropy")


def num_parameters(num_features, hidden_units, num_outputs):
    d, last = 0, int(num_features)
    for width in list(hidden_units) + [int(num_outputs)]:
        d += last * int(width) + int(width)
        last = int(width)
    return d


def unpack(w, num_features, hidden_units, num_outputs):
    """[D] -> [(W [in, out], b [out])] in the reference's layout."""
    layers, start, last = [], 0, int(num_features)
    for width in list(hidden_units) + [int(num_outputs)]:
        W = w[start:start + last * width].reshape(last, width)
        start += last * width
        b = w[start:start + width]
        start += width
        layers.append((W, b))
        last = width
    assert start == w.shape[-1]
    return layers


def sigmoid(z):
    one = z.dtype.type(1)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, one / (one + e), e / (one + e))


def activate(name, z):
    if name == "sigmoid":
        return sigmoid(z)
    if name == "relu":
        return np.maximum(z, z.dtype.type(0))
    if name == "tanh":
        return np.tanh(z)
    assert name == "linear"
    return z


def activation_derivative(name, z, h):
    """d act / d z at the pre-activation z with value h (ReLU: 1 where z > 0, else 0)."""
    one = z.dtype.type(1)
    if name == "sigmoid":
        return h * (one - h)
    if name == "relu":
        return (z > 0).astype(z.dtype)
    if name == "tanh":
        return one - h * h
    return np.ones_like(z)


def log_softmax(l):
    mx = l.max(-1, keepdims=True)
    return l - (mx + np.log(np.exp(l - mx).sum(-1, keepdims=True)))


class BNNMlpRef:
    """s (-T mean_m loss_m - 0.5 |w|^2 / sd^2) with its gradient, minibatches from the stream."""

    def __init__(self, features, labels, hidden_units, activations, loss, num_classes=None, likelihood_scaling=1.0,
                 prior_std=1.0, batch_size=128, seed=0, dtype=np.float64):
        assert loss in LOSSES and all(a in ACTIVATIONS for a in activations)
        assert len(activations) == len(hidden_units) + 1 and activations[-1] == "linear"
        self.dtype = np.dtype(dtype)
        self.X = np.asarray(features, self.dtype)
        self.loss = loss
        self.y = np.asarray(labels, self.dtype if loss == "mse" else np.int64)
        self.hidden_units, self.activations = tuple(int(h) for h in hidden_units), tuple(activations)
        self.C = 1 if loss == "mse" else int(num_classes)
        self.s, self.prior_std, self.B, self.seed = float(likelihood_scaling), float(prior_std), int(batch_size), seed
        self.T, self.F = self.X.shape
        self.D = num_parameters(self.F, self.hidden_units, self.C)
        self.call_count = 0

    def get_num_dimensions(self):
        return self.D

    def next_rows(self, n):
        rows = minibatch_rows(self.seed, self.call_count, n, self.B, self.T)
        if n >= 1:
            self.call_count += 1
        return rows

    def forward(self, wi, x):
        """-> (pre-activations z_l, values h_l with h_0 = x) of one weight vector on the rows x."""
        zs, hs = [], [x]
        for (W, b), a in zip(unpack(wi, self.F, self.hidden_units, self.C), self.activations):
            zs.append(hs[-1] @ W + b)
            hs.append(activate(a, zs[-1]))
        return zs, hs

    def evaluate_rows(self, w, rows, want_grad=True):
        """lp [N], grad [N, D] (or None) of the weight vectors w [N, D] on the given batch rows [N, B]."""
        t = self.dtype.type
        w = np.atleast_2d(np.asarray(w, self.dtype))
        n = w.shape[0]
        lp = np.empty(n, self.dtype)
        grad = np.empty((n, self.D), self.dtype) if want_grad else None
        c, s, inv_var = t(self.T / self.B), t(self.s), t(1.0 / self.prior_std ** 2)
        for i in range(n):
            layers = unpack(w[i], self.F, self.hidden_units, self.C)
            x, y = self.X[rows[i]], self.y[rows[i]]
            zs, hs = self.forward(w[i], x)
            out = hs[-1]
            if self.loss == "mse":
                r = y - out[:, 0]
                total = np.sum(r * r)
                d = (t(2) * c * r)[:, None]                              # d(-c sum loss) / d out
            else:
                ls = log_softmax(out)
                total = np.sum(-ls[np.arange(len(y)), y])
                d = np.exp(ls)
                d[np.arange(len(y)), y] -= t(1)
                d *= -c
            lp[i] = s * (-c * total - t(0.5) * np.sum(w[i] ** 2) * inv_var)
            if want_grad:
                parts = []
                for l in range(len(layers) - 1, -1, -1):                 # d = d lp / d z_l
                    parts.append(d.sum(0))
                    parts.append((hs[l].T @ d).ravel())
                    if l > 0:
                        d = (d @ layers[l][0].T) * activation_derivative(self.activations[l - 1], zs[l - 1], hs[l])
                g = np.concatenate(parts[::-1])
                grad[i] = s * (g - w[i] * inv_var)
        return lp, grad

    def min_abs_relu_preactivation(self, w, rows):
        """Smallest |z| over the ReLU layers, the samples and their batch rows: the distance from the kink (inf: no ReLU)."""
        w = np.atleast_2d(np.asarray(w, self.dtype))
        best = np.inf
        for i in range(w.shape[0]):
            zs, _ = self.forward(w[i], self.X[rows[i]])
            for z, a in zip(zs, self.activations):
                if a == "relu":
                    best = min(best, float(np.abs(z).min()))
        return best

    def log_density(self, w):
        w = np.atleast_2d(np.asarray(w, self.dtype))
        return self.evaluate_rows(w, self.next_rows(w.shape[0]), want_grad=False)[0]

    def log_density_and_grad(self, w):
        w = np.atleast_2d(np.asarray(w, self.dtype))
        return self.evaluate_rows(w, self.next_rows(w.shape[0]), want_grad=True)

    def predict(self, w, features):
        """[S, M] outputs ("mse") or [S, M, C] logits, in fp64."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        ref = self if self.dtype == np.float64 else BNNMlpRef(self.X, self.y, self.hidden_units, self.activations,
                                                              self.loss, self.C)
        outs = np.stack([ref.forward(wi, np.asarray(features, np.float64))[1][-1] for wi in w])
        return outs[..., 0] if self.loss == "mse" else outs
