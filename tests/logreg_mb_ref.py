"""fp64 NumPy reference of the minibatch logistic-regression targets (reference: target_distributions/
logistic_regression.py:70-174).  ``LogRegMbRef`` has the oracle's target interface (oracle/targets.py), so
``oracle.train.OracleGMMVI`` runs on it; it keeps its own call counter and restates the batch map of DESIGN.md 6 on its
own, with ``oracle.philox.philox4x32_10`` for the Feistel round function (stream 4, epoch word 0)."""
import numpy as np

from logreg_ref import LOG_2PI, log_sigmoid, sigmoid
from oracle.philox import philox4x32_10

STREAM = 4


def rho(seed, call, positions, num_data):
    """rho_{seed,call}(p) for an int array of positions p < T: a 4-round Feistel network on 2h bits, h =
    ceil(ceil(log2 T) / 2), applied again while the value is >= T; round i: (L, R) -> (R, L xor (F_i(R) & (2^h - 1))),
    F_i(R) = word 0 of Philox4x32-10, key (seed lo, seed hi), counter (R | i << 24, 0, call, 4)."""
    T = int(num_data)
    bits = 0
    while (1 << bits) < T:
        bits += 1
    h = -(-bits // 2)
    mask = np.uint32((1 << h) - 1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
    out = np.asarray(positions, np.int64).astype(np.uint32).reshape(-1)
    zero = np.zeros_like(out)
    done = np.zeros(out.shape, bool)
    while not done.all():
        left, right = out >> np.uint32(h), out & mask
        for i in range(4):
            ctr = np.stack([right | np.uint32(i << 24), zero, np.full_like(out, int(call) & 0xFFFFFFFF),
                            np.full_like(out, STREAM)], axis=-1)
            left, right = right, left ^ (philox4x32_10(ctr, key)[..., 0] & mask)
        nxt = (left << np.uint32(h)) | right
        out = np.where(done, out, nxt)
        done = out < T
    return out.astype(np.int64).reshape(np.shape(positions))


def batch_rows(seed, call, n, batch_size, num_data, num_batches):
    """int64 [n, B]: row j of sample i is rho((i mod nb) B + j)."""
    i = np.arange(int(n))[:, None]
    j = np.arange(int(batch_size))[None, :]
    return rho(seed, call, (i % int(num_batches)) * int(batch_size) + j, num_data)


def upstream_start_loop_rows(perm, n, batch_size, use_own_batch_per_sample):
    """Upstream's log_density (:123-142) literally, with ``perm`` standing for the shuffled order of the training rows:
    ``start`` advances by B and resets to 0 when start + B > T; without own batches every sample takes the first B."""
    T, B = len(perm), int(batch_size)
    rows = []
    if use_own_batch_per_sample:
        start = 0
        for _ in range(int(n)):
            if start + B > T:
                start = 0
            rows.append(perm[np.arange(T)[start:start + B]])
            start = start + B
    else:
        rows = [perm[np.arange(T)[0:B]]] * int(n)
    return np.asarray(rows, np.int64).reshape(int(n), B)


class LogRegMbRef:
    """(T / B) sum_j log sigma(a_row . w) + isotropic normal prior, with its gradient, in fp64 on the training rows A."""

    def __init__(self, A, batch_size, use_own_batch_per_sample=True, seed=0, prior_mean=0.0, prior_std=10.0):
        self.A = np.asarray(A, np.float64)
        self.T, self.D = self.A.shape
        self.B, self.seed = int(batch_size), int(seed)
        self.nb = self.T // self.B if use_own_batch_per_sample else 1
        self.prior_mean, self.prior_std = float(prior_mean), float(prior_std)
        self.call_count = 0

    def get_num_dimensions(self):
        return self.D

    def rows(self, call, n):
        return batch_rows(self.seed, call, n, self.B, self.T, self.nb)

    def _prior(self, w):
        z = (w - self.prior_mean) / self.prior_std
        return np.sum(-np.log(self.prior_std) - 0.5 * LOG_2PI - 0.5 * z * z, axis=1)

    def evaluate_rows(self, w, rows, want_grad=True):
        """lp [N], grad [N, D] (or None) of w [N, D] on the given batch rows [N, B] (samples that share a batch are
        evaluated together)."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        batches, cls = np.unique(np.asarray(rows), axis=0, return_inverse=True)
        cls = np.asarray(cls).reshape(-1)
        c = self.T / self.B
        lp = self._prior(w)
        grad = -(w - self.prior_mean) / self.prior_std ** 2 if want_grad else None
        for k, batch in enumerate(batches):
            idx = np.nonzero(cls == k)[0]
            Ab = self.A[batch]                                     # [B, D]
            t = w[idx] @ Ab.T
            lp[idx] += c * log_sigmoid(t).sum(1)
            if want_grad:
                grad[idx] += c * (sigmoid(-t) @ Ab)
        return lp, grad

    def abs_terms(self, w, rows):
        """Scales of the f32 rounding, with u_j = sum_d |a_jd w_d| (the rounding of t_j is a multiple of u_j, not of
        |t_j|): (T / B) sum_j (|log sigma(t_j)| + sigma(-t_j) u_j) + |prior| for lp, and
        (T / B) max_d sum_j (sigma(-t_j) + sigma(t_j) sigma(-t_j) u_j) |a_jd| + max_d |w_d - mu| / sd^2 for the gradient
        -> ([N], [N])."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        batches, cls = np.unique(np.asarray(rows), axis=0, return_inverse=True)
        cls = np.asarray(cls).reshape(-1)
        c = self.T / self.B
        lps, gs = np.abs(self._prior(w)), np.abs(w - self.prior_mean).max(1) / self.prior_std ** 2
        for k, batch in enumerate(batches):
            idx = np.nonzero(cls == k)[0]
            Ab = self.A[batch]
            t = w[idx] @ Ab.T
            u = np.abs(w[idx]) @ np.abs(Ab).T
            sm, sp = sigmoid(-t), sigmoid(t)
            lps[idx] += c * (np.abs(log_sigmoid(t)) + sm * u).sum(1)
            gs[idx] += c * ((sm + sp * sm * u) @ np.abs(Ab)).max(1)
        return lps, gs

    def _next_rows(self, n):
        rows = self.rows(self.call_count, n)
        if n >= 1:
            self.call_count += 1
        return rows

    def log_density(self, w):
        w = np.atleast_2d(np.asarray(w, np.float64))
        return self.evaluate_rows(w, self._next_rows(w.shape[0]), want_grad=False)[0]

    def log_density_and_grad(self, w):
        w = np.atleast_2d(np.asarray(w, np.float64))
        return self.evaluate_rows(w, self._next_rows(w.shape[0]), want_grad=True)

    def log_density_fb(self, w):
        """The full-batch posterior on the training rows (no call)."""
        w = np.atleast_2d(np.asarray(w, np.float64))
        return log_sigmoid(w @ self.A.T).sum(1) + self._prior(w)
