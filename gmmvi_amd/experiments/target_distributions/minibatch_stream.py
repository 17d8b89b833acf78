"""The minibatch streams in NumPy (the device's copy is csrc/feistel.h) and the call-counter protocol of the
targets that draw from them.

A stream permutes the T training rows by pi_{seed,call,epoch}, a balanced 4-round Feistel network on 2h bits
(h = ceil(ceil(log2 T) / 2)) with cycle walking, round i mapping (L, R) -> (R, L xor (F_i(R) & (2^h - 1))), F_i(R) = word 0
of Philox4x32-10 with key (seed lo, seed hi) and counter (R | i << 24, epoch, call, stream).  Stream ids 0-2 are the
samplers (component normals, categorical draws, mixture normals); 3 is the Bayesian neural networks' stream
(``minibatch_rows`` below), 4 the minibatch logistic regressions' (epoch word 0, ``logistic_regression.minibatch_rows``), 5
the minibatches of user-defined targets summed over a data set (``data_minibatch_rows`` below: epoch word 0, one batch per
call; ``data_minibatch_rows_per_sample``: the BNN stream's layout, a batch per sample).
"""
import numpy as np

from .lnpdf import LNPDF

STREAM_BNN_MINIBATCH, STREAM_LOGREG_MINIBATCH, STREAM_DATA_MINIBATCH = 3, 4, 5

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


def permute_rows(seed, call, epoch, rank, num_data, stream=STREAM_BNN_MINIBATCH):
    """pi_{seed,call,epoch}(rank) for int arrays epoch, rank (rank < num_data) -> int64 rows.  ``stream`` is the counter's
    last word: 3 (the default) for the BNN minibatches, 4 for the minibatch logistic regressions."""
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
    """The data rows of the n BNN minibatches of call ``call``: int64 [n, batch_size].  Row j of sample i has stream
    position p = i * batch_size + j, epoch p div T and rank p mod T: every epoch visits every row once."""
    p = np.arange(int(n) * int(batch_size), dtype=np.int64)
    return permute_rows(seed, call, p // num_data, p % num_data, num_data).reshape(int(n), int(batch_size))


def data_minibatch_rows(seed, call, batch_size, num_data):
    """The data rows of the minibatch of call ``call`` of a ``DeviceDataLNPDF``: int64 [batch_size], row j = pi(j) of epoch 0 on
    stream 5.  One batch per call, shared by all samples; batch_size == num_data is a permutation of all rows."""
    if not 1 <= int(batch_size) <= int(num_data):
        raise ValueError(f"batch_size must be in 1..{num_data}, got {batch_size}")
    j = np.arange(int(batch_size), dtype=np.int64)
    return permute_rows(seed, call, np.zeros_like(j), j, num_data, stream=STREAM_DATA_MINIBATCH)


def data_minibatch_rows_per_sample(seed, call, n, batch_size, num_data):
    """The data rows of the n minibatches of call ``call`` of a ``DeviceDataLNPDF(use_own_batch_per_sample=True)``: int64
    [n, batch_size].  Row j of sample i has stream position p = i * batch_size + j, epoch p div T and rank p mod T on stream 5
    (the layout of ``minibatch_rows``).  Row 0 is ``data_minibatch_rows`` of the same call; the batches of one epoch are
    disjoint; a batch that straddles an epoch boundary takes its tail from the next epoch and may hold one row twice;
    batch_size == num_data gives every sample a permutation of all rows."""
    if not 1 <= int(batch_size) <= int(num_data):
        raise ValueError(f"batch_size must be in 1..{num_data}, got {batch_size}")
    p = np.arange(int(n) * int(batch_size), dtype=np.int64)
    rows = permute_rows(seed, call, p // num_data, p % num_data, num_data, stream=STREAM_DATA_MINIBATCH)
    return rows.reshape(int(n), int(batch_size))


class MinibatchLNPDF(LNPDF):
    """A target whose every evaluation draws fresh minibatches from the stream of (``seed``, ``call_count``).  The call
    counter advances after every ``log_density`` / ``log_density_and_grad`` that receives at least one sample.  A subclass
    sets ``self.ctx`` and implements ``_launch``."""

    def __init__(self, seed):
        super().__init__(use_log_density_and_grad=True)
        self.seed = int(seed)
        self._call = 0

    @property
    def call_count(self):
        return self._call

    def _launch(self, x, call, want_grad):
        """-> (lp [n], grad [n, D] or None) of the device array x [n, D] on the batches of call ``call``."""
        raise NotImplementedError

    def _evaluate(self, x, want_grad):
        x = self.ctx.asarray(x)
        lp, grad = self._launch(x, self._call, want_grad)
        if x.shape[0] >= 1:
            self._call += 1
        return lp, grad

    def log_density(self, x):
        return self._evaluate(x, False)[0]

    def log_density_and_grad(self, x):
        return self._evaluate(x, True)
