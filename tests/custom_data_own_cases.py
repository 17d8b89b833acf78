"""Own minibatch per sample for user-defined device targets summed over a data set (gmmvi_target_custom_data_own_batches,
gmmvi_target_custom_data_tape_own_batches, ``use_own_batch_per_sample=True``): the NumPy restatement whose row list is per
sample, its planted faults and the kernel cases.

The sources and the per-row restatements are those of tests/custom_data_cases.py and tests/custom_data_tape_cases.py (logit,
student, ragged), unchanged.  ``OwnBatches`` wraps one of them: sample n of an evaluation is evaluated on row n of
``minibatch_stream.data_minibatch_rows_per_sample(seed, call, N, B, T)`` with n its index in the call.  float64 is the reference;
the fp32 twin is the same object in float32, the row sum accumulated sequentially in the order of j, s applied once to the
finished sum and the prior added last; ``evaluate(..., order="waves" | "tape", plan=...)`` forms the sum the way the forward
kernels (wave w adds positions w, w + 4, ..., wave 0 adds waves 1, 2, 3, chunks in index order) or the tape kernels (a lane adds
a chunk's positions in order, chunks in index order) form it.

Planted faults (``FAULTS``), each a mistake a kernel of this kind can make and the shared-batch kernels cannot:
  - ``tile_local_index``: the lane's index inside its 64-sample tile taken for n;
  - ``slab_local_index``: the index inside a slab of ``slab`` samples taken for n (what a slabbed tape launch would do);
  - ``epoch_stuck``: the epoch word never advanced (rank p mod T, epoch 0 for every sample);
  - ``batch_of_sample_0``: sample 0's batch used for every lane (what a row index made wave-uniform would do);
  - ``scale_per_row``: s applied at every row, to the running sum (sum = s * (sum + term)), instead of once to the finished sum.
tests/test_custom_data_own_host.py shows that each moves a committed case by more than 100 times the bound of the GPU test."""
import numpy as np

import custom_data_tape_cases as tape_cases
from custom_data_cases import Case, MINIBATCH_SEED, fp32_twin  # noqa: F401  (re-exported for the two test files)
from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms

SOURCES = tape_cases.SOURCES
FAULTS = ("tile_local_index", "slab_local_index", "epoch_stuck", "batch_of_sample_0", "scale_per_row")


def case_id(c):
    return f"{c.name}-D{c.d}-N{c.n}-T{c.rows}-B{c.batch}-chunks{c.chunks}-call{c.call}"


class OwnBatches:
    """``tgt``: a DataTarget with a batch size (its data, params, dtype, seed and call counter are this object's).  The object
    follows the call counter of MinibatchLNPDF like ``tgt`` does: one step per evaluation that receives a sample."""

    def __init__(self, tgt):
        assert tgt.batch_size is not None
        self.tgt = tgt

    def as_dtype(self, dtype):
        return OwnBatches(self.tgt.as_dtype(dtype))

    def get_num_dimensions(self):
        return self.tgt.get_num_dimensions()

    @property
    def call_count(self):
        return self.tgt.call_count

    def row_lists(self, n, fault=None, slab=None):
        """-> int64 [n, B]: the batch of every sample of an evaluation of n samples at the current call."""
        t = self.tgt
        T, B = t.num_data, t.batch_size
        if fault == "epoch_stuck":
            p = np.arange(n * B, dtype=np.int64)
            return ms.permute_rows(t.seed, t.call_count, np.zeros_like(p), p % T, T, stream=ms.STREAM_DATA_MINIBATCH).reshape(n, B)
        rows = ms.data_minibatch_rows_per_sample(t.seed, t.call_count, n, B, T)
        index = np.arange(n)
        if fault == "tile_local_index":
            index = index % 64
        elif fault == "slab_local_index":
            index = index % int(slab)
        elif fault == "batch_of_sample_0":
            index = index * 0
        return rows[index]

    def evaluate(self, x, fault=None, slab=None, order="sequence", plan=None):
        """-> (lp [N], grad [N, D]) in the target's dtype at the current call, counter untouched."""
        assert fault is None or fault in FAULTS
        t = self.tgt
        dt = t.dtype
        x = np.asarray(x, dt)
        lists = self.row_lists(x.shape[0], fault, slab)
        lp, grad = np.zeros(x.shape[0], dt), np.zeros(x.shape, dt)
        for n in range(x.shape[0]):
            one = t.as_dtype(dt)
            one.row_list = lambda call=None, rows=lists[n]: rows
            xn = x[n:n + 1]
            if fault == "scale_per_row":
                s = one.scale()
                v, g = np.zeros(1, dt), np.zeros(xn.shape, dt)
                for r in lists[n]:
                    rv, rg = one.row_term(xn, one.data[r].astype(dt))
                    v, g = (s * (v + rv).astype(dt)).astype(dt), (s * (g + rg).astype(dt)).astype(dt)
                pv, pg = one.prior(xn)
                v, g = (v + pv).astype(dt), (g + pg).astype(dt)
            elif order == "waves":
                v, g = one.evaluate_in_device_order(xn, plan)
            elif order == "tape":
                v, g = tape_cases.evaluate_in_tape_order(one, xn, plan)
            else:
                v, g = one.evaluate(xn)
            lp[n], grad[n] = v[0], g[0]
        return lp, grad

    def log_density_and_grad(self, x):
        out = self.evaluate(x)
        self.tgt._advance(x)
        return out

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------
STAGED_CAP = 120            # _lib.CUSTOM_STAGED_MAX_DIM (tests/test_custom_data_own_host.py checks it)
FORWARD_CAP = tape_cases.OLD_CAP
SLAB_CASE = Case("logit", 5, 130, 9, 0, 5, 3)        # three tiles: a tape budget of one tile makes three slabs


def kernel_cases():
    """Each at the smallest shape that reaches its seam, rows = T, batch = B.  N: one lane, the 64-sample tile from both sides,
    more than two tiles.  (T, B): a batch that straddles an epoch boundary (9, 5), B = T (9, 9) and (257, 257), a batch cut into
    chunks (257, 64), fewer positions than the four waves (5, 1), (7, 2), (7, 3).  D: 1, the pass width of forward mode from both
    sides, the staged route's cap from both sides; the forward mode's cap from both sides and 1100 (the gradient of 513 and 1100
    is the tape class's alone).  Chunk requests 0 .. 3 at B = 64.  ragged: tape lengths that differ lane by lane at every
    position, in one chunk and in three."""
    return ([Case("logit", 5, n, 9, 0, 5, 3) for n in (1, 63, 64, 65, 130)]
            + [Case("logit", 5, 65, t, 0, b, 0) for t, b in ((9, 9), (257, 64), (5, 1), (7, 2), (7, 3))]
            + [Case("student", 5, 65, 257, 0, 257, 3)]
            + [Case("logit", d, 65, 9, 0, 5, 3) for d in (1, 16, 17, STAGED_CAP, STAGED_CAP + 1)]
            + [Case("logit", d, 65, 9, 0, 5, 3) for d in (FORWARD_CAP, FORWARD_CAP + 1, 1100)]
            + [Case("logit", 17, 65, 257, k, 64, 3) for k in (1, 2, 3)]
            + [Case("ragged", 6, 65, 9, 0, 5, 3), Case("ragged", 6, 65, 257, 3, 64, 0)])


def build_case(c):
    """-> (fp64 OwnBatches, x [n, d] fp32) on the data and samples of custom_data_tape_cases.build_case."""
    tgt, x = tape_cases.build_case(c)
    return OwnBatches(tgt), x


_refs = {}


def reference(c):
    """-> (target, x, lp64, g64, lp32, g32), computed once per case and read-only."""
    if c not in _refs:
        tgt, x = build_case(c)
        lp64, g64 = tgt.evaluate(x.astype(np.float64))
        lp32, g32 = tgt.as_dtype(np.float32).evaluate(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[c] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[c]
