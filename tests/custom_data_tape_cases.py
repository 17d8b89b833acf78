"""Reverse-mode gradients of user-defined device targets summed over a data set (csrc/custom_target_data_tape.inc,
DeviceDataTapeLNPDF): the kernel cases, one more test target, three more planted faults and the device's summation order.

The sources and restatements of tests/custom_data_cases.py (logit, student, nodata) are the reference as they are; ``ragged``
is added here because its tape length differs from row to row and from lane to lane, which none of those three shows.  The bound
is the one of tests/test_hip_custom_target.py (_bound), unchanged."""
import numpy as np

import custom_data_cases as base
from custom_data_cases import Case, case_id, fp32_twin  # noqa: F401  (re-exported for the two test files)

# ---- ragged: rows [features (D) | response | repeat count 0 .. 3], params = [prior std] -----------------------------------------
# The record count of a row term depends on the row (the repeat count) and on x (the branch on the sign of the residual).  Both
# extra terms vanish with their first derivative's jump at r = 0: 0.25 r exp(-r) is 0 there, so the value is continuous.
RAGGED_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T r = row[D];
    for (int i = 0; i < D; ++i) r -= row[i] * x[i];
    T v = -0.5f * r * r;
    const int repeats = (int)row[D + 1];
    for (int j = 0; j < repeats; ++j) v -= 0.1f * log1p(r * r);
    if (r > 0.f) v -= 0.25f * r * exp(-r);
    return v;
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float s = params[0];
    T q = 0.f;
    for (int i = 0; i < D; ++i) q += x[i] * x[i];
    return -0.5f * q / (s * s);
}
"""

SOURCES = dict(base.SOURCES, ragged=RAGGED_SRC)


class Ragged(base.DataTarget):
    """The restatement of RAGGED_SRC; ``as_dtype(np.float32)`` is its fp32 twin."""

    def __init__(self, data, params, dtype=np.float64, batch_size=None, seed=0, call=0, d=None):
        super().__init__(data, params, dtype, batch_size, seed, call, np.shape(data)[1] - 2 if d is None else d)

    def row_term(self, x, row):
        dt = self.dtype
        a, t, repeats = row[:-2], row[-2], int(row[-1])
        r = (t - (x @ a).astype(dt)).astype(dt)
        v = dt(-0.5) * r * r
        dr = -r
        for _ in range(repeats):
            v = v - dt(0.1) * np.log1p(r * r)
            dr = dr - dt(0.2) * r / (dt(1) + r * r)
        e = np.exp(-r)
        v = v - np.where(r > 0, dt(0.25) * r * e, dt(0))
        dr = dr - np.where(r > 0, dt(0.25) * (dt(1) - r) * e, dt(0))
        return v.astype(dt), ((-dr)[:, None] * a[None, :]).astype(dt)

    def prior(self, x):
        dt = self.dtype
        s = dt(self.p[0])
        v = dt(-0.5) * np.sum(x * x, axis=1, dtype=dt) / (s * s)
        return v.astype(dt), (-x / (s * s)).astype(dt)


CLASSES = dict(base.CLASSES, ragged=Ragged)

# the faults a kernel of this kind can have and the forward-mode kernels cannot
TAPE_FAULTS = ("scaled_prior", "row_gradient_kept", "prior_gradient_dropped")


def evaluate_with_tape_fault(tgt, x, fault):
    """DataTarget.evaluate with one of TAPE_FAULTS: ``scaled_prior``: s applied to the prior as well; ``row_gradient_kept``: the
    gradient of the previous row added once more to the current one (what an adjoint left over from the previous row would
    do); ``prior_gradient_dropped``: the prior's value added, its gradient not."""
    assert fault in TAPE_FAULTS
    dt = tgt.dtype
    x = np.asarray(x, dt)
    lp, grad = np.zeros(x.shape[0], dt), np.zeros(x.shape, dt)
    previous = None
    for r in tgt.row_list():
        v, g = tgt.row_term(x, tgt.data[r].astype(dt))
        lp, grad = (lp + v).astype(dt), (grad + g).astype(dt)
        if fault == "row_gradient_kept" and previous is not None:
            grad = (grad + previous).astype(dt)
        previous = g
    s = tgt.scale()
    lp, grad = (s * lp).astype(dt), (s * grad).astype(dt)
    v, g = tgt.prior(x)
    if fault == "scaled_prior":
        v, g = s * v, s * g
    if fault == "prior_gradient_dropped":
        g = np.zeros_like(g)
    return (lp + v).astype(dt), (grad + g).astype(dt)


def evaluate_in_tape_order(tgt, x, plan):
    """evaluate() with the sums formed the way the kernels of custom_target_data_tape.inc form them for plan = (chunks,
    rows_per_chunk): one lane adds the rows of a chunk in position order, the chunks are added in index order, then s * sum, then
    + prior."""
    dt = tgt.dtype
    x = np.asarray(x, dt)
    rows = tgt.row_list()
    chunks, per = plan
    lp = grad = None
    for c in range(chunks):
        c_lp, c_grad = np.zeros(x.shape[0], dt), np.zeros(x.shape, dt)
        for r in rows[c * per:(c + 1) * per]:
            v, g = tgt.row_term(x, tgt.data[r].astype(dt))
            c_lp, c_grad = (c_lp + v).astype(dt), (c_grad + g).astype(dt)
        lp, grad = (c_lp, c_grad) if c == 0 else ((lp + c_lp).astype(dt), (grad + c_grad).astype(dt))
    s = tgt.scale()
    v, g = tgt.prior(x)
    return ((s * lp).astype(dt) + v).astype(dt), ((s * grad).astype(dt) + g).astype(dt)


# ---- the kernel cases --------------------------------------------------------------------------------------------------------------
OLD_CAP = 512               # the forward mode's cap, from both sides
DEFAULT_CAPACITY = 1024     # logit records 2 D + 5 per row: D = 4096 needs the second attempt

SLAB_CASE = Case("logit", 5, 130, 5, 0, None, 0)


def kernel_cases():
    """Each at the smallest shape that reaches its seam.  N: one lane, the 64-sample tile from both sides, more than two tiles.
    D: 1, 2, the forward mode's cap from both sides, 1100, and 4096, whose tape exceeds the default capacity.  rows: 1, 2, 3 (the
    tape is reused from the second row on); 67 rows cut into 2 and 3 chunks (a ragged last chunk); 257 rows on the automatic
    plan; a chunk request above the row count.  Minibatches: B = 1, 5 and T at T = 9, 257 and 1025, at two calls, and one above
    the old cap.  nodata: every row term a constant.  ragged: tapes of different lengths, in one chunk and in three."""
    full = ([Case("logit", 5, n, 5, 0, None, 0) for n in (1, 63, 64, 65, 130)]
            + [Case("logit", d, 65, 5, 0, None, 0) for d in (1, 2, OLD_CAP, OLD_CAP + 1, 1100, 4096)]
            + [Case("student", 3, 65, t, 0, None, 0) for t in (1, 2, 3)]
            + [Case(name, 17, 65, 67, k, None, 0) for name in ("logit", "student") for k in (2, 3)]
            + [Case("logit", 5, 65, 257, 0, None, 0)]
            + [Case("student", 3, 65, 3, 9, None, 0)]
            + [Case("nodata", 4, 65, 5, 0, None, 0), Case("nodata", 4, 65, 67, 3, None, 0)]
            + [Case("ragged", 6, 65, 13, k, None, 0) for k in (1, 3)])
    mini = [Case("logit" if t != 257 else "student", 5, 65, t, 0, b, call)
            for t in (9, 257, 1025) for b in (1, 5, t) for call in (0, 3)]
    mini += [Case("logit", OLD_CAP + 1, 65, 257, 2, 257, 3)]
    return full + mini


def build_case(c, seed=5):
    """custom_data_cases.build_case, and for ``ragged``: rows ~ N(0, 1 / D), responses of order one, repeat counts 0 .. 3 with
    every count present."""
    if c.name != "ragged":
        return base.build_case(c, seed)
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = rng.normal(size=(c.n, c.d)).astype(np.float32)
    repeats = (np.arange(c.rows) * 3 + 1) % 4
    data = np.concatenate([rng.normal(size=(c.rows, c.d)) / np.sqrt(c.d), rng.normal(size=(c.rows, 1)), repeats[:, None]], axis=1)
    return Ragged(data, [3.0], batch_size=c.batch, seed=base.MINIBATCH_SEED, call=c.call), x


_refs = {}


def reference(c):
    """-> (target, x, lp64, g64, lp32, g32), computed once per case and read-only."""
    if c not in _refs:
        tgt, x = build_case(c)
        lp64, g64 = tgt.evaluate(x.astype(np.float64))
        lp32, g32 = fp32_twin(tgt).evaluate(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[c] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[c]
