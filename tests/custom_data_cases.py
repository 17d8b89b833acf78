"""User-defined device targets summed over a data set (csrc/custom_target_data.inc, DeviceDataLNPDF): the sources of the test
targets, each one row's term and the prior as value-only templates, the NumPy restatements they are checked against, and the
kernel cases.

A restatement is  lp(x) = prior(x) + s * sum over the row list of row(x, data[r])  in its dtype.  float64 is the reference;
``fp32_twin`` is the same operations rounded to fp32 after each step, with the row sum accumulated sequentially in row-list
order, s applied once to the finished sum and the prior added last (the order include/gmmvi_hip.h states).  The row list is all
rows in index order, or ``minibatch_stream.data_minibatch_rows(seed, call, B, T)``.

A restatement can also be evaluated with one planted fault (``FAULTS``): tests/test_custom_data_host.py shows that each of them
moves the result by far more than the bound the GPU test uses, so that bound can tell a kernel with such a mistake from a
correct one."""
from collections import namedtuple

import numpy as np

from gmmvi_amd.experiments.target_distributions.minibatch_stream import data_minibatch_rows

HALF_LOG_2PI = 0.9189385332046727

# ---- logit: rows [features (D) | label +-1], params = [prior mean, prior std] -------------------------------------------------
LOGIT_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T z = 0.f;
    for (int i = 0; i < D; ++i) z += row[i] * x[i];
    z *= row[D];
    return -(fmax(-z, 0.f) + log1p(exp(-fabs(z))));        // log sigmoid(z)
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    T q = 0.f;
    for (int i = 0; i < D; ++i) {
        const T r = (x[i] - m) / s;
        q += r * r;
    }
    return -0.5f * q - D * (logf(s) + 0.9189385332046727f);
}
"""

# ---- student: robust regression, rows [features (D) | response], params = [nu, prior std] -------------------------------------
STUDENT_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    const float nu = params[0];
    T r = row[D];
    for (int i = 0; i < D; ++i) r -= row[i] * x[i];
    return -0.5f * (nu + 1.f) * log1p(r * r / nu);
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float s = params[1];
    T q = 0.f;
    for (int i = 0; i < D; ++i) q += x[i] * x[i];
    return -0.5f * q / (s * s);
}
"""

# ---- nodata: the row term ignores x (its tangents are zero), rows [c0 | c1], params = [scale] ----------------------------------
NODATA_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    return params[0] * row[0] + row[1];
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    T q = 0.f;
    for (int i = 0; i < D; ++i) q += x[i] * x[i];
    return -0.5f * q;
}
"""

SOURCES = {"logit": LOGIT_SRC, "student": STUDENT_SRC, "nodata": NODATA_SRC}

FAULTS = ("drop_last_row", "drop_first_row_of_wave_1", "drop_first_row_of_last_chunk", "unit_scale", "next_call", "no_prior")


class DataTarget:
    """Base of the restatements: ``data`` [T, C] and ``params`` hold fp32 numbers (what the device sees), the arithmetic runs
    in ``dtype``.  batch_size None: full data.  With a batch size the object follows the call counter of MinibatchLNPDF:
    ``call_count`` advances after every evaluation that receives at least one sample."""

    def __init__(self, data, params, dtype=np.float64, batch_size=None, seed=0, call=0, d=None):
        self.data = np.asarray(data, np.float32)
        self.d = self.data.shape[1] - 1 if d is None else int(d)
        self.p = np.asarray(params, np.float32)
        self.dtype = dtype
        self.batch_size = None if batch_size is None else int(batch_size)
        self.seed, self.call_count = int(seed), int(call)

    def as_dtype(self, dtype):
        return type(self)(self.data, self.p, dtype, self.batch_size, self.seed, self.call_count, self.d)

    def full(self):
        """The full-data target of the same rows (no stream, no counter)."""
        return type(self)(self.data, self.p, self.dtype, d=self.d)

    def params(self):
        return self.p.copy()

    def get_num_dimensions(self):
        return self.d

    @property
    def num_data(self):
        return self.data.shape[0]

    def row_list(self, call=None):
        if self.batch_size is None:
            return np.arange(self.num_data)
        return data_minibatch_rows(self.seed, self.call_count if call is None else call, self.batch_size, self.num_data)

    def scale(self):
        if self.batch_size is None:
            return self.dtype(1)
        return self.dtype(np.float32(self.num_data) / np.float32(self.batch_size))       # the device's (float)T / (float)B

    # one row's term and the prior: -> (value [N], gradient [N, D]) in self.dtype
    def row_term(self, x, row):
        raise NotImplementedError

    def prior(self, x):
        raise NotImplementedError

    def evaluate(self, x, fault=None, plan=None):
        """-> (lp [N], grad [N, D]) at the current call, counter untouched.  fault: None or one of FAULTS; plan: (chunks,
        rows_per_chunk) of the launch, which the chunk fault needs."""
        dt = self.dtype
        x = np.asarray(x, dt)
        rows = list(self.row_list(self.call_count + 1 if fault == "next_call" else None))
        if fault == "drop_last_row":
            del rows[-1]
        elif fault == "drop_first_row_of_wave_1":
            del rows[1]
        elif fault == "drop_first_row_of_last_chunk":
            del rows[(plan[0] - 1) * plan[1]]
        lp = np.zeros(x.shape[0], dt)
        grad = np.zeros(x.shape, dt)
        for r in rows:                                   # sequentially, in row-list order
            v, g = self.row_term(x, self.data[r].astype(dt))
            lp = (lp + v).astype(dt)
            grad = (grad + g).astype(dt)
        s = dt(1) if fault == "unit_scale" else self.scale()
        lp, grad = (s * lp).astype(dt), (s * grad).astype(dt)
        if fault != "no_prior":
            v, g = self.prior(x)
            lp, grad = (lp + v).astype(dt), (grad + g).astype(dt)
        return lp, grad

    def evaluate_in_device_order(self, x, plan):
        """evaluate() with the row sum formed the way the kernels form it for plan = (chunks, rows_per_chunk): wave w of a chunk
        adds the chunk's positions w, w + 4, ... in order, wave 0 adds waves 1, 2, 3, the chunks are added in index order."""
        dt = self.dtype
        x = np.asarray(x, dt)
        rows = self.row_list()
        chunks, per = plan
        lp, grad = np.zeros(x.shape[0], dt), np.zeros(x.shape, dt)
        for c in range(chunks):
            part = rows[c * per:(c + 1) * per]
            c_lp, c_grad = None, None
            for w in range(4):
                w_lp, w_grad = np.zeros(x.shape[0], dt), np.zeros(x.shape, dt)
                for r in part[w::4]:
                    v, g = self.row_term(x, self.data[r].astype(dt))
                    w_lp, w_grad = (w_lp + v).astype(dt), (w_grad + g).astype(dt)
                c_lp, c_grad = (w_lp, w_grad) if w == 0 else ((c_lp + w_lp).astype(dt), (c_grad + w_grad).astype(dt))
            lp, grad = (c_lp, c_grad) if chunks == 1 else ((lp + c_lp).astype(dt), (grad + c_grad).astype(dt))
        s = self.scale()
        v, g = self.prior(x)
        return (s * lp + v).astype(dt), (s * grad + g).astype(dt)

    def _advance(self, x):
        if self.batch_size is not None and np.shape(x)[0] >= 1:
            self.call_count += 1

    def log_density_and_grad(self, x):
        out = self.evaluate(x)
        self._advance(x)
        return out

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


class Logit(DataTarget):
    def row_term(self, x, row):
        dt = self.dtype
        a, y = row[:-1], row[-1]
        z = ((x @ a).astype(dt) * y).astype(dt)
        e = np.exp(-np.abs(z))
        v = -(np.maximum(-z, dt(0)) + np.log1p(e))
        # the derivative the dual numbers form: fmax takes its first operand's tangent unless the second strictly wins, fabs has
        # tangent 0 at 0; d/dz = [z <= 0] + sign(z) e / (1 + e) = sigmoid(-z) away from z = 0
        dz = (z <= 0).astype(dt) + np.sign(z) * (e / (dt(1) + e))
        return v.astype(dt), ((dz * y)[:, None] * a[None, :]).astype(dt)

    def prior(self, x):
        dt = self.dtype
        m, s = dt(self.p[0]), dt(self.p[1])
        r = (x - m) / s
        d = x.shape[1]
        v = dt(-0.5) * np.sum(r * r, axis=1, dtype=dt) - dt(d) * (np.log(s) + dt(HALF_LOG_2PI))
        return v.astype(dt), (-r / s).astype(dt)


class Student(DataTarget):
    def row_term(self, x, row):
        dt = self.dtype
        nu = dt(self.p[0])
        a, t = row[:-1], row[-1]
        r = (t - (x @ a).astype(dt)).astype(dt)
        u = r * r / nu
        v = dt(-0.5) * (nu + dt(1)) * np.log1p(u)
        dr = -(nu + dt(1)) * r / (nu * (dt(1) + u))
        return v.astype(dt), ((-dr)[:, None] * a[None, :]).astype(dt)

    def prior(self, x):
        dt = self.dtype
        s = dt(self.p[1])
        v = dt(-0.5) * np.sum(x * x, axis=1, dtype=dt) / (s * s)
        return v.astype(dt), (-x / (s * s)).astype(dt)


class NoData(DataTarget):
    def row_term(self, x, row):
        dt = self.dtype
        v = dt(self.p[0]) * row[0] + row[1]
        return np.full(x.shape[0], v, dt), np.zeros(x.shape, dt)

    def prior(self, x):
        dt = self.dtype
        return (dt(-0.5) * np.sum(x * x, axis=1, dtype=dt)).astype(dt), (-x).astype(dt)


CLASSES = {"logit": Logit, "student": Student, "nodata": NoData}


def fp32_twin(tgt):
    return tgt.as_dtype(np.float32)


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------
# rows: T; chunks: the request (0 auto); batch: None (full data) or B; call: the call of a minibatch case
Case = namedtuple("Case", "name d n rows chunks batch call")
MINIBATCH_SEED = 9


def case_id(c):
    tail = "" if c.batch is None else f"-B{c.batch}-call{c.call}"
    return f"{c.name}-D{c.d}-N{c.n}-T{c.rows}-chunks{c.chunks}{tail}"


def kernel_cases(w, staged_cap=120):
    """The smallest shapes at which the kernels can go wrong; ``w`` the tangents per pass, ``staged_cap`` the largest staged D.
    N: one lane, the 64-sample tile from both sides, more than two tiles.  D: the pass width from both sides, two passes and a
    partial one, the staged route's cap from both sides.  rows: fewer rows than waves, one each, one wave with two; 67 rows cut
    into 2 and 3 chunks (a ragged last chunk); 257 rows on the automatic plan; a chunk request above the row count.  Minibatches:
    B = 1, 5 and T at T = 9, 257 and 1025 (Feistel domains 16, 1024 and 4096: cycle walking on both sides of a power of four),
    at two calls."""
    full = ([Case("logit", 5, n, 5, 0, None, 0) for n in (1, 63, 64, 65, 130)]
            + [Case("logit", d, 65, 5, 0, None, 0) for d in (w - 1, w, w + 1, 2 * w + 1, staged_cap, staged_cap + 1)]
            + [Case("student", 3, 65, t, 0, None, 0) for t in (1, 3, 4, 5)]
            + [Case(name, w + 1, 65, 67, k, None, 0) for name in ("logit", "student") for k in (2, 3)]
            + [Case("logit", 5, 65, 257, 0, None, 0), Case("student", 3, 130, 257, 0, None, 0)]
            + [Case("student", 3, 65, 3, 9, None, 0)]
            + [Case("nodata", 4, 65, 5, 0, None, 0), Case("nodata", 4, 65, 67, 3, None, 0)])
    mini = [Case("logit" if t != 257 else "student", 5, 65, t, 0, b, call)
            for t in (9, 257, 1025) for b in (1, 5, t) for call in (0, 3)]
    mini += [Case("logit", staged_cap + 1, 65, 257, 2, 257, 3), Case("nodata", 4, 65, 257, 0, 5, 3)]
    return full + mini


def build_case(c, seed=5):
    """-> (fp64 target, x [n, d] fp32): rows ~ N(0, 1 / D) (so that a row's inner product with x ~ N(0, 1) is of order one),
    labels +-1 / responses of order one."""
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = rng.normal(size=(c.n, c.d)).astype(np.float32)
    kw = dict(batch_size=c.batch, seed=MINIBATCH_SEED, call=c.call)
    if c.name == "logit":
        data = np.concatenate([rng.normal(size=(c.rows, c.d)) / np.sqrt(c.d), rng.choice([-1.0, 1.0], size=(c.rows, 1))], axis=1)
        return Logit(data, [0.25, 2.0], **kw), x
    if c.name == "student":
        data = np.concatenate([rng.normal(size=(c.rows, c.d)) / np.sqrt(c.d), rng.normal(size=(c.rows, 1))], axis=1)
        return Student(data, [4.0, 3.0], **kw), x
    data = rng.normal(size=(c.rows, 2)) + np.array([2.0, 0.0])
    return NoData(data, [1.5], d=c.d, **kw), x


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
