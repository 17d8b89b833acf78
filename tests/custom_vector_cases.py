"""The vector primitives of user-defined device targets (csrc/custom_target_vector.inc: gmmvi_dot, gmmvi_sqdist, gmmvi_sumsq, and
their overloads in the two number types): the probe wrappers, the fp64 and fp32 NumPy restatements of one primitive, the sources
of the test targets and their restatements.

The fp32 restatement of a primitive follows the order include/gmmvi_hip.h states: four partial sums, element i into partial
i mod 4 by one fused multiply-add (formed here in fp64 and rounded once to fp32: the product of two fp32 numbers is exact in
fp64), i ascending, then (s0 + s1) + (s2 + s3).

Targets: ``logit_vec`` is the logistic regression of tests/custom_data_cases.py (``logit``) with the row's inner product as one
gmmvi_dot and the normal prior as one gmmvi_sumsq; ``rbf_vec`` has the row term -0.5 |x - row|^2 / params[0] and no prior;
``logit_vec_density`` / ``rbf_vec_density`` are one fixed row of each as a plain density for the modes without a data set, the
row kept in params.  ``mixed`` takes gmmvi_dot for x[0] > 0 and the scalar loop otherwise; ``ranges`` calls the primitives on
overlapping sub-ranges; ``single`` is an unscaled gmmvi_dot and nothing else."""
import ctypes as C

import numpy as np

import custom_data_cases as base
from custom_data_cases import Case, case_id, fp32_twin  # noqa: F401  (re-exported for the two test files)
from gmmvi_amd import _lib

W = 16                       # GMMVI_CUSTOM_AUTODIFF_TANGENTS
EPS32 = float(np.finfo(np.float32).eps)
# A value may differ from the fp64 sum of its terms by VALUE_EPS * eps32 * sum |terms|.  Where it comes from: a partial sum of m
# terms by fused multiply-adds carries at most m roundings, the two-level merge two more, so the largest case here (n = 33:
# m = 9) is within 11 / 2 units of eps32 times sum |terms|; gmmvi_sqdist and gmmvi_sumsq round each difference first, which moves
# a term d^2 by at most 2 * (eps32 / 2) of itself: 13 / 2.  8 covers that and the second-order terms this count drops.
VALUE_EPS = 8.0


def _fptr(a):
    return a.ctypes.data_as(C.c_void_p)


def probe_forward(op, x, first, n, c, center, seed_first):
    """gmmvi_autodiff_probe_vector -> (value, tangents [W])."""
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    v, t = C.c_float(), np.zeros(W, np.float32)
    rc = _lib.load().gmmvi_autodiff_probe_vector(_lib.VECTOR_OPS.index(op), _fptr(x), x.size, first, n, _fptr(c), float(center),
                                                 seed_first, C.byref(v), _fptr(t))
    assert rc == 0, rc
    return np.float32(v.value), t


def probe_forward_gradient(op, x, first, n, c, center):
    """Every pass seed 0, 16, ...: -> (the values of the passes, the concatenated tangents cut to D)."""
    out = [probe_forward(op, x, first, n, c, center, s) for s in range(0, len(x), W)]
    return [v for v, _ in out], np.concatenate([t for _, t in out])[:len(x)]


def probe_tape(op, x, first, n, c, center):
    """gmmvi_tape_probe_vector -> (value, gradient [D], records)."""
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    v, records, g = C.c_float(), C.c_int(-1), np.full(x.size, np.nan, np.float32)
    rc = _lib.load().gmmvi_tape_probe_vector(_lib.VECTOR_OPS.index(op), _fptr(x), x.size, first, n, _fptr(c), float(center),
                                             C.byref(v), _fptr(g), C.byref(records))
    assert rc == 0, rc
    return np.float32(v.value), g, records.value


def terms64(op, x, first, n, c, center):
    """-> (terms [n], partials [n]) of the primitive in fp64 at the fp32 operands."""
    xs = np.asarray(x, np.float64)[first:first + max(n, 0)]
    cs = np.asarray(c, np.float64)[:max(n, 0)]
    if op == "dot":
        return cs * xs, cs.copy()
    d = xs - (cs if op == "sqdist" else np.float64(np.float32(center)))
    return d * d, 2.0 * d


def value32(op, x, first, n, c, center):
    """The fp32 restatement in the header's order."""
    f = np.float32
    xs = np.asarray(x, f)[first:first + max(n, 0)]
    cs = np.asarray(c, f)[:max(n, 0)]
    s = [f(0)] * 4
    for i in range(max(n, 0)):
        if op == "dot":
            a, b = cs[i], xs[i]
        else:
            a = b = f(xs[i] - (cs[i] if op == "sqdist" else f(center)))
        s[i % 4] = f(np.float64(a) * np.float64(b) + np.float64(s[i % 4]))
    return f(f(s[0] + s[1]) + f(s[2] + s[3]))


def primitive_cases():
    """(D, first, n): every D with the whole range, n = 0 at both ends, one element at both ends, and where D allows it an
    interior range; at D = 33 the interior range crosses both 16-boundaries, at D = 17 the one."""
    out = []
    for d in (1, 15, 16, 17, 33):
        out += [(d, 0, d), (d, 0, 0), (d, d, 0), (d, 0, 1), (d, d - 1, 1)]
        if d == 15:
            out += [(d, 3, 9)]
        if d == 16:
            out += [(d, 5, 11), (d, 1, 14)]
        if d == 17:
            out += [(d, 14, 3), (d, 3, 13), (d, 15, 2)]
        if d == 33:
            out += [(d, 14, 5), (d, 7, 20), (d, 13, 20), (d, 16, 16), (d, 15, 18)]
    return out


def primitive_operands(d, seed=3):
    rng = np.random.default_rng(seed + 17 * d)
    return rng.normal(size=d).astype(np.float32), rng.normal(size=d).astype(np.float32), np.float32(0.375)


# ---- the sources ---------------------------------------------------------------------------------------------------------------
LOGIT_VEC_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T z = gmmvi_dot(x, 0, row, D);
    z *= row[D];
    return -(fmax(-z, 0.f) + log1p(exp(-fabs(z))));        // log sigmoid(z)
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    return -0.5f * gmmvi_sumsq(x, 0, D, m) / (s * s) - D * (logf(s) + 0.9189385332046727f);
}
"""

# the loop row of ``logit`` with the prior of logit_vec: its tape length is the row's, 2 D + 9 (the loop prior's 4 D + 2 hides it)
LOGIT_LOOP_ROW_SRC = base.LOGIT_SRC[:base.LOGIT_SRC.index("template <class T, class X>\n__device__ T gmmvi_user_prior")] + \
    LOGIT_VEC_SRC[LOGIT_VEC_SRC.index("template <class T, class X>\n__device__ T gmmvi_user_prior"):]

RBF_VEC_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    return -0.5f * gmmvi_sqdist(x, 0, row, D) / params[0];
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) { return 0.f; }
"""

# params = [prior mean, prior std, label, features (D)] / [bandwidth, centre (D)]
LOGIT_VEC_DENSITY_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    T z = gmmvi_dot(x, 0, params + 3, D);
    z *= params[2];
    return -(fmax(-z, 0.f) + log1p(exp(-fabs(z)))) + (-0.5f / (s * s)) * gmmvi_sumsq(x, 0, D, m);
}
"""

RBF_VEC_DENSITY_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    return -0.5f * gmmvi_sqdist(x, 0, params + 1, D) / params[0];
}
"""

# the hand-written mode: the float primitives give the value, the gradient is coded by hand
LOGIT_VEC_HAND_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    const float m = params[0], s = params[1], scale = -0.5f / (s * s);
    const float z = gmmvi_dot(x, 0, params + 3, D) * params[2];
    const float e = expf(-fabsf(z));
    if (grad) {
        const float dz = ((z <= 0.f ? 1.f : 0.f) + (z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f)) * (e / (1.f + e))) * params[2];
        for (int i = 0; i < D; ++i) grad[i] = dz * params[3 + i] + scale * 2.f * (x[i] - m);
    }
    return -(fmaxf(-z, 0.f) + log1pf(e)) + scale * gmmvi_sumsq(x, 0, D, m);
}
"""

RBF_VEC_HAND_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    if (grad)
        for (int i = 0; i < D; ++i) grad[i] = -(x[i] - params[1 + i]) / params[0];
    return -0.5f * gmmvi_sqdist(x, 0, params + 1, D) / params[0];
}
"""

# gmmvi_dot for x[0] > 0, the scalar loop otherwise: two kinds of record at the same record index in one wave
MIXED_ROW = r"""
    T z = 0.f;
    if (x[0] > 0.f) {
        z = gmmvi_dot(x, 0, COEF, D);
    } else {
        for (int i = 0; i < D; ++i) z += COEF[i] * x[i];
    }
    return -0.5f * z * z + 0.25f * z;
"""
MIXED_SRC = ("template <class T, class X>\n__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {"
             + MIXED_ROW.replace("COEF", "row") + "}\n"
             "template <class T, class X>\n__device__ T gmmvi_user_prior(X x, int D, const float* params) {\n"
             "    return -0.125f * gmmvi_sumsq(x, 0, D, 0.f);\n}\n")
MIXED_DENSITY_SRC = ("template <class T, class X>\n__device__ T gmmvi_user_density(X x, int D, const float* params) {"
                     + MIXED_ROW.replace("COEF", "params") + "}\n")

# D = 40: two calls on overlapping ranges and a gmmvi_sumsq on [16, 32); params = [c (40)]
RANGES_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const T a = gmmvi_dot(x, 3, params, 20);
    const T b = gmmvi_sqdist(x, 10, params + 5, 30);
    const T q = gmmvi_sumsq(x, 16, 16, 0.5f);
    return a * 0.5f - 0.25f * b - 0.125f * q + 0.0625f * a * q;
}
"""
RANGES_D = 40

SINGLE_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) { return gmmvi_dot(x, 0, params, D); }
"""

# one source per mode that calls all three primitives
ALL_THREE_DENSITY = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    return gmmvi_dot(x, 0, params, D) - gmmvi_sqdist(x, 0, params, D) - 0.5f * gmmvi_sumsq(x, 0, D, params[0]);
}
"""
ALL_THREE_DATA = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    return gmmvi_dot(x, 0, row, D) - gmmvi_sqdist(x, 0, row, D);
}
template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) { return -0.5f * gmmvi_sumsq(x, 0, D, params[0]); }
"""
ALL_THREE_HAND = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    if (grad)
        for (int i = 0; i < D; ++i) grad[i] = params[i] - 2.f * (x[i] - params[i]) - (x[i] - params[0]);
    return gmmvi_dot(x, 0, params, D) - gmmvi_sqdist(x, 0, params, D) - 0.5f * gmmvi_sumsq(x, 0, D, params[0]);
}
"""
ALL_THREE = {"hand": ALL_THREE_HAND, "autodiff": ALL_THREE_DENSITY, "tape": ALL_THREE_DENSITY, "data": ALL_THREE_DATA,
             "data_tape": ALL_THREE_DATA}

SOURCES = {"logit_vec": LOGIT_VEC_SRC, "rbf_vec": RBF_VEC_SRC, "mixed": MIXED_SRC, "logit_loop_row": LOGIT_LOOP_ROW_SRC}
DENSITY_SOURCES = {"logit_vec": LOGIT_VEC_DENSITY_SRC, "rbf_vec": RBF_VEC_DENSITY_SRC, "mixed": MIXED_DENSITY_SRC,
                   "ranges": RANGES_SRC, "single": SINGLE_SRC}
HAND_SOURCES = {"logit_vec": LOGIT_VEC_HAND_SRC, "rbf_vec": RBF_VEC_HAND_SRC}


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def _logistic(z, dt):
    """log sigmoid(z) and the derivative the number types form (custom_data_cases.Logit.row_term)."""
    e = np.exp(-np.abs(z))
    v = -(np.maximum(-z, dt(0)) + np.log1p(e))
    return v.astype(dt), ((z <= 0).astype(dt) + np.sign(z) * (e / (dt(1) + e))).astype(dt)


class LogitVec(base.Logit):
    """``logit`` with the prior of LOGIT_VEC_SRC: -0.5 sum (x - m)^2 / s^2 - D (log s + log sqrt(2 pi)), in that order.  The text
    ends in a difference, as the loop prior of ``logit`` does: the library adds the prior to a product (s * sum), and a prior that
    ends in a product of its own would leave the compiler two multiply-adds to choose from, one choice per instantiation."""

    def prior(self, x):
        dt = self.dtype
        m, s = dt(self.p[0]), dt(self.p[1])
        r = (x - m).astype(dt)
        q = ((dt(-0.5) * np.sum(r * r, axis=1, dtype=dt)).astype(dt) / (s * s)).astype(dt)
        v = q - dt(x.shape[1]) * (np.log(s) + dt(base.HALF_LOG_2PI))
        return v.astype(dt), ((dt(-0.5) * (dt(2) * r)).astype(dt) / (s * s)).astype(dt)


class RbfVec(base.DataTarget):
    def row_term(self, x, row):
        dt = self.dtype
        h = dt(self.p[0])
        r = (x - row[None, :self.d]).astype(dt)
        return (dt(-0.5) * np.sum(r * r, axis=1, dtype=dt) / h).astype(dt), (-r / h).astype(dt)

    def prior(self, x):
        return np.zeros(x.shape[0], self.dtype), np.zeros(x.shape, self.dtype)


class Mixed(base.DataTarget):
    """Both branches of MIXED_SRC compute the same function: z = row . x, -0.5 z^2 + 0.25 z; prior -0.125 |x|^2."""

    def row_term(self, x, row):
        dt = self.dtype
        a = row[:self.d]
        z = (x @ a).astype(dt)
        return (dt(-0.5) * z * z + dt(0.25) * z).astype(dt), ((dt(0.25) - z)[:, None] * a[None, :]).astype(dt)

    def prior(self, x):
        dt = self.dtype
        return (dt(-0.125) * np.sum(x * x, axis=1, dtype=dt)).astype(dt), (dt(-0.25) * x).astype(dt)


CLASSES = {"logit_vec": LogitVec, "rbf_vec": RbfVec, "mixed": Mixed, "logit": base.Logit, "logit_loop_row": LogitVec}


class Density:
    """A plain density with params [P] -> log_density_and_grad(x) -> (lp [N], grad [N, D]) in ``dtype``."""

    def __init__(self, name, params, dtype=np.float64):
        self.name, self.p, self.dtype = name, np.asarray(params, np.float32), dtype

    def as_dtype(self, dtype):
        return Density(self.name, self.p, dtype)

    def params(self):
        return self.p.copy()

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        p = self.p.astype(dt)
        d = x.shape[1]
        if self.name == "logit_vec":
            m, s, y, a = p[0], p[1], p[2], p[3:3 + d]
            z = ((x @ a).astype(dt) * y).astype(dt)
            v, dz = _logistic(z, dt)
            k = dt(-0.5) / (s * s)
            r = (x - m).astype(dt)
            return ((v + k * np.sum(r * r, axis=1, dtype=dt)).astype(dt),
                    ((dz * y)[:, None] * a[None, :] + k * dt(2) * r).astype(dt))
        if self.name == "rbf_vec":
            r = (x - p[None, 1:1 + d]).astype(dt)
            return (dt(-0.5) * np.sum(r * r, axis=1, dtype=dt) / p[0]).astype(dt), (-r / p[0]).astype(dt)
        if self.name == "mixed":
            a = p[:d]
            z = (x @ a).astype(dt)
            return (dt(-0.5) * z * z + dt(0.25) * z).astype(dt), ((dt(0.25) - z)[:, None] * a[None, :]).astype(dt)
        if self.name == "single":
            a = p[:d]
            return (x @ a).astype(dt), np.broadcast_to(a, x.shape).astype(dt)
        assert self.name == "ranges" and d == RANGES_D
        a = (x[:, 3:23] @ p[:20]).astype(dt)
        rb = (x[:, 10:40] - p[None, 5:35]).astype(dt)
        rq = (x[:, 16:32] - dt(0.5)).astype(dt)
        b, q = np.sum(rb * rb, axis=1, dtype=dt), np.sum(rq * rq, axis=1, dtype=dt)
        v = a * dt(0.5) - dt(0.25) * b - dt(0.125) * q + dt(0.0625) * a * q
        g = np.zeros(x.shape, dt)
        g[:, 3:23] += (dt(0.5) + dt(0.0625) * q)[:, None] * p[None, :20]
        g[:, 10:40] += dt(-0.25) * dt(2) * rb
        g[:, 16:32] += (dt(-0.125) + dt(0.0625) * a)[:, None] * dt(2) * rq
        return v.astype(dt), g.astype(dt)


def build_data_case(c, seed=5):
    """-> (fp64 target, x [n, d] fp32) for a Case of ``logit_vec``, ``logit`` (the same rows and x as logit_vec), ``rbf_vec`` or
    ``mixed``; rows ~ N(0, 1 / D) as in custom_data_cases.build_case.  ``mixed``: x[:, 0] has both signs within every 64 lanes."""
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = rng.normal(size=(c.n, c.d)).astype(np.float32)
    kw = dict(batch_size=c.batch, seed=base.MINIBATCH_SEED, call=c.call)
    feats = rng.normal(size=(c.rows, c.d)) / np.sqrt(c.d)
    if c.name in ("logit_vec", "logit", "logit_loop_row"):
        data = np.concatenate([feats, rng.choice([-1.0, 1.0], size=(c.rows, 1))], axis=1)
        return CLASSES[c.name](data, [0.25, 2.0], **kw), x
    if c.name == "rbf_vec":
        return RbfVec(feats * np.sqrt(c.d), [1.5], d=c.d, **kw), x
    assert c.name == "mixed"
    x[:, 0] = np.where(np.arange(c.n) % 3 == 0, -1.0, 1.0) * (np.abs(x[:, 0]) + 0.125)
    return Mixed(feats, [0.0], d=c.d, **kw), x


def build_density_case(name, d, n, seed=7):
    rng = np.random.default_rng(seed + 1000 * d + 7 * n)
    x = rng.normal(size=(n, d)).astype(np.float32)
    a = rng.normal(size=d) / np.sqrt(d)
    if name == "logit_vec":
        return Density(name, np.concatenate([[0.25, 2.0, -1.0], a])), x
    if name == "rbf_vec":
        return Density(name, np.concatenate([[1.5], a * np.sqrt(d)])), x
    if name == "mixed":
        x[:, 0] = np.where(np.arange(n) % 3 == 0, -1.0, 1.0) * (np.abs(x[:, 0]) + 0.125)
    return Density(name, a), x


_refs = {}


def reference(c):
    """A data Case, or (name, d, n) of a plain density -> (target, x, lp64, g64, lp32, g32), computed once, read-only."""
    if c not in _refs:
        if isinstance(c, Case):
            tgt, x = build_data_case(c)
            lp64, g64 = tgt.evaluate(x.astype(np.float64))
            lp32, g32 = fp32_twin(tgt).evaluate(x)
        else:
            tgt, x = build_density_case(*c)
            lp64, g64 = tgt.log_density_and_grad(x.astype(np.float64))
            lp32, g32 = tgt.as_dtype(np.float32).log_density_and_grad(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[c] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[c]
