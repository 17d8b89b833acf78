"""The primitives of user-defined device targets on arrays of the mode's number type (csrc/custom_target_vector.inc: gmmvi_wdot,
gmmvi_logsumexp, and their overloads in the two number types): the probe wrappers, the fp64 and fp32 NumPy restatements of one
primitive with the bounds that follow from the order include/gmmvi_hip.h states, the sources of the test targets and their
restatements.

The probes build the array themselves: h[i] = tanh(x[src + i]), i < n, every ``every``-th entry a constant.  ``entries`` reads the
fp32 entries back through the probe (gmmvi_logsumexp of one entry is the entry itself), so that the restatements work on the
operands the primitive saw, whatever the host's tanhf rounds to.
``probe_inputs`` calls the second pair of probes, whose array is x[src .. src + n) itself: the gradient of gmmvi_logsumexp is then
its partials and nothing else, and x may hold -inf.

Targets.  x holds blocks [weights | bias]; a row is [features (F) | label], C = F + 1.
``softmax_vec``: K = D / C classes, z[k] = gmmvi_dot(x, k C, row, F) + x[k C + F], the row term z[label] - gmmvi_logsumexp(z, K).
``mlp_vec``: H = params[2] hidden units h[j] = tanh(gmmvi_dot(x, j C, row, F) + x[j C + F]), then K = (D - H C) / (H + 1) classes
z[k] = gmmvi_wdot(x, off + k (H + 1), h, H) + x[off + k (H + 1) + H] with off = H C, and the same row term.
Both have the prior of logit_vec (tests/custom_vector_cases.py): one gmmvi_sumsq, ending in a difference.
``softmax_loop`` / ``mlp_loop``: the same functions with scalar loops and a chain of gmmvi_logaddexp.
The density forms keep one fixed row in params = [prior mean, prior std, H, C, row (C)].
``mixed_nodes`` takes both primitives for x[0] > 0 and the loops otherwise; ``single_wdot`` / ``single_lse`` are one call and
nothing else."""
import ctypes as C
import math

import numpy as np

import custom_vector_cases as vec
from custom_data_cases import Case, case_id, fp32_twin  # noqa: F401  (re-exported for the two test files)
from gmmvi_amd import _lib

W = vec.W
EPS32 = vec.EPS32
MAX_N = 64                                                           # the probes' largest array

# gmmvi_wdot has the order of gmmvi_dot: the bound of tests/custom_vector_cases.py holds as it is derived there.
WDOT_VALUE_EPS = vec.VALUE_EPS


def logsumexp_value_bound(n, want):
    """|value - fp64 value at the fp32 operands| for entries in [-1, 1], in absolute terms.  value = m + logf(s), s the sum of
    expf(a[i] - m) in four partial sums.  a[i] - m is one rounding of a number of magnitude <= 2: an absolute eps32, which moves
    the exponential by a relative eps32; expf is within 1 ulp (ROCm's and glibc's documented accuracy), another relative eps32;
    a partial sum of ceil(n / 4) positive terms and the two-level merge round at most ceil(n / 4) + 2 times, eps32 / 2 each.  A
    relative error r of s is an absolute r of log s.  logf is within 1 ulp of a number of magnitude log n at most; the final add
    rounds once, eps32 / 2 of |value|."""
    if n <= 0:
        return 0.0
    return EPS32 * (2.0 + (math.ceil(n / 4) + 2) / 2.0 + math.log(n) + 0.5 * abs(want))


def gradient_eps(op, n):
    """The multiple of eps32 * sum over the paths of |contribution| a gradient entry may be off by.  The tanh partial
    4 e / ((1 + e) (1 + e)), e = expf(-2 |a|): 1 for expf, 1 for 1 + e (e / (1 + e) <= 1 / 2 of e's error and one rounding),
    doubled by the square with half a rounding more, half for the division: 4.  gmmvi_wdot: the entry's partial x[first + i] and
    the input's h[i] are exact; two products and the add of two paths: 1.5.  gmmvi_logsumexp: p_i = expf(a[i] - m) / s carries
    2 for its numerator, 2 + (ceil(n / 4) + 2) / 2 for s (logsumexp_value_bound) and half for the division."""
    if op == "wdot":
        return 4.0 + 1.5
    return 4.0 + 1.5 + 4.5 + (math.ceil(n / 4) + 2) / 2.0


def _fptr(a):
    return a.ctypes.data_as(C.c_void_p)


def probe_forward(op, x, first, n, src, every, seed_first):
    """gmmvi_autodiff_probe_nodes -> (value, tangents [W])."""
    x = np.ascontiguousarray(x, np.float32)
    v, t = C.c_float(), np.zeros(W, np.float32)
    rc = _lib.load().gmmvi_autodiff_probe_nodes(_lib.NODE_OPS.index(op), _fptr(x), x.size, first, n, src, every, seed_first,
                                                C.byref(v), _fptr(t))
    assert rc == 0, rc
    return np.float32(v.value), t


def probe_forward_gradient(op, x, first, n, src, every):
    """Every pass seed 0, 16, ...: -> (the values of the passes, the concatenated tangents cut to D)."""
    out = [probe_forward(op, x, first, n, src, every, s) for s in range(0, len(x), W)]
    return [v for v, _ in out], np.concatenate([t for _, t in out])[:len(x)]


def probe_tape(op, x, first, n, src, every):
    """gmmvi_tape_probe_nodes -> (value, gradient [D], records)."""
    x = np.ascontiguousarray(x, np.float32)
    v, records, g = C.c_float(), C.c_int(-1), np.full(x.size, np.nan, np.float32)
    rc = _lib.load().gmmvi_tape_probe_nodes(_lib.NODE_OPS.index(op), _fptr(x), x.size, first, n, src, every, C.byref(v), _fptr(g),
                                            C.byref(records))
    assert rc == 0, rc
    return np.float32(v.value), g, records.value


def probe_inputs(op, x, first, n, src):
    """gmmvi_autodiff_probe_nodes_inputs at every pass seed and gmmvi_tape_probe_nodes_inputs: the array is x[src .. src + n)
    itself -> (values of the passes, tangents cut to D, tape value, tape gradient [D], records)."""
    x = np.ascontiguousarray(x, np.float32)
    lib, op_i = _lib.load(), _lib.NODE_OPS.index(op)
    values, tangents = [], []
    for seed in range(0, x.size, W):
        v, t = C.c_float(), np.zeros(W, np.float32)
        assert lib.gmmvi_autodiff_probe_nodes_inputs(op_i, _fptr(x), x.size, first, n, src, seed, C.byref(v), _fptr(t)) == 0
        values.append(np.float32(v.value))
        tangents.append(t)
    v, records, g = C.c_float(), C.c_int(-1), np.full(x.size, np.nan, np.float32)
    assert lib.gmmvi_tape_probe_nodes_inputs(op_i, _fptr(x), x.size, first, n, src, C.byref(v), _fptr(g), C.byref(records)) == 0
    return values, np.concatenate(tangents)[:x.size], np.float32(v.value), g, records.value


def entries(x, src, n):
    """The fp32 entries h[i] = tanhf(x[src + i]) as the probes form them."""
    return np.array([probe_tape("logsumexp", x, 0, 1, src + i, 0)[0] for i in range(n)], np.float32)


def constants(n, every):
    return np.array([every > 0 and i % every == every - 1 for i in range(n)], bool)


def reference64(op, x, first, n, src, every, h):
    """-> (value, sum |terms| of gmmvi_wdot or 0, gradient [D], sum over the paths of |contribution| [D], p [n]) in fp64 at the
    fp32 operands x and h."""
    x64, h64 = np.asarray(x, np.float64), np.asarray(h, np.float64)
    dh = np.where(constants(n, every), 0.0, 1.0 - np.tanh(x64[src:src + n]) ** 2)
    g, scale = np.zeros(x64.size), np.zeros(x64.size)
    if op == "wdot":
        xs = x64[first:first + n]
        g[first:first + n] += h64
        scale[first:first + n] += np.abs(h64)
        g[src:src + n] += xs * dh
        scale[src:src + n] += np.abs(xs * dh)
        return float(h64 @ xs), float(np.abs(h64 * xs).sum()), g, scale, None
    if n == 0:
        return -np.inf, 0.0, g, scale, np.zeros(0)
    m = h64.max()
    s = np.exp(h64 - m).sum()
    p = np.exp(h64 - m) / s
    g[src:src + n] += p * dh
    scale[src:src + n] += np.abs(p * dh)
    return float(m + np.log(s)), 0.0, g, scale, p


def value32(op, x, first, n, h):
    """The fp32 restatement in the header's order.  expf and logf are the fp64 functions rounded once: within 1 ulp."""
    f = np.float32
    h = np.asarray(h, f)
    if op == "wdot":
        return vec.value32("dot", x, first, n, h, 0.0)
    m = f(-np.inf)
    for i in range(n):
        m = np.fmax(m, h[i])
    if m == f(-np.inf):
        return m
    s = [f(0)] * 4
    for i in range(n):
        s[i % 4] = f(s[i % 4] + f(np.exp(np.float64(f(h[i] - m)))))
    total = f(f(s[0] + s[1]) + f(s[2] + s[3]))
    return f(m + f(np.log(np.float64(total))))


def probe_cases():
    """(n, first, src, every, overlapping): D = n + 16.  The array from x[0 .. n) with the inputs from first = 16, and the other
    way round with first = 0: disjoint ranges up to n = 16 (D = n + 16 has no room for two disjoint ranges of 17 or 33, where
    these two cases overlap in part); a first range that crosses a 16-boundary (first = 9); src = first, and src = first + 1 for
    n >= 2.  ``overlapping``: the two ranges share an input, which then reaches a gmmvi_wdot along two paths (gmmvi_logsumexp
    does not read x[first ..), so every input has one path there)."""
    out = []
    for n in (1, 2, 3, 15, 16, 17, 33):
        d = n + 16
        for every in (0, 2, 1):
            for first, src in ((16, 0), (0, d - n), (9, 0), (5, 5)) + (((7, 8),) if n >= 2 else ()):
                out.append((n, first, src, every, first < src + n and src < first + n))
    return out


def probe_operands(n, seed=11):
    return np.random.default_rng(seed + 29 * n).normal(size=n + 16).astype(np.float32)


# ---- the sources ---------------------------------------------------------------------------------------------------------------
PRIOR_BODY = r"""
template <class T, class X>
__device__ T nodes_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    return -0.5f * gmmvi_sumsq(x, 0, D, m) / (s * s) - D * (logf(s) + 0.9189385332046727f);
}
"""

SOFTMAX_VEC_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, K = D / C;
    T z[16];
    for (int k = 0; k < K; ++k) z[k] = gmmvi_dot(x, k * C, row, F) + x[k * C + F];
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}
"""

SOFTMAX_LOOP_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, K = D / C;
    T z[16];
    for (int k = 0; k < K; ++k) {
        T a = x[k * C + F];
        for (int i = 0; i < F; ++i) a += row[i] * x[k * C + i];
        z[k] = a;
    }
    T l = z[0];
    for (int k = 1; k < K; ++k) l = gmmvi_logaddexp(l, z[k]);
    return z[(int)row[F]] - l;
}
"""

MLP_VEC_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H = (int)params[2], off = H * C, K = (D - off) / (H + 1);
    T h[32], z[16];
    for (int j = 0; j < H; ++j) h[j] = tanh(gmmvi_dot(x, j * C, row, F) + x[j * C + F]);
    for (int k = 0; k < K; ++k) z[k] = gmmvi_wdot(x, off + k * (H + 1), h, H) + x[off + k * (H + 1) + H];
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}
"""

MLP_LOOP_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H = (int)params[2], off = H * C, K = (D - off) / (H + 1);
    T h[32], z[16];
    for (int j = 0; j < H; ++j) {
        T a = x[j * C + F];
        for (int i = 0; i < F; ++i) a += row[i] * x[j * C + i];
        h[j] = tanh(a);
    }
    for (int k = 0; k < K; ++k) {
        T a = x[off + k * (H + 1) + H];
        for (int j = 0; j < H; ++j) a += h[j] * x[off + k * (H + 1) + j];
        z[k] = a;
    }
    T l = z[0];
    for (int k = 1; k < K; ++k) l = gmmvi_logaddexp(l, z[k]);
    return z[(int)row[F]] - l;
}
"""

# h[j] = tanh(x[j]), j < 8; a = sum h[j] x[8 + j]; l = logsumexp(h); SCALE (a - l).  D >= 16.
MIXED_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    T h[8];
    for (int j = 0; j < 8; ++j) h[j] = tanh(x[j]);
    T a = 0.f, l = h[0];
    if (x[0] > 0.f) {
        a = gmmvi_wdot(x, 8, h, 8);
        l = gmmvi_logsumexp(h, 8);
    } else {
        for (int j = 0; j < 8; ++j) a += h[j] * x[8 + j];
        for (int j = 1; j < 8; ++j) l = gmmvi_logaddexp(l, h[j]);
    }
    return row[0] * (a - l);
}
"""

DATA_TAIL = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) { return nodes_row<T, X>(x, D, row, C, params); }
template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) { return nodes_prior<T, X>(x, D, params); }
"""

# params = [prior mean, prior std, H, C, row (C)]
DENSITY_TAIL = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    return nodes_row<T, X>(x, D, params + 4, (int)params[3], params) + nodes_prior<T, X>(x, D, params);
}
"""

SOURCES = {name: body + PRIOR_BODY + DATA_TAIL for name, body in
           (("softmax_vec", SOFTMAX_VEC_BODY), ("softmax_loop", SOFTMAX_LOOP_BODY), ("mlp_vec", MLP_VEC_BODY),
            ("mlp_loop", MLP_LOOP_BODY), ("mixed_nodes", MIXED_BODY))}
DENSITY_SOURCES = {name: body + PRIOR_BODY + DENSITY_TAIL for name, body in
                   (("softmax_vec", SOFTMAX_VEC_BODY), ("softmax_loop", SOFTMAX_LOOP_BODY), ("mlp_vec", MLP_VEC_BODY),
                    ("mlp_loop", MLP_LOOP_BODY), ("mixed_nodes", MIXED_BODY))}

# the hand-written mode: the float primitives give the value, the gradient is coded by hand (D = K C)
SOFTMAX_VEC_HAND_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    const float m = params[0], s = params[1];
    const int C = (int)params[3], F = C - 1, K = D / C;
    const float* row = params + 4;
    const int label = (int)row[F];
    float z[16];
    for (int k = 0; k < K; ++k) z[k] = gmmvi_dot(x, k * C, row, F) + x[k * C + F];
    const float l = gmmvi_logsumexp(z, K);
    if (grad) {
        for (int k = 0; k < K; ++k) {
            const float dz = (k == label ? 1.f : 0.f) - expf(z[k] - l);
            for (int i = 0; i < C; ++i)
                grad[k * C + i] = dz * (i < F ? row[i] : 1.f) + (-0.5f * (2.f * (x[k * C + i] - m))) / (s * s);
        }
    }
    return (z[label] - l) + (-0.5f * gmmvi_sumsq(x, 0, D, m) / (s * s) - D * (logf(s) + 0.9189385332046727f));
}
"""
HAND_SOURCES = {"softmax_vec": SOFTMAX_VEC_HAND_SRC}

# one call and nothing else: sum of x[j]^2 over j < min(D, 16) with every entry an input node, and the log-sum-exp of the same
SINGLE_WDOT_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const int n = D < 16 ? D : 16;
    T h[16];
    for (int j = 0; j < n; ++j) h[j] = x[j];
    return gmmvi_wdot(x, 0, h, n);
}
"""
SINGLE_LSE_SRC = SINGLE_WDOT_SRC.replace("gmmvi_wdot(x, 0, h, n)", "gmmvi_logsumexp(h, n)")
# an array of nodes whose values are all -inf: the constant -inf and no record; the density is x[0] + 1
ALL_MINUS_INF_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    T a[3];
    for (int j = 0; j < 3; ++j) a[j] = (x[j] - 3.0e38f) - 3.0e38f;    // -inf by overflow: a node with the finite partial 1
    const T l = gmmvi_logsumexp(a, 3), e = gmmvi_logsumexp(a, 0);
    T one[1] = {x[0]};
    return gmmvi_logsumexp(one, 1) + (gmmvi_value(l) < -3.0e38f && gmmvi_value(e) < -3.0e38f ? 1.f : 1000.f);
}
"""
DENSITY_SOURCES.update({"single_wdot": SINGLE_WDOT_SRC, "single_lse": SINGLE_LSE_SRC, "all_minus_inf": ALL_MINUS_INF_SRC})

# one source per mode that calls both primitives
BOTH_DENSITY = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    T h[4];
    for (int j = 0; j < 4; ++j) h[j] = tanh(x[j] * params[j]);
    return gmmvi_wdot(x, 0, h, 4) - gmmvi_logsumexp(h, 4);
}
"""
BOTH_DATA = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T h[4];
    for (int j = 0; j < 4; ++j) h[j] = tanh(x[j] * row[j]);
    return gmmvi_wdot(x, 0, h, 4) - gmmvi_logsumexp(h, 4);
}
template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) { return -0.5f * gmmvi_sumsq(x, 0, D, params[0]); }
"""
BOTH_HAND = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    float h[4];
    for (int j = 0; j < 4; ++j) h[j] = tanhf(x[j] * params[j]);
    const float l = gmmvi_logsumexp(h, 4);
    if (grad) {
        for (int i = 0; i < D; ++i) grad[i] = 0.f;
        for (int j = 0; j < 4; ++j) grad[j] = h[j] + (x[j] - expf(h[j] - l)) * (1.f - h[j] * h[j]) * params[j];
    }
    return gmmvi_wdot(x, 0, h, 4) - l;
}
"""
BOTH = {"hand": BOTH_HAND, "autodiff": BOTH_DENSITY, "tape": BOTH_DENSITY, "data": BOTH_DATA, "data_tape": BOTH_DATA}

# a const float* where the input view belongs: no overload in the gradient modes
WDOT_ON_FLOATS_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    T h[2] = {x[0], x[1]};
    return gmmvi_wdot(params, 0, h, 2);
}
"""


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def _softmax_term(z, label, dt):
    """z [N, K] -> (z[label] - logsumexp(z) [N], d / dz [N, K]) in dt, with the max shift of the primitive."""
    m = z.max(axis=1)
    e = np.exp((z - m[:, None]).astype(dt)).astype(dt)
    s = np.sum(e, axis=1, dtype=dt)
    lse = (m + np.log(s).astype(dt)).astype(dt)
    dz = (-e / s[:, None]).astype(dt)
    dz[:, label] += dt(1)
    return (z[:, label] - lse).astype(dt), dz


class Softmax(vec.LogitVec):
    """SOFTMAX_VEC_BODY / SOFTMAX_LOOP_BODY with the prior of LogitVec; d = K C is given, the rows are [features (F) | label]."""

    def row_term(self, x, row):
        dt = self.dtype
        c = row.size
        f, k = c - 1, self.d // c
        xb = x[:, :k * c].reshape(-1, k, c)
        z = ((xb[:, :, :f] @ row[:f]).astype(dt) + xb[:, :, f]).astype(dt)
        v, dz = _softmax_term(z, int(row[f]), dt)
        g = np.zeros(x.shape, dt)
        g[:, :k * c] = (dz[:, :, None] * np.concatenate([row[:f], [dt(1)]]).astype(dt)[None, None, :]).reshape(-1, k * c)
        return v, g


class Mlp(vec.LogitVec):
    """MLP_VEC_BODY / MLP_LOOP_BODY: params = [prior mean, prior std, H]."""

    def row_term(self, x, row):
        dt = self.dtype
        c = row.size
        f, hid = c - 1, int(self.p[2])
        off = hid * c
        k = (self.d - off) // (hid + 1)
        x1 = x[:, :off].reshape(-1, hid, c)
        x2 = x[:, off:off + k * (hid + 1)].reshape(-1, k, hid + 1)
        h = np.tanh(((x1[:, :, :f] @ row[:f]).astype(dt) + x1[:, :, f]).astype(dt)).astype(dt)
        z = (np.einsum("nkh,nh->nk", x2[:, :, :hid], h).astype(dt) + x2[:, :, hid]).astype(dt)
        v, dz = _softmax_term(z, int(row[f]), dt)
        da = (np.einsum("nk,nkh->nh", dz, x2[:, :, :hid]).astype(dt) * (dt(1) - h * h)).astype(dt)
        g = np.zeros(x.shape, dt)
        g[:, :off] = (da[:, :, None] * np.concatenate([row[:f], [dt(1)]]).astype(dt)[None, None, :]).reshape(-1, off)
        g[:, off:off + k * (hid + 1)] = np.concatenate([dz[:, :, None] * h[:, None, :], dz[:, :, None]], axis=2).reshape(-1, k * (hid + 1))
        return v, g


class MixedNodes(vec.LogitVec):
    """Both branches of MIXED_BODY compute row[0] (sum_j h[j] x[8 + j] - logsumexp(h)), h = tanh(x[0 .. 8))."""

    def row_term(self, x, row):
        dt = self.dtype
        h = np.tanh(x[:, :8]).astype(dt)
        a = np.sum(h * x[:, 8:16], axis=1, dtype=dt)
        m = h.max(axis=1)
        e = np.exp(h - m[:, None]).astype(dt)
        s = np.sum(e, axis=1, dtype=dt)
        g = np.zeros(x.shape, dt)
        g[:, :8] = row[0] * (x[:, 8:16] - e / s[:, None]) * (dt(1) - h * h)
        g[:, 8:16] = row[0] * h
        return (row[0] * (a - (m + np.log(s)))).astype(dt), g.astype(dt)


CLASSES = {"softmax_vec": Softmax, "softmax_loop": Softmax, "mlp_vec": Mlp, "mlp_loop": Mlp, "mixed_nodes": MixedNodes}
PRIOR = [0.25, 2.0]


def softmax_dim(f, k):
    return k * (f + 1)


def mlp_dim(f, h, k):
    return h * (f + 1) + k * (h + 1)


def rows_for(rng, name, t, f, k):
    """[t, f + 1] rows: features ~ N(0, 1 / f), a label in [0, k); mixed_nodes: [scale, unused]."""
    if name == "mixed_nodes":
        return np.concatenate([rng.uniform(0.5, 1.5, size=(t, 1)), np.zeros((t, 1))], axis=1)
    return np.concatenate([rng.normal(size=(t, f)) / np.sqrt(f), rng.integers(0, k, size=(t, 1)).astype(np.float64)], axis=1)


def build_data_case(c, shape, seed=5):
    """c: a Case whose d matches ``shape`` = (F, K) for the softmax targets, (F, H, K) for the MLPs, () for mixed_nodes
    -> (fp64 target, x [n, d] fp32).  x ~ N(0, 1 / 4): class scores of order one.  mixed_nodes: x[:, 0] has both signs within
    every 64 lanes."""
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = (0.5 * rng.normal(size=(c.n, c.d))).astype(np.float32)
    kw = dict(batch_size=c.batch, seed=vec.base.MINIBATCH_SEED, call=c.call, d=c.d)
    if c.name == "mixed_nodes":
        x[:, 0] = np.where(np.arange(c.n) % 3 == 0, -1.0, 1.0) * (np.abs(x[:, 0]) + 0.125)
        return MixedNodes(rows_for(rng, c.name, c.rows, 1, 1), PRIOR, **kw), x
    if c.name.startswith("softmax"):
        f, k = shape
        assert c.d == softmax_dim(f, k)
        return Softmax(rows_for(rng, c.name, c.rows, f, k), PRIOR, **kw), x
    f, h, k = shape
    assert c.d == mlp_dim(f, h, k)
    return Mlp(rows_for(rng, c.name, c.rows, f, k), PRIOR + [h], **kw), x


class Density:
    """The density form: one fixed row in params, lp = row term + prior, from the data restatement with that one row."""

    def __init__(self, tgt):
        self.tgt = tgt

    def as_dtype(self, dtype):
        return Density(self.tgt.as_dtype(dtype))

    def params(self):
        p = self.tgt.params()
        row = self.tgt.data[0]
        return np.concatenate([p[:2], [p[2] if p.size > 2 else 0.0, row.size], row]).astype(np.float32)

    def log_density_and_grad(self, x):
        return self.tgt.evaluate(x)


def build_density_case(name, shape, d, n):
    tgt, x = build_data_case(Case(name, d, n, 1, 0, None, 0), shape, seed=7)
    return Density(tgt), x


class Plain:
    """single_wdot: sum of x[j]^2, j < min(D, 16); single_lse: the log-sum-exp of the same entries; all_minus_inf: x[0] + 1."""

    def __init__(self, name, dtype=np.float64):
        self.name, self.dtype = name, dtype

    def as_dtype(self, dtype):
        return Plain(self.name, dtype)

    def params(self):
        return np.zeros(1, np.float32)

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        n = min(x.shape[1], 16)
        g = np.zeros(x.shape, dt)
        if self.name == "single_wdot":
            g[:, :n] = dt(2) * x[:, :n]
            return np.sum(x[:, :n] * x[:, :n], axis=1, dtype=dt), g
        if self.name == "all_minus_inf":
            g[:, 0] = 1
            return (x[:, 0] + dt(1)).astype(dt), g
        m = x[:, :n].max(axis=1)
        e = np.exp(x[:, :n] - m[:, None]).astype(dt)
        s = np.sum(e, axis=1, dtype=dt)
        g[:, :n] = e / s[:, None]
        return (m + np.log(s)).astype(dt), g


_refs = {}


def reference(c, shape=()):
    """(a data Case, shape), or (name, shape, d, n) of a density form, or (plain name, d, n) -> (target, x, lp64, g64, lp32,
    g32), computed once, read-only."""
    key = (c, shape)
    if key not in _refs:
        if isinstance(c, Case):
            tgt, x = build_data_case(c, shape)
            lp64, g64 = tgt.evaluate(x.astype(np.float64))
            lp32, g32 = fp32_twin(tgt).evaluate(x)
        else:
            if len(c) == 4:
                tgt, x = build_density_case(*c)
            else:
                tgt = Plain(c[0])
                x = np.random.default_rng(3 + 1000 * c[1] + 7 * c[2]).normal(size=(c[2], c[1])).astype(np.float32)
            lp64, g64 = tgt.log_density_and_grad(x.astype(np.float64))
            lp32, g32 = tgt.as_dtype(np.float32).log_density_and_grad(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[key] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[key]
