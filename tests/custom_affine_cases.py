"""gmmvi_affine of user-defined device targets (csrc/custom_target_vector.inc and its overloads in the two number types; contract:
include/gmmvi_hip.h, "vector primitives"): the probe wrappers, the fp64 and fp32 NumPy restatements of one call with the bounds
that follow from the stated order, the sources of the test targets and their restatements.

    gmmvi_affine(x, w, si, sj, b, sb, h, n, out, m):  out[j] = (sum over i < n of h[i] * x[w + i si + j sj]) + x[b + j sb], j < m

The probes build h as those of tests/custom_nodes_cases.py do (h[i] = tanh(x[src + i]), every ``every``-th entry a constant), or,
with ``inputs``, as the inputs themselves, or, with ``floats``, as a const float*; the output is out[pick], or with pick == -1
gmmvi_logsumexp(out, m), which consumes every output.

Bounds of one call.
Value of out[j]: the sum has the order of gmmvi_wdot, so custom_nodes_cases.WDOT_VALUE_EPS * eps32 * sum |terms| as derived in
tests/custom_vector_cases.py; the bias is one more add, half an eps32 of |out[j]|.
Gradient entry: a multiple of eps32 * the sum over the paths of |contribution|.  custom_nodes_cases.gradient_eps("wdot", n) = 4
+ 1.5 counts the tanh partial of an entry (4) and, for one output, two products and the add of two paths (1.5).  One call now
has m outputs with adjoints a_0 .. a_m-1.  The share of an entry is the sum over jj of x[weight (i, jj)] * a_jj, gathered by
fmaf: m roundings of partial sums that never exceed the sum of |terms|, m / 2.  (The forward mode gathers the same m terms in
gmmvi_logsumexp, sum over j of p_j * out[j].d[t] by fmaf: m / 2 as well.  With pick >= 0 all terms but one are zero and the sum
is exact.)  The adjoints themselves: with pick >= 0 they are 1 and 0, exact.  With pick == -1 they are the partials p_j of
gmmvi_logsumexp at the fp32 outputs, each within a relative eps32 * (spread + 2 + (ceil(m / 4) + 2) / 2 + 1 / 2) of the fp64
softmax, spread = max |out[j] - max|, as derived in test_the_partials_of_logsumexp_sum_to_one of tests/test_custom_nodes_host.py.
So:  gradient_eps(n, m, pick, spread) = 4 + 1.5 + m / 2 + (pick == -1: spread + 2 + (ceil(m / 4) + 2) / 2 + 1 / 2).

Targets.  Rows are [features (F) | label], C = F + 1; the prior is that of logit_vec (tests/custom_vector_cases.py).
``mlp2_affine`` / ``mlp2_vec``: (F, H1, H2, K); x holds, layer by layer, one block [weights | bias] per unit (si = 1);
params = [prior mean, prior std, H1, H2].  Three gmmvi_affine calls, the first with h = row, against gmmvi_dot / gmmvi_wdot and
bias adds.  ``keras_affine`` / ``keras_loop``: (F, H, K); x = W1 [F, H] | b1 [H] | W2 [H, K] | b2 [K], row-major (si = out,
sj = 1); params = [prior mean, prior std, H, 0].  ``mixed_affine``: gmmvi_affine for x[0] > 0, scalar loops otherwise.
The density forms keep one fixed row in params = [.., .., .., .., C, row (C)].
``pick_affine``: h[i] = x[i], i < n = (D - 3) / 4, blocks [weights (n) | bias] x 3 from x[n]; returns out[params[0]]."""
import ctypes as C
import math

import numpy as np

import custom_nodes_cases as nodes
import custom_vector_cases as vec
from custom_data_cases import Case, case_id, fp32_twin  # noqa: F401  (re-exported for the two test files)
from gmmvi_amd import _lib

W = vec.W
EPS32 = vec.EPS32
MAX_N = 64
WDOT_VALUE_EPS = nodes.WDOT_VALUE_EPS


def slots(n, m):
    """The slots of one record group."""
    return (n + 1) // 2 + 2 + m if n > 0 and m > 0 else 0


def gradient_eps(n, m, pick, spread=0.0):
    """The module docstring derives it."""
    eps = nodes.gradient_eps("wdot", n) + m / 2.0
    if pick < 0:
        eps += spread + 2.0 + (math.ceil(m / 4) + 2) / 2.0 + 0.5
    return eps


def _fptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Layout:
    """One call's arguments: w, si, sj, b (-1: none), sb, n, m -> the index arrays."""

    def __init__(self, w, si, sj, b, sb, n, m):
        self.w, self.si, self.sj, self.b, self.sb, self.n, self.m = w, si, sj, b, sb, n, m

    def args(self):
        return self.w, self.si, self.sj, self.b, self.sb, self.n, self.m

    def weights(self):
        """[n, m] indices into x."""
        return self.w + np.arange(self.n)[:, None] * self.si + np.arange(self.m)[None, :] * self.sj

    def biases(self):
        return None if self.b < 0 else self.b + np.arange(self.m) * self.sb

    def __repr__(self):
        return "affine(w=%d, si=%d, sj=%d, b=%d, sb=%d, n=%d, m=%d)" % self.args()


def unit_layout(w, n, m, bias=True):
    """Blocks [weights (n) | bias] per output."""
    return Layout(w, 1, n + 1, w + n if bias else -1, n + 1, n, m)


def keras_layout(w, n, m, bias=True):
    """W [n, m] row-major, then b [m]."""
    return Layout(w, max(m, 1), 1, w + n * m if bias else -1, 1, n, m)


def probe_forward(x, lay, src, every, pick, seed_first, inputs=False, floats=False):
    """gmmvi_autodiff_probe_affine -> (out [m], value, tangents [W])."""
    x = np.ascontiguousarray(x, np.float32)
    v, t, out = C.c_float(), np.zeros(W, np.float32), np.full(max(lay.m, 1), np.nan, np.float32)
    rc = _lib.load().gmmvi_autodiff_probe_affine(_fptr(x), x.size, *lay.args(), src, every, int(inputs), int(floats), pick,
                                                 seed_first, _fptr(out), C.byref(v), _fptr(t))
    assert rc == 0, rc
    return out[:lay.m], np.float32(v.value), t


def probe_forward_gradient(x, lay, src, every, pick, inputs=False, floats=False):
    """Every pass seed 0, 16, ...: -> (the outs of the passes, the values of the passes, the concatenated tangents cut to D)."""
    res = [probe_forward(x, lay, src, every, pick, s, inputs, floats) for s in range(0, len(x), W)]
    return [r[0] for r in res], [r[1] for r in res], np.concatenate([r[2] for r in res])[:len(x)]


def probe_tape(x, lay, src, every, pick, inputs=False, floats=False):
    """gmmvi_tape_probe_affine -> (out [m], value, gradient [D], records behind the call)."""
    x = np.ascontiguousarray(x, np.float32)
    v, records = C.c_float(), C.c_int(-1)
    g, out = np.full(x.size, np.nan, np.float32), np.full(max(lay.m, 1), np.nan, np.float32)
    rc = _lib.load().gmmvi_tape_probe_affine(_fptr(x), x.size, *lay.args(), src, every, int(inputs), int(floats), pick, _fptr(out),
                                             C.byref(v), _fptr(g), C.byref(records))
    assert rc == 0, rc
    return out[:lay.m], np.float32(v.value), g, records.value


def out32(x, lay, h):
    """The fp32 restatement of the m values in the header's order: the sum of gmmvi_wdot, then the bias by one add."""
    f = np.float32
    x = np.asarray(x, f)
    idx, bias = lay.weights(), lay.biases()
    out = np.zeros(lay.m, f)
    for j in range(lay.m):
        s = nodes.value32("wdot", x[idx[:, j]], 0, lay.n, h)
        out[j] = s if bias is None else f(s + x[bias[j]])
    return out


def reference64(x, lay, src, h, const, tanh_entries, out_seen, pick):
    """fp64 at the fp32 operands x and h.  ``const``: which entries are constants [n]; ``tanh_entries``: an entry that is not a
    constant is tanh(x[src + i]), else x[src + i] itself; ``out_seen``: the fp32 outputs the probe formed, whose softmax gives the
    adjoints for pick == -1.  -> (out [m], sum |terms| [m], gradient [D], sum over the paths of |contribution| [D], spread)."""
    x64, h64 = np.asarray(x, np.float64), np.asarray(h, np.float64)
    idx, bias = lay.weights(), lay.biases()
    terms = h64[:, None] * x64[idx]                                      # [n, m]
    out = terms.sum(axis=0) + (0.0 if bias is None else x64[bias])
    spread = 0.0
    if pick >= 0:
        a = np.zeros(lay.m)
        a[pick] = 1.0
    else:
        z = np.asarray(out_seen, np.float64)
        a = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
        spread = float(z.max() - z.min())
    g, scale = np.zeros(x64.size), np.zeros(x64.size)
    np.add.at(g, idx, h64[:, None] * a[None, :])
    np.add.at(scale, idx, np.abs(h64[:, None] * a[None, :]))
    if bias is not None:
        np.add.at(g, bias, a)
        np.add.at(scale, bias, np.abs(a))
    dh = np.where(const, 0.0, 1.0 - np.tanh(x64[src:src + lay.n]) ** 2 if tanh_entries else 1.0)
    np.add.at(g, src + np.arange(lay.n), (x64[idx] * a[None, :]).sum(axis=1) * dh)
    np.add.at(scale, src + np.arange(lay.n), np.abs(x64[idx] * a[None, :]).sum(axis=1) * np.abs(dh))
    return out, np.abs(terms).sum(axis=0), g, scale, spread


def probe_cases():
    """(n, m, layout name, bias, every): the array from x[0 .. n), one spare input, the weights from x[n + 1], two spare inputs
    at the end.  D = n + 1 + m (n + 1) + 2 runs from 6 to 74 and crosses 16 and 32."""
    return [(n, m, name, bias, every) for n in (1, 2, 3, 4, 5, 17) for m in (1, 2, 3) for name in ("unit", "keras")
            for bias in (True, False) for every in (0, 2, 1)]


def probe_layout(n, m, name, bias):
    """-> (the Layout, D)."""
    w = n + 1
    return (unit_layout if name == "unit" else keras_layout)(w, n, m, bias), w + m * (n + 1) + 2


def probe_operands(d, seed=13):
    return np.random.default_rng(seed + 31 * d).normal(size=d).astype(np.float32)


# ---- the sources ---------------------------------------------------------------------------------------------------------------
MLP2_AFFINE_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H1 = (int)params[2], H2 = (int)params[3];
    const int o2 = H1 * C, o3 = o2 + H2 * (H1 + 1), K = (D - o3) / (H2 + 1);
    T a[32], h1[32], h2[32], z[16];
    gmmvi_affine(x, 0, 1, C, F, C, row, F, a, H1);
    for (int j = 0; j < H1; ++j) h1[j] = tanh(a[j]);
    gmmvi_affine(x, o2, 1, H1 + 1, o2 + H1, H1 + 1, h1, H1, a, H2);
    for (int j = 0; j < H2; ++j) h2[j] = tanh(a[j]);
    gmmvi_affine(x, o3, 1, H2 + 1, o3 + H2, H2 + 1, h2, H2, z, K);
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}
"""

MLP2_VEC_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H1 = (int)params[2], H2 = (int)params[3];
    const int o2 = H1 * C, o3 = o2 + H2 * (H1 + 1), K = (D - o3) / (H2 + 1);
    T h1[32], h2[32], z[16];
    for (int j = 0; j < H1; ++j) h1[j] = tanh(gmmvi_dot(x, j * C, row, F) + x[j * C + F]);
    for (int j = 0; j < H2; ++j) h2[j] = tanh(gmmvi_wdot(x, o2 + j * (H1 + 1), h1, H1) + x[o2 + j * (H1 + 1) + H1]);
    for (int k = 0; k < K; ++k) z[k] = gmmvi_wdot(x, o3 + k * (H2 + 1), h2, H2) + x[o3 + k * (H2 + 1) + H2];
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}
"""

KERAS_AFFINE_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H = (int)params[2], o2 = F * H + H, K = (D - o2) / (H + 1);
    T a[32], h[32], z[16];
    gmmvi_affine(x, 0, H, 1, F * H, 1, row, F, a, H);
    for (int j = 0; j < H; ++j) h[j] = tanh(a[j]);
    gmmvi_affine(x, o2, K, 1, o2 + H * K, 1, h, H, z, K);
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}
"""

KERAS_LOOP_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H = (int)params[2], o2 = F * H + H, K = (D - o2) / (H + 1);
    T h[32], z[16];
    for (int j = 0; j < H; ++j) {
        T a = x[F * H + j];
        for (int i = 0; i < F; ++i) a += row[i] * x[i * H + j];
        h[j] = tanh(a);
    }
    for (int k = 0; k < K; ++k) {
        T a = x[o2 + H * K + k];
        for (int j = 0; j < H; ++j) a += h[j] * x[o2 + j * K + k];
        z[k] = a;
    }
    T l = z[0];
    for (int k = 1; k < K; ++k) l = gmmvi_logaddexp(l, z[k]);
    return z[(int)row[F]] - l;
}
"""

# h[i] = tanh(x[i]), i < 4; z[j] = sum_i h[i] x[4 + 5 j + i] + x[8 + 5 j], j < 2; row[0] (z[0] - logaddexp(z[0], z[1])).  D >= 14.
MIXED_AFFINE_BODY = r"""
template <class T, class X>
__device__ T nodes_row(X x, int D, const float* row, int C, const float* params) {
    T h[4], z[2];
    for (int i = 0; i < 4; ++i) h[i] = tanh(x[i]);
    if (x[0] > 0.f) {
        gmmvi_affine(x, 4, 1, 5, 8, 5, h, 4, z, 2);
    } else {
        for (int j = 0; j < 2; ++j) {
            T a = x[8 + 5 * j];
            for (int i = 0; i < 4; ++i) a += h[i] * x[4 + 5 * j + i];
            z[j] = a;
        }
    }
    return row[0] * (z[0] - gmmvi_logaddexp(z[0], z[1]));
}
"""

# params = [prior mean, prior std, H1 | H, H2 | 0, C, row (C)]
DENSITY_TAIL = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    return nodes_row<T, X>(x, D, params + 5, (int)params[4], params) + nodes_prior<T, X>(x, D, params);
}
"""

_BODIES = (("mlp2_affine", MLP2_AFFINE_BODY), ("mlp2_vec", MLP2_VEC_BODY), ("keras_affine", KERAS_AFFINE_BODY),
           ("keras_loop", KERAS_LOOP_BODY), ("mixed_affine", MIXED_AFFINE_BODY))
SOURCES = {name: body + nodes.PRIOR_BODY + nodes.DATA_TAIL for name, body in _BODIES}
DENSITY_SOURCES = {name: body + nodes.PRIOR_BODY + DENSITY_TAIL for name, body in _BODIES}

PICK_AFFINE_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const int n = (D - 3) / 4;
    T h[8], out[3];
    for (int i = 0; i < n; ++i) h[i] = x[i];
    gmmvi_affine(x, n, 1, n + 1, 2 * n, n + 1, h, n, out, 3);
    return out[(int)params[0]];
}
"""
DENSITY_SOURCES["pick_affine"] = PICK_AFFINE_SRC

# the hand-written mode: two outputs over constants from params, D = 2 (n + 1) with n = 3; the gradient is coded by hand
AFFINE_HAND_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    float out[2];
    gmmvi_affine(x, 0, 1, 4, 3, 4, params, 3, out, 2);
    if (grad) {
        for (int i = 0; i < D; ++i) grad[i] = 0.f;
        for (int j = 0; j < 2; ++j) {
            for (int i = 0; i < 3; ++i) grad[4 * j + i] = params[i] * (j == 0 ? 1.f : -0.5f);
            grad[4 * j + 3] = j == 0 ? 1.f : -0.5f;
        }
    }
    return out[0] - 0.5f * out[1];
}
"""
HAND_SOURCES = {"affine_hand": AFFINE_HAND_SRC}

# a const float* where the input view belongs: no overload in the gradient modes
AFFINE_ON_FLOATS_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    T h[2] = {x[0], x[1]}, out[1];
    gmmvi_affine(params, 0, 1, 3, 2, 3, h, 2, out, 1);
    return out[0];
}
"""


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def _split(x, off, n, m, keras):
    """-> (W [N, m, n], b [N, m]) of the layer at ``off``."""
    if keras:
        return x[:, off:off + n * m].reshape(-1, n, m).transpose(0, 2, 1), x[:, off + n * m:off + n * m + m]
    blk = x[:, off:off + m * (n + 1)].reshape(-1, m, n + 1)
    return blk[:, :, :n], blk[:, :, n]


def _join(g, off, dw, db, keras):
    n, m = dw.shape[2], dw.shape[1]
    if keras:
        g[:, off:off + n * m] = dw.transpose(0, 2, 1).reshape(-1, n * m)
        g[:, off + n * m:off + n * m + m] = db
    else:
        g[:, off:off + m * (n + 1)] = np.concatenate([dw, db[:, :, None]], axis=2).reshape(-1, m * (n + 1))


class Network(vec.LogitVec):
    """tanh layers and a softmax row term with the prior of LogitVec.  Subclasses give ``sizes(c)`` -> [F, .., K] and KERAS."""
    KERAS = False

    def row_term(self, x, row):
        dt = self.dtype
        sizes = self.sizes(row.size)
        acts, mats, offs, off = [np.broadcast_to(row[:sizes[0]].astype(dt), (x.shape[0], sizes[0]))], [], [], 0
        for n, m in zip(sizes[:-1], sizes[1:]):
            wgt, b = _split(x, off, n, m, self.KERAS)
            a = (np.einsum("nmi,ni->nm", wgt, acts[-1]).astype(dt) + b).astype(dt)
            mats.append(wgt)
            offs.append(off)
            off += m * (n + 1)
            acts.append(np.tanh(a).astype(dt) if len(acts) < len(sizes) - 1 else a)
        v, da = nodes._softmax_term(acts[-1], int(row[sizes[0]]), dt)
        g = np.zeros(x.shape, dt)
        for layer in range(len(mats) - 1, -1, -1):
            h = acts[layer]
            _join(g, offs[layer], (da[:, :, None] * h[:, None, :]).astype(dt), da, self.KERAS)
            if layer > 0:
                da = (np.einsum("nm,nmi->ni", da, mats[layer]).astype(dt) * (dt(1) - h * h)).astype(dt)
        return v, g


class Mlp2(Network):
    """MLP2_AFFINE_BODY / MLP2_VEC_BODY: params = [prior mean, prior std, H1, H2]."""

    def sizes(self, c):
        f, h1, h2 = c - 1, int(self.p[2]), int(self.p[3])
        return [f, h1, h2, (self.d - h1 * c - h2 * (h1 + 1)) // (h2 + 1)]


class Keras(Network):
    """KERAS_AFFINE_BODY / KERAS_LOOP_BODY: params = [prior mean, prior std, H, 0]."""
    KERAS = True

    def sizes(self, c):
        f, h = c - 1, int(self.p[2])
        return [f, h, (self.d - f * h - h) // (h + 1)]


class MixedAffine(vec.LogitVec):
    """Both branches of MIXED_AFFINE_BODY."""

    def row_term(self, x, row):
        dt = self.dtype
        h = np.tanh(x[:, :4]).astype(dt)
        wgt, b = _split(x, 4, 4, 2, False)
        z = (np.einsum("nmi,ni->nm", wgt, h).astype(dt) + b).astype(dt)
        hi = np.maximum(z[:, 0], z[:, 1])
        lae = (hi + np.log1p(np.exp(-np.abs(z[:, 0] - z[:, 1])))).astype(dt)
        p0 = (dt(1) / (dt(1) + np.exp(z[:, 1] - z[:, 0]))).astype(dt)   # d logaddexp / d z0
        dz = (row[0] * np.stack([dt(1) - p0, -(dt(1) - p0)], axis=1)).astype(dt)
        g = np.zeros(x.shape, dt)
        _join(g, 4, (dz[:, :, None] * h[:, None, :]).astype(dt), dz, False)
        g[:, :4] = (np.einsum("nm,nmi->ni", dz, wgt).astype(dt) * (dt(1) - h * h)).astype(dt)
        return (row[0] * (z[:, 0] - lae)).astype(dt), g


CLASSES = {"mlp2_affine": Mlp2, "mlp2_vec": Mlp2, "keras_affine": Keras, "keras_loop": Keras, "mixed_affine": MixedAffine}
PRIOR = nodes.PRIOR


def mlp2_dim(f, h1, h2, k):
    return h1 * (f + 1) + h2 * (h1 + 1) + k * (h2 + 1)


def keras_dim(f, h, k):
    return f * h + h + h * k + k


def dim(name, shape):
    return mlp2_dim(*shape) if name.startswith("mlp2") else keras_dim(*shape) if name.startswith("keras") else shape[0]


def mlp2_lengths(f, h1, h2, k):
    """-> the row tapes of (mlp2_affine, mlp2_vec): the groups and the tanh records, gmmvi_logsumexp, the final -."""
    tail = 1 + (k + 1) // 2 + 1
    return (slots(f, h1) + h1 + slots(h1, h2) + h2 + slots(h2, k) + tail,
            3 * h1 + h2 * (3 + (h1 + 1) // 2) + k * (2 + (h2 + 1) // 2) + tail)


def rows_for(rng, name, t, f, k):
    return nodes.rows_for(rng, "mixed_nodes" if name == "mixed_affine" else name, t, f, k)


def build_data_case(c, shape, seed=5):
    """c: a Case whose d matches ``shape`` = (F, H1, H2, K), (F, H, K), or (D,) for mixed_affine -> (fp64 target, x [n, d] fp32).
    x ~ N(0, 1 / 4).  mixed_affine: x[:, 0] has both signs within every 64 lanes."""
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = (0.5 * rng.normal(size=(c.n, c.d))).astype(np.float32)
    kw = dict(batch_size=c.batch, seed=vec.base.MINIBATCH_SEED, call=c.call, d=c.d)
    assert c.d == dim(c.name, shape)
    if c.name == "mixed_affine":
        x[:, 0] = np.where(np.arange(c.n) % 3 == 0, -1.0, 1.0) * (np.abs(x[:, 0]) + 0.125)
        return MixedAffine(rows_for(rng, c.name, c.rows, 1, 1), PRIOR + [0, 0], **kw), x
    hidden = list(shape[1:-1]) + [0] * (3 - len(shape[1:]))
    return CLASSES[c.name](rows_for(rng, c.name, c.rows, shape[0], shape[-1]), PRIOR + hidden, **kw), x


class Density:
    """The density form: one fixed row in params = [the target's four, C, row], from the data restatement with that one row."""

    def __init__(self, tgt):
        self.tgt = tgt

    def as_dtype(self, dtype):
        return Density(self.tgt.as_dtype(dtype))

    def params(self):
        row = self.tgt.data[0]
        return np.concatenate([self.tgt.params()[:4], [row.size], row]).astype(np.float32)

    def log_density_and_grad(self, x):
        return self.tgt.evaluate(x)


class Pick:
    """PICK_AFFINE_SRC: out[pick] = sum over i < n of x[i] x[n + pick (n + 1) + i] + x[n + pick (n + 1) + n].  Every product is
    formed once and the gradient is a copy of inputs and ones: the fp32 restatement's gradient is exact."""

    def __init__(self, pick, dtype=np.float64):
        self.pick, self.dtype = int(pick), dtype

    def as_dtype(self, dtype):
        return Pick(self.pick, dtype)

    def params(self):
        return np.array([self.pick], np.float32)

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        n = (x.shape[1] - 3) // 4
        at = n + self.pick * (n + 1)
        g = np.zeros(x.shape, dt)
        g[:, at:at + n] = x[:, :n]
        g[:, at + n] = 1
        g[:, :n] = x[:, at:at + n]
        return (np.sum(x[:, :n] * x[:, at:at + n], axis=1, dtype=dt) + x[:, at + n]).astype(dt), g


_refs = {}


def reference(c, shape=()):
    """(a data Case, shape), or (name, shape, d, n) of a density form, or ("pick_affine", pick, d, n) -> (target, x, lp64, g64,
    lp32, g32), computed once, read-only."""
    key = (c, shape)
    if key not in _refs:
        if isinstance(c, Case):
            tgt, x = build_data_case(c, shape)
            lp64, g64 = tgt.evaluate(x.astype(np.float64))
            lp32, g32 = fp32_twin(tgt).evaluate(x)
        else:
            if c[0] == "pick_affine":
                tgt = Pick(c[1])
                x = np.random.default_rng(3 + 1000 * c[2] + 7 * c[3]).normal(size=(c[3], c[2])).astype(np.float32)
            else:
                data_tgt, x = build_data_case(Case(c[0], c[2], c[3], 1, 0, None, 0), c[1], seed=7)
                tgt = Density(data_tgt)
            lp64, g64 = tgt.log_density_and_grad(x.astype(np.float64))
            lp32, g32 = tgt.as_dtype(np.float32).log_density_and_grad(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[key] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[key]
