"""The special functions of user-defined device targets (csrc/custom_target_special.inc and their rules in the two number types):
the operand grids and fp64 rules of the probe tests, the sources of the test targets and the NumPy / SciPy restatements they are
checked against.

``negbin`` and ``erfmix`` are data-set targets on the base of tests/custom_data_cases.py (same row-list order, same fp32 twin);
``specials`` is a density at D = 6 in the style of ``allops`` that calls every new function at least once; ``every_source(mode)``
is one source per mode that calls every new function, for the compiler alone."""
import numpy as np
from scipy import special as sp

from custom_data_cases import MINIBATCH_SEED, Case, DataTarget, case_id, fp32_twin  # noqa: F401

TWO_OVER_SQRT_PI = 1.1283791670955126
SQRT_HALF = 0.7071067811865476


def _trigamma(a):
    """polygamma has no float32 loop: fp64, rounded to the dtype of the operand."""
    return sp.polygamma(1, np.asarray(a, np.float64)).astype(np.asarray(a).dtype)


def _softplus(a):
    return -sp.log_expit(-a)


# ---- the probes: rule -> (value, d/da, d/db or None), each in the dtype of its operands; SciPy in fp64 is the reference ----------
RULES = {
    "lgamma": (sp.gammaln, sp.digamma, None),
    "erf": (sp.erf, lambda a: TWO_OVER_SQRT_PI * np.exp(-a * a), None),
    "erfc": (sp.erfc, lambda a: -TWO_OVER_SQRT_PI * np.exp(-a * a), None),
    "digamma": (sp.digamma, _trigamma, None),
    "trigamma": (_trigamma, lambda a: 0.0 * a, None),                   # a float function: a constant
    "sigmoid": (sp.expit, lambda a: sp.expit(a) * sp.expit(-a), None),
    "softplus": (_softplus, sp.expit, None),
    "log_sigmoid": (sp.log_expit, lambda a: sp.expit(-a), None),
    "logaddexp": (np.logaddexp, lambda a, b: sp.expit(a - b), lambda a, b: sp.expit(b - a)),
}
GAMMA_FAMILY = ("lgamma", "digamma", "trigamma")
SIGMOID_FAMILY = ("sigmoid", "softplus", "log_sigmoid")

DIGAMMA_ROOT = 1.4616321
GAMMA_GRID = np.unique(np.concatenate([np.geomspace(1e-6, 1e4, 41), np.linspace(0.05, 8.0, 54), [1.0, 2.0, DIGAMMA_ROOT]]))
_SIGMOID_POSITIVE = np.concatenate([np.linspace(0.25, 20.0, 24), [30.0, 45.0, 60.0, 75.0, 87.0, 88.0, 89.0, 90.0, 1e-6, 1e-30]])
SIGMOID_GRID = np.concatenate([_SIGMOID_POSITIVE, -_SIGMOID_POSITIVE[:-1], [0.0, -0.0]])
ERF_GRID = np.linspace(-6.0, 9.5, 125)
LOGADDEXP_EXTRA = [-float(np.log(2.0)), 30.0, -30.0, 88.0, -88.0]


def split(op):
    """'lgammaf' -> ('lgamma', 'tt'), 'logaddexp_tf' -> ('logaddexp', 'tf'): the rule and which operands are numbers."""
    form = "tt"
    for suffix in ("_tf", "_ft"):
        if op.endswith(suffix):
            op, form = op[:-3], suffix[1:]
    if op not in RULES and op.endswith("f") and op[:-1] in RULES:
        op = op[:-1]
    return op, form


def unary_grid(rule):
    return GAMMA_GRID if rule in GAMMA_FAMILY else SIGMOID_GRID if rule in SIGMOID_FAMILY else ERF_GRID


def source_name(op):
    """The name a source calls the operation by."""
    rule, _ = split(op)
    return op if rule in ("lgamma", "erf", "erfc") else "gmmvi_" + rule


# ---- negbin: rows [features (D - 1) | count y], params = [prior mean, prior std] ------------------------------------------------
NEGBIN_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T eta = 0.f;
    for (int i = 0; i < D - 1; ++i) eta += row[i] * x[i];
    const float y = row[D - 1];
    const T r = gmmvi_softplus(x[D - 1]);
    const T u = log(r) - eta;
    return lgamma(y + r) - lgamma(r) - lgammaf(y + 1.f) + r * gmmvi_log_sigmoid(u) + y * gmmvi_log_sigmoid(-u);
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

# ---- erfmix: a probit with label noise, rows [features (D) | y in {0, 1}], params = [prior mean, prior std, eps] -------------------
ERFMIX_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    const float eps = params[2];
    T eta = 0.f;
    for (int i = 0; i < D; ++i) eta += row[i] * x[i];
    const float sign = 1.f - 2.f * row[D];                        // y = 1: Phi(eta) = erfc(-eta / sqrt 2) / 2
    return log(eps + (1.f - 2.f * eps) * 0.5f * erfc(sign * 0.70710678f * eta));
}
""" + NEGBIN_SRC[NEGBIN_SRC.index("template <class T, class X>\n__device__ T gmmvi_user_prior"):]


class _NormalPrior(DataTarget):
    def prior(self, x):
        dt = self.dtype
        m, s = dt(self.p[0]), dt(self.p[1])
        r = (x - m) / s
        v = dt(-0.5) * np.sum(r * r, axis=1, dtype=dt) - dt(x.shape[1]) * (np.log(s) + dt(0.9189385332046727))
        return v.astype(dt), (-r / s).astype(dt)


class NegBin(_NormalPrior):
    def row_term(self, x, row):
        dt = self.dtype
        a, y = row[:-1], row[-1]
        eta = (x[:, :-1] @ a).astype(dt)
        t = x[:, -1]
        r = _softplus(t).astype(dt)
        u = np.log(r) - eta
        ls_u, ls_mu = sp.log_expit(u), sp.log_expit(-u)
        v = sp.gammaln(y + r) - sp.gammaln(r) - sp.gammaln(y + dt(1)) + r * ls_u + y * ls_mu
        du = r * sp.expit(-u) - y * sp.expit(u)                       # d v / d u
        dr = sp.digamma(y + r) - sp.digamma(r) + ls_u + du / r
        g = np.concatenate([(-du)[:, None] * a[None, :], (dr * sp.expit(t))[:, None]], axis=1)
        return v.astype(dt), g.astype(dt)


class ErfMix(_NormalPrior):
    def row_term(self, x, row):
        dt = self.dtype
        eps = dt(self.p[2])
        a, y = row[:-1], row[-1]
        eta = (x @ a).astype(dt)
        z = (dt(1) - dt(2) * y) * dt(np.float32(0.70710678)) * eta
        k = (dt(1) - dt(2) * eps) * dt(0.5)
        p = eps + k * sp.erfc(z)
        dp = -k * dt(TWO_OVER_SQRT_PI) * np.exp(-z * z) * (dt(1) - dt(2) * y) * dt(np.float32(0.70710678))
        return np.log(p).astype(dt), ((dp / p)[:, None] * a[None, :]).astype(dt)


DATA_SOURCES = {"negbin": NEGBIN_SRC, "erfmix": ERFMIX_SRC}


def build_data_case(c, seed=5):
    """-> (fp64 target, x [n, d] fp32) of a Case of tests/custom_data_cases.py.  negbin: features ~ N(0, 1 / D), counts of a
    negative binomial of mean 3; erfmix: features scaled so that |eta| stays below about 3, labels 0 / 1."""
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = rng.normal(size=(c.n, c.d)).astype(np.float32)
    kw = dict(batch_size=c.batch, seed=MINIBATCH_SEED, call=c.call)
    if c.name == "negbin":
        features = rng.normal(size=(c.rows, c.d - 1)) / np.sqrt(c.d)
        counts = rng.negative_binomial(2.0, 0.4, size=(c.rows, 1)).astype(np.float64)
        return NegBin(np.concatenate([features, counts], axis=1), [0.25, 2.0], d=c.d, **kw), x
    features = rng.normal(size=(c.rows, c.d)) / np.sqrt(c.d)
    labels = rng.integers(0, 2, size=(c.rows, 1)).astype(np.float64)
    return ErfMix(np.concatenate([features, labels], axis=1), [0.25, 2.0, 0.02], d=c.d, **kw), x


def data_kernel_cases():
    """D = 4; N one lane and more than a tile; T = 3 (fewer rows than waves), 67 cut into 3 chunks (a ragged last chunk), 257 on
    the automatic plan; full data, and a minibatch of B = 5 at call 3."""
    return [Case(name, 4, n, t, k, batch, 3 if batch else 0)
            for name in ("negbin", "erfmix") for n in (1, 65) for t, k in ((3, 0), (67, 3), (257, 0)) for batch in (None, 5)
            if batch is None or batch <= t]


_refs = {}


def data_reference(c):
    """-> (target, x, lp64, g64, lp32, g32), computed once per case and read-only."""
    if c not in _refs:
        tgt, x = build_data_case(c)
        lp64, g64 = tgt.evaluate(x.astype(np.float64))
        lp32, g32 = fp32_twin(tgt).evaluate(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[c] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[c]


# ---- specials: D = 6, params = [p0 .. p5]; every new function at least once, the gamma family on arguments mapped positive -------
SPECIALS_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float p0 = params[0], p1 = params[1], p2 = params[2], p3 = params[3], p4 = params[4], p5 = params[5];
    const T x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4], x5 = x[5];
    T s = 0.f;
    for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i];                 // A
    s += 0.1f * lgamma(1.5f + x0 * x0);                                  // B
    s -= 0.05f * lgamma(0.5f + x1 * x1) + 0.01f * lgammaf(1.f + p5);     // C
    s += 0.3f * erf(x2);                                                 // D
    s += 0.2f * erff(p0 * x3);                                           // E
    s += 0.25f * erfc(x4);                                               // F
    s -= 0.1f * erfcf(x5 - p1);                                          // G
    s += 0.1f * gmmvi_digamma(1.5f + x1 * x1);                           // H
    s += gmmvi_sigmoid(x2 + x3);                                         // I
    s -= 0.5f * gmmvi_softplus(x4 * p2);                                 // J
    s += 0.5f * gmmvi_log_sigmoid(x5 - x0);                              // K
    s += 0.2f * gmmvi_logaddexp(x0, x1);                                 // L
    s += 0.2f * gmmvi_logaddexp(x2, p3);                                 // M
    s -= 0.1f * gmmvi_logaddexp(p4, x3 * x4);                            // N
    s += gmmvi_softplus(p5) + 0.01f * gmmvi_trigamma(1.f + p5);          // O: floats in every instantiation
    return s;
}
"""


class Specials:
    """The fp64 (or, as its own twin, fp32) restatement of SPECIALS_SRC, term by term under the letters of the source."""

    def __init__(self, dtype=np.float64):
        self.p = np.array([0.5, 0.4, 0.3, 0.7, 0.2, 0.35], np.float32)
        self.dtype = dtype

    def as_dtype(self, dtype):
        return Specials(dtype)

    def params(self):
        return self.p.copy()

    def get_num_dimensions(self):
        return 6

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        p0, p1, p2, p3, p4, p5 = (dt(v) for v in self.p)
        x0, x1, x2, x3, x4, x5 = (x[:, i] for i in range(6))
        c = dt
        k = dt(TWO_OVER_SQRT_PI)
        g = [-x[:, i] for i in range(6)]                                 # A
        s = np.zeros(x.shape[0], dt)
        for i in range(6):
            s = s - c(0.5) * x[:, i] * x[:, i]
        u = c(1.5) + x0 * x0                                             # B
        s = s + c(0.1) * sp.gammaln(u); g[0] = g[0] + c(0.2) * sp.digamma(u) * x0
        u = c(0.5) + x1 * x1                                             # C
        s = s - (c(0.05) * sp.gammaln(u) + c(0.01) * sp.gammaln(c(1) + p5)); g[1] = g[1] - c(0.1) * sp.digamma(u) * x1
        s = s + c(0.3) * sp.erf(x2); g[2] = g[2] + c(0.3) * k * np.exp(-x2 * x2)           # D
        u = p0 * x3                                                      # E
        s = s + c(0.2) * sp.erf(u); g[3] = g[3] + c(0.2) * p0 * k * np.exp(-u * u)
        s = s + c(0.25) * sp.erfc(x4); g[4] = g[4] - c(0.25) * k * np.exp(-x4 * x4)        # F
        u = x5 - p1                                                      # G
        s = s - c(0.1) * sp.erfc(u); g[5] = g[5] + c(0.1) * k * np.exp(-u * u)
        u = c(1.5) + x1 * x1                                             # H
        s = s + c(0.1) * sp.digamma(u); g[1] = g[1] + c(0.2) * _trigamma(u) * x1
        u = x2 + x3                                                      # I
        d = sp.expit(u) * sp.expit(-u)
        s = s + sp.expit(u); g[2] = g[2] + d; g[3] = g[3] + d
        u = x4 * p2                                                      # J
        s = s - c(0.5) * _softplus(u); g[4] = g[4] - c(0.5) * p2 * sp.expit(u)
        u = x5 - x0                                                      # K
        d = c(0.5) * sp.expit(-u)
        s = s + c(0.5) * sp.log_expit(u); g[5] = g[5] + d; g[0] = g[0] - d
        s = s + c(0.2) * np.logaddexp(x0, x1)                            # L
        g[0] = g[0] + c(0.2) * sp.expit(x0 - x1); g[1] = g[1] + c(0.2) * sp.expit(x1 - x0)
        s = s + c(0.2) * np.logaddexp(x2, p3); g[2] = g[2] + c(0.2) * sp.expit(x2 - p3)    # M
        u = x3 * x4                                                      # N
        d = c(0.1) * sp.expit(u - p4)
        s = s - c(0.1) * np.logaddexp(p4, u); g[3] = g[3] - d * x4; g[4] = g[4] - d * x3
        s = s + (_softplus(p5) + c(0.01) * _trigamma(c(1) + p5))         # O
        return s.astype(dt), np.stack(g, axis=1).astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


def build_specials(n, seed=5):
    """-> (fp64 target, x [n, 6] fp32) on standard normal samples."""
    rng = np.random.default_rng(seed + 6000 + n)
    return Specials(), rng.normal(size=(n, 6)).astype(np.float32)


# ---- one source per mode that calls every new function ---------------------------------------------------------------------------
EVERY_FN = r"""
template <class T>
__device__ T every_special(T a, T b, float c) {
    T s = lgamma(1.5f + a * a) + lgamma(2.5f + b * b) + lgammaf(1.f + c * c);
    s += erf(a) + erff(b) + erfc(a) + erfcf(b);
    s += gmmvi_digamma(1.5f + b * b) + gmmvi_sigmoid(a) + gmmvi_softplus(b) + gmmvi_log_sigmoid(a);
    s += gmmvi_logaddexp(a, b) + gmmvi_logaddexp(a, c) + gmmvi_logaddexp(c, b);
    s += gmmvi_digamma(1.f + c * c) * gmmvi_trigamma(1.f + c * c) + gmmvi_sigmoid(c) + gmmvi_logaddexp(c, 1.f);
    return s;
}
"""


def every_source(mode):
    """mode: 'hand', 'density' (the forward and the tape mode) or 'data' (the two data modes)."""
    if mode == "hand":
        return EVERY_FN + ("__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {\n"
                           "    if (grad) grad[0] = gmmvi_sigmoid(x[0]) + gmmvi_trigamma(1.f + x[0] * x[0]);\n"
                           "    return every_special<float>(x[0], x[D - 1], params[0]);\n}\n")
    if mode == "density":
        return EVERY_FN + ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
                           "    return every_special<T>(x[0], x[D - 1], params[0]);\n}\n")
    return EVERY_FN + ("template <class T, class X> __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {\n"
                       "    return every_special<T>(x[0] * row[0], x[D - 1], row[C - 1]);\n}\n"
                       "template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params) {\n"
                       "    return every_special<T>(x[0], x[D - 1], params[0]);\n}\n")
