"""The normal distribution's functions of user-defined device targets (gmmvi_erfcx, gmmvi_ndtr, gmmvi_log_ndtr of
csrc/custom_target_special.inc) and sinh, cosh, asin, acos with their rules in the two number types: the operand grids and fp64
rules of the probe tests, the sources of the test targets and the NumPy / SciPy restatements they are checked against.

``probit`` and ``tobit`` are data-set targets on the base of tests/custom_data_cases.py (same row-list order, same fp32 twin);
``normals`` is a density at D = 4 in the style of ``specials`` that calls all seven functions; ``every_source(mode)`` is one source
per mode that calls every new function, for the compiler alone.

The branch points of the implementation (csrc/custom_target_special.inc writes them down next to the code) are part of the grids,
each with its two neighbours in fp32: the sign of x (all three functions and their partials); the x below which 2 e^(x^2) overflows
(gmmvi_erfcx, ERFCX_OVERFLOW); the |x| above which e^(-x^2 / 2) underflows to zero (PHI_UNDERFLOW); the x below which x^2 / 2
overflows (gmmvi_log_ndtr, HALF_SQUARE_OVERFLOW)."""
import numpy as np
from scipy import special as sp

from custom_data_cases import MINIBATCH_SEED, Case, DataTarget, case_id, fp32_twin  # noqa: F401
from custom_special_cases import NEGBIN_SRC, TWO_OVER_SQRT_PI, _NormalPrior, _softplus

SQRT_2PI = 2.5066282746310002
SQRT_2_OVER_PI = 0.7978845608028654
FLT_MAX = float(np.finfo(np.float32).max)
f32 = np.float32


# ---- the probes: rule -> (value, d/da), SciPy / NumPy in fp64 at the fp32 operand ------------------------------------------------
def erfcx_partial(a):
    """2a erfcx(a) - 2 / sqrt(pi).  In fp64 the difference cancels by 2 a^2 ulp, which is nothing on the grid up to 40 (4e-13) and
    everything at 1e18, where it gives 0 or +-2e-16 for -5.6e-37: from a = 50 on the same function is taken from its asymptotic
    series -1 / sqrt(pi) sum (-1)^n (2n + 1)!! / 2^n a^-(2n + 2), whose terms fall by 2e-3 or more there."""
    a = np.asarray(a, np.float64)
    big = a >= 50.0
    with np.errstate(all="ignore"):
        plain = 2.0 * a * sp.erfcx(a) - TWO_OVER_SQRT_PI
        r2 = 1.0 / np.where(big, a, 1.0) ** 2
        series, term = np.zeros_like(a), r2.copy()
        for n in range(8):
            series = series + term
            term = -term * (2 * n + 3) * 0.5 * r2
        return np.where(big, -0.5 * TWO_OVER_SQRT_PI * series, plain)


def _log_ndtr_partial(a):
    """exp(-a^2 / 2 - log Phi(a)) / sqrt(2 pi).  The exponent is a difference of two numbers of size a^2 / 2, exact to 1e-13 on the
    grid down to -38 and to nothing at the branch point -2.6e19: below -1000 the same quotient phi / Phi is taken as
    sqrt(2 / pi) / erfcx(-a / sqrt 2), which has no difference in it."""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        far = a < -1000.0
        near = np.exp(-0.5 * a * a - sp.log_ndtr(np.where(far, 0.0, a))) / SQRT_2PI
        return np.where(far, SQRT_2_OVER_PI / sp.erfcx(-a * np.sqrt(0.5)), near)


def _asin_partial(a):
    with np.errstate(all="ignore"):
        return 1.0 / np.sqrt(1.0 - a * a)


RULES = {
    "erfcx": (sp.erfcx, erfcx_partial),
    "ndtr": (sp.ndtr, lambda a: np.exp(-0.5 * a * a) / SQRT_2PI),
    "log_ndtr": (sp.log_ndtr, _log_ndtr_partial),
    "sinh": (np.sinh, np.cosh),
    "cosh": (np.cosh, np.sinh),
    "asin": (np.arcsin, _asin_partial),
    "acos": (np.arccos, lambda a: -_asin_partial(a)),
}
NORMAL_FAMILY = ("erfcx", "ndtr", "log_ndtr")


def rule_of(op):
    """'sinhf' -> 'sinh'."""
    return op if op in RULES else op[:-1]


def source_name(op):
    """The name a source calls the operation by."""
    return "gmmvi_" + op if op in NORMAL_FAMILY else op


def _bisect(f, lo, hi):
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) else (lo, mid)
    return lo


# fp64 positions of the branches that depend on the range of fp32
ERFCX_OVERFLOW = _bisect(lambda x: sp.erfcx(x) > FLT_MAX, -9.5, -9.0)                    # -9.3819...: below it 2 e^(x^2) > FLT_MAX
PHI_UNDERFLOW = float(np.sqrt(2.0 * 150.0 * np.log(2.0)))                                # 14.42: e^(-x^2 / 2) < 2^-150 above it
HALF_SQUARE_OVERFLOW = -float(np.sqrt(2.0 * FLT_MAX))                                    # -2.6087e19: x^2 / 2 > FLT_MAX below it


def _around(t):
    t = f32(t)
    return [np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf))]


NDTR_THRESHOLDS = [0.0, -PHI_UNDERFLOW, PHI_UNDERFLOW, HALF_SQUARE_OVERFLOW]
ERFCX_THRESHOLDS = [0.0, ERFCX_OVERFLOW]

_GEOM = np.geomspace(1e-6, 1.0, 13)
NDTR_GRID = np.concatenate([np.linspace(-38.0, 9.0, 189), _GEOM, -_GEOM, [0.0, -0.0, -14.5, -20.0]]
                           + [_around(t) for t in NDTR_THRESHOLDS]).astype(np.float32)
ERFCX_GRID = np.concatenate([np.linspace(-9.0, 40.0, 197), [1e-6, 1e3, 1e18, 1e30]]
                            + [_around(t) for t in ERFCX_THRESHOLDS]).astype(np.float32)
HYPERBOLIC_GRID = np.linspace(-80.0, 80.0, 129).astype(np.float32)
ARC_GRID = np.linspace(-0.999, 0.999, 129).astype(np.float32)


def unary_grid(rule):
    return {"erfcx": ERFCX_GRID, "ndtr": NDTR_GRID, "log_ndtr": NDTR_GRID, "sinh": HYPERBOLIC_GRID, "cosh": HYPERBOLIC_GRID,
            "asin": ARC_GRID, "acos": ARC_GRID}[rule]


# ---- the restatements' own normal functions, in the dtype of the operand -----------------------------------------------------------
def mills(u):
    """phi(u) / Phi(u) in the dtype of u: sqrt(2 / pi) / erfcx(-u / sqrt 2) for u < 0, phi(u) / Phi(u) for u >= 0 (the quotient of
    the probes' rule, exp(-u^2 / 2 - log Phi), cancels in fp32 by u^2 / 2 ulp)."""
    dt = u.dtype.type
    with np.errstate(all="ignore"):
        neg = dt(SQRT_2_OVER_PI) / sp.erfcx(-u * dt(np.sqrt(0.5)))
        pos = np.exp(dt(-0.5) * u * u) / dt(SQRT_2PI) / sp.ndtr(u)
    return np.where(u < 0, neg, pos).astype(dt)


# ---- probit: rows [features (D) | y in {0, 1}], params = [prior mean, prior std] -----------------------------------------------------
_PRIOR_SRC = NEGBIN_SRC[NEGBIN_SRC.index("template <class T, class X>\n__device__ T gmmvi_user_prior"):]

PROBIT_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T eta = 0.f;
    for (int i = 0; i < D; ++i) eta += row[i] * x[i];
    return gmmvi_log_ndtr((2.f * row[D] - 1.f) * eta);
}
""" + _PRIOR_SRC

# the same posterior by the plain form: what a source had to write before gmmvi_log_ndtr
PROBIT_PLAIN_SRC = PROBIT_SRC.replace("gmmvi_log_ndtr((2.f * row[D] - 1.f) * eta)",
                                      "log(0.5f * erfc(-0.70710678f * ((2.f * row[D] - 1.f) * eta)))")
assert PROBIT_PLAIN_SRC != PROBIT_SRC

# ---- tobit: rows [features (D - 1) | y >= 0], sigma = softplus(x[D - 1]) + 0.05 ---------------------------------------------------------
TOBIT_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T eta = 0.f;
    for (int i = 0; i < D - 1; ++i) eta += row[i] * x[i];
    const float y = row[D - 1];
    const T sigma = gmmvi_softplus(x[D - 1]) + 0.05f;
    if (y > 0.f) {
        const T r = (y - eta) / sigma;
        return -log(sigma) - 0.5f * r * r - 0.9189385f;
    }
    return gmmvi_log_ndtr(-eta / sigma);                       // censored at 0: P(eta + sigma eps <= 0)
}
""" + _PRIOR_SRC


class Probit(_NormalPrior):
    def row_term(self, x, row):
        dt = self.dtype
        a, y = row[:-1], row[-1]
        s = dt(2) * y - dt(1)
        u = (s * (x @ a).astype(dt)).astype(dt)
        return sp.log_ndtr(u).astype(dt), ((mills(u) * s)[:, None] * a[None, :]).astype(dt)


class Tobit(_NormalPrior):
    def row_term(self, x, row):
        dt = self.dtype
        a, y = row[:-1], row[-1]
        eta = (x[:, :-1] @ a).astype(dt)
        t = x[:, -1]
        sigma = (_softplus(t) + dt(np.float32(0.05))).astype(dt)
        if y > 0:
            r = (y - eta) / sigma
            v = -np.log(sigma) - dt(0.5) * r * r - dt(np.float32(0.9189385))
            d_eta, d_sigma = r / sigma, (r * r - dt(1)) / sigma
        else:
            u = (-eta / sigma).astype(dt)
            m = mills(u)
            v = sp.log_ndtr(u)
            d_eta, d_sigma = -m / sigma, m * eta / (sigma * sigma)
        g = np.concatenate([d_eta[:, None] * a[None, :], (d_sigma * sp.expit(t))[:, None]], axis=1)
        return v.astype(dt), g.astype(dt)


DATA_SOURCES = {"probit": PROBIT_SRC, "tobit": TOBIT_SRC}
PLANTED_ETA = -20.0


def probit_rows(rng, x0, t, d):
    """Labels 0 / 1 on features ~ N(0, 1 / D); row 0 is planted: a = -20 x0 / |x0|^2 with y = 1, so that the signed predictor of
    (x0, row 0) is -20 by construction and not by seed."""
    features = rng.normal(size=(t, d)) / np.sqrt(d)
    labels = rng.integers(0, 2, size=(t, 1)).astype(np.float64)
    x0 = np.asarray(x0, np.float64)
    features[0] = PLANTED_ETA * x0 / (x0 @ x0)
    labels[0] = 1.0
    return np.concatenate([features, labels], axis=1)


def tobit_rows(rng, t, d):
    """y = max(0, eta* + noise) on features ~ N(0, 1 / D); with T >= 3 row 0 is censored and row 1 is not, whatever the draw."""
    features = rng.normal(size=(t, d - 1)) / np.sqrt(d)
    y = np.maximum(0.0, features @ rng.normal(size=d - 1) + 0.3 * rng.normal(size=t))
    if t >= 3:
        y[0] = 0.0
        y[1] = max(y[1], 0.25)
    return np.concatenate([features, y[:, None]], axis=1)


def build_data_case(c, seed=5):
    """-> (fp64 target, x [n, d] fp32) of a Case of tests/custom_data_cases.py."""
    rng = np.random.default_rng(seed + 1000 * c.d + 7 * c.n + 100003 * c.rows)
    x = rng.normal(size=(c.n, c.d)).astype(np.float32)
    kw = dict(batch_size=c.batch, seed=MINIBATCH_SEED, call=c.call)
    if c.name == "probit":
        return Probit(probit_rows(rng, x[0], c.rows, c.d), [0.25, 2.0], d=c.d, **kw), x
    return Tobit(tobit_rows(rng, c.rows, c.d), [0.25, 2.0], d=c.d, **kw), x


def data_kernel_cases():
    """The seams of tests/custom_special_cases.py for both names: D = 4; N one lane and more than a tile; T = 3, 67 cut into 3
    chunks, 257 on the automatic plan; full data, and a minibatch of B = 5 at call 3."""
    return [Case(name, 4, n, t, k, batch, 3 if batch else 0)
            for name in ("probit", "tobit") for n in (1, 65) for t, k in ((3, 0), (67, 3), (257, 0)) for batch in (None, 5)
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


# ---- normals: D = 4, params = [p0 .. p3]; all seven functions, each spelling once ---------------------------------------------------
NORMALS_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float p0 = params[0], p1 = params[1], p2 = params[2], p3 = params[3];
    const T x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    T s = 0.f;
    for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i];                 // A
    s += 0.5f * gmmvi_log_ndtr(3.f * x0 - 2.f);                          // B
    s += 0.3f * gmmvi_ndtr(p0 * x1);                                     // C
    s -= 0.1f * log(gmmvi_erfcx(x2 + x3));                               // D
    s += 0.05f * sinh(p1 * x0);                                          // E
    s -= 0.05f * coshf(x1);                                              // F
    s += 0.2f * asin(0.9f * tanh(x2));                                   // G
    s += 0.1f * acosf(0.9f * sin(x3));                                   // H
    s += 0.05f * sinhf(0.5f * x3) - 0.02f * cosh(x2);                    // I
    s += 0.1f * asinf(0.5f * sin(x0)) + 0.1f * acos(0.5f * cos(x1));     // J
    s += gmmvi_ndtr(p2) + 0.1f * gmmvi_log_ndtr(-p3) + 0.01f * gmmvi_erfcx(p1) + 0.01f * sinhf(p0) * acosf(p1);   // K: floats
    return s;
}
"""


class Normals:
    """The fp64 (or, as its own twin, fp32) restatement of NORMALS_SRC, term by term under the letters of the source."""

    def __init__(self, dtype=np.float64):
        self.p = np.array([0.8, 0.6, 0.3, 1.7], np.float32)
        self.dtype = dtype

    def as_dtype(self, dtype):
        return Normals(dtype)

    def params(self):
        return self.p.copy()

    def get_num_dimensions(self):
        return 4

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        p0, p1, p2, p3 = (dt(v) for v in self.p)
        x0, x1, x2, x3 = (x[:, i] for i in range(4))
        c = dt
        g = [-x[:, i] for i in range(4)]                                 # A
        s = np.zeros(x.shape[0], dt)
        for i in range(4):
            s = s - c(0.5) * x[:, i] * x[:, i]
        u = c(3) * x0 - c(2)                                             # B
        s = s + c(0.5) * sp.log_ndtr(u); g[0] = g[0] + c(1.5) * mills(u)
        u = p0 * x1                                                      # C
        s = s + c(0.3) * sp.ndtr(u); g[1] = g[1] + c(0.3) * p0 * np.exp(c(-0.5) * u * u) / c(SQRT_2PI)
        u = x2 + x3                                                      # D
        e = sp.erfcx(u)
        d = -c(0.1) * (c(2) * u - c(TWO_OVER_SQRT_PI) / e)
        s = s - c(0.1) * np.log(e); g[2] = g[2] + d; g[3] = g[3] + d
        u = p1 * x0                                                      # E
        s = s + c(0.05) * np.sinh(u); g[0] = g[0] + c(0.05) * p1 * np.cosh(u)
        s = s - c(0.05) * np.cosh(x1); g[1] = g[1] - c(0.05) * np.sinh(x1)                 # F
        th = np.tanh(x2)                                                 # G
        u = c(0.9) * th
        s = s + c(0.2) * np.arcsin(u); g[2] = g[2] + c(0.2) * c(0.9) * (c(1) - th * th) / np.sqrt(c(1) - u * u)
        u = c(0.9) * np.sin(x3)                                          # H
        s = s + c(0.1) * np.arccos(u); g[3] = g[3] - c(0.1) * c(0.9) * np.cos(x3) / np.sqrt(c(1) - u * u)
        u = c(0.5) * x3                                                  # I
        s = s + (c(0.05) * np.sinh(u) - c(0.02) * np.cosh(x2))
        g[3] = g[3] + c(0.025) * np.cosh(u); g[2] = g[2] - c(0.02) * np.sinh(x2)
        u, w = c(0.5) * np.sin(x0), c(0.5) * np.cos(x1)                  # J
        s = s + (c(0.1) * np.arcsin(u) + c(0.1) * np.arccos(w))
        g[0] = g[0] + c(0.05) * np.cos(x0) / np.sqrt(c(1) - u * u); g[1] = g[1] + c(0.05) * np.sin(x1) / np.sqrt(c(1) - w * w)
        s = s + (sp.ndtr(p2) + c(0.1) * sp.log_ndtr(-p3) + c(0.01) * sp.erfcx(p1) + c(0.01) * np.sinh(p0) * np.arccos(p1))   # K
        return s.astype(dt), np.stack(g, axis=1).astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


def build_normals(n, seed=5):
    """-> (fp64 target, x [n, 4] fp32) on standard normal samples."""
    rng = np.random.default_rng(seed + 4000 + n)
    return Normals(), rng.normal(size=(n, 4)).astype(np.float32)


# ---- one source per mode that calls every new function ---------------------------------------------------------------------------
EVERY_FN = r"""
template <class T>
__device__ T every_normal(T a, T b, float c) {
    T s = gmmvi_erfcx(a) + gmmvi_ndtr(b) + gmmvi_log_ndtr(a * b);
    s += sinh(a) + sinhf(b) + cosh(a) + coshf(b);
    s += asin(0.5f * tanh(a)) + asinf(0.5f * tanh(b)) + acos(0.5f * tanh(a)) + acosf(0.5f * tanh(b));
    s += gmmvi_erfcx(c) * gmmvi_ndtr(c) + gmmvi_log_ndtr(c) + sinhf(c) + coshf(c) + asinf(0.5f * c) + acosf(0.5f * c);
    return s;
}
"""


def every_source(mode):
    """mode: 'hand', 'density' (the forward and the tape mode) or 'data' (the two data modes)."""
    if mode == "hand":
        return EVERY_FN + ("__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {\n"
                           "    if (grad) grad[0] = gmmvi_erfcx(x[0]) + gmmvi_ndtr(x[0]) + gmmvi_log_ndtr(x[0]);\n"
                           "    return every_normal<float>(x[0], x[D - 1], params[0]);\n}\n")
    if mode == "density":
        return EVERY_FN + ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
                           "    return every_normal<T>(x[0], x[D - 1], params[0]);\n}\n")
    return EVERY_FN + ("template <class T, class X> __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {\n"
                       "    return every_normal<T>(x[0] * row[0], x[D - 1], row[C - 1]);\n}\n"
                       "template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params) {\n"
                       "    return every_normal<T>(x[0], x[D - 1], params[0]);\n}\n")
