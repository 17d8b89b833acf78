"""Differentiated user-defined device targets (csrc/custom_target_autodiff.inc, DeviceAutodiffLNPDF): the sources of the test
targets, each the log density alone as a template over the number type, and the NumPy restatements they are checked against.
Rosenbrock, Quartic and Planar are the formulas of tests/custom_target_cases.py with the gradient code deleted, and their
restatements are the ones of that file; ``allops`` calls every operation of the dual-number text at least once and has its own
restatement with a closed-form gradient."""
import numpy as np

import custom_target_cases as base
from custom_target_cases import Planar, Quartic, Rosenbrock, fp32_twin as _base_fp32_twin  # noqa: F401

ROSENBROCK_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float a = params[0], b = params[1];
    const T u = a - x[0];
    const T t = x[1] - x[0] * x[0];
    return -(u * u + b * t * t);
}
"""

QUARTIC_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float* m = params;
    const float* P = params + D;
    const float c = params[D + D * (D + 1) / 2];
    T lp = 0.f;
    for (int i = 0; i < D; ++i) {
        T s = 0.f;
        for (int j = 0; j < D; ++j) {
            const float pij = j <= i ? P[i * (i + 1) / 2 + j] : P[j * (j + 1) / 2 + i];
            s += pij * (x[j] - m[j]);
        }
        const T d = x[i] - m[i];
        const T d3 = d * d * d;
        lp -= 0.5f * d * s + c * d3 * d;
    }
    return lp;
}
"""

# no per-lane arrays and no reverse loop: the max over the goals is a branch on a comparison
PLANAR_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float* prior_std = params;
    const float lik_std = params[D];
    const int G = (int)params[D + 1];
    const float* goals = params + D + 2;
    T c = 0.f, px = 0.f, py = 0.f, prior = 0.f;
    for (int i = 0; i < D; ++i) {
        const T t = x[i];
        c += t;
        px += cosf(c); py += sinf(c);
        const float sd = prior_std[i];
        const T r = t / sd;
        prior += -0.5f * r * r - logf(sd);
    }
    prior -= 0.5f * D * 1.8378770664093453f;
    const float inv_var = 1.f / (lik_std * lik_std);
    T best = -3.0e38f;
    for (int g = 0; g < G; ++g) {
        const T dx = px - goals[2 * g], dy = py - goals[2 * g + 1];
        const T ll = -0.5f * (dx * dx + dy * dy) * inv_var - 2.f * logf(lik_std) - 1.8378770664093453f;
        if (ll > best) best = ll;
    }
    return prior + best;
}
"""

# ---- allops: D = 6, params = [p0 .. p5]; every operation of the surface at least once ------------------------------------------
ALLOPS_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float p0 = params[0], p1 = params[1], p2 = params[2], p3 = params[3], p4 = params[4], p5 = params[5];
    const T x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4], x5 = x[5];
    T s = 0.f;
    for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i];                 // A
    s += exp(p0 * x0) * 0.1f;                                            // B
    s += expm1f(x1 * p1);                                                // C
    s -= log(1.f + x2 * x2);                                             // D
    s += log1pf(x3 * x3) / 2.f;                                          // E
    s += sqrtf(x4 * x4 + p2);                                            // F
    s += rsqrtf(p3 + x5 * x5);                                           // G
    s += sin(x0) * cosf(x1);                                             // H
    s += tanf(p4 * x2) - p4 * x2;                                        // I
    s += tanh(x3 - p5);                                                  // J
    s += p5 - atanf(x4);                                                 // K
    s += -fabsf(x5);                                                     // L
    s += 0.25f * fmax(x0, x1) + 0.25f * fminf(x2, p5) + 0.1f * fmaxf(p5, x3) + 0.1f * fmin(x4, x5);   // M
    T q = x0 / (1.f + x1 * x1);                                          // N
    q *= 0.5f;
    q /= 2.f + cos(x2);
    q /= 2.f;
    s += q;
    s += 1.f / (2.f + sinf(x3));                                         // O
    T w = 1.f + x4 * x4;                                                 // P
    w *= w;
    s -= 0.01f * pow(w, 0.75f);
    s += 0.05f * powf(1.f + x5 * x5, 0.5f * x0);                         // Q
    if (x5 > 0.f) s += 0.1f * x5 * x5; else s -= 0.1f * x5 * x5;         // R
    if (x0 < x1) s += 0.05f * (x1 - x0) * (x1 - x0);                     // S
    if (p5 <= x2) { const T h = x2 - p5; s -= 0.05f * h * h; }           // T
    const float v3 = gmmvi_value(x3), v4 = gmmvi_value(x4);
    if (x3 >= x4 && v3 >= v4) { T h = x3; h -= x4; s += 0.05f * h * h; } // U
    if (x1 != x1 || x2 == 1.0e30f) return x1;                            // never taken on finite inputs below 1e30
    s += p5;
    s -= 0.25f;
    return s;
}
"""


class AllOps:
    """The fp64 (or, as its own twin, fp32) restatement of ALLOPS_SRC, term by term under the letters of the source."""

    def __init__(self, dtype=np.float64):
        self.p = np.array([0.5, 0.4, 0.3, 0.7, 0.2, 0.35], np.float32)
        self.dtype = dtype

    def as_dtype(self, dtype):
        return AllOps(dtype)

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
        g = [np.zeros(x.shape[0], dt) for _ in range(6)]
        s = np.zeros(x.shape[0], dt)
        for i in range(6):                                               # A
            s = s - c(0.5) * x[:, i] * x[:, i]
            g[i] = g[i] - x[:, i]
        e = np.exp(p0 * x0)                                              # B
        s = s + e * c(0.1); g[0] = g[0] + c(0.1) * p0 * e
        s = s + np.expm1(x1 * p1); g[1] = g[1] + p1 * np.exp(x1 * p1)    # C
        u = c(1) + x2 * x2                                               # D
        s = s - np.log(u); g[2] = g[2] - c(2) * x2 / u
        s = s + np.log1p(x3 * x3) / c(2); g[3] = g[3] + x3 / (c(1) + x3 * x3)   # E
        r = np.sqrt(x4 * x4 + p2)                                        # F
        s = s + r; g[4] = g[4] + x4 / r
        u = p3 + x5 * x5                                                 # G
        s = s + c(1) / np.sqrt(u); g[5] = g[5] - x5 / (u * np.sqrt(u))
        s = s + np.sin(x0) * np.cos(x1)                                  # H
        g[0] = g[0] + np.cos(x0) * np.cos(x1); g[1] = g[1] - np.sin(x0) * np.sin(x1)
        t = np.tan(p4 * x2)                                              # I
        s = s + (t - p4 * x2); g[2] = g[2] + p4 * t * t
        s = s + np.tanh(x3 - p5); g[3] = g[3] + c(1) / np.cosh(x3 - p5) ** 2   # J
        s = s + (p5 - np.arctan(x4)); g[4] = g[4] - c(1) / (c(1) + x4 * x4)    # K
        s = s - np.abs(x5); g[5] = g[5] - np.sign(x5)                    # L
        s = s + (c(0.25) * np.maximum(x0, x1) + c(0.25) * np.minimum(x2, p5) + c(0.1) * np.maximum(p5, x3)
                 + c(0.1) * np.minimum(x4, x5))                          # M
        g[0] = g[0] + c(0.25) * (x0 >= x1); g[1] = g[1] + c(0.25) * (x1 > x0)
        g[2] = g[2] + c(0.25) * (x2 <= p5); g[3] = g[3] + c(0.1) * (x3 > p5)
        g[4] = g[4] + c(0.1) * (x4 <= x5); g[5] = g[5] + c(0.1) * (x5 < x4)
        a, b = c(1) + x1 * x1, c(2) + np.cos(x2)                         # N
        q = c(0.25) * x0 / (a * b)
        s = s + q
        g[0] = g[0] + c(0.25) / (a * b); g[1] = g[1] - q * c(2) * x1 / a; g[2] = g[2] + q * np.sin(x2) / b
        b = c(2) + np.sin(x3)                                            # O
        s = s + c(1) / b; g[3] = g[3] - np.cos(x3) / (b * b)
        u = c(1) + x4 * x4                                               # P
        s = s - c(0.01) * u * np.sqrt(u); g[4] = g[4] - c(0.03) * x4 * np.sqrt(u)
        u = c(1) + x5 * x5                                               # Q
        v = np.power(u, c(0.5) * x0)
        s = s + c(0.05) * v
        g[0] = g[0] + c(0.05) * v * c(0.5) * np.log(u); g[5] = g[5] + c(0.05) * v * x0 * x5 / u
        s = s + c(0.1) * x5 * np.abs(x5); g[5] = g[5] + c(0.2) * np.abs(x5)    # R
        h = np.where(x0 < x1, x1 - x0, c(0))                             # S
        s = s + c(0.05) * h * h; g[0] = g[0] - c(0.1) * h; g[1] = g[1] + c(0.1) * h
        h = np.where(p5 <= x2, x2 - p5, c(0))                            # T
        s = s - c(0.05) * h * h; g[2] = g[2] - c(0.1) * h
        h = np.where(x3 >= x4, x3 - x4, c(0))                            # U
        s = s + c(0.05) * h * h; g[3] = g[3] + c(0.1) * h; g[4] = g[4] - c(0.1) * h
        s = s + p5 - c(0.25)
        return s.astype(dt), np.stack(g, axis=1).astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


SOURCES = {"rosenbrock": ROSENBROCK_SRC, "quartic": QUARTIC_SRC, "planar": PLANAR_SRC, "allops": ALLOPS_SRC}


def kernel_cases(w):
    """(name, D, N, routes) with route 0 auto, 1 staged, 2 direct; ``w`` the tangents per pass.  Rosenbrock: one partial pass
    and the 64-sample tile seams.  Quartic: a partial pass, one pass less one, exactly one, one and a partial one; two passes
    and two and a partial one; the cap of the staged route from both sides; a direct-only D."""
    return ([("rosenbrock", 2, n, (0,)) for n in (1, 63, 64, 65, 200)]
            + [("quartic", d, 70, (1, 2)) for d in (3, w - 1, w, w + 1)]
            + [("quartic", 50, 130, (1, 2)), ("quartic", 120, 130, (1, 2))]
            + [("quartic", 2 * w, 70, (0,)), ("quartic", 2 * w + 1, 70, (0,)), ("quartic", 121, 130, (0,)),
               ("quartic", 300, 90, (0,))]
            + [("planar", 10, 300, (0,)), ("allops", 6, 200, (0,))])


def build_case(name, d, n, seed=5):
    """-> (fp64 target, x [n, d] fp32): the inputs of custom_target_cases.build_case; allops on standard normal samples."""
    if name != "allops":
        return base.build_case(name, d, n, seed)
    rng = np.random.default_rng(seed + 1000 * d + n)
    return AllOps(), rng.normal(size=(n, 6)).astype(np.float32)


def fp32_twin(tgt):
    return tgt.as_dtype(np.float32) if isinstance(tgt, AllOps) else _base_fp32_twin(tgt)
