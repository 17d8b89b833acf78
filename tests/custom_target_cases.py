"""User-defined device targets (csrc/custom_target.hip, DeviceLNPDF): the sources of the test targets and NumPy restatements
of the same formulas.  Every restatement takes a dtype: float64 is the reference, float32 (the same operations rounded to
fp32 after each step) gives the scale of the error an fp32 evaluation of that formula carries on the same inputs."""
import numpy as np

# ---- Rosenbrock (examples/4 of upstream): D = 2, params = [a, b] -------------------------------------------------------------
ROSENBROCK_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    const float a = params[0], b = params[1];
    const float u = a - x[0];
    const float t = x[1] - x[0] * x[0];
    if (grad) {
        grad[0] = 2.f * u + 4.f * b * t * x[0];
        grad[1] = -2.f * b * t;
    }
    return -(u * u + b * t * t);
}
"""


class Rosenbrock:
    def __init__(self, a=1.0, b=100.0, dtype=np.float64):
        self.a, self.b, self.dtype = a, b, dtype

    def params(self):
        return np.array([self.a, self.b], np.float32)

    def get_num_dimensions(self):
        return 2

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        a, b = dt(self.a), dt(self.b)
        u = a - x[:, 0]
        t = x[:, 1] - x[:, 0] * x[:, 0]
        lp = -(u * u + b * t * t)
        g = np.stack([dt(2) * u + dt(4) * b * t * x[:, 0], dt(-2) * b * t], axis=1)
        return lp.astype(dt), g.astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


# ---- quadratic plus quartic: -1/2 (x - m)^T P (x - m) - c sum_i (x_i - m_i)^4 -----------------------------------------------
# params = [m (D) | lower triangle of P by rows (D (D + 1) / 2) | c]
QUARTIC_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    const float* m = params;
    const float* P = params + D;
    const float c = params[D + D * (D + 1) / 2];
    float lp = 0.f;
    for (int i = 0; i < D; ++i) {
        float s = 0.f;
        for (int j = 0; j < D; ++j) {
            const float pij = j <= i ? P[i * (i + 1) / 2 + j] : P[j * (j + 1) / 2 + i];
            s += pij * (x[j] - m[j]);
        }
        const float d = x[i] - m[i];
        const float d3 = d * d * d;
        lp -= 0.5f * d * s + c * d3 * d;
        if (grad) grad[i] = -s - 4.f * c * d3;
    }
    return lp;
}
"""


class Quartic:
    def __init__(self, m, P, c, dtype=np.float64):
        self.m, self.P, self.c, self.dtype = np.asarray(m, np.float64), np.asarray(P, np.float64), float(c), dtype

    @staticmethod
    def random(d, c, seed):
        rng = np.random.default_rng(seed)
        a = rng.normal(size=(d, d))
        P = a @ a.T / d + np.eye(d)
        # what the device sees is the fp32 rounding of the numbers: the references take exactly those
        return Quartic(rng.normal(size=d).astype(np.float32), ((P + P.T) / 2).astype(np.float32), c)

    def as_dtype(self, dtype):
        return Quartic(self.m, self.P, self.c, dtype)

    def params(self):
        d = self.m.shape[0]
        tri = np.concatenate([self.P[i, :i + 1] for i in range(d)])
        return np.concatenate([self.m, tri, [self.c]]).astype(np.float32)

    def get_num_dimensions(self):
        return self.m.shape[0]

    def log_density_and_grad(self, x):
        dt = self.dtype
        d = np.asarray(x, dt) - self.m.astype(dt)
        s = (d @ self.P.astype(dt)).astype(dt)
        d3 = d * d * d
        c = dt(self.c)
        lp = -np.sum(dt(0.5) * d * s + c * d3 * d, axis=1, dtype=dt)
        return lp.astype(dt), (-s - dt(4) * c * d3).astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


# ---- the planar n-link robot ("planar robot"; csrc/targets.hip is the built-in kernel) -------------------
# params = [prior_std (D) | likelihood_std | G | goals (2 G)], D <= 64
PLANAR_SRC = r"""
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    const float* prior_std = params;
    const float lik_std = params[D];
    const int G = (int)params[D + 1];
    const float* goals = params + D + 2;
    float sinc[64], cosc[64];
    float c = 0.f, px = 0.f, py = 0.f, prior = 0.f;
    for (int i = 0; i < D; ++i) {
        const float t = x[i];
        c += t;
        float s, co;
        sincosf(c, &s, &co);
        sinc[i] = s; cosc[i] = co;
        px += co; py += s;
        const float sd = prior_std[i];
        const float r = t / sd;
        prior += -0.5f * r * r - logf(sd);
    }
    prior -= 0.5f * D * 1.8378770664093453f;
    const float inv_var = 1.f / (lik_std * lik_std);
    float best = -3.0e38f, gx = 0.f, gy = 0.f;
    for (int g = 0; g < G; ++g) {
        const float dx = px - goals[2 * g], dy = py - goals[2 * g + 1];
        const float ll = -0.5f * (dx * dx + dy * dy) * inv_var - 2.f * logf(lik_std) - 1.8378770664093453f;
        if (ll > best) { best = ll; gx = dx; gy = dy; }
    }
    if (grad) {
        float ssum = 0.f, csum = 0.f;
        for (int j = D - 1; j >= 0; --j) {
            ssum += sinc[j]; csum += cosc[j];
            const float sd = prior_std[j];
            grad[j] = -x[j] / (sd * sd) - (gx * (-ssum) + gy * csum) * inv_var;
        }
    }
    return prior + best;
}
"""


class Planar:
    def __init__(self, num_links=10, prior_std=2e-1, likelihood_std=1e-2, dtype=np.float64):
        stds = prior_std * np.ones(num_links)
        stds[0] = 1.0
        self.prior_stds = stds.astype(np.float32)
        self.goals = np.array([[7., 0.], [-7., 0.], [0., 7.], [0., -7.]], np.float32)
        self.likelihood_std = np.float32(likelihood_std)
        self.dtype = dtype

    def as_dtype(self, dtype):
        p = Planar(self.prior_stds.shape[0], dtype=dtype)
        p.prior_stds, p.likelihood_std = self.prior_stds, self.likelihood_std
        return p

    def params(self):
        return np.concatenate([self.prior_stds, [self.likelihood_std, self.goals.shape[0]], self.goals.ravel()]).astype(np.float32)

    def get_num_dimensions(self):
        return self.prior_stds.shape[0]

    def log_density_and_grad(self, theta):
        dt = self.dtype
        theta = np.asarray(theta, dt)
        d = theta.shape[1]
        s = self.prior_stds.astype(dt)
        ls = dt(self.likelihood_std)
        log2pi = dt(1.8378770664093453)
        r = theta / s
        prior = np.sum(dt(-0.5) * r * r - np.log(s), axis=1, dtype=dt) - dt(0.5 * d) * log2pi
        c = np.cumsum(theta, axis=1, dtype=dt)
        sinc, cosc = np.sin(c), np.cos(c)
        px, py = cosc.sum(axis=1, dtype=dt), sinc.sum(axis=1, dtype=dt)
        dpx = -np.cumsum(sinc[:, ::-1], axis=1, dtype=dt)[:, ::-1]
        dpy = np.cumsum(cosc[:, ::-1], axis=1, dtype=dt)[:, ::-1]
        inv_var = dt(1) / (ls * ls)
        goals = self.goals.astype(dt)
        ll = np.stack([dt(-0.5) * ((px - g[0]) ** 2 + (py - g[1]) ** 2) * inv_var - dt(2) * np.log(ls) - log2pi for g in goals])
        best = np.argmax(ll, axis=0)
        g = goals[best]
        glik = -((px - g[:, 0])[:, None] * dpx + (py - g[:, 1])[:, None] * dpy) * inv_var
        return (prior + ll[best, np.arange(theta.shape[0])]).astype(dt), (-theta / (s * s) + glik).astype(dt)

    def log_density(self, theta):
        return self.log_density_and_grad(theta)[0]


SOURCES = {"rosenbrock": ROSENBROCK_SRC, "quartic": QUARTIC_SRC, "planar": PLANAR_SRC}

# ---- the kernel cases: (name, target, D, N, routes) with route 0 auto, 1 staged, 2 direct --------------------------------------
# Rosenbrock: the tile seams of the staged route (64 samples per workgroup).  Quartic: even D (row stride D + 1) and odd D
# (stride D), the cap of the staged route from both sides, a direct-only D.
KERNEL_CASES = (
    [("rosenbrock", 2, n, (0,)) for n in (1, 63, 64, 65, 200)]
    + [("quartic", 3, 70, (1, 2)), ("quartic", 50, 130, (1, 2)), ("quartic", 119, 130, (0,)), ("quartic", 120, 130, (1, 2)),
       ("quartic", 121, 130, (0,)), ("quartic", 300, 90, (0,)), ("planar", 10, 300, (0,))]
)


def build_case(name, d, n, seed=5):
    """-> (fp64 target, x [n, d] fp32)."""
    rng = np.random.default_rng(seed + 1000 * d + n)
    if name == "rosenbrock":
        tgt = Rosenbrock()
        x = rng.normal(size=(n, 2)) * np.array([1.5, 2.0])
    elif name == "quartic":
        tgt = Quartic.random(d, 0.05, seed)
        x = tgt.m + rng.normal(size=(n, d))
    else:
        tgt = Planar(d)
        x = rng.normal(size=(n, d)) * tgt.prior_stds
        x[: n // 2, 0] += np.pi / 2            # some samples near another goal: the argmax is exercised
    return tgt, x.astype(np.float32)


def fp32_twin(tgt):
    if isinstance(tgt, Rosenbrock):
        return Rosenbrock(tgt.a, tgt.b, np.float32)
    return tgt.as_dtype(np.float32)
