"""User-defined device targets differentiated on a tape (csrc/custom_target_tape.inc, DeviceTapeLNPDF): the test targets and the
NumPy restatements they are checked against.  The sources of tests/custom_autodiff_cases.py run here unchanged (the tape mode
takes the text of the forward mode); two more are added.  ``chain`` couples neighbouring dimensions, so its tape grows as O(D)
and its gradient cannot be had coordinate by coordinate; it runs far above the forward mode's cap.  ``branchy`` loops a number of
times that depends on the sign of x[0], so the lanes of one wave record tapes of different lengths."""
import numpy as np

import custom_autodiff_cases as auto
from custom_autodiff_cases import AllOps, Planar, Quartic, Rosenbrock  # noqa: F401

# ---- chain: lp = -1/2 sum_i x_i^2 / sigma^2 - c sum_{i < D - 1} (x_{i+1} - x_i^2)^2; params = [sigma, c] ------------------------
CHAIN_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float inv_var = 1.f / (params[0] * params[0]), c = params[1];
    T q = 0.f, r = 0.f;
    for (int i = 0; i < D; ++i) {
        const T t = x[i] * x[i];
        q += t;
        if (i + 1 < D) {
            const T d = x[i + 1] - t;
            r += d * d;
        }
    }
    return -0.5f * inv_var * q - c * r;
}
"""


def _running_sum(terms, dt):
    """The last entry of the running sum along axis 1 in ``dt``: the order and the roundings of ``s += term`` in a loop (NumPy's
    sum adds pairwise, which an fp32 loop does not)."""
    if terms.shape[1] == 0:
        return np.zeros(terms.shape[0], dt)
    return np.cumsum(terms, axis=1, dtype=dt)[:, -1]


class Chain:
    def __init__(self, d, sigma=2.0, c=0.5, dtype=np.float64):
        self.d, self.sigma, self.c, self.dtype = int(d), float(sigma), float(c), dtype

    def as_dtype(self, dtype):
        return Chain(self.d, self.sigma, self.c, dtype)

    def params(self):
        return np.array([self.sigma, self.c], np.float32)

    def get_num_dimensions(self):
        return self.d

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        sigma, c = dt(np.float32(self.sigma)), dt(np.float32(self.c))
        inv_var = dt(1) / (sigma * sigma)
        t = x * x
        d = x[:, 1:] - t[:, :-1]
        lp = dt(-0.5) * inv_var * _running_sum(t, dt) - c * _running_sum(d * d, dt)
        g = -inv_var * x
        g[:, 1:] = g[:, 1:] - dt(2) * c * d
        g[:, :-1] = g[:, :-1] + dt(4) * c * d * x[:, :-1]
        return lp.astype(dt), g.astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


# ---- branchy: D = 4; the loop runs 9 times where x[0] > 0 and twice elsewhere ---------------------------------------------------
BRANCHY_LONG, BRANCHY_SHORT = 9, 2
BRANCHY_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const int trips = x[0] > 0.f ? 9 : 2;
    T s = -0.5f * x[0] * x[0];
    for (int k = 0; k < trips; ++k) {
        const T u = x[k % D] * (0.5f + 0.25f * k);
        s -= 0.1f * u * u + 0.05f * cos(u);
    }
    return s;
}
"""


class Branchy:
    def __init__(self, dtype=np.float64):
        self.dtype = dtype

    def as_dtype(self, dtype):
        return Branchy(dtype)

    def params(self):
        return np.zeros(1, np.float32)

    def get_num_dimensions(self):
        return 4

    def log_density_and_grad(self, x):
        dt = self.dtype
        x = np.asarray(x, dt)
        trips = np.where(x[:, 0] > 0, BRANCHY_LONG, BRANCHY_SHORT)
        s = dt(-0.5) * x[:, 0] * x[:, 0]
        g = np.zeros_like(x)
        g[:, 0] = -x[:, 0]
        c1, c2 = dt(np.float32(0.1)), dt(np.float32(0.05))         # the constants as the device's fp32 literals hold them
        for k in range(BRANCHY_LONG):
            on = (k < trips).astype(dt)
            a = dt(np.float32(0.5) + np.float32(0.25) * np.float32(k))
            u = x[:, k % 4] * a
            s = s - on * (c1 * u * u + c2 * np.cos(u))
            g[:, k % 4] = g[:, k % 4] - on * a * (dt(2) * c1 * u - c2 * np.sin(u))
        return s.astype(dt), g.astype(dt)

    def log_density(self, x):
        return self.log_density_and_grad(x)[0]


SOURCES = dict(auto.SOURCES, chain=CHAIN_SRC, branchy=BRANCHY_SRC)

MAX_DIM = 131072

# (name, D, N): the table of the feature's issue.  Rosenbrock: the seams of the 64-lane wave.  Quartic: the pass-width and
# staged-cap dimensions of the forward mode's tests.  Planar, allops: branches, lane-dependent ones included.  Branchy: tape
# lengths differ inside a wave.  Chain: the smallest D, one above the forward mode's cap of 512, and eight times the cap.
KERNEL_CASES = ([("rosenbrock", 2, n) for n in (1, 63, 64, 65, 200)]
                + [("quartic", d, 70) for d in (3, 15, 16, 17, 50, 120)]
                + [("planar", 10, 300), ("allops", 6, 200), ("branchy", 4, 130)]
                + [("chain", d, 70) for d in (2, 513, 4096)])
MAX_DIM_CASE = ("chain", MAX_DIM, 2)


def build_case(name, d, n, seed=5):
    """-> (fp64 target, x [n, d] fp32).  The cases of custom_autodiff_cases on their own inputs; chain on samples of standard
    deviation 0.7 (x_i^2 and x_{i+1} of the same size); branchy on standard normal samples, both signs of x[0] in every wave."""
    if name == "chain":
        rng = np.random.default_rng(seed + 1000 * (d % 1000) + n)
        return Chain(d), (0.7 * rng.normal(size=(n, d))).astype(np.float32)
    if name == "branchy":
        rng = np.random.default_rng(seed + 4000 + n)
        x = rng.normal(size=(n, 4)).astype(np.float32)
        x[:, 0] = np.abs(x[:, 0]) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)      # every third sample takes the short loop
        return Branchy(), x
    return auto.build_case(name, d, n, seed)


def fp32_twin(tgt):
    return tgt.as_dtype(np.float32) if isinstance(tgt, (Chain, Branchy)) else auto.fp32_twin(tgt)
