"""Predictive density of user-defined device targets summed over a data set (the predictive kernels of
csrc/custom_target_data.inc, gmmvi_custom_data_predictive, ``log_predictive`` / ``waic`` of the data targets): the sources, the
references and the cases.

With l[n, m] = row(x_n, rows[m]) the outputs per row m are
    lpd = log sum_n exp(l[n, m]) - log N,   mean = sum_n l[n, m] / N,   var = the unbiased variance of l[:, m] (0 for N = 1).
``reference64`` takes them straight from the fp64 matrix.  ``twin32`` follows the order include/gmmvi_hip.h states, rounded to
fp32 after each step: per tile of 64 samples the maximum, the sum of exp(l - shift) with shift = the maximum if finite else 0,
the sum of l over the tile's count and the centred sum of squares, each sum the pairwise tree of the xor butterfly; the tiles are
then merged in index order.  ``twin32`` can carry one planted fault (``FAULTS``): tests/test_custom_predictive_host.py shows that
each of them exceeds ten times the bound of the GPU test on the references alone.

Sources and restatements are those of tests/custom_data_cases.py plus ``affine``, row = row[0] * x[0] + row[1], which lets a
test place any l, including +-inf and NaN, through fp32 data."""
from collections import namedtuple

import numpy as np

import custom_data_cases as data_cases

F32 = np.float32

AFFINE_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    return row[0] * x[0] + row[1];
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    T q = 0.f;
    for (int i = 0; i < D; ++i) q += x[i] * x[i];
    return -0.5f * q;
}
"""

SOURCES = dict(data_cases.SOURCES, affine=AFFINE_SRC)

FAULTS = ("drop_last_tile", "duplicate_tail", "no_shift", "no_log_n", "naive_variance", "biased_variance")


class Affine(data_cases.DataTarget):
    def row_term(self, x, row):
        dt = self.dtype
        with np.errstate(all="ignore"):
            v = (dt(row[0]) * x[:, 0]).astype(dt) + dt(row[1])
        g = np.zeros(x.shape, dt)
        g[:, 0] = row[0]
        return v.astype(dt), g

    def prior(self, x):
        dt = self.dtype
        return (dt(-0.5) * np.sum(x * x, axis=1, dtype=dt)).astype(dt), (-x).astype(dt)


CLASSES = dict(data_cases.CLASSES, affine=Affine)


def row_terms(tgt, x, rows=None):
    """l [N, M] in the target's dtype: the row term of every sample on every row of ``rows`` (None: the target's data)."""
    dt = tgt.dtype
    x = np.asarray(x, dt)
    rows = tgt.data if rows is None else np.asarray(rows, np.float32)
    return np.stack([tgt.row_term(x, r.astype(dt))[0] for r in rows], axis=1).astype(dt)


def reference64(l):
    """-> (lpd, mean, var), each [M] fp64, straight from l [N, M]."""
    l = np.asarray(l, np.float64)
    n = l.shape[0]
    with np.errstate(all="ignore"):
        mx = np.max(l, axis=0)
        shift = np.where(np.isfinite(mx), mx, 0.0)
        lpd = shift + np.log(np.sum(np.exp(l - shift), axis=0)) - np.log(n)
        mean = np.mean(l, axis=0)
        var = np.var(l, axis=0, ddof=1) if n > 1 else np.zeros(l.shape[1])
    return lpd, mean, var


def _tree(v):
    """The sum an xor butterfly (1, 2, ..., 32) leaves in every lane: v [64, M] fp32 -> [M]."""
    while v.shape[0] > 1:
        v = (v[0::2] + v[1::2]).astype(F32)
    return v[0]


def _shift(mx):
    return np.where(np.isfinite(mx), mx, F32(0)).astype(F32)


def twin32(l, fault=None):
    """-> (lpd, mean, var), each [M] fp32, in the documented order; fault: None or one of FAULTS."""
    assert fault is None or fault in FAULTS
    l = np.asarray(l, F32)
    n, m = l.shape
    tiles = (n + 63) // 64
    parts = []
    with np.errstate(all="ignore"):
        for t in range(tiles):
            tile = l[64 * t:64 * (t + 1)]
            count = tile.shape[0]
            lanes = np.zeros((64, m), F32)
            lanes[:count] = tile
            valid = np.arange(64)[:, None] < count
            if fault == "duplicate_tail":                  # lanes past N repeat the tile's last sample and are not masked out
                lanes[count:] = tile[-1]
                valid = np.ones((64, 1), bool)
            mx = np.fmax.reduce(np.where(valid, lanes, F32(-np.inf)), axis=0).astype(F32)
            shift = np.zeros(m, F32) if fault == "no_shift" else _shift(mx)
            sumexp = _tree(np.where(valid, np.exp((lanes - shift).astype(F32)).astype(F32), F32(0)).astype(F32))
            mean = (_tree(np.where(valid, lanes, F32(0)).astype(F32)) / F32(count)).astype(F32)
            d = (lanes - mean).astype(F32)
            m2 = _tree(np.where(valid, (d * d).astype(F32), F32(0)).astype(F32))
            parts.append((mx, sumexp, mean, m2, count, shift))
        if fault == "drop_last_tile" and tiles > 1:
            parts = parts[:-1]
        mx, sumexp, mean, m2, done, shift = parts[0]
        for t_mx, t_sumexp, t_mean, t_m2, c, t_shift in parts[1:]:
            new_mx = np.fmax(mx, t_mx).astype(F32)
            new_shift = shift if fault == "no_shift" else _shift(new_mx)
            a = np.where(sumexp == 0, F32(0), sumexp * np.exp((shift - new_shift).astype(F32)).astype(F32)).astype(F32)
            b = np.where(t_sumexp == 0, F32(0), t_sumexp * np.exp((t_shift - new_shift).astype(F32)).astype(F32)).astype(F32)
            mx, shift, sumexp = new_mx, new_shift, (a + b).astype(F32)
            total = F32(done + c)
            delta = (t_mean - mean).astype(F32)
            mean = (mean + (delta * F32(c) / total).astype(F32)).astype(F32)
            m2 = (m2 + (t_m2 + (delta * delta * F32(done) * F32(c) / total).astype(F32)).astype(F32)).astype(F32)
            done += c
        lpd = (shift + np.log(sumexp).astype(F32)).astype(F32)
        if fault != "no_log_n":
            lpd = (lpd - np.log(F32(n))).astype(F32)
        if fault == "naive_variance":                      # sum l^2 - (sum l)^2 / N
            s1, s2 = np.zeros(m, F32), np.zeros(m, F32)
            for row in l:
                s1, s2 = (s1 + row).astype(F32), (s2 + (row * row).astype(F32)).astype(F32)
            m2 = (s2 - (s1 * s1 / F32(n)).astype(F32)).astype(F32)
        if n == 1:
            var = np.zeros(m, F32)
        else:
            var = (m2 / F32(n if fault == "biased_variance" else n - 1)).astype(F32)
    return lpd, mean.astype(F32), var


def compare(bound_fn, out, ref64, ref32):
    """One output [M] against its fp64 reference under the project's bound (``bound_fn``: _bound of
    tests/test_hip_custom_target.py) over the entries whose reference is finite -> (error, bound, ratio to the twin's error,
    whether the entries with a non-finite reference are exactly the reference's)."""
    out, ref64, ref32 = np.asarray(out), np.asarray(ref64), np.asarray(ref32)
    finite = np.isfinite(ref64)
    exact = bool(np.all((out[~finite] == ref64[~finite]) | (np.isnan(out[~finite]) & np.isnan(ref64[~finite]))))
    if not finite.any():
        return 0.0, 0.0, 0.0, exact
    with np.errstate(all="ignore"):
        e, b, r = bound_fn(out[finite], ref64[finite], ref32[finite])
    return e, b, r, exact


def within(e, b):
    """A NaN or infinite error (a non-finite output where the reference is finite) is outside every bound."""
    return bool(np.isfinite(e) and e <= b)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# name: the source; d, n: the samples' shape; m: the evaluation rows; chunks: the request (0 auto)
Case = namedtuple("Case", "name d n m chunks")


def case_id(c):
    return f"{c.name}-D{c.d}-N{c.n}-M{c.m}-chunks{c.chunks}"


def kernel_cases(staged_cap=120):
    """The smallest shapes at which the kernels can go wrong.  N: one lane, the 64-sample tile from both sides (the in-place
    finish against the merge kernel), three tiles with a ragged last one.  M: fewer rows than waves, one each, one wave with two;
    67 rows forced into 2 and 3 chunks; 257 rows on the automatic plan.  D: the staged route's cap from both sides."""
    return ([Case("logit", 5, n, 5, 0) for n in (1, 63, 64, 65, 130)]
            + [Case("student", 3, 65, m, 0) for m in (1, 3, 4)] + [Case("student", 3, 130, 5, 0)]
            + [Case(name, 5, 130, 67, k) for name in ("logit", "student") for k in (2, 3)]
            + [Case("logit", 5, 65, 257, 0), Case("student", 3, 130, 257, 0)]
            + [Case("logit", d, 65, 5, 0) for d in (staged_cap, staged_cap + 1)]
            + [Case("student", staged_cap + 1, 130, 4, 0)])


def build_case(c):
    """-> (fp64 target whose data are the evaluation rows, x [n, d] fp32), by the generator of tests/custom_data_cases.py."""
    return data_cases.build_case(data_cases.Case(c.name, c.d, c.n, c.m, 0, None, 0))


def build_affine(n, slope, offset, m=3, seed=17):
    """-> (fp64 Affine target, x [n, 2] fp32): rows m copies of (slope, offset) with offsets one apart, x[:, 0] ~ N(0, 1)."""
    rng = np.random.default_rng(seed + n)
    x = rng.normal(size=(n, 2)).astype(np.float32)
    rows = np.array([[slope, offset - j] for j in range(m)], np.float32)
    return Affine(rows, [0.0], d=2), x


def fault_cases():
    """The four cases of the planted-fault table: (tag, target, x)."""
    out = []
    for n in (65, 130):
        tgt, x = build_case(Case("logit", 5, n, 5, 0))
        out.append((f"logit-N{n}", tgt, x))
    out.append(("affine-30x-300", *build_affine(130, 30.0, -300.0)))
    out.append(("affine-0.1x-1000", *build_affine(130, 0.1, -1000.0)))
    return out


_refs = {}


def reference(key, tgt, x):
    """-> (l64, l32, (lpd, mean, var) fp64, (lpd, mean, var) of the fp32 twin), computed once per key and read-only."""
    if key not in _refs:
        l64 = row_terms(tgt, x.astype(np.float64))
        l32 = row_terms(data_cases.fp32_twin(tgt), x)
        ref, twin = reference64(l64), twin32(l32)
        for a in (l64, l32) + ref + twin:
            a.setflags(write=False)
        _refs[key] = (l64, l32, ref, twin)
    return _refs[key]


NAN, INF = float("nan"), float("inf")
Edge = namedtuple("Edge", "name x0 rows lpd")        # lpd: per row the exact value the rules fix, or None (finite: the bound)


def edge_cases(n=65):
    """l[n, m] = rows[m, 0] * x0[n] + rows[m, 1], through the affine source.  Every case has an ordinary last column next to
    the one that carries the edge value, where x0 allows one."""
    rng = np.random.default_rng(23)
    base = rng.normal(size=n).astype(np.float32)

    def x0(**at):
        v = base.copy()
        for k, value in at.items():
            v[int(k[1:])] = value
        return v

    only = lambda k: np.where(np.arange(n) == k, base, -np.inf).astype(np.float32)
    return [
        Edge("all -inf", base, [[0.0, -INF], [1.0, 0.5]], [-INF, None]),
        Edge("one finite entry", only(3), [[1.0, 2.0]], [None]),
        Edge("one finite entry in the second tile only", only(n - 1), [[1.0, 2.0]], [None]),
        Edge("+inf entry", x0(_7=INF), [[1.0, 0.0], [0.5, 1.0]], [INF, INF]),
        Edge("NaN in the first tile", x0(_5=NAN), [[1.0, 0.0]], [NAN]),
        Edge("NaN in the last valid lane of the last tile", x0(**{f"_{n - 1}": NAN}), [[1.0, 0.0]], [NAN]),
    ]


def edge_matrix(e, dtype=np.float64):
    """l [n, m] of an edge case in ``dtype``."""
    rows = np.asarray(e.rows, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        return ((rows[None, :, 0] * e.x0.astype(dtype)[:, None]).astype(dtype) + rows[None, :, 1]).astype(dtype)
