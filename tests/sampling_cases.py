"""Inputs, fp64 reference, error bounds and planted faults shared by test_hip_sampling.py (GPU), sampling_route_child.py and
test_sampling_cases_cpu.py: component-ordered sampling x = mu_k + L_k eps on its four routes -- the register route
(csrc/sample_block.h: the stand-alone launch of csrc/sampling.hip, extra blocks of that launch in the single-call iteration,
a rider of the expected-log-ratio launch, csrc/riders.h), the blocked contraction (gmmvi_blocked_sample, csrc/blocked.hip) and
the diagonal kernel (gmmvi_diag_sample, csrc/diag_sweep.hip).  Nothing here touches the device.

    reference(case)        fp64 x on the fp32-rounded means, factors and normals, and the mapping
    bound(case)            element-wise: 2 (D + 2) 2^-24 (|mu_i| + sum_j |L_ij| |eps_j|); one fp32 ulp of the reference on the
                           diagonal route
    philox_bound(case)     bound + sum_j |L_ij| (2e-5 |eps_j| + 2e-6): draws from the device's Philox stream against the oracle's
    evaluate_f32(case, o)  the same sums in NumPy float32, in two orders
    planted_faults(case)   [(name, argument, against)]: what a subtly wrong kernel would return, built from the reference

(D + 2) 2^-24 (...) is the standard bound for D fused multiply-adds, one bias add and the rounding of the result in any order of
summation (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_n with u = 2^-24).  The factor 2 covers the
internal accumulation of the matrix cores and the split-operand route of the blocked contraction, which drops terms below 2^-25
of a product (test_hip_blocked.py); both are documented, not derived here.  The diagonal kernel does ONE fmaf per element: a
correctly rounded result lies within half an ulp, the bound is one.  The second term of philox_bound is the tolerance
test_hip_kernels.test_philox_bits_and_normals grants the device's normals (rtol 2e-5, atol 2e-6), propagated through |L|.
None of these figures comes from a device run.
"""
import numpy as np

from oracle import philox
from weight_step_cases import f32

U32 = 2.0 ** -24
PHILOX_RTOL, PHILOX_ATOL = 2e-5, 2e-6                # test_hip_kernels.test_philox_bits_and_normals

ROUTES = ("register", "register64", "blocked", "diag")
# edges of the 16-row tile, the 64-sample wave and the 256-sample chunk of sample_block, three chunks, empty components in
# front, behind and next to one another: K = 15, N = 1522
REGISTER_COUNTS = (0, 1, 15, 16, 17, 0, 0, 63, 64, 65, 255, 256, 257, 513, 0)
# edges of the 128-row tile (BM) of the blocked contraction, three tiles: K = 8, N = 685
BLOCKED_COUNTS = (0, 1, 127, 128, 129, 0, 300, 0)
BLOCKED_BM = 128

# sample_block's scalar branch (DP < 32): both parities of the LDS row stride D | 1
REGISTER_SCALAR_DIMS = (1, 2, 3, 23, 24)
# its matrix-core branch: DP = 32, 40, 50 -- D == DP and D == previous DP + 1, ragged column tiles, a ragged last k-step
REGISTER_MFMA_DIMS = (25, 32, 33, 40, 41, 49, 50)
# GMMVI_BLOCKED_ABOVE=64: the DP = 64 instance (a child process, sampling_route_child.py)
REGISTER64_DIMS = (51, 52, 53, 63)
# default threshold: 51 ... 64 take the blocked route too; bgemm's split-operand route starts at 160 columns, 161 gives rows
# that are not 16-byte aligned
BLOCKED_DIMS = (51, 64, 65, 161)
# one thread per four values: one partly filled block, one full, one and a quarter, many
DIAG_DIMS = (1, 3, 4, 5, 33, 513)

SEED = 0x5EED0123456789AB                            # both halves of the Philox key in use
FIRST_INDEX = 1000
WRAP_HI = 3                                          # the wrapping cases pass 3 * 2^32 inside a component
# (route, D) -> in-component sample at which the low word of the Philox sample index becomes 0: inside the second chunk of
# the 513-sample component / the second row tile of the 300-sample component
WRAP_AT = {("register", 24): 300, ("register", 50): 300, ("register64", 63): 300, ("blocked", 65): 150, ("diag", 5): 300}
STREAM_2 = {("register", 41), ("register", 3), ("register64", 52), ("blocked", 161), ("diag", 33)}

# the twins of the single-call iteration (test_hip_sampling.py): (D, samples per component), K = 3 -- two chunks, the second
# with 44 or 4 samples
TWIN_SHAPES = ((24, 300), (32, 300), (41, 300), (50, 260))
TWIN_K = 3
TWIN64_SHAPE = (53, 300)                             # under GMMVI_BLOCKED_ABOVE=64


def padded_dim(d):
    """csrc/common.h gmmvi_padded_dim."""
    return next(dp for dp in (2, 4, 8, 10, 12, 16, 20, 24, 32, 40, 50, 64) if d <= dp)


def lds_bytes(d):
    """Dynamic LDS of a register-route launch: csrc/sampling.hip launch_sample, csrc/common.h riders_lds_bytes."""
    return (d * d + d + 256 * (d | 1)) * 4


def counts_of(route):
    return BLOCKED_COUNTS if route == "blocked" else REGISTER_COUNTS


def _spec(route, d):
    counts = counts_of(route)
    big = int(np.argmax(counts))
    first = FIRST_INDEX
    if (route, d) in WRAP_AT:
        first = (WRAP_HI << 32) - (int(np.sum(counts[:big])) + WRAP_AT[(route, d)])
    stream = 2 if (route, d) in STREAM_2 else 0
    tag = ("-wrap" if (route, d) in WRAP_AT else "") + ("-stream2" if stream else "")
    return dict(route=route, d=d, k=len(counts), n=int(np.sum(counts)), counts=counts, seed=SEED, first_index=first,
                stream_id=stream, id=f"{route}-D{d}{tag}")


def case_table():
    """The cases of the default process: register, blocked and diagonal routes."""
    return ([_spec("register", d) for d in REGISTER_SCALAR_DIMS + REGISTER_MFMA_DIMS] + [_spec("blocked", d) for d in BLOCKED_DIMS]
            + [_spec("diag", d) for d in DIAG_DIMS])


def register64_table():
    return [_spec("register64", d) for d in REGISTER64_DIMS]


def spec_by_id(case_id):
    return next(s for s in case_table() + register64_table() if s["id"] == case_id)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def random_factors(rng, k, d):
    """Means and Cholesky factors by the law of test_hip_kernels.random_gmm (means 3 N(0, 1), covariances A A^T / D + 0.3 I),
    rounded to fp32.  The factors are lower triangular with an exactly zero upper triangle: L and L^T differ everywhere off
    the diagonal."""
    means = f32(rng.normal(size=(k, d)) * 3.0)
    chols = np.empty((k, d, d))
    for i in range(k):
        a = rng.normal(size=(d, d))
        chols[i] = np.linalg.cholesky(a @ a.T / d + 0.3 * np.eye(d))
    return means, f32(chols)


def make_case(spec):
    """-> dict of fp32-representable fp64 arrays: means [K, D], chols [K, D, D] (sigma [K, D] on the diagonal route), eps [N, D]
    = the oracle's Philox normals of (seed, first_index, stream_id) rounded to fp32; offsets [K + 1] int32."""
    route, d, k, n = spec["route"], spec["d"], spec["k"], spec["n"]
    rng = np.random.default_rng([ROUTES.index(route), d, 77])
    case = dict(spec)
    if route == "diag":
        # the law of diag_highd_cases.random_diag_gmm
        case.update(means=f32(rng.normal(size=(k, d)) * 3.0), sigma=f32(np.sqrt(rng.uniform(0.3, 3.0, size=(k, d)))))
    else:
        means, chols = random_factors(rng, k, d)
        case.update(means=means, chols=chols)
    case["offsets"] = np.concatenate([[0], np.cumsum(spec["counts"])]).astype(np.int32)
    case["eps"] = f32(philox.normals(spec["seed"], spec["first_index"], n, d, spec["stream_id"]))
    return case


def mapping_of(case):
    return np.repeat(np.arange(case["k"], dtype=np.int32), case["counts"])


def _apply(case, eps, means=None, factors=None, absolute=False):
    """mu_k + L_k eps (mu_k + sigma_k eps) per component in fp64; ``absolute``: every term replaced by its absolute value."""
    diag = case["route"] == "diag"
    means = case["means"] if means is None else means
    fac = (case["sigma"] if diag else case["chols"]) if factors is None else factors
    if absolute:
        means, fac, eps = np.abs(means), np.abs(fac), np.abs(eps)
    x = np.empty((case["n"], case["d"]))
    off = case["offsets"]
    for i in range(case["k"]):
        e = eps[off[i]:off[i + 1]]
        x[off[i]:off[i + 1]] = means[i] + (fac[i] * e if diag else e @ fac[i].T)
    return x


def reference(case, eps=None):
    """-> (x [N, D] fp64, mapping [N] int32) on the case's fp32-rounded inputs (``eps``: other normals, also fp32-rounded)."""
    return _apply(case, case["eps"] if eps is None else eps), mapping_of(case)


def bound(case, eps=None):
    eps = case["eps"] if eps is None else eps
    if case["route"] == "diag":
        return np.spacing(np.abs(_apply(case, eps)).astype(np.float32)).astype(np.float64)
    return 2.0 * (case["d"] + 2) * U32 * _apply(case, eps, absolute=True)


def philox_bound(case):
    """For draws made from the device's own stream, compared with the reference on the oracle's normals."""
    slack = PHILOX_RTOL * np.abs(case["eps"]) + PHILOX_ATOL
    return bound(case) + _apply(case, slack, means=np.zeros_like(case["means"]), absolute=True)


def excess(x, ref, bnd):
    """max |x - ref| / bound: the GPU test asserts that this is at most 1 (inf where x is not finite)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(np.asarray(x, np.float64) - ref) / bnd
    return float(np.max(np.where(np.isnan(q), np.inf, q))) if q.size else 0.0


def evaluate_f32(case, order):
    """The sums in NumPy float32 (a rounding after every product and every sum).  order "mean_first_ascending": v = mu, then
    j = 0 ... D - 1; "mean_last_descending": v = 0, j = D - 1 ... 0, then + mu.  The diagonal route has one product and one sum:
    as the kernel's fmaf, the exact result rounded once (the product of two fp32 numbers is exact in fp64)."""
    if case["route"] == "diag":
        return reference(case)[0].astype(np.float32).astype(np.float64)
    d, off = case["d"], case["offsets"]
    x = np.empty((case["n"], d), np.float32)
    mu, lo, eps = case["means"].astype(np.float32), case["chols"].astype(np.float32), case["eps"].astype(np.float32)
    for i in range(case["k"]):
        e = eps[off[i]:off[i + 1]]
        if order == "mean_first_ascending":
            v = np.broadcast_to(mu[i], e.shape).copy()
            for j in range(d):
                v += e[:, j:j + 1] * lo[i][None, :, j]
        else:
            v = np.zeros(e.shape, np.float32)
            for j in range(d - 1, -1, -1):
                v += e[:, j:j + 1] * lo[i][None, :, j]
            v += mu[i]
        x[off[i]:off[i + 1]] = v
    return x.astype(np.float64)


# ---- planted faults ------------------------------------------------------------------------------------------------------------
def seam_samples(case):
    """{name: in-component index} of the first sample of a row tile, a wave and a chunk (of the second 128-row tile on the
    blocked route)."""
    return {"row_tile": BLOCKED_BM} if case["route"] == "blocked" else {"row_tile": 16, "wave": 64, "chunk": 256}


def planted_faults(case):
    """[(name, argument, against)]: ``against`` is "eps" for results the supplied-eps assertion (bound) must reject and "philox"
    for results the device-stream assertion (philox_bound) must reject --
    drop_corner_term       the L[D - 1, 0] eps_0 term left out
    transposed             L read transposed
    stale_eps s            the first sample of a row tile / wave / chunk computed from the previous sample's normals
    next_mean              the last sample of every component centred on the next component's mean
    philox_index           the Philox sample index off by one
    philox_ragged_block    the ragged last block of four normals taken from block 0"""
    d, full = case["d"], case["route"] != "diag"
    faults = []
    if full and d >= 2:
        faults += [("drop_corner_term", None, "eps"), ("transposed", None, "eps")]
    faults += [("stale_eps", s, "eps") for s in seam_samples(case)]
    faults += [("next_mean", None, "eps"), ("philox_index", None, "philox")]
    if d % 4 and d > 4:
        faults.append(("philox_ragged_block", None, "philox"))
    return faults


def faulty(case, fault):
    """The "device result" of a kernel that is wrong in the named way."""
    name, arg, _ = fault
    x, mapping = reference(case)
    d, off, counts = case["d"], case["offsets"], np.asarray(case["counts"])
    if name == "drop_corner_term":
        return x - np.pad((case["chols"][mapping, d - 1, 0] * case["eps"][:, 0])[:, None], ((0, 0), (d - 1, 0)))
    if name == "transposed":
        return _apply(case, case["eps"], factors=np.swapaxes(case["chols"], 1, 2))
    if name == "stale_eps":
        eps = case["eps"].copy()
        at = seam_samples(case)[arg]
        rows = [off[i] + at for i in range(case["k"]) if counts[i] > at]
        assert rows
        eps[rows] = case["eps"][np.asarray(rows) - 1]
        return _apply(case, eps)
    if name == "next_mean":
        last = [off[i + 1] - 1 for i in range(case["k"] - 1) if counts[i] > 0]
        x[last] += case["means"][mapping[last] + 1] - case["means"][mapping[last]]
        return x
    if name == "philox_index":
        return _apply(case, f32(philox.normals(case["seed"], case["first_index"] + 1, case["n"], d, case["stream_id"])))
    if name == "philox_ragged_block":
        eps = case["eps"].copy()
        eps[:, d - d % 4:] = eps[:, :d % 4]
        return _apply(case, eps)
    raise ValueError(name)


# ---- the twins of the single-call iteration ------------------------------------------------------------------------------------
def twin_reference(means, chols, seed, first_index, per_component):
    """First-iteration draw of the single-call iteration from the initial components: K * per_component samples in component
    order, Philox stream 0 from ``first_index`` -> (case dict for bound / philox_bound, x fp64, component indices)."""
    k, d = means.shape
    counts = (per_component,) * k
    case = dict(route="register", d=d, k=k, n=k * per_component, counts=counts, seed=seed, first_index=first_index, stream_id=0,
                means=f32(means), chols=f32(chols), offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    case["eps"] = f32(philox.normals(seed, first_index, case["n"], d, 0))
    x, mapping = reference(case)
    return case, x, mapping
