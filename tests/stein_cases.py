"""Inputs, fp64 reference, error scale and planted faults shared by test_hip_stein.py (GPU), stein_route_child.py and
test_stein_cases_cpu.py: the three device implementations of the Stein estimate (csrc/stein.hip + stein_finalize.h,
gmmvi_blocked_stein in csrc/blocked.hip, diag_stein_kernel in csrc/diag_sweep.hip) on THEIR OWN inputs.  Nothing here touches
the device.

The entry points read x, grad log p~, grad log q, ld, bg and the mapping as plain arrays; so do the per-component functions of
oracle/stein.py.  Every array of a case is fp32-representable fp64 (f32()), ld and bg are built directly (no mixture is
evaluated), so the device and the reference read the same numbers and the log weights a = ld - bg can be shaped freely.

    reference(case, snis)       fp64, built on oracle/stein.py's per-component functions
    abs_bound(case, snis)       the same sums with every term replaced by its absolute value: the element-wise magnitude B that
                                fp32 rounding errors scale with
    reference_f32(case, snis)   the same formulas in NumPy float32 throughout
    planted_faults(case, snis)  fp64 variants that are wrong in one way a kernel could be wrong

The GPU test asserts |device - reference| <= C * EPS32 * B element-wise.  C is not tuned on the device: it is 8 times the
largest |reference_f32 - reference| / (EPS32 * B) over the case table (the device sums in another order -- N / (4 R) samples per
wave, four waves, R partials -- and uses the fast exponential).  Measured on the table below (test_stein_cases_cpu.py asserts
that no case exceeds its route's figure, and that every planted fault moves some element by 10 C EPS32 B or more):

    route        largest |f32 - fp64| / (EPS32 B)      where
    register     15.3 -> RATIO_F32 = 16                D = 50, K = 3, N = 300, wide weights, plain importance weights
                 (12.2 in the DP = 64 instance: D = 63, K = 3, N = 1025, wide weights)
    blocked      10.1 -> RATIO_F32 = 11                D = 64, K = 3, N = 1025, wide weights, self-normalised
    diag         14.0 -> RATIO_F32 = 14                D = 600, K = 5, N = 1025, wide weights, plain importance weights
    C = 8 * 16 = 128
(with a ~ N(0, 1) no case exceeds 4.3: the wide cases lose their bits in ld - bg, a difference of up to 60 rounded to fp32
before the exponential.  The figures are rounded up to the next integer: the float32 matrix products may be summed in another
order on another host.)  The smallest shift of a planted fault over the table is 1.7e4 EPS32 B (one seam sample of 3841 left out).
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import stein as ostein
import diag_highd_cases
from weight_step_cases import f32

EPS32 = float(np.finfo(np.float32).eps)
RATIO_F32 = {"register": 16.0, "blocked": 11.0, "diag": 14.0}
C = 8.0 * max(RATIO_F32.values())
FAULT_FACTOR = 10.0                      # every planted fault moves some element by at least FAULT_FACTOR * C * EPS32 * B

ROUTES = ("register", "register64", "blocked", "diag")
KINDS = ("normal", "wide", "neginf", "own")
MAP_BASE = 7                             # the mapping holds data-base indices: component + MAP_BASE, map_offset = -MAP_BASE


# ---- the dispatch arithmetic of the kernels, restated (the seams below are placed by it) -----------------------------------------
PADDED_DIMS = (2, 4, 8, 10, 12, 16, 20, 24, 32, 40, 50, 64)


def padded_dim(d):
    return next(dp for dp in PADDED_DIMS if d <= dp)


def stein_tile(dp):
    """csrc/stein_tile.h SteinTile<DP> -> (MT row tiles, NT column tiles, NB components per stack)."""
    d1 = min(dp + 1, 64)
    mt = (d1 + 15) // 16
    best, best_num, best_den = 1, 0, 1
    for nt in range(1, (6 if mt <= 3 else 7) + 1):
        nb = min(16 * nt // d1, 5)
        if nb >= 1 and nb * d1 * best_den > best_num * 16 * nt:
            best, best_num, best_den = nt, nb * d1, 16 * nt
    return mt, best, min(16 * best // d1, 5)


def register_geometry(d, k, n, num_cus=256):
    """csrc/stein.hip launch_stein_moment -> dict(MT, NB, stacks, R0 = resident workgroups per stack before the clamps, R =
    partials per component, wave_range = samples per wave)."""
    mt, _, nb = stein_tile(padded_dim(d))
    stacks = (k + nb - 1) // nb
    r0 = (2 if mt == 1 else 1) * num_cus // stacks
    r = max(1, min(r0, (n + 255) // 256))
    wave_range = (((n + r - 1) // r + 3) // 4 + 3) // 4 * 4
    return dict(MT=mt, NB=nb, stacks=stacks, R0=r0, R=(n + 4 * wave_range - 1) // (4 * wave_range), wave_range=wave_range)


def n_for_partials(r, d, num_cus=256):
    """The smallest N of the form 256 (R - 1) + 1 at which one stack (K = 1) is summed from exactly R partials, or None."""
    n = 256 * (r - 1) + 1
    return n if register_geometry(d, 1, n, num_cus)["R"] == r else None


def blocked_geometry(d, n):
    """csrc/blocked.hip gmmvi_blocked_stein -> dict(LP = row stride of the augmented matrices, split = bgemm_use_split(LP, N) of
    the contraction over the samples, S = sample ranges of the f32 route, split_dd = the route of the two D x D x D products)."""
    lp = (d + 1 + 3) // 4 * 4
    return dict(LP=lp, split=lp >= 160 or n >= 512, S=max(1, min(n // 256, 16)), split_dd=d >= 160)


# ---- the case table --------------------------------------------------------------------------------------------------------------
def _spec(route, d, k, n, kind="normal", tag=""):
    return dict(route=route, d=d, k=k, n=n, kind=kind, id=f"{route}-{tag + '-' if tag else ''}D{d}-K{k}-N{n}-{kind}")


# every padded class at D == DP (vector loads) and D == PREV + 1 (scalar instance); K = 7 leaves the last stack partly filled for
# every NB > 1 (NB = 5, 3, 5, 4, 1, 5, 3, 3, 2, 1, 2 for DP = 2 ... 50; 7 % NB = 2, 1, 2, 3, 0, 2, 1, 1, 1, 0, 1)
REGISTER_CLASS_DIMS = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 24, 25, 32, 33, 40, 41, 50)
# K = 3 is one stack at D = 3 and 20 (NB = 3) and two stacks, the second half filled, at D = 50 (NB = 2); the wave range is
# ceil4(ceil(ceil(N / R) / 4)):
# N = 1: one wave with one sample, three empty; 3, 4, 5: wave_range 4, the second wave empty / holding one sample; 63 ... 65:
# wave_range 16 / 16 / 20, a last 16-sample block with 15 / 16 / 5 samples; 255 ... 257: R = 1, 1, 2 (wave_range 64, 64, 36);
# 1023, 1025: R = 4, 5 (wave_range 64, 52: every wave ends in a partly filled block)
REGISTER_SEAM_NS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
# R partials of one stack: eight interleaved chains in stein_slab_sum (R = 8, 16: no tail; 1, 7, 9, 17: the clamped tail alone /
# after one / two rounds).  N = 256 (R - 1) + 1 with 256 compute units; the GPU test recomputes N from the device
PARTIAL_COUNTS = (1, 7, 8, 9, 16, 17)
# 520 and 267 stacks: R0 = 512 / 520 = 0 and 256 / 267 = 0, bumped to 1
MANY_STACKS = ((2, 2600, 40), (20, 800, 64))
# LP = ceil4(D + 1): 52, 64 | 68, 68 | 128 | 132, 132 (a second 128-row tile) | 516; S = min(N / 256, 16) = 1, 1, 1, 2, 2 (16 at
# N = 4097); bgemm_use_split(LP, N): LP >= 160 or N >= 512 -- N = 511 | 512 at every D, and LP = 156 | 160 at D = 155 | 156
BLOCKED_DIMS = (51, 63, 64, 65, 127, 128, 129, 512)
BLOCKED_NS = (255, 256, 511, 512, 513)
# 4-component groups (K = 1, 4, 5: a quarter group, a full one, one and a quarter), 16-dimension pieces (D = 15, 16, 17), 256
# threads striding over the samples (N = 255, 256, 257, 1025)
DIAG_DIMS = (1, 15, 16, 17, 600)
DIAG_NS = (1, 255, 256, 257, 1025)
# the weight shapes "wide", "neginf" and "own" run at these shapes of every route (own needs K >= 3; from N = 769 on a whole
# 256-sample range holds no seam sample, so that under "wide" its maximum lies tens of nats below the others)
SHAPED = {"register": ((4, 7, 1023), (20, 7, 1025), (50, 3, 300)), "blocked": ((64, 3, 1025), (129, 3, 512)),
          "diag": ((17, 5, 257), (600, 5, 1025))}
# GMMVI_BLOCKED_ABOVE=64: the DP = 64 instance of the register route (a child process, stein_route_child.py)
REGISTER64 = ((51, 3, 130, "normal"), (63, 3, 130, "normal"), (51, 3, 1025, "normal"), (63, 3, 1025, "wide"), (63, 3, 300, "own"))


def case_table():
    t = []
    t += [_spec("register", d, 7, 130, tag="class") for d in REGISTER_CLASS_DIMS]
    t += [_spec("register", d, 3, n, tag="seam") for d in (3, 20, 50) for n in REGISTER_SEAM_NS]
    t += [_spec("register", d, 1, 256 * (r - 1) + 1, tag=f"R{r}") for d in (4, 20) for r in PARTIAL_COUNTS]
    t += [_spec("register", d, k, n, tag="stacks") for d, k, n in MANY_STACKS]
    t += [_spec("blocked", d, k, n) for d in BLOCKED_DIMS for k in (1, 3) for n in BLOCKED_NS]
    t += [_spec("blocked", 64, 1, 4097), _spec("blocked", 155, 1, 256, tag="f32"), _spec("blocked", 156, 1, 256, tag="split")]
    t += [_spec("diag", d, k, n) for d in DIAG_DIMS for k in (1, 4, 5) for n in DIAG_NS]
    t += [_spec("diag", 131072, k, 8) for k in (1, 4, 5)]
    for route, shapes in SHAPED.items():
        t += [_spec(route, d, k, n, kind, tag="shape") for d, k, n in shapes for kind in KINDS[1:]]
    return t


def register64_table():
    return [_spec("register64", d, k, n, kind) for d, k, n, kind in REGISTER64]


def spec_by_id(case_id):
    return next(s for s in case_table() + register64_table() if s["id"] == case_id)


def modes(spec):
    """(self-normalised?) for the case: both weightings, always."""
    return (True, False)


def seam_indices(spec, n=None):
    """Sample indices at which the kernels change hands: the 64-sample chunk, the 256-sample range / thread stride, the last
    sample, and on the register route the end of the first wave and of the first workgroup's range."""
    n = spec["n"] if n is None else n
    s = {0, 63, 64, 255, 256, n - 1}
    if spec["route"] in ("register", "register64"):
        wr = register_geometry(spec["d"], spec["k"], n)["wave_range"]
        s |= {wr - 1, wr, 4 * wr - 1, 4 * wr}
    return sorted(i for i in s if 0 <= i < n)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_case(spec, n=None):
    """-> dict of fp32-representable fp64 arrays: means [K, D], chols [K, D, D] (sigma [K, D] on the diagonal route), x, tgrad,
    qgrad [N, D], ld [K, N], bg [N], mapping [N] int32, map_offset; own (bool), seams.  ``n`` overrides the table's N (the
    partial-count cases on a device with another number of compute units)."""
    route, d, k, kind = spec["route"], spec["d"], spec["k"], spec["kind"]
    n = spec["n"] if n is None else n
    rng = np.random.default_rng([ROUTES.index(route), KINDS.index(kind), d, k, n])
    case = dict(spec, n=n, own=kind == "own")
    comp = rng.integers(0, k, size=n)
    if route == "diag":
        m = diag_highd_cases.random_diag_gmm(rng, k, d)
        means, sigma = f32(m.means), f32(m.chol_cov)
        case.update(means=means, sigma=sigma)
        x = means[comp] + sigma[comp] * rng.normal(size=(n, d))
    else:
        # the law of test_hip_kernels.random_gmm: means 3 N(0, 1), covariances A A^T / D + 0.3 I
        means = f32(rng.normal(size=(k, d)) * 3.0)
        chols = np.empty((k, d, d))
        for i in range(k):
            a = rng.normal(size=(d, d))
            chols[i] = np.linalg.cholesky(a @ a.T / d + 0.3 * np.eye(d))
        chols = f32(chols)
        case.update(means=means, chols=chols)
        x = means[comp] + np.einsum("nij,nj->ni", chols[comp], rng.normal(size=(n, d))) if n * d * d < 1 << 24 else \
            means[comp] + np.stack([chols[c] @ e for c, e in zip(comp, rng.normal(size=(n, d)))])
    seams = seam_indices(spec, n)
    a = rng.normal(size=(k, n))
    a[:, seams] = 3.0 + 0.5 * rng.normal(size=(k, len(seams)))                     # the seam samples carry real weight
    if kind == "wide":
        # [-120, 60]: the weight sits on the seam samples (within three nats of 60), a twentieth of the others lies 10 ... 40
        # nats below, the rest 90 ... 180 nats below -- chunks and ranges without a seam sample have maxima tens of nats down
        a = rng.uniform(-120.0, -30.0, size=(k, n))
        mid = rng.random((k, n)) < 0.05
        a[mid] = rng.uniform(20.0, 50.0, size=int(mid.sum()))
        a[:, seams] = 60.0 - rng.uniform(0.0, 3.0, size=(k, len(seams)))
        a[:, seams[0]] = 60.0
        if n > 1:
            a[0, rng.integers(0, n)] = -120.0
    bg = f32(rng.normal(size=n) * 2.0 - 12.0)
    ld = f32(a + bg[None, :])
    if kind == "neginf":
        dead = rng.random(n) < 1.0 / 3.0
        dead[seams] = False
        ld[k // 2, dead] = -np.inf
    mapping = comp.copy()
    if kind == "own":
        # component 1 has no sample, component K - 1 only row N - 1, the others share the rest
        others = [c for c in range(k) if c not in (1, k - 1)]
        mapping = np.asarray(others)[rng.integers(0, len(others), size=n)]
        mapping[n - 1] = k - 1
    case.update(x=f32(x), tgrad=f32(rng.normal(size=(n, d)) * 2.0), qgrad=f32(rng.normal(size=(n, d)) * 2.0), ld=ld, bg=bg,
                mapping=(mapping + MAP_BASE).astype(np.int32), map_offset=-MAP_BASE, seams=seams)
    return case


def log_weights(case, dtype=np.float64):
    """[K, N]: ld - bg, or over the own samples 0 and -inf elsewhere (the kernels' own form)."""
    if case["own"]:
        mine = (case["mapping"] + case["map_offset"])[None, :] == np.arange(case["k"])[:, None]
        return np.where(mine, 0.0, -np.inf).astype(dtype)
    with np.errstate(invalid="ignore"):
        return case["ld"].astype(dtype) - case["bg"].astype(dtype)[None, :]


# ---- the reference: oracle/stein.py per component ----------------------------------------------------------------------------------
# the plain estimator of the oracle forms an [n, D, D] array (and solves for all of y per call): it is called for blocks of rows
# of H of _BLOCK_ELEMS elements, and up to _ORACLE_PLAIN_ELEMS in all.  Beyond that (D = 512 from N = 64 on) the plain-weight
# reference is estimate() in fp64, which test_stein_cases_cpu.py holds to 1e-10 B of the oracle's functions on every smaller
# case, at these shapes under self-normalised weights (the same moments and solves), and once at D = 512 under plain weights
_BLOCK_ELEMS = 1 << 22
_ORACLE_PLAIN_ELEMS = 1 << 24


def reference(case, snis, force_oracle=False):
    """fp64 -> (H_neg [K, D, D] or [K, D], g_neg [K, D]) through expected_gradient_and_hessian_self_normalized / _standard of
    oracle/stein.py, fed as get_rewards_for_comp feeds them: all samples with (ld[k], bg), or the component's own samples with
    equal densities (log weights 0).  An empty own set gives zeros (self-normalised) or NaN (plain), csrc/stein_finalize.h."""
    k, d, n = case["k"], case["d"], case["n"]
    diag = case["route"] == "diag"
    if not snis and not diag and n * d * d > _ORACLE_PLAIN_ELEMS and not force_oracle:
        return estimate(case, snis)
    gr = case["tgrad"] - case["qgrad"]
    hs = np.empty((k, d) if diag else (k, d, d))
    gs = np.empty((k, d))
    rel = case["mapping"] + case["map_offset"]
    for i in range(k):
        idx = np.where(rel == i)[0] if case["own"] else np.arange(n)
        if idx.size == 0:
            hs[i], gs[i] = (0.0, 0.0) if snis else (np.nan, np.nan)
            continue
        cld, bgi = (np.zeros(idx.size), np.zeros(idx.size)) if case["own"] else (case["ld"][i], case["bg"])
        chol = case["sigma"][i] if diag else case["chols"][i]
        xs, gi = case["x"][idx], gr[idx]
        if snis:
            g, h = ostein.expected_gradient_and_hessian_self_normalized(chol, case["means"][i], cld, xs, bgi, gi)
        elif diag:
            g, h = ostein.expected_gradient_and_hessian_standard(chol, case["means"][i], cld, xs, bgi, gi)
        else:
            # row block r of H and of g only needs the columns r of the gradients
            step = max(1, _BLOCK_ELEMS // (idx.size * d))
            g, h = np.empty(d), np.empty((d, d))
            for r in range(0, d, step):
                g[r:r + step], h[r:r + step] = ostein.expected_gradient_and_hessian_standard(chol, case["means"][i], cld, xs, bgi,
                                                                                             gi[:, r:r + step])
        hs[i], gs[i] = -h, -g
    return hs, gs


# ---- the same formulas, written out: any dtype, absolute values, planted faults ----------------------------------------------------
def _tri_inverse_f32(chol):
    """L^-1 by forward substitution, float32 throughout."""
    d = chol.shape[0]
    lo = chol.astype(np.float32)
    inv = np.zeros((d, d), np.float32)
    for i in range(d):
        row = -(lo[i, :i] @ inv[:i, :]) if i else np.zeros(d, np.float32)
        row[i] += np.float32(1.0)
        inv[i] = row / lo[i, i]
    return inv


def _inverse_factors(case, dtype, absolute):
    key = "_linv32" if dtype == np.float32 else "_linv64"
    if key not in case:
        if dtype == np.float32:
            case[key] = np.stack([_tri_inverse_f32(c) for c in case["chols"]])
        else:
            case[key] = np.stack([solve_triangular(c, np.eye(case["d"]), lower=True) for c in case["chols"]])
    return np.abs(case[key]) if absolute else case[key]


def estimate(case, snis, dtype=np.float64, absolute=False, fault=None):
    """The estimate as the kernels form it -- weights exp(a - M) against the component's maximum, the moment sums
    sum w g (x - mu)^T and sum w g, Sigma^-1 = L^-T L^-1 from the right (1 / sigma^2 on the diagonal route), 1 / sum w or
    exp(M) / N, symmetrised under self-normalised weights -- in ``dtype`` throughout.  ``absolute``: every term replaced by its
    absolute value, not negated (abs_bound).  ``fault``: (name, argument) of planted_faults."""
    t = dtype
    k, d, n = case["k"], case["d"], case["n"]
    diag = case["route"] == "diag"
    name, arg = fault if fault else (None, None)
    a = log_weights(case, t).copy()
    if name == "drop_sample":
        a[:, arg] = -np.inf
    elif name == "drop_range":
        a[:, 256 * arg:256 * (arg + 1)] = -np.inf
    elif name == "chunk_not_rescaled":
        a[:, 64 * arg:64 * (arg + 1)] += t(1.0)
    means = case["means"].astype(t)
    if name == "neighbour_mean":
        means = np.roll(means, -1, axis=0)
    x = case["x"].astype(t)
    gr = case["tgrad"].astype(t) - case["qgrad"].astype(t)
    if absolute:
        gr = np.abs(gr)
    if diag:
        isq = t(1.0) / np.square(case["sigma"].astype(t))
    else:
        linv = _inverse_factors(case, t, absolute)
    hs = np.empty((k, d) if diag else (k, d, d), t)
    gs = np.empty((k, d), t)
    sign = t(1.0) if absolute else t(-1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(k):
            live = a[i] > -np.inf
            cnt = int(live.sum())
            if cnt == 0:
                hs[i], gs[i] = (0.0, 0.0) if snis or absolute else (np.nan, np.nan)
                continue
            m = a[i].max()
            w = np.exp(a[i] - m)
            dx = x - means[i]
            if absolute:
                dx = np.abs(dx)
            wg = w[:, None] * gr
            div = cnt if case["own"] else n
            if name == "divisor_all_samples":
                div = n
            elif name == "divisor_live_samples":
                div = cnt
            scale = t(1.0) / w.sum(dtype=t) if snis else np.exp(m) / t(div)
            gs[i] = sign * wg.sum(axis=0, dtype=t) * scale
            if diag:
                hs[i] = sign * (wg * dx).sum(axis=0, dtype=t) * scale * isq[i]
                continue
            h = ((wg.T @ dx) @ linv[i].T) @ linv[i]
            if snis != (name == "symmetrisation"):
                h = t(0.5) * (h + h.T)
            if name == "transposed":
                h = h.T
            hs[i] = sign * h * scale
    return hs, gs


def abs_bound(case, snis):
    """B: sum_n w_n |g_n| |x_n - mu|^T |L^-1|^T |L^-1| (|g| |x - mu| / sigma^2), symmetrised and scaled as the estimate is."""
    return estimate(case, snis, absolute=True)


def reference_f32(case, snis):
    h, g = estimate(case, snis, dtype=np.float32)
    return h.astype(np.float64), g.astype(np.float64)


def planted_faults(case, snis):
    """[(name, argument)]: what a subtly wrong kernel would compute, each applicable to this case and weighting --
    drop_sample i          the weighted sample at seam index i left out
    drop_range r           the 256 samples of range r left out
    chunk_not_rescaled c   the weights of 64-sample chunk c not referred to the common maximum (off by e)
    symmetrisation         none under self-normalised weights / one under plain weights
    transposed             the plain-weight Hessian in the other orientation
    neighbour_mean         centred on the next component's mean
    divisor_all_samples    N where the number of own samples is right
    divisor_live_samples   the number of samples with a finite weight where N is right (ld = -inf still counts)"""
    n, d, k = case["n"], case["d"], case["k"]
    full = case["route"] != "diag"
    faults = [("drop_sample", i) for i in case["seams"]]
    if n > 256:
        faults.append(("drop_range", 0))
    if n > 64:
        faults.append(("chunk_not_rescaled", 1))
    if full and d >= 2:
        faults.append(("symmetrisation", None))
        if not snis:
            faults.append(("transposed", None))
    if k >= 2:
        faults.append(("neighbour_mean", None))
    if case["own"] and not snis:
        faults.append(("divisor_all_samples", None))
    if case["kind"] == "neginf" and not snis:
        faults.append(("divisor_live_samples", None))
    return faults


def error_ratio(got, ref, bound):
    """max |got - ref| / (EPS32 B) over the elements with B > 0; elements with B == 0 (an empty own set) and non-finite
    reference values must agree exactly, else inf."""
    worst = 0.0
    for g, r, b in zip(got, ref, bound):
        g, r, b = np.asarray(g, np.float64), np.asarray(r, np.float64), np.asarray(b, np.float64)
        exact = (b == 0) | ~np.isfinite(r)
        same = (g == r) | (np.isnan(g) & np.isnan(r))
        if not np.all(same[exact]):
            return np.inf
        if np.any(~exact):
            with np.errstate(invalid="ignore"):
                q = np.abs(g - r)[~exact] / (EPS32 * b[~exact])
            worst = max(worst, float(np.max(np.where(np.isnan(q), np.inf, q))))
    return worst
