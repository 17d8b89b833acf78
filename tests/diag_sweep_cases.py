"""Inputs, fp64 reference, error scale and planted faults shared by test_hip_diag_sweep.py (GPU) and test_diag_sweep_cases_cpu.py:
the density sweep of diagonal-covariance mixtures, gmmvi_diag_mixture_eval (csrc/diag_sweep.hip: diag_eval_kernel<false>,
diag_eval_kernel<true> above D = 512, diag_grad_kernel, and the chunk merge of csrc/combine.h), ON ITS OWN INPUTS.  Nothing here
touches the device.

The sweep reads the component block [mu (D) | 1 / sigma (D) | 1 / sigma^2 (D) | log-normaliser | zeros], the log weights and x as
plain arrays.  make_case() builds the block on the host: the three derived vectors are computed in fp64 from the fp32 sigma and
rounded to fp32 once, so the device and the reference read the same numbers (gmmvi_diag_pack has its own test: pack_reference).

    geometry(k, d, n, num_cus)  the dispatch arithmetic of gmmvi_diag_mixture_eval and the kernels' index arithmetic, restated
    reference(case)             fp64: ld [K, N], lp [N], lp2 [N], grad [N, D]
    abs_bound(case)             the same sums with every term replaced by its absolute value, propagated to first order: the
                                element-wise magnitude B that fp32 rounding errors scale with
    reference_f32(case)         the same formulas in NumPy float32 throughout; above D = 512 the sums of the 32-dimension pieces
                                of the quadratic form are formed in float64, where diag_eval_kernel<true> forms them
    planted_faults(case)        fp64 variants that are wrong in one way this code could be wrong

The GPU test asserts |device - reference| <= C[route] * EPS32 * B element-wise.  C is not tuned on the device: it is 8 times the
largest |reference_f32 - reference| / (EPS32 * B) over the case table, per route (the device sums in another order -- two chains
of multiply-adds per piece, components strided over the waves, an online log-sum-exp per wave, a merge per workgroup and one over
the chunks -- and uses __expf / __logf).  Measured on the table below (test_diag_sweep_cases_cpu.py asserts that no case exceeds
the figure of its route and output, and that every planted fault moves some element by FAULT_FACTOR C EPS32 B or more):

    route  output   float32   RATIO_F32   where it occurred
    f32    ld       1.85      2           K257-D5-N64-far
    f32    lp       0.64      1           K9-D33-N129-far
    f32    lp2      0.71      1           K9-D33-N129-far
    f32    grad     0.34      1           dim-K3-D512-N65-normal
    hd     ld       0.49      1           K40-D1024-N65-far
    hd     lp       0.40      1           K3-D545-N65-far
    hd     lp2      0.40      1           dim-K3-D1024-N65-normal
    hd     grad     0.32      1           extreme-K2-D131072-N65-normal
    C["f32"] = 8 * 2 = 16, C["hd"] = 8 * 1 = 8
(the figures are rounded up to the next integer.  B_ld carries sum |log sigma| + D/2 log 2 pi: at D = 5 the quadratic form is most
of it and the float32 error of its sum reaches 1.85 EPS32 B; from D = 33 on it stays below 0.7.)  The smallest shift of a planted
fault over the table is 116 EPS32 B = 14.5 C (extreme-K2-D131071-N3-normal, the selects missing: the 31 dimensions of the ragged
last piece against 131071 others); on the f32 route it is 782 EPS32 B = 48.9 C (comp-K255-D33-N65-normal, the last of 255
components left out of lp).

Where a fault does not apply (planted_faults):
  - "far": every third sample lies 300 sigma out, |ld| ~ 1e5 ... 5e7 there and one fp32 ulp of it is up to several nats: the faults
    that move ld itself are placed on those samples, the others are those of the "normal" kind at the same shape.
  - D > 4096 (the two extremes): B_ld is 2.3e5 and FAULT_FACTOR C EPS32 B_ld = 2.2 nats.  Weights and responsibilities lie below
    that resolution (the wrong weights shift lp2 by 49 EPS32 B = 6 C, a wave's share missing from the gradient by 13 = 1.6 C):
    only the ragged piece, the selects and the row faults apply; one dimension alone left out would need a whitened residual
    above 2.1.
  - sequential_f32_piece_sums, the fault of the hd route, is NOT separable and is not asserted at any D: adding the pieces in
    order in float32 shifts ld by 6.2 EPS32 B = 0.78 C at D = 131072 (extreme-K2-D131072-N65-normal), by 2.8 at D = 131071 and
    by at most 2.7 at D <= 1024 -- inside the GPU test's bound, let alone ten times outside it.  The bound is per element and
    scales with B ~ D, the loss of a sequential float32 sum of D / 32 pieces with sqrt(D / 32) ulps of D: the fp64 second-level
    sums of diag_eval_kernel<true> are held by the ulp bound of test_highd_sweep_kernels, not here.
test_diag_sweep_cases_cpu.py prints these figures with -s.
"""
import numpy as np

from weight_step_cases import f32
from blocked_sweep_cases import _lse, error_ratio                                       # noqa: F401  (error_ratio: for the tests)

EPS32 = float(np.finfo(np.float32).eps)
OUTPUTS = ("ld", "lp", "lp2", "grad")
ROUTES = ("f32", "hd")
RATIO_F32 = {"f32": {"ld": 2.0, "lp": 1.0, "lp2": 1.0, "grad": 1.0}, "hd": {"ld": 1.0, "lp": 1.0, "lp2": 1.0, "grad": 1.0}}
C = {route: 8.0 * max(per.values()) for route, per in RATIO_F32.items()}
FAULT_FACTOR = 10.0                      # every planted fault moves some element by at least FAULT_FACTOR * C * EPS32 * B

KINDS = ("normal", "far", "far_weights", "neginf")
LOG_FLOOR = float(np.log(1e-30))         # the model's weight floor (weights.hip)
LOG_2PI = float(np.log(2.0 * np.pi))
PIECE = 32                               # DS_CH: dimensions per piece
MAX_DIM_F32 = 512                        # GMMVI_MAX_DIM_BLOCKED: above it the HD instances run
# the input law: one shared scale vector s0, log-uniform in [0.5, 2]; sigma_k = s0 exp(SIGMA_SPREAD / sqrt(D) N(0, 1)),
# mu_k = MEAN_SPREAD s0 / sqrt(D) N(0, 1); x drawn from the components.  Both spreads shrink with sqrt(D): the log densities of
# two components at a sample differ by O(1) nats at every D, and the responsibilities stay mixed
SIGMA_SPREAD, MEAN_SPREAD = 0.3, 1.5
FAR_SIGMAS = 300.0


# ---- the dispatch arithmetic, restated (the case table below is placed by it) ------------------------------------------------------
def ceil4(v):
    return (v + 3) // 4 * 4


def block_stride(d):
    """csrc/diag_sweep.hip ds_stride: floats per component block (one piece of padding: whole pieces are fetched past D)."""
    return ceil4(3 * d + 1 + PIECE)


def geometry(k, d, n, num_cus=256):
    """csrc/diag_sweep.hip gmmvi_diag_mixture_eval -> dict(nw = waves per workgroup, tiles = 64-sample tiles, ky = component chunks
    after both roundings, kchunk = components per chunk, chunks = [(k_lo, k_hi)], per_wave[c][w] = components of chunk c that
    wave w walks (k_lo + w, k_lo + w + nw, ...; 0 for a wave without one), gw = waves of the gradient kernel (they stride over all
    K), pieces, ragged = D % 32, vec4 (with a 16-byte aligned X), one_piece, hd, pack_threads, stride)."""
    nw = min(k, 8)
    tiles = (n + 63) // 64
    ky = 1
    if 2 * tiles < 3 * num_cus:
        ky = (2 * num_cus + tiles // 2) // tiles
    ky = min(ky, k // (2 * nw))
    ky = min(max(ky, 1), 16)
    kchunk = (k + ky - 1) // ky
    ky = (k + kchunk - 1) // kchunk
    chunks = [(c * kchunk, min(k, (c + 1) * kchunk)) for c in range(ky)]
    per_wave = [[len(range(lo + w, hi, nw)) for w in range(nw)] for lo, hi in chunks]
    return dict(nw=nw, tiles=tiles, ky=ky, kchunk=kchunk, chunks=chunks, per_wave=per_wave, gw=min(k, 8),
                pieces=(d + PIECE - 1) // PIECE, ragged=d % PIECE, vec4=d % 4 == 0, one_piece=d <= PIECE, hd=d > MAX_DIM_F32,
                pack_threads=256 if d > MAX_DIM_F32 else 64, stride=block_stride(d))


def case_geometry(case, num_cus=256):
    return geometry(case["k"], case["d"], case["n"], num_cus)


def route(spec):
    return "hd" if spec["d"] > MAX_DIM_F32 else "f32"


# ---- the case table --------------------------------------------------------------------------------------------------------------
DIMS_F32 = (1, 2, 3, 4, 5, 31, 32, 33, 36, 63, 64, 65, 96, 127, 128, 129, 511, 512)      # K = 3, N = 65
DIMS_HD = (513, 516, 544, 545, 1023, 1024)
EXTREMES = ((2, 131072, 65), (2, 131071, 3))
COMPONENTS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 100, 255, 256, 257, 300)     # D = 5 and 33, N = 65
SAMPLES = (1, 2, 63, 64, 65, 127, 128, 129, 257)                                         # (K, D) = (9, 33) and (33, 33)
TILES = (8192, 19200, 24512, 24576)                                                      # (K, D) = (64, 8)
KIND_SHAPES = ((9, 33, 129), (33, 65, 65), (257, 5, 64), (48, 5, 65), (3, 545, 65), (40, 1024, 65))


def _spec(k, d, n, kind="normal", tag=""):
    return dict(k=k, d=d, n=n, kind=kind, id="-".join(p for p in (tag, f"K{k}-D{d}-N{n}", kind) if p))


def case_table():
    t = [_spec(3, d, 65, tag="dim") for d in DIMS_F32 + DIMS_HD]
    t += [_spec(k, d, n, tag="extreme") for k, d, n in EXTREMES]
    t += [_spec(k, d, 65, tag="comp") for d in (5, 33) for k in COMPONENTS]
    t += [_spec(k, 33, n, tag="samp") for k in (9, 33) for n in SAMPLES]
    t += [_spec(64, 8, n, tag="tile") for n in TILES]
    t += [_spec(k, d, n, kind) for kind in ("far", "far_weights", "neginf") for k, d, n in KIND_SHAPES]
    seen, out = set(), []
    for s in t:                                                    # (9, 33, 65) and (33, 33, 65) sit in two classes: once
        key = (s["k"], s["d"], s["n"], s["kind"])
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


def spec_by_id(case_id):
    return next(s for s in case_table() if s["id"] == case_id)


def reaches(geo):
    """What the GPU test requires of the table as a whole on the device it runs on."""
    sizes = [hi - lo for lo, hi in geo["chunks"]]
    return dict(chunked=geo["ky"] > 1, unequal_last_chunk=geo["ky"] > 1 and sizes[-1] < sizes[0],
                empty_wave=any(c == 0 for per in geo["per_wave"] for c in per))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def neginf_components(geo):
    """The components without weight of a "neginf" case, placed by the geometry: every component of one whole chunk (the one
    before the last; none where the sweep runs in one chunk), everything wave 1 (wave 0 of a one-wave workgroup) owns in another
    chunk, and further ones up to a third of K -- never the last component and never all."""
    k, nw, chunks = geo["chunks"][-1][1], geo["nw"], geo["chunks"]
    dead = set()
    whole = None
    if geo["ky"] > 1:
        whole = max(geo["ky"] - 2, 0)
        dead |= set(range(*chunks[whole]))
    other = 0 if whole != 0 else geo["ky"] - 1
    lo, hi = chunks[other]
    wave = min(1, nw - 1)
    dead |= set(range(lo + wave, hi, nw))
    dead.discard(k - 1)
    for i in range(2, k - 1, 3):                                                        # top up to a third
        if len(dead) * 3 >= k:
            break
        dead.add(i)
    assert len(dead) < k
    return sorted(dead), whole, (other, wave)


def make_case(spec):
    """-> dict of fp32-representable fp64 arrays: mu, sigma [K, D], isig = 1 / sigma, isig2 = 1 / sigma^2, c [K] (log-normaliser),
    logw, logw2 [K], x [N, D]; block [K, stride] float32, the component block as the device reads it; comp [N]."""
    k, d, n, kind = spec["k"], spec["d"], spec["n"], spec["kind"]
    rng = np.random.default_rng([KINDS.index(kind), k, d, n])
    s0 = np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=d))
    sigma = f32(s0 * np.exp(SIGMA_SPREAD / np.sqrt(d) * rng.normal(size=(k, d))))
    mu = f32(MEAN_SPREAD * s0 / np.sqrt(d) * rng.normal(size=(k, d)))
    comp = rng.integers(0, k, size=n)
    comp[-1] = k - 1                                                 # the last sample (a ragged tile's last row) has an owner
    noise = rng.normal(size=(n, d))
    x = mu[comp] + sigma[comp] * noise
    if kind == "far":
        far = np.arange(n) % 3 == 2
        x[far] = mu[comp[far]] + FAR_SIGMAS * sigma[comp[far]] * np.sign(noise[far])
    x = f32(x)
    logw = np.log(rng.dirichlet(np.ones(k) * 2.0))
    logw2 = np.log(rng.integers(1, 50, k) / (50.0 * k))              # background weights (counts), unnormalised
    if kind == "far_weights":
        logw = np.linspace(LOG_FLOOR, 0.0, k) if k > 1 else np.zeros(1)              # the last component dominates
        logw2 = np.sort(rng.uniform(LOG_FLOOR, 0.0, size=k))[::-1].copy()            # the first one
        logw2[0] = 0.0
    if kind == "neginf":
        logw[neginf_components(geometry(k, d, n))[0]] = -np.inf
    if k > 1 and np.argmax(logw) == np.argmax(logw2):
        logw2 = np.roll(logw2, 1)
    logw, logw2 = f32(logw), f32(logw2)
    case = dict(spec, mu=mu, sigma=sigma, logw=logw, logw2=logw2, x=x, comp=comp)
    case.update(block_vectors(sigma, rounded=True))
    block = np.zeros((k, block_stride(d)), np.float32)
    block[:, :d], block[:, d:2 * d], block[:, 2 * d:3 * d], block[:, 3 * d] = mu, case["isig"], case["isig2"], case["c"]
    case["block"] = block
    return case


def block_vectors(sigma, rounded):
    """1 / sigma, 1 / sigma^2 and the log-normaliser -sum log sigma - D/2 log 2 pi in fp64; rounded: to fp32, once."""
    r = f32 if rounded else (lambda a: a)
    return dict(isig=r(1.0 / sigma), isig2=r(1.0 / (sigma * sigma)),
                c=r(-np.sum(np.log(sigma), axis=1) - 0.5 * sigma.shape[1] * LOG_2PI))


def exact_case(case):
    """The same case with the three derived vectors not rounded: what oracle.gmm.DiagonalGMM computes from mu and sigma."""
    out = {key: v for key, v in case.items() if not key.startswith("_")}
    out.update(block_vectors(case["sigma"], rounded=False))
    return out


# ---- the formulas --------------------------------------------------------------------------------------------------------------------
def _resp(a, lp):
    """exp(a - lp), 0 where a is -inf; lp [N] or [K, N]."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.exp(a - lp)
    return np.where(np.isneginf(a), 0.0, r)


def _terms(case):
    """fp64, cached: q [K, N] = sum_d ((x - mu) / sigma)^2; q_whole: over the whole pieces only; z2_last: the term of dimension
    D - 1; unmasked [K]: what the lanes past D of the last piece would add without the selects (x reads as 0 there, the block goes
    on with the neighbouring vector)."""
    if "_terms" not in case:
        k, d, n = case["k"], case["d"], case["n"]
        whole = d // PIECE * PIECE
        q, q_whole, z2_last = np.empty((k, n)), np.empty((k, n)), np.empty((k, n))
        for i in range(k):
            z2 = np.square((case["x"] - case["mu"][i]) * case["isig"][i])
            q[i], q_whole[i], z2_last[i] = z2.sum(axis=1), z2[:, :whole].sum(axis=1), z2[:, d - 1]
        flat = case["block"].astype(np.float64)
        past = np.arange(d, (d + PIECE - 1) // PIECE * PIECE)
        unmasked = np.sum(np.square(flat[:, past] * flat[:, d + past]), axis=1)
        case["_terms"] = dict(q=q, q_whole=q_whole, z2_last=z2_last, unmasked=unmasked)
    return case["_terms"]


def _gradient(case, r, scale):
    """-sum_k r[k, n] (x[n, d] - mu[k, d]) scale[k, d] as two matrix products."""
    with np.errstate(invalid="ignore"):                    # (a planted fault may leave lp at -inf: r is inf there, the result NaN)
        return -(case["x"] * (r.T @ scale) - r.T @ (case["mu"] * scale))


def evaluate(case, fault=None):
    """fp64 -> dict(ld, lp, lp2, grad, parts = the log values per component chunk [ky, N]).  ``fault``: (name, argument) of
    planted_faults."""
    name, arg = fault if fault else (None, None)
    k, n, d = case["k"], case["n"], case["d"]
    geo = case_geometry(case)
    t = _terms(case)
    q = t["q"]
    if name == "ragged_piece_left_out":
        q = t["q_whole"]
    elif name == "last_dimension_left_out":
        q = q - t["z2_last"]
    elif name == "mask_missing":
        q = q + t["unmasked"][:, None]
    ld = case["c"][:, None] - 0.5 * q
    a, a2 = case["logw"][:, None] + ld, case["logw2"][:, None] + ld
    if name == "lp2_from_logw":
        a2 = a
    parts, parts2 = (np.stack([_lse(v[lo:hi]) for lo, hi in geo["chunks"]]) for v in (a, a2))
    lp, lp2 = _lse(a), _lse(a2)
    if name == "last_component_left_out_of_lp":
        lp, lp2 = _lse(a[:-1]), _lse(a2[:-1])
    elif name == "empty_wave_counts_one":
        empty = np.array([sum(c == 0 for c in per) for per in geo["per_wave"]], np.float64)
        with np.errstate(divide="ignore"):
            extra = np.broadcast_to(np.log(empty)[:, None], parts.shape)
        lp, lp2 = _lse(np.concatenate([parts, extra])), _lse(np.concatenate([parts2, extra]))
    elif name == "chunk_dropped":
        lp, lp2 = _lse(np.delete(parts, arg, axis=0)), _lse(np.delete(parts2, arg, axis=0))
    r = _resp(a, lp)
    if name == "gradient_by_chunk_lp":
        chunk_of = np.repeat(np.arange(geo["ky"]), [hi - lo for lo, hi in geo["chunks"]])
        r = _resp(a, parts[chunk_of])
    elif name == "gradient_wave_missing":
        r = r.copy()
        r[arg::geo["gw"]] = 0.0
    grad = _gradient(case, r, case["isig"] if name == "gradient_with_inverse_sigma" else case["isig2"])
    out = dict(ld=ld, lp=lp, lp2=lp2, grad=grad, parts=parts)
    if name == "gradient_last_piece_not_written":
        out["grad"] = grad.copy()
        out["grad"][:, (geo["pieces"] - 1) * PIECE:] = 0.0
    elif name == "last_row_read_for_the_one_before":
        out = {key: v.copy() for key, v in out.items()}
        out["ld"][:, n - 2], out["lp"][n - 2], out["lp2"][n - 2], out["grad"][n - 2] = ld[:, n - 1], lp[n - 1], lp2[n - 1], grad[n - 1]
    return out


def reference(case):
    if "_ref" not in case:
        case["_ref"] = evaluate(case)
    return case["_ref"]


def abs_bound(case):
    """B per output.  zb = (|x| + |mu|) / sigma, qb = sum zb^2, B_ld = sum |log sigma| + D/2 log 2 pi + qb / 2 (the magnitude of
    the log-normaliser is that of the terms it is the sum of).
    B_lp = sum_k r_k (|logw_k| + B_ld_k) + |lp|, likewise lp2 with its own responsibilities.
    B_grad = sum_k r_k (|x| + |mu_k|) / sigma_k^2 + sum_k r_k (B_ld_k + B_lp) |x - mu_k| / sigma_k^2 (the sensitivity of the
    responsibilities to the error of ld and lp: it dominates where two components tie)."""
    ref = reference(case)
    k, d = case["k"], case["d"]
    ax, amu = np.abs(case["x"]), np.abs(case["mu"])
    qb = np.stack([np.square((ax + amu[i]) * case["isig"][i]).sum(axis=1) for i in range(k)])
    b_ld = (np.abs(np.log(case["sigma"])).sum(axis=1) + 0.5 * d * LOG_2PI)[:, None] + 0.5 * qb
    out = dict(ld=b_ld)
    r = {}
    for key, lw in (("lp", case["logw"]), ("lp2", case["logw2"])):
        r[key] = _resp(lw[:, None] + ref["ld"], ref[key])
        with np.errstate(invalid="ignore"):
            terms = np.where(r[key] > 0, r[key] * (np.abs(lw)[:, None] + b_ld), 0.0)
        out[key] = terms.sum(axis=0) + np.abs(ref[key])
    g = ax * (r["lp"].T @ case["isig2"]) + r["lp"].T @ (amu * case["isig2"])
    sens = r["lp"] * (b_ld + out["lp"][None, :])
    for i in range(k):
        g += sens[i][:, None] * (np.abs(case["x"] - case["mu"][i]) * case["isig2"][i])
    out["grad"] = g
    return out


# ---- the same formulas in float32 ------------------------------------------------------------------------------------------------
def reference_f32(case, sequential_f32=False):
    """float32 throughout -> dict(ld, lp, lp2, grad) as float64 arrays.  The quadratic form is summed per 32-dimension piece in
    float32; the pieces are added in order in float32 up to D = 512 and in float64 above (diag_eval_kernel<true>: qd), where
    ld = (float)(c - qd / 2) is formed in float64 too.  sequential_f32: the planted fault of the hd route, the pieces added in
    order in float32 at every D."""
    t = np.float32
    k, d, n = case["k"], case["d"], case["n"]
    hd = d > MAX_DIM_F32 and not sequential_f32
    pieces = (d + PIECE - 1) // PIECE
    x, mu, isig, isig2, c = (case[key].astype(t) for key in ("x", "mu", "isig", "isig2", "c"))
    ld = np.empty((k, n), t)
    z2 = np.zeros((n, pieces * PIECE), t)
    for i in range(k):
        z = (x - mu[i]) * isig[i]
        z2[:, :d] = z * z
        part = np.sum(z2.reshape(n, pieces, PIECE), axis=2, dtype=t)
        if hd:
            ld[i] = (c[i].astype(np.float64) - 0.5 * part.astype(np.float64).sum(axis=1)).astype(t)
        else:
            q = np.cumsum(part, axis=1, dtype=t)[:, -1]                    # in order, every partial sum rounded to float32
            ld[i] = c[i] - t(0.5) * q
    out = dict(ld=ld)
    for key, lw in (("lp", case["logw"].astype(t)), ("lp2", case["logw2"].astype(t))):
        a = lw[:, None] + ld
        m = np.max(a, axis=0)
        with np.errstate(divide="ignore"):
            out[key] = m + np.log(np.sum(np.exp(a - m), axis=0, dtype=t))
    with np.errstate(over="ignore"):
        r = np.exp(case["logw"].astype(t)[:, None] + ld - out["lp"][None, :])
    grad = np.zeros((n, d), t)
    for i in range(k):
        grad -= r[i][:, None] * ((x - mu[i]) * isig2[i])
    out["grad"] = grad
    assert all(v.dtype == t for v in out.values())
    return {key: v.astype(np.float64) for key, v in out.items()}


# ---- planted faults ------------------------------------------------------------------------------------------------------------------
LD_ONLY_ABOVE_D = 4096          # above it only the piece, select and row faults apply (module docstring)


def planted_faults(case):
    """[(name, argument)]: what a subtly wrong sweep would compute, each applicable to this case --
    ragged_piece_left_out             the ragged last piece left out of the quadratic form
    last_dimension_left_out           dimension D - 1 alone left out of it
    mask_missing                      the selects missing: the lanes past D add the neighbouring vector's data
    last_row_read_for_the_one_before  sample N - 2 given the values of the last sample's row
    last_component_left_out_of_lp     the last component of the last chunk left out of lp and lp2
    empty_wave_counts_one             a wave without a component counted as a term exp(0) = 1
    chunk_dropped c                   the partial of chunk c dropped from the merge
    lp2_from_logw                     the second mixture formed with the first weights
    gradient_with_inverse_sigma       the gradient formed with 1 / sigma in place of 1 / sigma^2
    gradient_wave_missing w           the components wave w of the gradient kernel owns missing from the gradient
    gradient_by_chunk_lp              every gradient term normalised by its own chunk's lp, not by the merged one
    gradient_last_piece_not_written   the gradient's last piece left at zero
    sequential_f32_piece_sums         (hd) the pieces of the quadratic form added in order in float32: evaluated by
                                      reference_f32(case, sequential_f32=True), see the module docstring"""
    k, d, n, kind = case["k"], case["d"], case["n"], case["kind"]
    geo = case_geometry(case)
    faults = []
    if geo["ragged"] and geo["pieces"] > 1:
        faults.append(("ragged_piece_left_out", None))
    if d <= LD_ONLY_ABOVE_D:
        faults.append(("last_dimension_left_out", None))
    if geo["ragged"]:
        faults.append(("mask_missing", None))
    if n >= 2:
        faults.append(("last_row_read_for_the_one_before", None))
    if kind == "far" or d > LD_ONLY_ABOVE_D:
        # weights and responsibilities lie below the resolution of the densities: only the faults that move ld itself apply
        return faults
    if k >= 2:
        faults += [("last_component_left_out_of_lp", None), ("lp2_from_logw", None), ("gradient_wave_missing", (k - 1) % geo["gw"])]
    if reaches(geo)["empty_wave"]:
        faults.append(("empty_wave_counts_one", None))
    if geo["ky"] > 1:
        faults.append(("chunk_dropped", geo["ky"] - 1))
        if sum(np.isfinite(case["logw"][lo:hi]).any() for lo, hi in geo["chunks"]) > 1:       # two chunks that carry weight
            faults.append(("gradient_by_chunk_lp", None))
    faults += [("gradient_with_inverse_sigma", None), ("gradient_last_piece_not_written", None)]
    return faults


# ---- gmmvi_diag_pack -----------------------------------------------------------------------------------------------------------------
PACK_DIMS = (1, 63, 64, 65, 512, 513, 769, 131071)                                       # K = 3


def pack_inputs(d, k=3):
    """mu, sigma [K, D] (fp32-representable fp64) by the input law of make_case."""
    rng = np.random.default_rng([99, k, d])
    s0 = np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=d))
    return (f32(MEAN_SPREAD * s0 / np.sqrt(d) * rng.normal(size=(k, d))),
            f32(s0 * np.exp(SIGMA_SPREAD / np.sqrt(d) * rng.normal(size=(k, d)))))


def pack_reference(sigma):
    """fp64 -> (values, scales): 1 / sigma, 1 / sigma^2 and the log-normaliser, each with its absolute-value scale (the
    reciprocals their own magnitude, the log-normaliser sum |log sigma| + D/2 log 2 pi)."""
    v = block_vectors(sigma, rounded=False)
    scale = dict(isig=v["isig"], isig2=v["isig2"], c=np.abs(np.log(sigma)).sum(axis=1) + 0.5 * sigma.shape[1] * LOG_2PI)
    return v, scale


def pack_f32(sigma):
    """diag_pack_kernel / diag_pack_hd_kernel in NumPy float32: log sigma summed per thread (64, or 256 above D = 512) in float32
    -- float64 above D = 512 -- then over the threads."""
    t = np.float32
    k, d = sigma.shape
    hd = d > MAX_DIM_F32
    threads = 256 if hd else 64
    s = sigma.astype(t)
    logs = np.zeros((k, (d + threads - 1) // threads * threads), t)
    logs[:, :d] = np.log(s)
    acc = np.float64 if hd else t
    lsum = np.sum(np.cumsum(logs.reshape(k, -1, threads).astype(acc), axis=1, dtype=acc)[:, -1], axis=1, dtype=acc)
    c = (-lsum - 0.5 * d * LOG_2PI).astype(t) if hd else -lsum - t(0.5) * t(d) * t(LOG_2PI)
    return dict(isig=(t(1.0) / s).astype(np.float64), isig2=(t(1.0) / (s * s)).astype(np.float64), c=c.astype(np.float64))
