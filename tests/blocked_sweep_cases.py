"""Inputs, fp64 reference, error scale and planted faults shared by test_hip_blocked_sweep.py (GPU), blocked_sweep_child.py and
test_blocked_sweep_cases_cpu.py: the density sweep of the blocked path, gmmvi_blocked_mixture_eval (csrc/blocked.hip), which
gmmvi_mixture_eval and gmmvi_mixture_eval_dual run for every D in 51 ... 512, ON ITS OWN INPUTS.  Nothing here touches the device.

The sweep reads the component block of csrc/blocked.h, [mu (D) | log-normaliser | pad to 4 | L^-1 dense row-major D x D], the log
weights and x as plain arrays.  make_case() builds the block on the host: L^-1 and the log-normaliser are computed in fp64 and
rounded to fp32, and so is everything else, so the device and the reference read the same numbers (the conditioning of the
on-device inverse does not enter; gmmvi_pack_components keeps its own test).

    reference(case)             fp64: ld [K, N], lp [N], lp2 [N], grad [N, D]
    abs_bound(case)             the same sums with every term replaced by its absolute value, propagated to first order: the
                                element-wise magnitude B that fp32 rounding errors scale with
    reference_f32(case, split)  the same formulas in NumPy float32 throughout; split: both operands of every contraction replaced
                                by their three bf16 planes, the six partial products i + j <= 4 kept (csrc/bf16_split.h)
    geometry(...)               the dispatch arithmetic of gmmvi_blocked_mixture_eval and bgemm_tile_width, restated
    planted_faults(case)        fp64 variants that are wrong in one way this code could be wrong

The GPU test asserts |device - reference| <= C * EPS32 * B element-wise.  C is not tuned on the device: it is 8 times the largest
|reference_f32 - reference| / (EPS32 * B) over the case table (the device sums in another order -- 16-wide k steps on the matrix
cores, partial |z|^2 per column tile, partial gradients per component range and chunk, an online log-sum-exp -- and uses __expf /
__logf).  Measured on the table below (test_blocked_sweep_cases_cpu.py asserts that no case exceeds the figure of its output and
variant, and that every planted fault moves some element by 10 C EPS32 B or more):

    output   plain float32   three bf16 planes    RATIO_F32   where the larger one occurred
    ld       1.58            1.60                 2           K19-D96-N150-far_weights-gauss-chunked (both)
    lp       0.45            0.45                 1           K9-D72-N257-normal-student_t (both)
    lp2      0.42            0.42                 1           K9-D72-N257-normal-student_t (both)
    grad     0.24            0.22                 1           sweepD-K3-D159-N129-normal-gauss / K19-D96-N150-normal-gauss-chunked
    C = 8 * 2 = 16
(the figures are rounded up to the next integer: the float32 matrix products may be summed in another order on another host.  B
is formed from |x| + |mu| and |L^-1|: where L^-1 is nearly diagonal and the means lie on single coordinates -- the far_weights
cases -- it is tight and the float32 error reaches 1.6 EPS32 B; with dense factors the signed sums cancel and it stays below
0.5.)  The smallest shift of a planted fault over the table is 351 EPS32 B = 21.9 C (K19-D96-N150-far_weights-gauss-chunked, the
last component range of the last chunk -- one component -- left out of the gradient).  On the Gaussian "far" cases |ld| ~ 1e7
and one fp32 ulp of it is about a nat: only the faults that move ld itself apply there (planted_faults).
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import gammaln

from weight_step_cases import f32

EPS32 = float(np.finfo(np.float32).eps)
OUTPUTS = ("ld", "lp", "lp2", "grad")
RATIO_F32 = {"plain": {"ld": 2.0, "lp": 1.0, "lp2": 1.0, "grad": 1.0}, "split": {"ld": 2.0, "lp": 1.0, "lp2": 1.0, "grad": 1.0}}
C = 8.0 * max(v for r in RATIO_F32.values() for v in r.values())
FAULT_FACTOR = 10.0                      # every planted fault moves some element by at least FAULT_FACTOR * C * EPS32 * B

GAUSS, STUDENT_T = 0, 1                  # include/gmmvi_hip.h
NU = 2.0
KINDS = ("normal", "far_weights", "neginf", "far")
FAMILIES = ("gauss", "student_t")
LOG_FLOOR = float(np.log(1e-30))         # the model's weight floor (weights.hip)
# the "normal", "neginf" and "far" components: means MEAN_SPREAD / sqrt(D) N(0, 1) (about 3.5 standard deviations between two of
# them), covariances COV_MIX A A^T / D + (1 - COV_MIX) I with A = A0 + COV_SPREAD / sqrt(D) N(0, 1) per component
MEAN_SPREAD, COV_SPREAD, COV_MIX = 2.5, 0.25, 0.3
# Student-t: component i is scaled by T_SCALES[i % 3] (the density is nearly scale-free at nu = 2, so the responsibilities stay
# mixed, while q and with it the gradient coefficient -(nu + D) / (nu + q) differ by factors between the components)
T_SCALES = (0.6, 1.0, 1.6)


# ---- the dispatch arithmetic, restated (the case table below is placed by it) ------------------------------------------------------
def ceil4(v):
    return (v + 3) // 4 * 4


def block_stride(d):
    """csrc/blocked.h gmmvi_blocked_stride: floats per component block."""
    return ceil4(d + 1) + d * d


def tile_width(n, split):
    """csrc/blocked_gemm.hip bgemm_tile_width -> (NT 32-column tiles per workgroup, column tiles): the least padded total width,
    ties go to the wider tile."""
    nt, best = None, 1 << 30
    for cand in ((10, 8, 6, 5, 4, 3) if split else (5, 4, 3)):
        w = (n + 32 * cand - 1) // (32 * cand) * 32 * cand
        if w < best:
            best, nt = w, cand
    return nt, best // (32 * nt)


def geometry(k, d, n, zbytes=None, num_cus=256, f32_route=False):
    """csrc/blocked.hip gmmvi_blocked_mixture_eval with the gradient asked for -> dict(LP = row stride of Z, Kc = components per
    chunk, split = the route of the two contractions, NT, ctiles = column tiles, S = component ranges of the gradient, chunks =
    [(kn, inner, nz, size of the last range)], row_tiles, wtiles = tiles of the first whitening launch, gtiles = tiles of the
    first gradient launch).  zbytes: GMMVI_BLOCKED_ZBYTES (default 4 GiB); f32_route: GMMVI_BLOCKED_F32=1."""
    lp = ceil4(d + 1)
    budget = ((4 << 30) if zbytes is None else int(zbytes)) // 4
    kc = max(1, min(k, budget // (n * lp)))
    split = (not f32_route) and d >= 160                          # gmmvi_bgemm_use_split(D, D): n >= 160 or kd >= 512
    nt, ctiles = tile_width(d, split)
    row_tiles = (n + 127) // 128
    tiles = row_tiles * ((d + 159) // 160)
    s = max(1, min((8 * num_cus + tiles - 1) // tiles, kc // 4, 16))
    if split:
        tc, spb, best = row_tiles * ctiles, (d + 15) // 16, None
        for c in range(1, min(16, max(kc // 4, 1)) + 1):
            inner = (kc + c - 1) // c
            rounds = (tc * ((kc + inner - 1) // inner) + num_cus - 1) // num_cus
            cost = rounds * (inner * spb + 12)
            if best is None or cost < best:
                best, s = cost, c
    chunks = []
    for k0 in range(0, k, kc):
        kn = min(kc, k - k0)
        inner = (kn + s - 1) // s if s > 1 else kn
        nz = (kn + inner - 1) // inner
        chunks.append((kn, inner, nz, kn - (nz - 1) * inner))
    return dict(LP=lp, Kc=kc, split=split, NT=nt, ctiles=ctiles, S=s, chunks=chunks, row_tiles=row_tiles,
                wtiles=ctiles * row_tiles * chunks[0][0], gtiles=ctiles * row_tiles * chunks[0][2])


def case_geometry(case, num_cus=256):
    return geometry(case["k"], case["d"], case["n"], case["zbytes"], num_cus, case["f32"])


# ---- the case table --------------------------------------------------------------------------------------------------------------
def _spec(k, d, n, kind="normal", family="gauss", zbytes=None, f32_route=False, tag=""):
    name = "-".join(p for p in (tag, f"K{k}-D{d}-N{n}", kind, family, "chunked" if zbytes else "", "f32" if f32_route else "") if p)
    return dict(k=k, d=d, n=n, kind=kind, family=family, zbytes=zbytes, f32=f32_route, id=name)


# (K, D, N) -> what it reaches at 256 compute units (test_blocked_sweep_cases_cpu.py asserts each)
SHAPES = ((8, 51, 129),        # the smallest blocked D; S = 2, ranges 4 + 4
          (8, 64, 1),          # N = 1
          (9, 72, 257),        # S = 2, ranges 5 + 4; three row tiles, the last with one sample
          (13, 130, 128),      # NT = 5; S = 3, ranges 5 + 5 + 3; one exactly full row tile
          (25, 96, 127),       # S = 6 but inner = 5: nz = 5 < S, a slab of gpart nobody writes and the sum must not read
          (64, 65, 130),       # the cap S = 16
          (9, 161, 129),       # split route, NT = 6, D % 4 = 1 (element-wise staging); S = 2 from the cost rule
          (17, 201, 257),      # split, NT = 8; S = 4, ranges 5 + 5 + 5 + 2
          (12, 324, 130),      # split, two column tiles (NT = 6: 192 + 132 columns); S = 3
          (10, 512, 129),      # the largest D; two column tiles; S = 2
          (40, 161, 1000))     # 320 whitening tiles > 256 compute units (the persistent walk); S = 10
# GMMVI_BLOCKED_ZBYTES = 8 N LP 4: chunks 8 + 8 + 3 with S = 2 (accumulate = 1 in the slab sum, last chunk ranges 2 + 1), on both routes
CHUNKED = ((19, 96, 150, 8 * 150 * 100 * 4), (19, 201, 150, 8 * 150 * 204 * 4))
# GMMVI_BLOCKED_F32=1 (one child process): the f32 route with two column tiles (NT = 3 and NT = 5), the qpart sum over tiles there
F32_SHAPES = ((9, 161, 129), (9, 300, 129))
# K = 3, N = 129 (194 and 323: D % 4 = 2 and 3 on the split route)
SWEEP_D = (63, 65, 96, 97, 128, 129, 159, 160, 192, 193, 194, 256, 257, 320, 321, 323)
SWEEP_N = (1, 127, 128, 129, 255, 256, 257)                                            # (K, D) = (9, 72) and (9, 161)


def case_table():
    """The cases of the shared context (default route; the chunked ones set GMMVI_BLOCKED_ZBYTES per call)."""
    t = [_spec(k, d, n) for k, d, n in SHAPES]
    t += [_spec(k, d, n, zbytes=zb) for k, d, n, zb in CHUNKED]
    t += [_spec(3, d, 129, tag="sweepD") for d in SWEEP_D]
    t += [_spec(9, d, n, tag="sweepN") for d in (72, 161) for n in SWEEP_N if (d, n) not in ((72, 257), (161, 129))]
    # Student-t (nu = 2): S > 1 on both routes, the chunked cases, two column tiles
    t += [_spec(k, d, n, family="student_t") for k, d, n in ((9, 72, 257), (13, 130, 128), (17, 201, 257), (12, 324, 130),
                                                            (10, 512, 129))]
    t += [_spec(k, d, n, family="student_t", zbytes=zb) for k, d, n, zb in CHUNKED]
    t += [_spec(9, 72, 257, "far_weights"), _spec(9, 161, 129, "far_weights"), _spec(9, 201, 257, "far_weights", "student_t"),
          _spec(19, 96, 150, "far_weights", zbytes=CHUNKED[0][3])]
    t += [_spec(9, 72, 257, "neginf"), _spec(9, 161, 129, "neginf"), _spec(19, 201, 150, "neginf", zbytes=CHUNKED[1][3])]
    t += [_spec(9, 72, 257, "far"), _spec(9, 161, 129, "far"), _spec(9, 72, 257, "far", "student_t")]
    return t


def f32_table():
    """The cases of the GMMVI_BLOCKED_F32=1 child."""
    t = [_spec(k, d, n, f32_route=True) for k, d, n in F32_SHAPES]
    t += [_spec(9, 300, 129, family="student_t", f32_route=True), _spec(9, 161, 129, "far_weights", f32_route=True),
          _spec(9, 161, 129, "far", f32_route=True)]
    return t


def requirements(spec):
    """[(what, holds(geometry, num_cus))]: the properties a case is in the table for.  They depend on the compute units of the
    device (the rules for S); the GPU test asserts them on the device it runs on and fails, not skips, where one does not hold."""
    shape = (spec["k"], spec["d"], spec["n"])
    ranged = ("S > 1", lambda g, cus: g["S"] > 1 and all(c[2] > 1 for c in g["chunks"]))
    req = {(8, 51, 129): [ranged], (8, 64, 1): [ranged], (9, 72, 257): [ranged], (9, 161, 129): [ranged], (10, 512, 129): [ranged],
           (12, 324, 130): [ranged],
           (13, 130, 128): [ranged, ("a shorter last range", lambda g, cus: g["chunks"][0][3] < g["chunks"][0][1])],
           (17, 201, 257): [ranged, ("a shorter last range", lambda g, cus: g["chunks"][0][3] < g["chunks"][0][1])],
           (25, 96, 127): [("nz < S", lambda g, cus: 1 < g["chunks"][0][2] < g["S"])],
           (64, 65, 130): [("the cap S = 16", lambda g, cus: g["S"] == 16 and g["chunks"][0][2] == 16)],
           (40, 161, 1000): [ranged, ("more whitening tiles than compute units", lambda g, cus: g["wtiles"] > cus)],
           }.get(shape, [])
    if spec["zbytes"]:
        req = [ranged, ("chunks 8 + 8 + 3, the last with ranges 2 + 1",
                        lambda g, cus: [c[0] for c in g["chunks"]] == [8, 8, 3] and g["chunks"][2][1:] == (2, 2, 1))]
    if spec["f32"]:
        req = [("two column tiles on the f32 route", lambda g, cus: not g["split"] and g["ctiles"] == 2)]
    return req


def spec_by_id(case_id):
    return next(s for s in case_table() + f32_table() if s["id"] == case_id)


def unchunked(spec):
    """The same case without the budget knob (the same inputs: the seed does not depend on it)."""
    return dict(spec, zbytes=None, id=spec["id"].replace("-chunked", ""))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_case(spec):
    """-> dict of fp32-representable fp64 arrays: mu [K, D], linv [K, D, D] (lower triangular), c [K] (log-normaliser), logw,
    logw2 [K], x [N, D]; block [K, stride] float32, the component block as the device reads it; nu, family_id."""
    k, d, n, kind, family = spec["k"], spec["d"], spec["n"], spec["kind"], spec["family"]
    rng = np.random.default_rng([KINDS.index(kind), FAMILIES.index(family), int(spec["f32"]), k, d, n])
    student = family == "student_t"
    if kind == "far_weights":
        # test_hip_density_routes._far_weight_cases: well separated components, each alone near its own samples (the others lie
        # more than 150 nats lower there, weights included; the Student-t tails need the means 60 apart and D = 201 for that --
        # a wider spacing would enter B through |x| + |mu| and hide a missing component range)
        spacing = 60.0 if student else 40.0
        mu = np.zeros((k, d))
        mu[np.arange(k), np.arange(k)] = spacing
        chols = np.stack([np.eye(d) * (0.7 + 0.1 * (i % 6)) + np.tril(rng.normal(size=(d, d)), -1) * 0.05 for i in range(k)])
        comp = np.arange(n) % k
        x = mu[comp] + rng.normal(size=(n, d))
        logw = np.log(np.full(k, 1.0 / k))
        logw[0], logw[1] = -100.0, LOG_FLOOR
        logw2 = np.log(np.full(k, 0.2))
        logw2[2], logw2[0] = -100.0, 0.0
    else:
        # neighbouring components overlap: a common A0 with a small perturbation per component and means a few standard
        # deviations apart, so that most samples carry several responsibilities of 1e-3 ... 1 (independent covariances differ
        # by O(D) nats at every sample: all responsibilities would be 0 or 1).  The means are centred on 0 and L^-1 is
        # dominated by its diagonal: B is formed from |x| + |mu| and |L^-1|, and stays within 1e3 of the values themselves
        a0 = rng.normal(size=(d, d))
        mu = rng.normal(size=(k, d)) * MEAN_SPREAD / np.sqrt(d)
        chols = np.empty((k, d, d))
        for i in range(k):
            a = a0 + rng.normal(size=(d, d)) * COV_SPREAD / np.sqrt(d)
            chols[i] = np.linalg.cholesky(COV_MIX * a @ a.T / d + (1.0 - COV_MIX) * np.eye(d))
            if student:
                chols[i] *= T_SCALES[i % 3]
        comp = rng.integers(0, k, size=n)
        comp[-1] = k - 1                                             # the last sample (a ragged tile's last row) has an owner
        x = (rng.normal(size=(n, d)) * 200.0 if kind == "far" else
             mu[comp] + np.einsum("nij,nj->ni", chols[comp], rng.normal(size=(n, d))))
        if n == 1 and kind != "far":
            # the only sample lies between the first and the last mean: the first and the last component range carry responsibility
            x = 0.5 * (mu[0] + mu[k - 1]) + 0.5 * (chols[comp] @ rng.normal(size=d))
        logw = np.log(rng.dirichlet(np.ones(k) * 2.0))
        logw2 = np.log(rng.integers(1, 50, k) / (50.0 * k))          # background weights (counts), unnormalised
        if kind == "neginf":
            logw[k // 2] = -np.inf
    mu, x, logw, logw2 = f32(mu), f32(x), f32(logw), f32(logw2)
    linv = np.stack([solve_triangular(ch, np.eye(d), lower=True) for ch in chols])
    linv = f32(np.tril(linv))
    logdet = np.log(np.diagonal(chols, axis1=1, axis2=2)).sum(axis=1)
    if student:        # csrc/blocked.hip blk_pack_kernel
        c = gammaln(0.5 * (NU + d)) - gammaln(0.5 * NU) - 0.5 * d * np.log(NU * np.pi) - logdet
    else:
        c = -logdet - 0.5 * d * np.log(2.0 * np.pi)
    c = f32(c)
    lo = ceil4(d + 1)
    block = np.zeros((k, block_stride(d)), np.float32)
    block[:, :d], block[:, d], block[:, lo:] = mu, c, linv.reshape(k, d * d)
    return dict(spec, mu=mu, linv=linv, c=c, logw=logw, logw2=logw2, x=x, block=block, comp=comp, nu=NU if student else 0.0,
                family_id=STUDENT_T if student else GAUSS)




# ---- the formulas --------------------------------------------------------------------------------------------------------------------
def _lse(a):
    """log sum exp over axis 0, -inf where every term is -inf."""
    m = np.max(a, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = m + np.log(np.sum(np.exp(a - np.where(np.isneginf(m), 0.0, m)), axis=0))
    return np.where(np.isneginf(m), -np.inf, out)


def _whitened(case):
    """fp64, cached: z [K, N, D] = L^-1 (x - mu), q [K, N] = |z|^2, y [K, N, D] = L^-T z."""
    if "_w64" not in case:
        z = (case["x"][None] - case["mu"][:, None, :]) @ np.transpose(case["linv"], (0, 2, 1))
        case["_w64"] = (z, np.sum(z * z, axis=2), z @ case["linv"])
    return case["_w64"]


def _ld_coef(case, q, t=np.float64):
    """Component log densities and the family's gradient coefficient from q = |z|^2, in dtype t."""
    c, d = case["c"].astype(t)[:, None], case["d"]
    if case["family"] == "gauss":
        return c - t(0.5) * q, np.full(q.shape, -1.0, t)
    nu = t(case["nu"])
    return c - t(0.5) * (nu + t(d)) * np.log1p(q / nu), -(nu + t(d)) / (nu + q)


def _resp(a, lp):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.exp(a - lp[None, :])
    return np.where(np.isneginf(a), 0.0, r)


def evaluate(case, fault=None):
    """fp64 -> dict(ld, lp, lp2, grad).  ``fault``: (name, argument) of planted_faults."""
    name, arg = fault if fault else (None, None)
    k, n = case["k"], case["n"]
    geo = case_geometry(case)
    z, q, y = _whitened(case)
    if name == "second_tile_norm_left_out":
        w = 32 * geo["NT"]
        q = np.sum(z[:, :, :w] ** 2, axis=2)
    ld, coef = _ld_coef(case, q)
    a = case["logw"][:, None] + ld
    lp, lp2 = _lse(a), _lse(case["logw2"][:, None] + ld)
    lp_grad = lp
    if name == "lp2_from_logw":
        lp2 = lp.copy()
    elif name == "floor_weight_dropped_from_lp":
        lp = _lse(a[case["logw"] != -100.0])
    elif name == "gradient_lp_without_last":
        lp_grad = _lse(a[:-1])
    elif name == "coefficient_from_chunk_0":
        qc = q.copy()
        kc = geo["Kc"]
        qc[kc:kc + geo["chunks"][1][0]] = q[:geo["chunks"][1][0]]
        coef = _ld_coef(case, qc)[1]
    mult = np.ones(k)
    starts = np.cumsum([0] + [ch[0] for ch in geo["chunks"]])
    if name == "last_range_left_out":
        kn, inner, nz, last = geo["chunks"][arg]
        mult[starts[arg] + kn - last:starts[arg] + kn] = 0.0
    elif name == "slab_added_twice":
        kn, inner, nz, last = geo["chunks"][arg]
        mult[starts[arg]:starts[arg] + inner] = 2.0
    elif name == "chunk_overwrites":
        mult[:starts[-2]] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        grad = np.einsum("kn,knd->nd", mult[:, None] * _resp(a, lp_grad) * coef, y)
    out = dict(ld=ld, lp=lp, lp2=lp2, grad=grad)
    if name == "ragged_row_takes_neighbour":
        out = {key: v.copy() for key, v in out.items()}
        out["ld"][:, n - 1], out["lp"][n - 1], out["lp2"][n - 1], out["grad"][n - 1] = ld[:, n - 2], lp[n - 2], lp2[n - 2], grad[n - 2]
    return out


def reference(case):
    if "_ref" not in case:
        case["_ref"] = evaluate(case)
    return case["_ref"]


def abs_bound(case):
    """B per output.  zb = |L^-1| (|x| + |mu|), qb = sum zb^2, B_ld = |c| + qb / 2; Student-t: |c| + (nu + D) / 2 (log1p(q / nu) +
    qb / (nu + q)), the magnitude of the term and the error of q through d/dq log1p(q / nu) = 1 / (nu + q).
    B_lp = sum_k r_k (|logw_k| + B_ld_k) + |lp|.
    B_grad = sum_k r_k |coef_k| |L^-1|^T zb_k + sum_k r_k (B_ld_k + B_lp) |coef_k y_k| (the sensitivity of the responsibilities to
    the error of ld: it dominates where two components tie); Student-t adds sum_k r_k |coef_k y_k| qb_k / (nu + q_k), the error of
    q in the coefficient -(nu + D) / (nu + q)."""
    ref = reference(case)
    _, q, y = _whitened(case)
    alinv = np.abs(case["linv"])
    zb = (np.abs(case["x"])[None] + np.abs(case["mu"])[:, None, :]) @ np.transpose(alinv, (0, 2, 1))
    qb = np.sum(zb * zb, axis=2)
    yb = zb @ alinv
    coef = np.abs(_ld_coef(case, q)[1])
    ac = np.abs(case["c"])[:, None]
    if case["family"] == "gauss":
        b_ld, dcoef = ac + 0.5 * qb, 0.0
    else:
        nu = case["nu"]
        b_ld = ac + 0.5 * (nu + case["d"]) * (np.log1p(q / nu) + qb / (nu + q))
        dcoef = qb / (nu + q)
    out = dict(ld=b_ld)
    r = {}
    for key, lw in (("lp", case["logw"]), ("lp2", case["logw2"])):
        r[key] = _resp(lw[:, None] + ref["ld"], ref[key])
        with np.errstate(invalid="ignore"):
            terms = np.where(r[key] > 0, r[key] * (np.abs(lw)[:, None] + b_ld), 0.0)
        out[key] = terms.sum(axis=0) + np.abs(ref[key])
    rc = r["lp"] * coef
    out["grad"] = np.einsum("kn,knd->nd", rc, yb) + np.einsum("kn,knd->nd", rc * (b_ld + out["lp"][None, :] + dcoef), np.abs(y))
    return out


# ---- the same formulas in float32, plain or through the three bf16 planes --------------------------------------------------------
def _bf16(x):
    """float32 -> the nearest bf16 (ties to even) as float32, on the uint32 view."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def _planes(x):
    """csrc/bf16_split.h split_pair: x = p1 + p2 + p3, each the bf16 of the running remainder."""
    p1 = _bf16(x)
    r = x - p1
    p2 = _bf16(r)
    return p1, p2, _bf16(r - p2)


def _matmul(a, b, split):
    """a @ b in float32; split: the six partial products i + j <= 4 of the planes, smallest first (bgemm_ws_tile)."""
    if not split:
        return a @ b
    pa, pb = _planes(a), _planes(b)
    acc = pa[2] @ pb[0]
    for i, j in ((0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
        acc = acc + pa[i] @ pb[j]
    return acc


def reference_f32(case, split):
    """float32 throughout -> dict(ld, lp, lp2, grad) as float64 arrays."""
    t = np.float32
    k, d, n = case["k"], case["d"], case["n"]
    x, mu, linv = case["x"].astype(t), case["mu"].astype(t), case["linv"].astype(t)
    z = [_matmul(x - mu[i], np.ascontiguousarray(linv[i].T), split) for i in range(k)]
    q = np.stack([np.sum(zi * zi, axis=1, dtype=t) for zi in z])
    ld, coef = _ld_coef(case, q, t)
    out = dict(ld=ld)
    for key, lw in (("lp", case["logw"].astype(t)), ("lp2", case["logw2"].astype(t))):
        a = lw[:, None] + ld
        m = np.max(a, axis=0)
        with np.errstate(divide="ignore"):
            out[key] = m + np.log(np.sum(np.exp(a - m), axis=0, dtype=t))
    with np.errstate(invalid="ignore"):
        rw = np.exp(case["logw"].astype(t)[:, None] + ld - out["lp"][None, :]) * coef
    grad = np.zeros((n, d), t)
    for i in range(k):
        grad += _matmul(rw[i][:, None] * z[i], linv[i], split)
    out["grad"] = grad
    assert all(v.dtype == t for v in out.values())
    return {key: v.astype(np.float64) for key, v in out.items()}


# ---- planted faults ------------------------------------------------------------------------------------------------------------------
def planted_faults(case):
    """[(name, argument)]: what a subtly wrong sweep would compute, each applicable to this case --
    last_range_left_out c         the last component range of chunk c missing from the gradient
    slab_added_twice c            the first range of chunk c added twice
    chunk_overwrites              the last chunk overwriting the gradient instead of accumulating
    second_tile_norm_left_out     |z|^2 without the partial of the second column tile
    ragged_row_takes_neighbour    the last sample of a ragged row tile given the values of its neighbour
    coefficient_from_chunk_0      the Student-t coefficient of chunk 1 taken from q of chunk 0
    lp2_from_logw                 the second mixture formed with the first weights
    floor_weight_dropped_from_lp  the component whose log weight is -100 dropped from lp
    gradient_lp_without_last      lp of the gradient pass taken without the last component"""
    geo = case_geometry(case)
    chunks = geo["chunks"]
    faults = []
    if geo["ctiles"] > 1:
        faults.append(("second_tile_norm_left_out", None))
    if case["n"] % 128 and case["n"] > 1:
        faults.append(("ragged_row_takes_neighbour", None))
    if case["kind"] == "far" and case["family"] == "gauss":
        # |ld| ~ 1e7: one fp32 ulp of ld is about a nat, weights and responsibilities lie below the resolution of the
        # densities -- only the faults that move ld itself apply
        return faults
    faults.append(("lp2_from_logw", None))
    for c in sorted({0, len(chunks) - 1}):
        if chunks[c][2] > 1:
            faults += [("last_range_left_out", c), ("slab_added_twice", c)]
    if len(chunks) > 1:
        faults.append(("chunk_overwrites", None))
        if case["family"] == "student_t":
            faults.append(("coefficient_from_chunk_0", None))
    if case["kind"] == "far_weights":
        faults.append(("floor_weight_dropped_from_lp", None))
    if case["k"] >= 2:
        faults.append(("gradient_lp_without_last", None))
    return faults


def error_ratio(got, ref, bound):
    """max |got - ref| / (EPS32 B) over the elements with a finite reference; elements whose reference is not finite (-inf in lp
    where every weight is -inf) must agree exactly, else inf."""
    g, r, b = (np.asarray(v, np.float64) for v in (got, ref, bound))
    exact = ~np.isfinite(r)
    if not np.all(g[exact] == r[exact]):
        return np.inf
    if not np.any(~exact):
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(g - r)[~exact] / (EPS32 * b[~exact])
    return float(np.max(np.where(np.isnan(q), np.inf, q)))
