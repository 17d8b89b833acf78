"""Inputs, reference quantities, error measure, float32 model and planted faults shared by test_hip_more.py (GPU),
more_route_child.py and test_more_cases_cpu.py: the MORE estimators (csrc/more.hip register and tiled routes, more_blocked.hip,
more_diag.hip, more_common.h) on THEIR OWN inputs.  Nothing here touches the device.

The entry points read mu, L (or sigma), x, ld, bg, tlp, log q, the mapping and the ridge as plain arrays.  Every array of a case
is fp32-representable fp64 (f32()); ld, bg and log q are built directly (no mixture is evaluated), so the device and the
reference read the same numbers and the log weights a = ld - bg can be shaped freely.

The measure is the NORMAL-EQUATION RESIDUAL of the device's own answer, not its distance to a reference solve: the forward
error of a ridge regression grows with its conditioning (N < F with ridge 1e-12 has no useful forward bound), the residual does
not.  Per component, with W the whitening operator the kernel used (whitening()), z_n = W (x_n - mu), phi_n the feature row,
w_n the importance weights (weights()), r_n = tlp_n - log q_n, Lambda = lambda I' (zero at the bias):

    theta   the whitened coefficients of the device's fp32 (H, g): Q~ = W^-T H W^-1 symmetrised, theta_ii = -Q~_ii / 2,
            theta_ij = -Q~_ij, theta_lin = -W^-T g; the bias (not an output) from the bias row of the normal equations
    rho     Phi^T (w (Phi theta - r)) + Lambda theta                         two matrix-vector products, A is never built
    B_f     sum_n w_n |phi_nf| (|r_n| + sum_g |phi_ng| |theta_g|) + lambda |theta_f| + [(|A| + Lambda) theta_out]_f,
            theta_out the feature image of |W^-T| |H| |W^-1| and |W^-T| |g| (the rounding of the outputs to fp32)
    ratio   max_f |rho_f| / (EPS B_f),  EPS = 2^-24, over every row but the bias                          residual_ratio()

    model_f32(case, wh)          the kernels' formulation in NumPy float32 (substitution or L^-1 product, exp(0.5 (a - lse)), the
                                 two products of a feature row), fp64 Gram and solve, outputs rounded to fp32
    estimate(case, wh, fault)    the fp64 answer (fault=None: the reference) or what a subtly wrong kernel would compute
    planted_faults(case)         [(name, argument)] applicable to the case

C is not tuned on the device: per law class it is 8 times the largest ratio of model_f32 over case_table() + child_table(),
measured on the reference alone and rounded up (the fp64 solve may round an output the other way on another host).
test_more_cases_cpu.py asserts the figures and that every planted fault pushes some row beyond FAULT_FACTOR C EPS B on every
case designated for it:

    class            largest ratio of model_f32     where                                         RATIO_F32    C
    register         0.60                           D = 1, K = 1, N = 64                          1            8
    tiled            0.028                          D = 33, K = 2, N = 63                         0.05         0.4
    blocked          0.013                          D = 127, K = 1, N = 64                        0.025        0.2
    diag             0.51                           D = 300, K = 2, N = 64                        0.8          6.4
    tiled, offset    0.093                          D = 22, K = 3, N = 600, rewards - 1e4         0.2          1.6
    blocked, offset  0.25                           D = 64, K = 3, N = 130, rewards - 1e4         0.4          3.2
One constant does not fit all: B sums absolute values over F features where the rounding errors of the feature rows are
independent, so the ratio falls with F (dense routes: 0.6 at F = 3, 0.03 at F = 300, 0.01 at F = 2 000 and more).  The
rounding of a reward of size 1e4 (2^-24 x 1e4 per sample) is the same number in every feature row of its sample: it does not
average out over F, and the offset cases of the two large-F routes get a class of their own (on the register and diagonal
routes they stay below the route's figure: 0.07 and 0.21).  Log weights over [-120, 60] and [-60, 40] stay below these figures
(0.23 at most, diagonal route), and so does a row-scaled factor L of condition 1e3 (0.12 at most, register route): B needs no
term of its own for the rounding of ld - bg or for the forward substitution.
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import logsumexp

EPS = 2.0 ** -24
# worst ratio of model_f32 per law class over case_table() + child_table(), rounded up (test_more_cases_cpu.py)
RATIO_F32 = {"register": 1.0, "tiled": 0.05, "blocked": 0.025, "diag": 0.8, "tiled-offset": 0.2, "blocked-offset": 0.4}
C = {cls: 8.0 * r for cls, r in RATIO_F32.items()}
FAULT_FACTOR = 10.0

ROUTES = ("register", "tiled", "blocked", "diag")
KINDS = ("normal", "plain", "own", "ownplain", "neginf", "nonfinite", "nonfiniteown", "lam12", "lam05", "lam05plain", "wide",
         "wideplain", "offset", "cond")
MAP_BASE = 7                             # the mapping holds data-base indices: component + MAP_BASE, map_offset = -MAP_BASE
TB = 128                                 # block edge of G and panel width (more_common.h)


def f32(a):
    """fp32-representable fp64 values: the device and the reference read the same numbers."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def law_class(spec):
    offset = spec["kind"] == "offset" and spec["route"] in ("tiled", "blocked")
    return spec["route"] + ("-offset" if offset else "")


def bound_constant(spec):
    return C[law_class(spec)]


# ---- the dispatch arithmetic of the routes, restated (the seams below are placed by it) ------------------------------------------
PADDED_DIMS = (2, 4, 8, 10, 12, 16, 20, 24, 32, 40, 50, 64)
REGISTER_MAX_DIM = 21
REGISTER_PP = {2: 1, 4: 1, 8: 1, 10: 2, 12: 3, 16: 7, 20: 15, 24: 17}      # gmmvi_more: (DP, PP) instances
TILED_CLASSES = (24, 32, 40, 50, 64)


def padded_dim(d):
    return next(dp for dp in PADDED_DIMS if d <= dp)


def n_features(d, diag=False):
    return 2 * d + 1 if diag else d * (d + 1) // 2 + d + 1


def pick_chunks(k, cus, tiles):
    """csrc/more.hip more_pick_chunks."""
    best, best_eff = 1, 0.0
    hi = 1 if tiles < 4 else tiles // 4
    c = 1
    while c <= hi and c * k <= 6 * cus:
        wgs = c * k
        eff = wgs / (((wgs + cus - 1) // cus) * cus)
        enough = wgs >= cus or c == hi
        score = eff if enough else eff * 0.5
        if score > best_eff + 1e-9:
            best_eff, best = score, c
        c += 1
    return best


def register_geometry(d, k, n, num_cus=256):
    """csrc/more.hip launch_more -> dict(DP, PP, F, nb = 16-row tiles of G, pairs = lower-triangular tile pairs (<= 8 PP),
    tiles, chunks, tpc = tiles per chunk, short = tiles of the last chunk if it is shorter, else 0)."""
    dp = padded_dim(d)
    f = n_features(d)
    nb = (f + 1 + 15) // 16
    tiles = (n + 63) // 64
    chunks = pick_chunks(k, num_cus, tiles)
    tpc = (tiles + chunks - 1) // chunks
    chunks = (tiles + tpc - 1) // tpc
    last = tiles - (chunks - 1) * tpc
    return dict(DP=dp, PP=REGISTER_PP[dp], F=f, nb=nb, pairs=nb * (nb + 1) // 2, tiles=tiles, chunks=chunks, tpc=tpc,
                short=last if last < tpc else 0)


def tiled_geometry(d, n):
    """csrc/more.hip launch_more_big -> dict(DP, F, nblk = 128-row blocks of G, LDG, tiles, passes = four-tile staging passes)."""
    f = n_features(d)
    nblk = (f + 1 + TB - 1) // TB
    tiles = (n + 63) // 64
    return dict(DP=padded_dim(d), F=f, nblk=nblk, LDG=TB * nblk, tiles=tiles, passes=(tiles + 3) // 4)


def _align256(b):
    return (b + 255) // 256 * 256


def panel_geometry(route, d, k, n, ws_gb=8.0):
    """more_common.h more_panel_plan and gmmvi_more_panel_cholesky -> dict(F, nblk, LDG, panels, tiles, per_comp = workspace
    bytes of a component, KG = components per group under GMMVI_MORE_WS_GB, groups, last = size of the last group)."""
    diag = route == "diag"
    f = n_features(d, diag)
    nblk = (f + 1 + TB - 1) // TB
    ldg = TB * nblk
    tiles = (n + 63) // 64
    per_comp = ldg * ldg * 8 + _align256(tiles * (d + 3) * 64 * 4) + _align256(ldg * 8) + _align256(0 if diag else d * d * 8)
    fixed = 2 * _align256(k * 4)
    budget = int(ws_gb * (1 << 30))
    kg = max(1, (budget - fixed) // per_comp if budget > fixed else 0)
    kg = min(kg, k)
    return dict(F=f, nblk=nblk, LDG=ldg, panels=(f + TB - 1) // TB, tiles=tiles, per_comp=per_comp, KG=kg,
                groups=(k + kg - 1) // kg, last=k - (k - 1) // kg * kg)


def ws_gb_for_groups_of(route, d, k, n, kg):
    """A GMMVI_MORE_WS_GB under which more_panel_plan makes groups of ``kg`` components."""
    g = panel_geometry(route, d, k, n)
    return ((kg + 0.5) * g["per_comp"] + 2 * _align256(k * 4)) / float(1 << 30)


# (chunks, tiles per chunk, short last chunk) of one more_gram launch: the eight-tile staging pass alone (4, 7, 8), a second pass
# of one tile (9), three passes (17); two and three chunk partials in more_solve's slab sum, with a full and a short last chunk
CHUNK_SHAPES = ((1, 4, False), (1, 7, False), (1, 8, False), (1, 9, False), (1, 17, False), (2, 4, False), (2, 5, True),
                (3, 4, False), (3, 5, True), (2, 8, False), (2, 9, True))


def shape_for_chunks(chunks, tpc, short, d, num_cus=256):
    """The first (K, N) over K = 1, 2, CUs / 3, CUs / 2, CUs and up to 40 tiles at which launch_more gives this chunk shape on a
    device with ``num_cus`` compute units, or None."""
    for k in (1, 2, num_cus // 3, num_cus // 2, num_cus):
        if k < 1:
            continue
        for tiles in range(1, 41):
            n = 64 * tiles - 37
            g = register_geometry(d, k, n, num_cus)
            if (g["chunks"], g["tpc"], bool(g["short"])) == (chunks, tpc, short):
                return k, n
    return None


# ---- the case table --------------------------------------------------------------------------------------------------------------
def _spec(route, d, k, n, kind="normal", tag="", **extra):
    return dict(route=route, d=d, k=k, n=n, kind=kind, id=f"{route}-{tag + '-' if tag else ''}D{d}-K{k}-N{n}-{kind}", **extra)


REGISTER_DIMS = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21)
REGISTER_NS = (1, 63, 64, 65)
CHUNK_DIMS = (4, 21)                     # PP = 1 and the full tile-pair budget of the DP = 24 instance (136 = 8 x 17)
TILED_DIMS = (22, 24, 25, 30, 31, 32, 33, 40, 41, 43, 44, 50)
REPACKED_DIMS = (51, 63)                 # blocked-layout blocks re-packed by default; register layout under GMMVI_BLOCKED_ABOVE=64
# 1, 3, 4, 5 and 9 tiles (a four-tile staging pass alone, one more tile, two passes and one tile); N mod 64 = 1, 63, 0, 0, 1, 63
TILED_NS = (1, 63, 192, 256, 257, 575)
BLOCKED_SHAPES = tuple((d, 2 if d <= 67 else 1, n) for d in (64, 65, 67, 96, 127) for n in (64, 65, 257)) + ((128, 1, 130),)
DIAG_DIMS = (1, 2, 63, 64, 65, 127, 128, 129, 300, 1023, 1024)
DIAG_NS = (1, 64, 65, 200)
# the weight, ridge, reward and factor shapes run at one small D of every route (K = 3: the own sets need an empty component)
KIND_SHAPES = {"register": (5, 3, 130), "tiled": (22, 3, 600), "blocked": (64, 3, 130), "diag": (65, 3, 200)}
SHORT_N = {"register": 15, "tiled": 130, "blocked": 130, "diag": 64}         # N < F for the ridge of 1e-12


def case_table():
    t = []
    t += [_spec("register", d, k, n) for d in REGISTER_DIMS for k in (1, 3) for n in REGISTER_NS]
    t += [_spec("register", d, 0, 0, tag=f"chunks{c}x{tpc}{'s' if short else ''}", chunk_shape=(c, tpc, short))
          for d in CHUNK_DIMS for c, tpc, short in CHUNK_SHAPES]
    t += [_spec("tiled", d, 2, n) for d in TILED_DIMS + REPACKED_DIMS for n in TILED_NS]
    t += [_spec("blocked", d, k, n) for d, k, n in BLOCKED_SHAPES]
    t += [_spec("diag", d, 2, n) for d in DIAG_DIMS for n in DIAG_NS]
    for route, (d, k, n) in KIND_SHAPES.items():
        t += [_spec(route, d, k, SHORT_N[route] if kind == "lam12" else n, kind, tag="shape") for kind in KINDS[1:]]
    return t


def child_table():
    """Cases of the child process (more_route_child.py) under GMMVI_BLOCKED_ABOVE=64: D = 51 and 63 packed in the register
    layout, and one blocked call whose workspace budget makes groups of two components out of three (a ragged last group)."""
    t = [_spec("tiled", d, 2, n, tag="reglayout") for d in REPACKED_DIMS for n in TILED_NS]
    t.append(_spec("blocked", 65, 3, 65, tag="groups2", ws_gb=ws_gb_for_groups_of("blocked", 65, 3, 65, 2)))
    return t


def spec_by_id(case_id):
    return next(s for s in case_table() + child_table() if s["id"] == case_id)


def resolve(spec, num_cus=256):
    """The chunk cases take K and N from the compute units of the device: -> spec with k, n set, or None if ``num_cus`` cannot
    produce the chunk shape."""
    if "chunk_shape" not in spec:
        return spec
    kn = shape_for_chunks(*spec["chunk_shape"], d=spec["d"], num_cus=num_cus)
    return None if kn is None else dict(spec, k=kn[0], n=kn[1])


def snis_of(spec):
    return spec["kind"] not in ("plain", "ownplain", "lam05plain", "wideplain")


def own_of(spec):
    return spec["kind"] in ("own", "ownplain", "nonfiniteown")


def seam_indices(spec):
    """The last sample of a 64-sample tile and the first of the next, the ends of a four- and an eight-tile staging pass, the
    ends of the first chunk, and sample N - 1."""
    n = spec["n"]
    s = {0, 63, 64, 255, 256, 511, 512, n - 1}
    if spec["route"] == "register":
        tpc = register_geometry(spec["d"], spec["k"], n)["tpc"]
        s |= {64 * tpc - 1, 64 * tpc}
    return sorted(i for i in s if 0 <= i < n)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_case(spec):
    """-> dict of fp32-representable fp64 arrays: means [K, D], chols [K, D, D] (sigma [K, D] on the diagonal route), x [N, D],
    ld [K, N], bg, tlp, logq [N], mapping [N] int32, map_offset, l2 [K]; snis, own (bool), seams, dead (samples without weight
    under every component).  ``spec`` must be resolved (resolve())."""
    route, d, k, n, kind = spec["route"], spec["d"], spec["k"], spec["n"], spec["kind"]
    rng = np.random.default_rng([ROUTES.index(route), KINDS.index(kind), d, k, n])
    diag = route == "diag"
    case = dict(spec, snis=snis_of(spec), own=own_of(spec), diag=diag)
    comp = rng.integers(0, k, size=n)
    means = rng.normal(size=(k, d)) * 3.0
    eps = rng.normal(size=(n, d))
    # "cond" and "lam12": one factor for all components and means 0.3 whitened units apart, so that every sample is of ordinary
    # size in every component's whitened frame, as the samples that carry weight are in a run.  Under a factor of condition
    # 1e3 a sample of another component would be 1e3 times further out; with N < F and a ridge of 1e-12 features of 20^2 put
    # entries of 1e5 into G, whose fp64 rounding (1e-11) exceeds the ridge: the system handed to the Cholesky is then indefinite
    # as data (NumPy's fp64 Cholesky refuses it as well), and NaN is the documented answer
    shift = 0.3 * rng.normal(size=(k, d))
    near = kind in ("cond", "lam12")
    if diag:
        sigma = np.exp(0.5 * rng.normal(size=(k, d)))
        if kind == "cond":
            sigma = np.tile(10.0 ** rng.uniform(-3.0, 0.0, size=d), (k, 1))
            sigma[:, 0], sigma[:, -1] = 1.0, 1e-3
        if near:
            sigma[:] = sigma[0]
            means = means[0] + sigma * shift
        means, sigma = f32(means), f32(sigma)
        case.update(means=means, sigma=sigma)
        x = means[comp] + sigma[comp] * eps
    else:
        chols = np.empty((k, d, d))
        for i in range(k):
            a = rng.normal(size=(d, d))
            chols[i] = np.linalg.cholesky(a @ a.T / d + 0.3 * np.eye(d))           # the law of test_hip_kernels.random_gmm
        if kind == "cond":
            # condition 1e3 by row scaling, L = diag(s) L_0 with s from 1 down (variables of different units).  A factor whose
            # condition comes from a rotation loses the whitened coefficients in the fp32 rounding of H itself: theta_out then
            # exceeds |theta| by up to cond^2 and the measure, rightly, has that much slack -- no case for a sharp bound
            lo, hi = 0.0, 4.0
            for _ in range(40):
                e = 0.5 * (lo + hi)
                lo, hi = (e, hi) if np.linalg.cond(np.logspace(0.0, -e, d)[:, None] * chols[0]) < 1e3 else (lo, e)
            chols[0] = np.logspace(0.0, -lo, d)[:, None] * chols[0]
        if near:
            chols[:] = chols[0]
            means = means[0] + shift @ chols[0].T
        means, chols = f32(means), f32(chols)
        case.update(means=means, chols=chols)
        x = means[comp] + np.stack([chols[c] @ e for c, e in zip(comp, eps)])
    seams = seam_indices(spec)
    a = rng.normal(size=(k, n))
    a[:, seams] = 3.0 + 0.5 * rng.normal(size=(k, len(seams)))                     # the seam samples carry real weight
    if kind in ("wide", "wideplain"):
        # the weight sits on the seam samples and a tenth of the others (within three nats of the top), a tenth lies 10 ... 40
        # nats below, the rest down to the bottom of the range
        top, bottom = (60.0, -120.0) if kind == "wide" else (40.0, -60.0)
        a = rng.uniform(bottom, top - 90.0, size=(k, n))
        u = rng.random((k, n))
        a[u < 0.2] = rng.uniform(top - 40.0, top - 10.0, size=int((u < 0.2).sum()))
        a[u < 0.1] = top - rng.uniform(0.0, 3.0, size=int((u < 0.1).sum()))
        a[:, seams] = top - rng.uniform(0.0, 3.0, size=(k, len(seams)))
        a[:, seams[0]] = top
        if n > len(seams):
            a[0, [i for i in range(n) if i not in seams][0]] = bottom
    bg = f32(rng.normal(size=n) * 2.0 - 12.0)
    ld = f32(a + bg[None, :])
    dead = np.zeros(n, bool)
    if kind == "neginf":
        gone = rng.random(n) < 1.0 / 3.0
        gone[seams] = False
        ld[k // 2, gone] = -np.inf
    mapping = comp.copy()
    if case["own"]:
        # component 1 has no sample, component K - 1 only row N - 1, the others share the rest
        others = [c for c in range(k) if c not in (1, k - 1)]
        mapping = np.asarray(others)[rng.integers(0, len(others), size=n)]
        mapping[n - 1] = k - 1
    if kind in ("nonfinite", "nonfiniteown"):
        dead = rng.random(n) < 1.0 / 3.0
        dead[seams] = False
        ld[:, dead] = -np.inf
        if case["own"]:
            mapping[dead] = k + 5                                                  # the sample of a component that is not here
    # rewards of ordinary size: a few units, at least four on the seam samples
    logq = f32(rng.normal(size=n) * 2.0 - 8.0)
    tlp = f32(logq + rng.normal(size=n) * 3.0 - 1.0)
    tlp[seams] = f32(logq[seams] + 4.0 + rng.uniform(0.0, 2.0, size=len(seams)))
    if kind == "offset":
        tlp = f32(tlp - 1.0e4)
    lam = {"lam12": 1e-12, "lam05": 0.5, "lam05plain": 0.5}.get(kind, 1e-6)
    if kind == "wideplain":
        lam = 1e-6 * np.exp(40.0)            # the ridge of the self-normalised case, in the units of weights up to e^40
    case.update(x=f32(x), ld=ld, bg=bg, tlp=tlp, logq=logq, mapping=(mapping + MAP_BASE).astype(np.int32), map_offset=-MAP_BASE,
                l2=f32(np.full(k, lam)), seams=seams, dead=dead)
    return case


def with_nonfinite(case):
    """The same case with NaN, +inf and -inf in x, tlp and logq of the samples without weight (case["dead"])."""
    out = dict(case)
    idx = np.where(case["dead"])[0]
    vals = np.array([np.nan, np.inf, -np.inf])
    for j, name in enumerate(("x", "tlp", "logq")):
        arr = case[name].copy()
        if arr.ndim == 2:
            arr[idx, :] = vals[(np.arange(idx.size)[:, None] + np.arange(arr.shape[1])[None, :] + j) % 3]
        else:
            arr[idx] = vals[(np.arange(idx.size) + j) % 3]
        out[name] = arr
    return out


# ---- reference quantities ------------------------------------------------------------------------------------------------------------
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


def whitening(case, packed=None):
    """The whitening operator of the route, fp32-representable: register / tiled L from chols; blocked the dense fp32 L^-1 (read
    back from the packed blocks ``packed`` [K, stride], else computed in float32 here); diagonal the fp32 1 / sigma (read back,
    else computed here).  -> dict(winv [K, D, D] or [K, D]: z = winv (x - mu); m: its inverse, the un-whitening factor)."""
    route, d, k = case["route"], case["d"], case["k"]
    if route == "diag":
        rs = packed[:, d:2 * d].astype(np.float64) if packed is not None else \
            (np.float32(1.0) / case["sigma"].astype(np.float32)).astype(np.float64)
        return dict(winv=rs, m=1.0 / rs)
    eye = np.eye(d)
    if route == "blocked":
        ofs = (d + 1 + 3) // 4 * 4
        linv = packed[:, ofs:ofs + d * d].reshape(k, d, d).astype(np.float64) if packed is not None else \
            np.stack([_tri_inverse_f32(c) for c in case["chols"]]).astype(np.float64)
        linv = np.tril(linv)
        return dict(winv=linv, m=np.stack([solve_triangular(w, eye, lower=True) for w in linv]))
    return dict(winv=np.stack([solve_triangular(c, eye, lower=True) for c in case["chols"]]), m=case["chols"])


def features(z, diag):
    """Dense: [z_i z_j (i <= j, row-major upper triangle), z, 1] (least_squares.py:113-124); diagonal: [z^2, z, 1]."""
    n, d = z.shape
    one = np.ones((n, 1), z.dtype)
    if diag:
        return np.concatenate([z * z, z, one], axis=1)
    return np.concatenate([z[:, i:i + 1] * z[:, i:] for i in range(d)] + [z, one], axis=1)


def log_weights(case, k, dtype=np.float64, map_offset=None):
    """[N]: ld[k] - bg, or 0 over the component's own samples and -inf elsewhere (more_weight_reward)."""
    if case["own"]:
        ofs = case["map_offset"] if map_offset is None else map_offset
        return np.where(case["mapping"] + ofs == k, 0.0, -np.inf).astype(dtype)
    with np.errstate(invalid="ignore"):
        return case["ld"][k].astype(dtype) - case["bg"].astype(dtype)


def weights(a, snis):
    """ng_estimator.py:353-358 with its double normalisation: exp(a - logsumexp a) divided by its sum, or exp(a)."""
    if not np.any(a > -np.inf):
        return np.zeros_like(a)
    if not snis:
        return np.exp(a)
    w = np.exp(a - logsumexp(a))
    return w / w.sum()


def ridge_solve(rows, rhs, lam, bias_reg=0.0):
    """theta of (Phi^T Phi + lam I' + bias_reg e_b e_b^T) theta = Phi^T rhs for the weighted rows ``rows`` [n, F] (bias last),
    fp64.  With n + 1 < F and F large the solution lies in the row space of the non-bias columns: it is solved there (the
    same ridge problem in an orthonormal basis of that space, n + 1 unknowns)."""
    n, f = rows.shape
    reg = np.full(f, lam)
    reg[-1] = bias_reg
    if f <= 640 or n + 1 >= f:
        return np.linalg.solve(rows.T @ rows + np.diag(reg), rows.T @ rhs)
    q, r = np.linalg.qr(rows[:, :-1].T)                                     # [F - 1, n], [n, n]: rows = [r^T q^T, bias]
    red = np.concatenate([r.T, rows[:, -1:]], axis=1)
    c = ridge_solve(red, rhs, lam, bias_reg) if n + 1 <= 640 else \
        np.linalg.solve(red.T @ red + np.diag(np.r_[np.full(n, lam), bias_reg]), red.T @ rhs)
    return np.concatenate([q @ c[:-1], c[-1:]])


def _quad_indices(d):
    iu = np.triu_indices(d)
    return iu, np.where(iu[0] == iu[1])[0]


def theta_from_outputs(h, g, m, diag):
    """The whitened coefficients [quadratic, linear] (no bias) of one component's (H, g), fp64; ``m`` = W^-1."""
    if diag:
        return np.concatenate([-0.5 * h * m * m, -m * g])
    q = m.T @ h @ m
    q = 0.5 * (q + q.T)
    iu, on_diag = _quad_indices(h.shape[0])
    quad = -q[iu]
    quad[on_diag] *= 0.5
    return np.concatenate([quad, -(m.T @ g)])


def outputs_from_theta(theta, winv, diag, fault=None):
    """(H, g) of one component from [quadratic, linear, bias] (least_squares.py:177-189, ng_estimator.py:369-373), fp64."""
    d = winv.shape[-1]
    name = fault[0] if fault else None
    gsign = 1.0 if name == "g_sign" else -1.0
    dfac = -1.0 if name == "diagonal_factor" else -2.0
    if diag:
        return dfac * theta[:d] * winv * winv, gsign * theta[d:2 * d] * winv
    t2 = d * (d + 1) // 2
    qt = np.zeros((d, d))
    if name == "feature_order":
        qt.T[np.tril_indices(d)] = theta[:t2]              # the coefficients read in the order of the lower triangle
    else:
        qt[np.triu_indices(d)] = theta[:t2]
    q = -(qt + qt.T)
    q[np.diag_indices(d)] *= dfac / -2.0
    lin = theta[t2:t2 + d]
    if name == "l_for_lt":
        return winv @ q @ winv.T, gsign * (winv @ lin)
    return winv.T @ q @ winv, gsign * (winv.T @ lin)


def _dropped(case, fault):
    """Sample indices a drop fault leaves out."""
    name, arg = fault
    n = case["n"]
    if name == "drop_sample":
        return np.array([arg])
    if name == "drop_tile":
        return np.arange(64 * arg, min(n, 64 * (arg + 1)))
    tpc = register_geometry(case["d"], case["k"], n)["tpc"]
    return np.arange(64 * tpc * arg, min(n, 64 * tpc * (arg + 1)))


def estimate(case, wh, fault=None):
    """The fp64 MORE estimate from the case's arrays and the whitening ``wh`` -> (H_neg [K, D, D] or [K, D], g_neg [K, D]); NaN
    for a component without a weighted sample.  ``fault``: (name, argument) of planted_faults."""
    k, d, diag = case["k"], case["d"], case["diag"]
    name = fault[0] if fault else None
    hs = np.full((k, d) if diag else (k, d, d), np.nan)
    gs = np.full((k, d), np.nan)
    for i in range(k):
        a = log_weights(case, i, map_offset=case["map_offset"] + 1 if name == "map_offset" else None)
        if name in ("drop_sample", "drop_tile", "drop_chunk"):
            a = a.copy()
            a[_dropped(case, fault)] = -np.inf
        w = weights(a, case["snis"] and name != "weights_not_normalised")
        live = w > 0
        if not live.any():
            continue
        mu = case["means"][(i + 1) % k if name == "neighbour_mean" else i]
        dx = case["x"][live] - mu
        z = dx * wh["winv"][i] if diag else dx @ wh["winv"][i].T
        rew = case["tlp"][live] - (case["ld"][i][live] if name == "ld_in_reward" else case["logq"][live])
        sw = np.sqrt(w[live])
        lam = case["l2"][i]
        theta = ridge_solve(sw[:, None] * features(z, diag), sw * rew, lam, bias_reg=lam if name == "ridge_on_bias" else 0.0)
        hs[i], gs[i] = outputs_from_theta(theta, wh["winv"][i], diag, fault)
    return hs, gs


def model_f32(case, wh):
    """The kernels' own formulation in NumPy float32: x - mu, the forward substitution with the reciprocal diagonal (register,
    tiled) or the product with the fp32 L^-1 (blocked) or 1 / sigma (diagonal), the fp32 log-normaliser, sqrt(w) =
    exp(0.5 (a - lse)), the reward, the two products (sw phi_a) phi_b of a feature row; then the Gram matrix and the solve in
    fp64 and the outputs rounded to fp32."""
    t = np.float32
    k, d, diag, route = case["k"], case["d"], case["diag"], case["route"]
    hs = np.full((k, d) if diag else (k, d, d), np.nan, t)
    gs = np.full((k, d), np.nan, t)
    x = case["x"].astype(t)
    for i in range(k):
        a = log_weights(case, i, t)
        live = a > -np.inf
        if not live.any():
            continue
        lse = t(0.0)
        if case["snis"]:
            top = a[live].max()
            lse = top + np.log(np.exp(a[live] - top).sum(dtype=t))
        sw = np.exp(t(0.5) * (a[live] - lse)).astype(t)
        dx = x[live] - case["means"][i].astype(t)
        # the sums run over j in the kernels' order, one float32 operation at a time (no BLAS: the same figures on every host)
        z = np.zeros_like(dx)
        if diag:
            z = dx * wh["winv"][i].astype(t)
        elif route == "blocked":
            linv = wh["winv"][i].astype(t)
            for r in range(d):
                for j in range(r + 1):
                    z[:, r] += linv[r, j] * dx[:, j]
        else:
            lo = case["chols"][i].astype(t)
            rd = t(1.0) / np.diag(lo)
            for r in range(d):
                acc = dx[:, r].copy()
                for j in range(r):
                    acc -= lo[r, j] * z[:, j]
                z[:, r] = acc * rd[r]
        rew = (case["tlp"].astype(t) - case["logq"].astype(t))[live]
        keep = sw > 0
        sw, z, rew = sw[keep], z[keep], rew[keep]
        if diag:
            swz = sw[:, None] * z
            rows = np.concatenate([swz * z, swz, sw[:, None]], axis=1)
        else:
            rows = np.concatenate([(sw[:, None] * z[:, r:r + 1]) * z[:, r:] for r in range(d)] + [sw[:, None] * z, sw[:, None]],
                                  axis=1)
        assert rows.dtype == t
        theta = ridge_solve(rows.astype(np.float64), (sw * rew).astype(np.float64), case["l2"][i])
        h, g = outputs_from_theta(theta, wh["winv"][i], diag)
        hs[i], gs[i] = h.astype(t), g.astype(t)
    return hs, gs


def residual_ratio(case, wh, h, g, per_component=False):
    """max over the components and rows (bias excluded) of |rho_f| / (EPS B_f) for the outputs (h, g); inf where a component with
    weighted samples is not finite, where one without is not NaN in every element, or where B = 0 and rho != 0."""
    k, d, diag = case["k"], case["d"], case["diag"]
    worst = []
    for i in range(k):
        hi, gi = np.asarray(h[i], np.float64), np.asarray(g[i], np.float64)
        w = weights(log_weights(case, i), case["snis"])
        live = w > 0
        if not live.any():
            worst.append(0.0 if np.isnan(hi).all() and np.isnan(gi).all() else np.inf)
            continue
        if not (np.isfinite(hi).all() and np.isfinite(gi).all()):
            worst.append(np.inf)
            continue
        w = w[live]
        dx = case["x"][live] - case["means"][i]
        z = dx * wh["winv"][i] if diag else dx @ wh["winv"][i].T
        phi = features(z, diag)
        r = case["tlp"][live] - case["logq"][live]
        lam = case["l2"][i]
        m = wh["m"][i]
        th = theta_from_outputs(hi, gi, m, diag)
        bias = (w @ (r - phi[:, :-1] @ th)) / w.sum()
        theta = np.append(th, bias)
        reg = np.append(np.full(th.size, lam), 0.0)
        rho = phi.T @ (w * (phi @ theta - r)) + reg * theta
        th_out = np.append(np.abs(theta_from_outputs(np.abs(hi), np.abs(gi), np.abs(m), diag)), 0.0)
        aphi = np.abs(phi)
        b = aphi.T @ (w * (np.abs(r) + aphi @ (np.abs(theta) + th_out))) + reg * (np.abs(theta) + th_out)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(b[:-1] > 0, np.abs(rho[:-1]) / (EPS * b[:-1]), np.where(rho[:-1] == 0, 0.0, np.inf))
        worst.append(float(q.max()))
    return worst if per_component else max(worst)


def forward_deviation(h, g, ref):
    """Largest |device - reference| over a component's largest reference entry, for (H, g): printed, never asserted."""
    out = []
    for got, r in zip((h, g), ref):
        dev = 0.0
        for gi, ri in zip(np.asarray(got, np.float64), r):
            if np.isfinite(ri).all() and np.isfinite(gi).all() and np.abs(ri).max() > 0:
                dev = max(dev, float(np.abs(gi - ri).max() / np.abs(ri).max()))
        out.append(dev)
    return out


def planted_faults(case):
    """[(name, argument)]: what a subtly wrong kernel would compute, each applicable to this case --
    drop_sample i            the weighted sample at seam index i left out
    drop_tile t              the 64 samples of tile t left out
    drop_chunk c             the partial Gram matrix of sample chunk c left out (register route, more than one chunk)
    weights_not_normalised   exp(a) where exp(a - lse) is right: shows through the ridge only (lambda = 0.5, self-normalised)
    ridge_on_bias            lambda on the bias row as well: shows through the ridge only (lambda = 0.5 against weights of sum 1)
    neighbour_mean           whitened around the next component's mean
    l_for_lt                 H = L^-1 Q L^-T, g = -L^-1 lin: L for L^T in the un-whitening
    diagonal_factor          -1 for -2 on the diagonal of Q
    feature_order            the quadratic coefficients read in the order of the lower triangle
    g_sign                   g with the wrong sign
    map_offset               the mapping shifted by one component
    ld_in_reward             tlp - ld[k] for tlp - log q"""
    n, d, k, kind = case["n"], case["d"], case["k"], case["kind"]
    dense = not case["diag"]
    faults = [("drop_sample", i) for i in case["seams"]]
    if n > 64:
        faults.append(("drop_tile", 1))
    if case["route"] == "register" and register_geometry(d, k, n)["chunks"] > 1:
        faults.append(("drop_chunk", 1))
    if kind == "lam05":
        faults += [("ridge_on_bias", None), ("weights_not_normalised", None)]
    if k >= 2:
        faults.append(("neighbour_mean", None))
    if dense and d >= 2:
        faults.append(("l_for_lt", None))
    if dense and d >= 3:
        faults.append(("feature_order", None))
    faults += [("diagonal_factor", None), ("g_sign", None)]
    if case["own"]:
        faults.append(("map_offset", None))
    if kind in ("normal", "plain", "lam05", "offset", "cond"):
        faults.append(("ld_in_reward", None))
    return faults
