"""Inputs, fp64 reference, error measure and planted faults shared by test_hip_update.py (GPU), update_route_child.py and
test_update_cases_cpu.py: the natural-gradient component updates (csrc/update_kl.hip, csrc/update.hip, gmmvi_blocked_update_kl /
gmmvi_blocked_update_plain in csrc/blocked_update.hip) on THEIR OWN inputs.  Nothing here touches the device.

A case is a dict(id, route, law, d, k, seed, mode ("kl" / "direct" / "iblr"), temperature, H_neg, g_neg, stepsizes, rounds);
every array is fp32-representable fp64 (f32()).  ``rounds`` is a list of dict(means, chols, last_eta, l2, num_updates) -- the
state the round starts from -- with the fp64 result of oracle.updaters on exactly that state under ``ref``.  The second round
starts from the first round's fp64 result ROUNDED TO FP32: the GPU test uploads that state for the warm round instead of
continuing from the device's own result, so that both sides read the same numbers in every round.

Error measure (all in fp64, the same for every route; element-wise rtol on chol means nothing once L is ill-conditioned):
    E_L  = max |L'_ref^-1 L'_dev - I|                       the new factor in its own coordinates
    E_mu = max |L'_ref^-1 (mu_dev - mu_ref)|                the new mean in standard deviations of the new component
    E_kl = |KL_dev - KL_ref(eta_dev)| / (EPS32 B_kl),       B_kl = 1/2 (sum |ln d_i| + D + tr B^-1 + |B^-1 w|^2 / eta^2)
           (the bound C_kl EPS32 B_kl is capped by 1e-5 + 5e-3 KL, kl_bound())
with d_i the pivots of the tridiagonal form of B = I + M / eta (what the kernels sum; logdet - D + tr cancels at large eta).
last_eta rtol 1e-5, l2 rtol 1e-6, success / num_updates / probe counts exact.

The bounds are not tuned on the device.  whitened(..., dtype=float32) evaluates the kernels' own formulation (DESIGN.md section
4, header of update_kl.hip: M = L^T R_sym L, w = L^T (g + (R_sym - R) mu), B = I + M / eta = U U^T, L' = L U^-T,
mu' = mu - L' U^-1 w / eta, KL from the tridiagonal form by pivot recurrences) in float32 NumPy at the oracle's accepted eta;
for the plain updates it is update_plain_kernel's formulation (_plain_kernel_f32: L^-1, Q = L^-T L^-1, Cholesky of the new precision,
its triangular inverse, W^T W, Cholesky; the full inverse for a non-symmetric reward).  The worst values over the table are recorded in F32_WORST, and the device bound is C = 8 x that (the factor of
stein_cases.C: room for another summation order and the 1-ulp v_rcp / v_sqrt, still below any dropped term), one set per
group(): the register routes, the blocked route, the illcond law, the kernel in the reference's arithmetic and the plain updates.  test_update_cases_cpu.py asserts that the float32 evaluation stays within its
recorded worst values, that the bounds are tighter than the old 1e-3 / 2e-3 / 5e-3 assertions on the benign law and that every
planted fault lies ten times outside them.

The plain updates (direct, iBLR) decide only whether the new precision factorises; a component on which the float32 evaluation
decides otherwise than fp64 is marked ``undecided`` and a device may reject it; the table holds none (test_update_cases_cpu.py).
Decision margins of the KL update: a case enters the table only if in the fp64 trace every probed KL is further than 2 C_kl EPS32 B_kl from
eps, 0.9 eps and 1.1 eps, every pivot of a feasible probe is above PIVOT_MARGIN (and the smallest eigenvalue of an infeasible one
below -PIVOT_MARGIN), and every bracket-width test is further than 1e-3 from 0.1; make_case asserts it.  The seeds of the table
are the first ones at which this holds (first_good_seed).
"""
import contextlib
import functools

import numpy as np
from scipy.linalg import get_lapack_funcs, solve_triangular

from oracle import gmm as ogmm, updaters as oupd
from oracle.gmm import FLOAT32_MAX
import weight_step_cases as wsc
from weight_step_cases import f32

try:
    from threadpoolctl import threadpool_limits
except ImportError:                                                  # (only slower without it)
    threadpool_limits = None


def _one_thread():
    """The matrices here are small and many: a multi-threaded BLAS spends its time waking its workers (six times slower)."""
    return threadpool_limits(limits=1) if threadpool_limits else contextlib.nullcontext()


EPS32 = float(np.finfo(np.float32).eps)
L2_INIT = 1e-12
WIDTH_MARGIN = 1e-3
PIVOT_MARGIN = 1e-3
FAULT_FACTOR = 10.0

# ---- measured: the float32 NumPy evaluation against fp64 over the whole table (test_update_cases_cpu.py) ---------------------
# group -> (E_L, E_mu, E_kl); the worst case of each figure is named in the CPU test's output
F32_WORST = {"register": (4e-7, 7e-7, 1.5), "illcond": (7e-5, 4e-7, 1.5), "blocked": (3e-7, 7e-7, 2.5),
             "reference": (2e-6, 5e-6, 3.5), "reference-illcond": (0.13, 3.5e-4, 6e5),
             "plain-register": (6e-7, 6e-6, 0.0), "plain-illcond": (3.5e-4, 7e-5, 0.0), "plain-blocked": (1e-6, 1e-5, 0.0)}
C_FACTOR = 8.0
C_L = {g: C_FACTOR * v[0] for g, v in F32_WORST.items()}
C_MU = {g: C_FACTOR * v[1] for g, v in F32_WORST.items()}
C_KL = {g: C_FACTOR * v[2] for g, v in F32_WORST.items()}
RTOL_ETA, RTOL_L2 = 1e-5, 1e-6
# A bracket without any feasible eta is bisected until min(e^ub - e^eta, e^eta - e^lb) < 0.1; from the cold bracket (ub = 80) that
# only happens once eta == ub in the number format: after 53 halvings in fp64, 24 in fp32.  Probe counts are compared up to here
MAX_EXACT_PROBES = 20


def group(case):
    """The set of constants a case is held to: the KL update on the register routes / on the blocked route / under the illcond law
    (condition 1e6: its float32 error is a hundred times that of every other law, and one constant for both would be looser on
    the benign law than the assertions this suite replaces), and the same three for the plain updates."""
    g = "blocked" if case["route"] == "blocked" else "illcond" if case["law"] == "illcond" else "register"
    return g if case["mode"] == "kl" else "plain-" + g


def reference_group(case):
    """The constants of update_kl_kernel (csrc/update.hip), which follows the reference's arithmetic -- L^-1, Q = L^-T L^-1,
    chol(Q + R / eta), its inverse, chol of the new covariance -- and not the whitened formulation: measured on the oracle's
    arithmetic in float32."""
    return "reference-illcond" if case["law"] == "illcond" else "reference"


# ---- the case table --------------------------------------------------------------------------------------------------------------
INSTANCE_DIMS = (1, 2, 3, 4, 10, 20, 24, 25, 32, 33, 40, 49, 50)
STRUCTURE_DIMS = (2, 20, 33, 40)
SCALE_EXPONENTS = (-80, -70, -66, -62, -40, 0, 20, 30)
BLOCKED_DIMS = (51, 64, 65, 128, 129, 192, 193, 256, 257, 304, 305, 320, 321, 512)
BLOCKED_PLAIN_DIMS = (65, 129, 321)
PLAIN_DIMS = (1, 2, 6, 20, 33, 50)
ROUTE64_KL_DIMS = (51, 54, 55, 63, 64)          # GMMVI_BLOCKED_ABOVE=64: generic four-wave instance, > 64 KB LDS from D = 55
ROUTE64_PLAIN_DIMS = (56, 57, 64)               # update_plain_kernel passes 64 KB between 56 and 57
MIN_STEPSIZE = 0.001                            # configs/defaults.py "R": the smallest stepsize the adaptation reaches
# (H = -1e6 I is feasible from eta ~ 1e6 on: fp64 accepts it, and so must the device.  The failing components carry l2 = 5e-7 and
# 1e-6 (cap reached), 5e-8 (not reached); 1e-12 on a failing component is the onefail and nofeasible cases)
FAIL_L2 = {"fail-a": (1e-12, 5e-7, 1.5e-12, 5e-8, 1e-3), "fail-b": (1e-3, 1e-6, 1e-12, 5e-7, 1.5e-12)}
FAIL_BAD = {"fail-a": ((1, "nan_h"), (3, "nan_g")), "fail-b": ((1, "inf_h"), (3, "neg_h"))}

# id -> seed where seed 0 does not meet the margins (first_good_seed)
SEEDS = {"register-kl-benign-D33": 1, "register-kl-benign-D32": 1, "register-kl-benign-D49": 1, "register-kl-illcond-D32": 5, "register-kl-illcond-D49": 3,
         "register-kl-nonsym-D50": 1, "register-kl-arrow-D40": 1, "register-kl-search-p7-D20": 1, "register-kl-search-p12-D20": 8,
         "blocked-kl-benign-D128": 2, "blocked-kl-benign-D192": 1, "blocked-kl-benign-D305": 1, "blocked-kl-benign-D321": 2,
         "blocked-kl-nonsym-D128": 1, "blocked-kl-nonsym-D129": 1, "blocked-kl-nonsym-D256": 3, "blocked-kl-nonsym-D257": 8,
         "blocked-kl-nonsym-D305": 3, "blocked-kl-nonsym-D321": 2, "blocked-kl-nonsym-D512": 1}


def _spec(route, law, d, k, mode="kl", temperature=1.0, tag=""):
    cid = f"{route}-{mode}-{law}{tag}-D{d}"
    return dict(id=cid, route=route, law=law, d=d, k=k, mode=mode, temperature=temperature, tag=tag, seed=SEEDS.get(cid, 0))


def case_table():
    t = []
    t += [_spec("register", law, d, 4) for law in ("benign", "illcond", "nonsym") for d in INSTANCE_DIMS]
    for d in STRUCTURE_DIMS:
        t += [_spec("register", law, d, 3) for law in ("diag", "blockdiag2", "arrow", "zero", "zerog", "smallstep")]
        t += [_spec("register", "scale", d, 3, tag=f"{s:+d}") for s in SCALE_EXPONENTS]
    t += [_spec("register", "search", 20, 6, tag=f"-p{p}") for p in (6, 7, 12, 13)]
    t += [_spec("register", "search", 20, 3, tag=t_) for t_ in ("-root", "-clamp", "-nofeasible")]
    t += [_spec("register", "search", 20, 6, temperature=30.0, tag="-temperature")]
    t += [_spec("register", "fail", d, 5, tag=name[4:]) for name in FAIL_L2 for d in (5, 40)]
    t += [_spec("register", law, d, 4, mode=mode) for mode in ("direct", "iblr") for law in ("benign", "illcond", "nonsym", "onefail")
          for d in PLAIN_DIMS]
    t += [_spec("blocked", law, d, 2) for law in ("benign", "nonsym") for d in BLOCKED_DIMS]
    t += [_spec("blocked", "benign", d, 2, mode=mode) for mode in ("direct", "iblr") for d in BLOCKED_PLAIN_DIMS]
    # the subnormal-range rewards on the blocked route: the register-resident tridiagonalisation and the global-memory one
    t += [_spec("blocked", "scale", d, 2, tag="-66") for d in (65, 321)]
    return t


def route64_table():
    """Run under GMMVI_BLOCKED_ABOVE=64 (update_route_child.py): the register kernels at D = 51 ... 64."""
    return [_spec("register64", "benign", d, 2) for d in ROUTE64_KL_DIMS] + \
           [_spec("register64", "benign", d, 2, mode=mode) for mode in ("direct", "iblr") for d in ROUTE64_PLAIN_DIMS]


def spec_by_id(case_id):
    return next(s for s in case_table() + route64_table() if s["id"] == case_id)


# ---- input laws ------------------------------------------------------------------------------------------------------------------
def _benign(rng, k, d):
    """The law of test_hip_kernels.random_gmm / _update_inputs -> (means, chols, H, g)."""
    means = rng.normal(size=(k, d)) * 3.0
    chols = np.stack([np.linalg.cholesky((lambda a: a @ a.T / d + 0.3 * np.eye(d))(rng.normal(size=(d, d)))) for _ in range(k)])
    hs = np.stack([(lambda b: b @ b.T / d)(rng.normal(size=(d, d))) for _ in range(k)])
    if k > 2:
        hs[2] = -0.01 * hs[2]                                               # one concave reward
    return means, chols, hs, rng.normal(size=(k, d))


def _inputs(spec):
    """-> dict(means, chols, H_neg, g_neg, stepsizes, last_eta, l2, num_updates), not yet rounded."""
    law, d, k, tag = spec["law"], spec["d"], spec["k"], spec["tag"]
    rng = np.random.default_rng([spec["seed"], d, k, sum(map(ord, law + tag + spec["mode"]))])
    means, chols, hs, gs = _benign(rng, k, d)
    steps = np.linspace(0.05, 0.5, k) if spec["mode"] == "kl" else np.full(k, 0.3)
    if spec["mode"] == "kl" and d >= 512:
        # B_kl >= D: at D = 512 the margin 2 C_kl EPS32 B_kl is half the accept window of eps = 0.05; no seed in 400 clears it
        steps = np.linspace(0.25, 0.5, k)
    last_eta, l2, nupd = -np.ones(k), np.full(k, L2_INIT), np.zeros(k)
    eye = np.eye(d)
    if law == "illcond":
        # L = Q diag(sigma) re-factored, sigma log-spaced over 1 ... 1e3; H with one (odd components: two) negative eigenvalues
        # that make B = I + M / eta indefinite in the lower part of the bracket
        for i in range(k):
            q = np.linalg.qr(rng.normal(size=(d, d)))[0]
            a = q * np.logspace(0.0, 3.0, d)[None, :] if d > 1 else q * 30.0
            chols[i] = np.linalg.cholesky(a @ a.T)
            for j in range(1 + i % 2):
                v = rng.normal(size=d)
                v /= np.linalg.norm(v)
                if spec["mode"] == "kl":
                    hs[i] -= (2.0 - j) * np.outer(v, v)
        if spec["mode"] != "kl":
            # the plain updates have no eta to climb with: an indefinite reward is simply rejected (Q has eigenvalues down to
            # 1e-6), and a reward of order 1 makes iBLR's correction step / 2 R Sigma R (Sigma up to 1e6) swamp the precision
            # beyond what float32 factorises.  A positive definite reward scaled by 1e-3 keeps every term of the new precision
            # within the condition of the old one, 1e6: the update is accepted and float32 decides as fp64 does
            if k > 2:
                hs[2] = -hs[2] / 0.01
            hs, gs = hs * 1e-3, gs * 1e-3
    elif law == "nonsym":
        hs = hs + 0.05 * rng.normal(size=hs.shape)
    elif law in ("diag", "blockdiag2", "arrow"):
        mask = eye.astype(bool)
        if law == "blockdiag2":
            for i in range(0, d - 1, 2):
                mask[i, i + 1] = mask[i + 1, i] = True
        for i in range(k):
            if law == "arrow":
                # L diagonal, H diagonal plus a first row / column: M = L H L has one column with a tail
                chols[i] = np.diag(np.abs(np.diag(chols[i])))
                h = np.diag(np.diag(hs[i]))
                h[0, 1:] = h[1:, 0] = 0.3 * rng.normal(size=d - 1) / np.sqrt(d)
                hs[i] = h
            else:
                chols[i] = np.linalg.cholesky(np.where(mask, chols[i] @ chols[i].T, 0.0))
                hs[i] = np.where(mask, hs[i], 0.0)
    elif law == "zero":
        hs, gs = np.zeros_like(hs), np.zeros_like(gs)
    elif law == "zerog":                                                    # H = 0, g != 0
        hs = np.zeros_like(hs)
    elif law == "scale":
        s = 2.0 ** int(tag)
        hs, gs = hs * s, gs * s
    elif law == "smallstep":
        # at eps = 0.001 the accept window (0.9 eps, 1.1 eps) is 2e-4 wide and 2 C_kl EPS32 B_kl is 1e-4 from D = 33 on (B_kl >= D):
        # no accepted probe can keep its margin there.  The rewards of those two components are scaled down until their search
        # ends on the bracket width (every probe far below 0.9 eps); the component with stepsize 1 searches as usual
        steps = np.array([MIN_STEPSIZE, 1.0, MIN_STEPSIZE])[:k]
        sc = np.array([2.0 ** -12, 1.0, 2.0 ** -14])[:k]
        hs, gs = hs * sc[:, None, None], gs * sc[:, None]
    elif law == "search":
        if tag.startswith("-p"):
            # reward scales 2^-6 ... 2^44 spread the accepted eta (and with it the depth of the search) over the components
            sc = 2.0 ** rng.integers(-6, 45, size=k)
            hs, gs = hs * sc[:, None, None], gs * sc[:, None]
            if tag == "-p13":
                # a warm bracket without a feasible eta ends on its width, min(e^ub - e^eta, e^eta - e^lb) < 0.1 with lb climbing
                # to ub = ln last_eta + 3: one more probe for every doubling of last_eta -- 11, 12, 13 and 14 for the four hopeless
                # components here; the other two search as usual from a cold bracket
                last_eta = np.array([3.0, 6.0, 10.0, 20.0, -1.0, -1.0])
                hs[:4] = -1e7 * eye
            elif int(tag[2:]) > 10:
                # where KL(eta) = eps << 1 the KL falls like 1 / eta^2 and a grid of 100 / 2^11 in ln eta always holds a point of
                # the accept window: eleven probes at the most.  Towards the infeasible end of a concave reward the KL rises
                # steeply, and with eps = 1 the bound is met there: the search has to go deeper
                hs, gs = -hs, gs * 2.0 ** -rng.integers(0, 8, size=k)[:, None]
                steps = np.ones(k)                                          # (the largest stepsize of configs/defaults.py)
        elif tag == "-temperature":
            m, hs, gs, steps = wsc.kl_update_inputs("dense", d, 30.0)
            means, chols = m.means, m.chol_cov
        elif tag == "-clamp":
            last_eta = np.array([2.0, 5.0, 15.0])                           # 1 < last_eta < e^3: the bracket starts at 0
            hs, gs = hs * 0.25, gs * 0.25
        elif tag == "-nofeasible":
            last_eta = np.array([2.0, 2.0, 2.0])
            hs[1] = -1000.0 * eye                                           # B indefinite for every eta <= 2 e^3
        # "-root": last_eta is set by make_case from the fp64 KL
    elif law == "fail":
        name = "fail" + tag
        l2 = np.array(FAIL_L2[name])
        for i, kind in FAIL_BAD[name]:
            if kind == "nan_h":
                hs[i, d // 2, 0] = np.nan
            elif kind == "nan_g":
                gs[i, d - 1] = np.nan
            elif kind == "inf_h":
                hs[i, d - 1, d - 1] = np.inf
            else:
                hs[i] = -1e6 * eye
    elif law == "onefail":
        # direct: hopelessly indefinite; iBLR: step^2 / 2 R Sigma R would make that one positive definite again, so a NaN
        if spec["mode"] == "direct":
            hs[1] = -1e6 * eye
        else:
            hs[1, d - 1, 0] = np.nan
    return dict(means=means, chols=chols, H_neg=hs, g_neg=gs, stepsizes=steps, last_eta=last_eta, l2=l2, num_updates=nupd)


# ---- fp64 reference --------------------------------------------------------------------------------------------------------------
def _wrapper(state, stepsizes):
    k, d = state["means"].shape
    m = ogmm.FullCovGMM(np.full(k, 1.0 / k), state["means"], np.stack([np.eye(d)] * k))
    m.replace_components(state["means"], state["chols"])
    w = ogmm.GmmWrapper(m, 0.1, L2_INIT, 4)
    w.stepsizes = stepsizes.copy()
    w.last_log_etas = state["last_eta"].copy()
    w.l2_regularizers = state["l2"].copy()
    w.num_received_updates = state["num_updates"].copy()
    return w


def run_oracle(state, h, g, stepsizes, mode, temperature=1.0):
    """One round of oracle.updaters in fp64 on ``state`` -> dict(success, means, chols, last_eta, l2, num_updates[, kls, probes,
    traces, lo])."""
    w = _wrapper(state, stepsizes)
    out = {}
    with np.errstate(all="ignore"):
        if mode == "kl":
            traces = []
            succ, etas, kls, probes = oupd.apply_ng_update_kl(w, h, g, stepsizes, temperature, traces=traces)
            out.update(kls=kls, probes=probes, traces=traces)
        elif mode == "direct":
            succ = oupd.apply_ng_update_direct(w, h, g, stepsizes)
        else:
            succ = oupd.apply_ng_update_iblr(w, h, g, stepsizes)
    out.update(success=np.asarray(succ, bool), means=w.model.means, chols=w.model.chol_cov, last_eta=w.last_log_etas,
               l2=w.l2_regularizers, num_updates=w.num_received_updates)
    return out


def _next_state(ref):
    return {n: f32(ref[n]) for n in ("means", "chols", "last_eta", "l2", "num_updates")}


# ---- the kernels' formulation, any dtype, with planted faults ------------------------------------------------------------------------
def _sym_lower(r, upper=False):
    return np.triu(r) + np.triu(r, 1).T if upper else np.tril(r) + np.tril(r, -1).T


def _householder_tridiag(m, w, skip_last_w=False):
    """Householder reduction column by column, as the kernels do it (fp64; only used by the planted fault that leaves the last
    reflector off w) -> (td, te, wt)."""
    m, wt = m.copy(), w.copy()
    d = m.shape[0]
    for c in range(d - 2):
        x = m[c + 1:, c].copy()
        if not np.any(x[1:] != 0):
            continue
        alpha = -np.copysign(np.linalg.norm(x), x[0]) if x[0] != 0 else np.linalg.norm(x)
        v = np.zeros(d)
        v[c + 1:] = x
        v[c + 1] -= alpha
        hh = np.eye(d) - 2.0 * np.outer(v, v) / (v @ v)
        m = hh @ m @ hh
        if not (skip_last_w and c == d - 3):
            wt = hh @ wt
    return np.diag(m).copy(), np.diag(m, -1).copy(), wt


def tridiagonal_form(m, w, dtype=np.float64, skip_last_w=False):
    """T = Q^T M Q, wt = Q^T w -> (td [D], te [D - 1], wt [D]) in ``dtype``."""
    d = m.shape[0]
    if skip_last_w:
        return _householder_tridiag(m, w, True)
    if d <= 2:
        return np.diag(m).astype(dtype), np.diag(m, -1).astype(dtype), w.astype(dtype)
    a = m.astype(dtype)
    sytrd, = get_lapack_funcs(("sytrd",), (a,))
    c, td, te, tau, info = sytrd(a, lower=1)
    assert info == 0
    wt = w.astype(dtype).copy()
    for i in range(d - 1):                                  # Q^T w = H(d-1) ... H(1) w, H(i) = I - tau v v^T, v = (1, c[i+2:, i])
        v = np.concatenate(([dtype(1.0)], c[i + 2:, i]))
        wt[i + 1:] -= tau[i] * (v @ wt[i + 1:]) * v
    return td.astype(dtype), te.astype(dtype), wt.astype(dtype)


def kl_tridiagonal(td, te, wt, eta, dtype=np.float64):
    """update_kl.hip kl_tridiag in ``dtype``: forward pivots d_i, backward pivots, (B^-1)_ii = 1 / (d_i + delta_i - a_i), Thomas
    solve -> (KL or FLOAT32_MAX, B_kl, smallest pivot)."""
    t = dtype
    n = td.shape[0]
    inv = t(1.0) / t(eta)
    a = (td.astype(t) * inv + t(1.0)).astype(t)
    b = (te.astype(t) * inv).astype(t)
    dp, cp = np.empty(n, t), np.empty(n, t)
    for i in range(n):
        d_, c_ = a[i], t(wt[i])
        if i:
            r = b[i - 1] / dp[i - 1]
            d_, c_ = t(a[i] - b[i - 1] * r), t(c_ - r * cp[i - 1])
        dp[i], cp[i] = d_, c_
    if not np.all(dp > 0):
        return FLOAT32_MAX, np.inf, float(np.min(dp)) if np.all(np.isfinite(dp)) else -np.inf
    logdet = np.sum(np.log(dp), dtype=t)
    labs = np.sum(np.abs(np.log(dp)), dtype=t)
    dn, yn, tr, yy = t(1.0), t(0.0), t(0.0), t(0.0)
    for i in range(n - 1, -1, -1):
        delta, y = a[i], t(cp[i] / dp[i])
        if i < n - 1:
            delta = t(a[i] - b[i] * b[i] / dn)
            y = t(y - b[i] / dp[i] * yn)
        tr = t(tr + t(1.0) / t(dp[i] + delta - a[i]))
        yy = t(yy + y * y)
        dn, yn = delta, y
    kl = t(0.5) * t(t(logdet - t(n)) + tr + yy * inv * inv)
    bkl = 0.5 * (float(labs) + n + float(tr) + float(yy) * float(inv) ** 2)
    return float(kl), bkl, float(np.min(dp))


def whitened_matrix(mean, chol, h, g, dtype=np.float64, fault=None):
    """-> (M = sym(L^T R_sym L), w = L^T (g + (R_sym - R) mu)) in ``dtype``."""
    t = dtype
    lo, mu, r, gg = chol.astype(t), mean.astype(t), h.astype(t), g.astype(t)
    rs = _sym_lower(r, upper=fault == "upper_triangle")
    m = (lo.T @ (rs @ lo)).astype(t)
    gt = gg if fault == "no_correction" else (gg + (rs - r) @ mu).astype(t)
    return (t(0.5) * (m + m.T)).astype(t), (lo.T @ gt).astype(t)


def whitened(mean, chol, h, g, eta, dtype=np.float64, fault=None, kl_eta=None):
    """The update of one component at ``eta`` in the kernels' formulation, ``dtype`` throughout -> (mu', L', KL, B_kl, column sums
    of squares of M below the sub-diagonal).  ``fault``: see fault(); ``kl_eta``: evaluate the KL at another eta."""
    t = dtype
    d = mean.shape[0]
    lo, mu = chol.astype(t), mean.astype(t)
    m, w = whitened_matrix(mean, chol, h, g, t, fault)
    if fault == "last_row_ignored" and d > 1:
        m[d - 1, :d - 1] = m[:d - 1, d - 1] = 0
    inv = t(1.0) / t(eta)
    b = (np.eye(d, dtype=t) + m * inv).astype(t)
    tails = np.array([np.sum(np.square(m[c + 2:, c].astype(np.float64))) for c in range(max(d - 2, 0))])
    td, te, wt = tridiagonal_form(m.astype(np.float64) if fault == "w_last_reflector" else m, w, t, fault == "w_last_reflector")
    kl, bkl, _ = kl_tridiagonal(td, te, wt, eta if kl_eta is None else kl_eta, t)
    try:
        c = np.linalg.cholesky(b[::-1, ::-1])                              # J B J = C C^T  ->  B = U U^T, U = J C J upper
    except np.linalg.LinAlgError:
        return mean, chol, FLOAT32_MAX, np.inf, tails
    u = c[::-1, ::-1]
    uinv = solve_triangular(u, np.eye(d, dtype=t), lower=False).astype(t)
    new_l = (lo @ (uinv if fault == "l_u_inverse" else uinv.T)).astype(t)
    step = inv * inv if fault == "mean_step_eta2" else inv
    new_mu = (mu - (new_l @ (uinv @ w)) * step).astype(t)
    return new_mu.astype(np.float64), new_l.astype(np.float64), kl, bkl, tails


def _tri64(state, case, i):
    tri = state.setdefault("_tri", {})
    if i not in tri:
        tri[i] = tridiagonal_form(*whitened_matrix(state["means"][i], state["chols"][i], case["H_neg"][i], case["g_neg"][i]))
    return tri[i]


def kl_ref(state, case, i, eta):
    """fp64 KL of component ``i`` at ``eta`` and its magnitude B_kl."""
    kl, bkl, _ = kl_tridiagonal(*_tri64(state, case, i), eta)
    return kl, bkl


# ---- error measure ---------------------------------------------------------------------------------------------------------------
def errors(ref_means, ref_chols, means, chols):
    """-> (E_L [K], E_mu [K]) of (means, chols) against the reference, in the reference's coordinates."""
    k, d = ref_means.shape
    el, em = np.empty(k), np.empty(k)
    for i in range(k):
        li = solve_triangular(ref_chols[i], np.eye(d), lower=True)
        el[i] = np.max(np.abs(li @ np.asarray(chols[i], np.float64) - np.eye(d)))
        em[i] = np.max(np.abs(li @ (np.asarray(means[i], np.float64) - ref_means[i])))
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(el), np.inf, el), np.where(np.isnan(em), np.inf, em)


def l2_rule(l2, success, cap=True, floor=True):
    """ng_based_component_updater.py:520-523, with the cap / the floor optionally left out (planted faults)."""
    ok = np.maximum(0.5 * l2, L2_INIT) if floor else 0.5 * l2
    bad = np.minimum(1e-6, 10 * l2) if cap else 10 * l2
    return np.where(success, ok, bad)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def probe_margins(state, case, ref):
    """-> (smallest (distance of a probed KL from a threshold) / (2 C_kl EPS32 B_kl), smallest pivot margin (the smallest eigenvalue
    of B at a feasible probe, minus that of an infeasible one), smallest distance of a bracket-width test from 0.1, lo [K]) over the
    components of one KL round."""
    ckl = C_KL[group(case)]
    klm = pvm = wm = np.inf
    lo = np.empty(case["k"])
    for i in range(case["k"]):
        eps = case["stepsizes"][i]
        lo[i], hi, _, w_ = wsc.replay_component_search(eps, state["last_eta"][i], ref["traces"][i])
        wm = min(wm, w_)
        if not (np.all(np.isfinite(case["H_neg"][i])) and np.all(np.isfinite(case["g_neg"][i]))):
            continue
        m, w = whitened_matrix(state["means"][i], state["chols"][i], case["H_neg"][i], case["g_neg"][i])
        ev = np.linalg.eigvalsh(m)
        td, te, wt = _tri64(state, case, i)
        for e, val in ref["traces"][i]:
            eta = np.exp(e)
            if val >= FLOAT32_MAX:
                pvm = min(pvm, -(1.0 + ev[0] / eta))
                continue
            kl, bkl, _ = kl_tridiagonal(td, te, wt, eta)
            assert abs(kl - val) <= 1e-6 * bkl + 1e-9 * abs(val), (case["id"], i, eta, kl, val)   # the two formulations agree
            pvm = min(pvm, 1.0 + ev[0] / eta)
            klm = min(klm, min(abs(val - t * eps) for t in wsc.KL_THRESHOLDS) / (2 * ckl * EPS32 * bkl))
    return klm, pvm, wm, lo


@functools.lru_cache(maxsize=None)
def _make_case(spec_items, check):
    spec = dict(spec_items)
    inp = _inputs(spec)
    case = dict(spec, H_neg=f32(inp["H_neg"]), g_neg=f32(inp["g_neg"]), stepsizes=f32(inp["stepsizes"]))
    state = {n: f32(inp[n]) for n in ("means", "chols", "last_eta", "l2", "num_updates")}
    if spec["law"] == "search" and spec["tag"] == "-root":
        # warm start whose first probe is accepted: last_eta solves KL(eta) = 0.95 eps (bisection on the fp64 KL)
        for i in range(spec["k"]):
            a, b = 0.0, 40.0
            for _ in range(200):
                mid = 0.5 * (a + b)
                a, b = (a, mid) if kl_ref(state, case, i, np.exp(mid))[0] < 0.95 * case["stepsizes"][i] else (mid, b)
            state["last_eta"][i] = f32(np.exp(b))
    rounds = []
    for r in range(2):
        ref = run_oracle(state, case["H_neg"], case["g_neg"], case["stepsizes"], spec["mode"], spec["temperature"])
        if spec["mode"] == "kl":
            klm, pvm, wm, lo = probe_margins(state, case, ref)
            ref.update(kl_margin=klm, pivot_margin=pvm, width_margin=wm, lo=lo)
            if check:
                assert klm > 1.0 and pvm > PIVOT_MARGIN and wm > WIDTH_MARGIN, (spec["id"], r, klm, pvm, wm)
        else:
            # the plain updates decide once, on the Cholesky factorisation of the new precision.  Where the float32 evaluation
            # decides otherwise than fp64 (illcond law: condition 1e6) the decision is not determined in fp32: a device may take
            # either branch for that component, and is held to the branch it took
            ref["undecided"] = _plain_kernel_f32(state, case)[2] != ref["success"]
        state["ref"] = ref
        rounds.append(state)
        state = _next_state(ref)
    case["rounds"] = rounds
    return case


def make_case(spec, check=True):
    """Rebuilds the case of ``spec`` (an entry of case_table()); asserts the decision margins.  Cached: treat as read-only."""
    with _one_thread():
        return _make_case(tuple(sorted(spec.items())), check)


def case_holds(spec):
    try:
        c = make_case(spec)
    except AssertionError:
        return False
    tag = spec["tag"]
    if spec["law"] == "search" and tag.startswith("-p"):
        return int(tag[2:]) in [int(p) for r in c["rounds"] for p in r["ref"]["probes"]]
    return True


def first_good_seed(spec, tries=400):
    for seed in range(tries):
        if case_holds(dict(spec, seed=seed)):
            return seed
    raise AssertionError(spec["id"])


# ---- the float32 evaluation ------------------------------------------------------------------------------------------------------
def _plain_kernel_f32(state, case):
    """update_plain_kernel's own formulation in float32 NumPy -> (means, chols, success): L^-1 by substitution, Q = L^-T L^-1,
    the new precision P; for a symmetric reward chol(P) (lower triangle), the mean by two substitutions, W = chol(P)^-1,
    Sigma' = W^T W and its Cholesky factor; for a non-symmetric one the inverse of the full P, the mean from it, and the
    Cholesky factor of its lower triangle."""
    t = np.float32
    means, chols = state["means"].astype(t), state["chols"].astype(t)
    succ = np.zeros(means.shape[0], bool)
    with np.errstate(all="ignore"):
        for i in range(means.shape[0]):
            lo, mu, r, g, st = chols[i], means[i], case["H_neg"][i].astype(t), case["g_neg"][i].astype(t), t(case["stepsizes"][i])
            if not (np.all(np.isfinite(r)) and np.all(np.isfinite(g))):
                continue
            linv = oupd._tri_inv(lo)
            q = linv.T @ linv
            if case["mode"] == "direct":
                p, lin, new_mu = q + st * r, q @ mu + st * (r @ mu - g), None
            else:
                sig = lo @ lo.T
                p = q + st * (r + t(0.5) * st * ((r @ sig) @ r))
                lin, new_mu = None, mu if state["num_updates"][i] == 0 else mu - st * (sig @ g)
            if np.array_equal(r, r.T):
                c = oupd._chol(np.tril(p) + np.tril(p, -1).T)
                if c is None:
                    continue
                if new_mu is None:
                    new_mu = solve_triangular(c.T, solve_triangular(c, lin, lower=True), lower=False)
                w = oupd._tri_inv(c)
                cov = w.T @ w
            else:
                try:
                    cov = np.linalg.inv(p)
                except np.linalg.LinAlgError:
                    continue
                if new_mu is None:
                    new_mu = cov @ lin
                cov = np.tril(cov) + np.tril(cov, -1).T
            new_l = oupd._chol(cov)
            if new_l is None or not np.all(np.isfinite(new_mu)):
                continue
            means[i], chols[i], succ[i] = new_mu, new_l, True
    return means.astype(np.float64), chols.astype(np.float64), succ


def whitened_f32(case):
    """-> list per round of (E_L [K], E_mu [K], E_kl [K]) of the float32 evaluation against fp64, successful components only (the
    others are nan)."""
    with _one_thread():
        return _whitened_f32(case)


def _oracle_kl_f32(mean, chol, h, g, eta):
    """updaters.kl and the new factor as apply_ng_update_kl forms it, float32 throughout -> (mu', L', KL)."""
    t = np.float32
    lo, mu, r, gg = (a.astype(t) for a in (chol, mean, h, g))
    inv_chol = oupd._tri_inv(lo)
    prec = inv_chol.T @ inv_chol
    kl_const = t(2.0) * np.sum(np.log(np.diag(lo))) - t(mu.shape[0])
    with np.errstate(all="ignore"):
        val, new_mean, _, cinv = oupd.kl(t(eta), prec @ mu, prec, inv_chol, r @ mu - gg, r, kl_const, mu, False)
        new_chol = oupd._chol(cinv.T @ cinv) if val < FLOAT32_MAX else None
    if new_chol is None:
        return np.full_like(mean, np.nan), np.full_like(chol, np.nan), np.nan
    return new_mean.astype(np.float64), new_chol.astype(np.float64), float(val)


def reference_f32(case):
    """whitened_f32 for the kernel in the reference's arithmetic (KL cases only)."""
    with _one_thread():
        return _whitened_f32(case, oracle_arithmetic=True)


def reference_kernel_holds(case):
    """The decision margins of the case under the constants of the reference-arithmetic kernel: only then is that kernel bound to
    take the oracle's path, and only then does the GPU test run it on the case."""
    q = C_KL[group(case)] / C_KL[reference_group(case)]
    return case["mode"] == "kl" and all(r["ref"]["kl_margin"] * q > 1.0 for r in case["rounds"])


def _whitened_f32(case, oracle_arithmetic=False):
    out = []
    for rnd in case["rounds"]:
        ref = rnd["ref"]
        k = case["k"]
        ekl = np.full(k, np.nan)
        if case["mode"] == "kl":
            means, chols = ref["means"].copy(), ref["chols"].copy()
            for i in np.where(ref["success"])[0]:
                eta = float(ref["last_eta"][i])
                args = (rnd["means"][i], rnd["chols"][i], case["H_neg"][i], case["g_neg"][i], eta)
                means[i], chols[i], kl = _oracle_kl_f32(*args) if oracle_arithmetic else whitened(*args, np.float32)[:3]
                k64, bkl = kl_ref(rnd, case, i, eta)
                ekl[i] = abs(kl - k64) / (EPS32 * bkl)
        else:
            means, chols, _ = _plain_kernel_f32(rnd, case)
        el, em = errors(ref["means"], ref["chols"], means, chols)
        el[~ref["success"]] = em[~ref["success"]] = np.nan
        out.append((el, em, ekl))
    return out


# ---- planted faults --------------------------------------------------------------------------------------------------------------
KL_FAULTS = ("upper_triangle", "no_correction", "w_last_reflector", "last_row_ignored", "l_u_inverse", "mean_step_eta2",
             "eta_lo", "kl_at_lo")
L2_FAULTS = ("l2_no_cap", "l2_no_floor")
PLAIN_FAULTS = ("iblr_first_mean", "direct_half_step")
# the cases each fault is shown on (test_update_cases_cpu.py); the reasons are given there
FAULT_CASES = {
    "upper_triangle": ("register-kl-nonsym-D20", "register-kl-nonsym-D40", "blocked-kl-nonsym-D65"),
    "no_correction": ("register-kl-nonsym-D20", "register-kl-nonsym-D33", "blocked-kl-nonsym-D129"),
    # (the last reflector mixes the last two coordinates of w only: it moves about 2 / D of |B^-1 w|^2, and from D = 32 on that
    # is less than ten times the KL bound on every case of the table -- 4.7 times at D = 33)
    "w_last_reflector": ("register-kl-benign-D4", "register-kl-benign-D10", "register-kl-nonsym-D20", "register-kl-benign-D25"),
    "last_row_ignored": ("register-kl-benign-D4", "register-kl-benign-D50", "blocked-kl-benign-D65"),
    "l_u_inverse": ("register-kl-benign-D4", "register-kl-benign-D32", "blocked-kl-benign-D64"),
    "mean_step_eta2": ("register-kl-benign-D10", "register-kl-benign-D40", "blocked-kl-benign-D51"),
    "eta_lo": ("register-kl-search-temperature-D20",),
    "kl_at_lo": ("register-kl-search-temperature-D20",),
    "l2_no_cap": ("register-kl-fail-b-D5",),
    "l2_no_floor": ("register-kl-fail-a-D5",),
    "iblr_first_mean": ("register-iblr-benign-D6", "blocked-iblr-benign-D65"),
    "direct_half_step": ("register-direct-benign-D6", "blocked-direct-benign-D65"),
}


def fault(case, name, rnd=0):
    """The fp64 result of a deliberately wrong update of round ``rnd`` -> dict(means, chols, kls, last_eta, l2):
    upper_triangle     the upper triangle of a non-symmetric H mirrored
    no_correction      the (R_sym - R) mu term dropped from w
    w_last_reflector   w not rotated by the last Householder reflector (only the KL sees it)
    last_row_ignored   the off-diagonal part of the last row / column of M ignored
    l_u_inverse        L' = L U^-1 instead of L U^-T
    mean_step_eta2     the mean step scaled by 1 / eta^2
    eta_lo             eta* = lo where the temperature is larger
    kl_at_lo           the search's KL (at lo) reported for the raised eta
    l2_no_cap / l2_no_floor
    iblr_first_mean    iBLR moving the mean on the first update
    direct_half_step   direct with stepsize / 2"""
    r = case["rounds"][rnd]
    ref = r["ref"]
    out = dict(means=ref["means"].copy(), chols=ref["chols"].copy(), last_eta=ref["last_eta"].copy(), l2=ref["l2"].copy(),
               kls=ref["kls"].copy() if "kls" in ref else None)
    if name in L2_FAULTS:
        out["l2"] = l2_rule(r["l2"], ref["success"], cap=name != "l2_no_cap", floor=name != "l2_no_floor")
    elif name in PLAIN_FAULTS:
        st = dict(r)
        if name == "iblr_first_mean":
            st["num_updates"] = r["num_updates"] + 1
        wrong = run_oracle(st, case["H_neg"], case["g_neg"], case["stepsizes"] * (0.5 if name == "direct_half_step" else 1.0),
                           case["mode"])
        out.update(means=wrong["means"], chols=wrong["chols"])
    else:
        for i in np.where(ref["success"])[0]:
            eta, kl_eta = float(ref["last_eta"][i]), None
            if name == "eta_lo":
                eta = float(ref["lo"][i])
                out["last_eta"][i] = eta
            elif name == "kl_at_lo":
                kl_eta = float(ref["lo"][i])
            f = None if name in ("eta_lo", "kl_at_lo") else name
            out["means"][i], out["chols"][i], out["kls"][i], _, _ = whitened(r["means"][i], r["chols"][i], case["H_neg"][i],
                                                                             case["g_neg"][i], eta, fault=f, kl_eta=kl_eta)
    return out


def kl_bound(g, kl, bkl):
    """C_kl EPS32 B_kl, capped by the assertion of the first-generation tests (rtol 5e-3, atol 1e-5): where the search ends on the
    bracket width the KL is far below eps, and B_kl >= D alone would admit more than that atol from D = 10 on."""
    return min(C_KL[g] * EPS32 * bkl, 1e-5 + 5e-3 * abs(kl))


def compare(case, rnd, got, g=None):
    """``got``: dict(means, chols[, kls, last_eta]) of round ``rnd`` from a device or a planted fault -> dict(E_L, E_mu, E_kl) as
    ratios to the bounds C_L, C_mu, C_kl EPS32 B_kl (<= 1 passes), the worst over the successful components."""
    r = case["rounds"][rnd]
    ref, g = r["ref"], g or group(case)
    ok = ref["success"] & np.asarray(got.get("success", ref["success"]), bool)
    el, em = errors(ref["means"], ref["chols"], got["means"], got["chols"])
    res = dict(E_L=float(np.max(el[ok] / C_L[g], initial=0.0)), E_mu=float(np.max(em[ok] / C_MU[g], initial=0.0)), E_kl=0.0)
    if case["mode"] == "kl" and got.get("kls") is not None:
        for i in np.where(ok)[0]:
            kl, bkl = kl_ref(r, case, i, float(got["last_eta"][i]))
            q = abs(float(got["kls"][i]) - kl) / kl_bound(g, kl, bkl)
            res["E_kl"] = max(res["E_kl"], np.inf if np.isnan(q) else q)
    return res


# ---- the update from the Stein moment slab (gmmvi_stein_update_kl: what the single-call iteration runs) ----------------------------
# Inputs: stein_cases.make_case (fp32-representable x, ld, qgrad, bg, tgrad, means, chols); the fp64 estimate (H, g) of
# stein_cases.reference goes to the fp64 updater unrounded.  The device's estimate carries the Stein error, at most
# C_stein EPS32 B element-wise (stein_cases.C, abs_bound); it is propagated through the step by re-evaluating the update at the
# oracle's eta on H +- C_stein EPS32 B_H, g +- C_stein EPS32 B_g: the spread of the two results, in the measure of errors(), is
# added to C_L and C_mu.  The decision margins take the same perturbation: every probed KL keeps
# 2 C_kl EPS32 B_kl + 2 max |KL(H+-) - KL(H)| from the thresholds.
SLAB_K = 3
SLAB_DIMS = (4, 10, 20, 32, 40, 50, 33)          # fused instances; 33 is not fused (finalize launch, then the update)
SLAB_PARTIALS = (1, 3)
SLAB_SEEDS = {}


def slab_table():
    return [dict(id=f"slab-D{d}-{'snis' if snis else 'plain'}-R{r}", d=d, k=SLAB_K, snis=snis, r=r,
                 seed=SLAB_SEEDS.get(f"slab-D{d}-{'snis' if snis else 'plain'}-R{r}", 0))
            for d in SLAB_DIMS for snis in (True, False) for r in SLAB_PARTIALS]


def slab_n(spec, num_cus=256):
    """N at which launch_stein_moment sums every component from spec['r'] partials on a device with ``num_cus`` compute units
    (stein_cases.n_for_partials for K components), or None."""
    import stein_cases
    n = 130 if spec["r"] == 1 else 256 * (spec["r"] - 1) + 1
    return n if stein_cases.register_geometry(spec["d"], spec["k"], n, num_cus)["R"] == spec["r"] else None


def slab_branch(d, snis, r):
    """update_kl.hip gmmvi_update_components_kl_from_slab and the kernel's ``direct`` predicate, restated -> "direct" (M whitened
    from the moment sums; H_neg / g_neg never written), "prologue" (stein_finalize_component inside the update kernel) or
    "finalize" (the stand-alone finalize launch, then the update)."""
    direct = snis and (d + 1) * (d + 1) + r + 4 + (d * d if d >= 32 else 0) <= 2 * d * 64
    fused = d in (4, 10, 20) or (d in (32, 40, 50) and direct)
    return ("direct" if direct else "prologue") if fused else "finalize"


@functools.lru_cache(maxsize=None)
def _make_slab_case(spec_items, n, check):
    import stein_cases
    spec = dict(spec_items)
    d, k, snis = spec["d"], spec["k"], spec["snis"]
    sc = stein_cases.make_case(dict(route="register", d=d, k=k, n=n, kind="normal", id=spec["id"]), n=n)
    h, g = stein_cases.reference(sc, snis)
    bh, bg = stein_cases.abs_bound(sc, snis)
    steps = f32(np.random.default_rng([spec["seed"], d, n]).uniform(0.05, 0.5, k))
    case = dict(spec, route="register", law="slab", mode="kl", temperature=1.0, n=n, stein=sc, H_neg=h, g_neg=g, stepsizes=steps,
                B_H=bh, B_g=bg)
    state = dict(means=sc["means"], chols=sc["chols"], last_eta=-np.ones(k), l2=np.full(k, L2_INIT), num_updates=np.zeros(k))
    ref = run_oracle(state, h, g, steps, "kl", 1.0)
    klm, pvm, wm, lo = probe_margins(state, case, ref)
    e = stein_cases.C * EPS32
    pert = [(h + sg * e * bh, g + sg * e * bg) for sg in (1.0, -1.0)]
    ckl = C_KL[group(case)]
    spread_l, spread_mu = np.zeros(k), np.zeros(k)
    for i in range(k):
        tris = [tridiagonal_form(*whitened_matrix(state["means"][i], state["chols"][i], hp[i], gp[i])) for hp, gp in pert]
        for le, val in ref["traces"][i]:
            if val >= FLOAT32_MAX:
                continue
            _, bkl = kl_ref(state, case, i, np.exp(le))
            dkl = max(abs(kl_tridiagonal(*tri, np.exp(le))[0] - val) for tri in tris)
            room = min(abs(val - t * steps[i]) for t in wsc.KL_THRESHOLDS)
            klm = min(klm, room / (2 * ckl * EPS32 * bkl + 2 * dkl))
        if ref["success"][i]:
            for hp, gp in pert:
                mu, lo_, _, _, _ = whitened(state["means"][i], state["chols"][i], hp[i], gp[i], float(ref["last_eta"][i]))
                el, em = errors(ref["means"][i:i + 1], ref["chols"][i:i + 1], mu[None], lo_[None])
                spread_l[i], spread_mu[i] = max(spread_l[i], el[0]), max(spread_mu[i], em[0])
    ref.update(kl_margin=klm, pivot_margin=pvm, width_margin=wm, lo=lo, spread_L=spread_l, spread_mu=spread_mu)
    if check:
        assert klm > 1.0 and pvm > PIVOT_MARGIN and wm > WIDTH_MARGIN, (spec["id"], klm, pvm, wm)
    state["ref"] = ref
    case["rounds"] = [state]
    return case


def make_slab_case(spec, n, check=True):
    with _one_thread():
        return _make_slab_case(tuple(sorted(spec.items())), n, check)


def compare_slab(case, got):
    """-> dict(E_L, E_mu) as ratios to C_L + spread_L, C_mu + spread_mu, the worst over the successful components."""
    ref, g = case["rounds"][0]["ref"], group(case)
    ok = ref["success"]
    el, em = errors(ref["means"], ref["chols"], got["means"], got["chols"])
    return dict(E_L=float(np.max((el / (C_L[g] + ref["spread_L"]))[ok], initial=0.0)),
                E_mu=float(np.max((em / (C_MU[g] + ref["spread_mu"]))[ok], initial=0.0)))
