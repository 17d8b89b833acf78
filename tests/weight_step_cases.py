"""Inputs and fp64 reference figures shared by test_hip_weight_step.py / test_hip_temperature.py (GPU) and
test_weight_step_cpu.py: the weight step and the component KL update at temperature != 1.  Nothing here touches the device.

Every bisection case is built so that fp32 and fp64 take the same path: each probed KL stays PROBE_MARGIN (relative to the
bound) away from the thresholds 0.9 eps, eps and 1.1 eps, each bracket-width test stays PROBE_MARGIN away from 0.1.  The seeds
below are the first ones at which that holds; test_weight_step_cpu.py asserts it."""
import numpy as np
from scipy.special import logsumexp

from oracle import gmm as ogmm, updaters as oupd, weights as oweights
import diag_highd_cases

PROBE_MARGIN = 1e-3
SEED_SEARCH_MARGIN = 5e-3      # the committed seeds were searched with five times the margin that is asserted
KL_THRESHOLDS = (0.9, 1.0, 1.1)
LOG_WEIGHT_FLOOR = oweights.LOG_WEIGHT_FLOOR


def f32(a):
    """fp32-representable fp64 values: the device and the oracle read the same numbers."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- component KL update --------------------------------------------------------------------------------------------------
# route -> dimensions; "dense" / "reference" / "blocked" are full-covariance kernels, "diag" the three diagonal ones (D = 64 runs
# on the blocked route: gmmvi_blocked_above() is 50 unless GMMVI_BLOCKED_ABOVE says otherwise)
KL_ROUTES = {"dense": (4, 20, 33, 50), "reference": (4, 33), "blocked": (64, 72, 130), "diag": (20, 600, 9000)}
KL_TEMPERATURES = (0.25, 30.0)
KL_K = 6
KL_STEPSIZES = np.linspace(0.05, 0.5, KL_K)
# reward scales per component: the accepted eta is proportional to the scale of (H, g), so at temperature 30 the scales 1 and 64
# put the warm round's result on both sides of the temperature.  The search cannot return less than 1: a cold bracket (-20, 80)
# stops bisecting at exp(5) (the next midpoint, exp(-7.5), fails the width test) and a warm one starts at max(0, log eta - 3).
# So ``eta == temperature > lo`` needs temperature > 1 and a warm start; the temperature 0.25 case keeps ``eta == lo`` everywhere
# and checks that a kernel does not raise or rescale eta there.
# Above D = 512 update_scale() already lifts the unscaled result to 33 ... 150: the scales there are 1/8 and 8.
KL_SCALES = {30.0: (1.0, 64.0, 1.0, 64.0, 1.0, 64.0), 0.25: (1.0,) * 6}
KL_SCALES_HIGHD = {30.0: (0.125, 8.0, 0.125, 8.0, 0.125, 8.0), 0.25: (1.0,) * 6}
# (route, d, temperature) -> seed, found by first_good_kl_seed()
KL_SEEDS = {("dense", 4, 0.25): 0, ("dense", 4, 30.0): 4, ("dense", 20, 0.25): 0, ("dense", 20, 30.0): 1, ("dense", 33, 0.25): 1,
            ("dense", 33, 30.0): 2, ("dense", 50, 0.25): 0, ("dense", 50, 30.0): 0, ("reference", 4, 0.25): 0,
            ("reference", 4, 30.0): 4, ("reference", 33, 0.25): 1, ("reference", 33, 30.0): 2, ("blocked", 64, 0.25): 1,
            ("blocked", 64, 30.0): 4, ("blocked", 72, 0.25): 1,
            ("blocked", 72, 30.0): 1, ("blocked", 130, 0.25): 0, ("blocked", 130, 30.0): 0, ("diag", 20, 0.25): 1,
            ("diag", 20, 30.0): 1, ("diag", 600, 0.25): 5, ("diag", 600, 30.0): 0, ("diag", 9000, 0.25): 1, ("diag", 9000, 30.0): 4}


def kl_case_ids():
    return [(route, d, t) for route, dims in KL_ROUTES.items() for d in dims for t in KL_TEMPERATURES]


def _random_full_gmm(rng, k, d):
    """(the law of tests/test_hip_kernels.py: random_gmm)"""
    means = rng.normal(size=(k, d)) * 3.0
    covs = []
    for _ in range(k):
        a = rng.normal(size=(d, d))
        covs.append(a @ a.T / d + 0.3 * np.eye(d))
    w = rng.random(k) + 0.1
    return ogmm.FullCovGMM(w / w.sum(), means, np.stack(covs))


def kl_update_inputs(route, d, temperature, seed=None):
    """-> (fp64 model with fp32-representable parameters, H_neg, g_neg (fp32-representable), stepsizes [K])."""
    if seed is None:
        seed = KL_SEEDS.get((route, d, temperature), 0)
    rng = np.random.default_rng(seed)
    k = KL_K
    scales = np.asarray((KL_SCALES_HIGHD if route == "diag" and d > 512 else KL_SCALES)[temperature])
    if route == "diag":
        m = diag_highd_cases.random_diag_gmm(rng, k, d)
        s = diag_highd_cases.update_scale(d)
        hs = (rng.normal(size=(k, d)) * 0.5 + 0.3) * s * scales[:, None]
        gs = rng.normal(size=(k, d)) * s * scales[:, None]
        m32 = ogmm.DiagonalGMM(m.weights, m.means.astype(np.float32), m.covs.astype(np.float32))
    else:
        m = _random_full_gmm(rng, k, d)
        hs = np.stack([(lambda b: b @ b.T / d)(rng.normal(size=(d, d))) for _ in range(k)])
        hs[2] = -0.01 * hs[2]                                            # one concave reward: small eta is infeasible
        hs = hs * scales[:, None, None]
        gs = rng.normal(size=(k, d)) * scales[:, None]
        m32 = ogmm.FullCovGMM(m.weights, m.means.astype(np.float32), m.covs.astype(np.float32))
    return m32, f32(hs), f32(gs), KL_STEPSIZES.copy()


def replay_component_search(kl_bound, last_eta, trace):
    """Replays updaters.bracketing_search (log space) on the probed values of ``trace`` -> (lo, hi, smallest distance of a
    probed KL from a threshold in units of the bound, smallest distance of a bracket-width test from 0.1)."""
    if last_eta < 0:
        lb, ub = -20.0, 80.0
    else:
        lb, ub = max(0.0, np.log(last_eta) - 3), np.log(last_eta) + 3
    eta = 0.5 * (ub + lb)
    ub_ok = False
    kl_margin = width_margin = np.inf
    i = 0
    for _ in range(1000):
        diff = min(np.exp(ub) - np.exp(eta), np.exp(eta) - np.exp(lb))
        width_margin = min(width_margin, abs(diff - 1e-1))
        if diff < 1e-1:
            break
        e, val = trace[i]
        i += 1
        assert e == eta
        if np.isfinite(val):
            kl_margin = min(kl_margin, min(abs(val - t * kl_bound) for t in KL_THRESHOLDS) / kl_bound)
        if abs(kl_bound - val) < 1e-1 * kl_bound:
            lb = ub = eta
            break
        if kl_bound > val:
            ub = eta
            ub_ok = True
        else:
            lb = eta
        eta = 0.5 * (ub + lb)
    assert i == len(trace)
    if ub_ok:
        lb = ub
    return np.exp(lb), np.exp(ub), kl_margin, width_margin


def run_kl_case(route, d, temperature, seed=None):
    """Two rounds (cold, warm) of the fp64 oracle -> list per round of dict(success, etas, kls, probes, lo [K] = the search's
    result before max(lo, temperature), kl_margin, width_margin)."""
    m, hs, gs, steps = kl_update_inputs(route, d, temperature, seed)
    w = ogmm.GmmWrapper(m, 0.1, 1e-12, 4)
    w.stepsizes = steps
    rounds = []
    for _ in range(2):
        last = w.last_log_etas.copy()
        traces = []
        succ, etas, kls, probes = oupd.apply_ng_update_kl(w, hs, gs, steps, temperature, traces=traces)
        lo = np.empty(KL_K)
        klm = wm = np.inf
        for i in range(KL_K):
            lo[i], hi, a, b = replay_component_search(steps[i], last[i], traces[i])
            klm, wm = min(klm, a), min(wm, b)
            assert succ[i] == (lo[i] == hi) or not succ[i]
        rounds.append(dict(success=succ, etas=etas, kls=kls, probes=probes, lo=lo, kl_margin=klm, width_margin=wm))
    return rounds


def kl_case_holds(rounds, temperature, margin=PROBE_MARGIN):
    """The preconditions for one case: every probe of both rounds clear of the thresholds; in the warm round a successful
    component with eta == lo > temperature and, at a temperature above 1 (see KL_SCALES), one with eta == temperature > lo."""
    r = rounds[1]
    s = r["success"]
    raised = np.any(s & (r["etas"] == temperature) & (r["lo"] < temperature))
    kept = np.any(s & (r["etas"] == r["lo"]) & (r["lo"] > temperature))
    clear = all(x["kl_margin"] >= margin and x["width_margin"] >= margin for x in rounds)
    return bool((raised or temperature < 1) and kept and clear)


def first_good_kl_seed(route, d, temperature, tries=200):
    for seed in range(tries):
        if kl_case_holds(run_kl_case(route, d, temperature, seed), temperature, SEED_SEARCH_MARGIN):
            return seed
    raise AssertionError((route, d, temperature))


# ---- categorical weight update ----------------------------------------------------------------------------------------------
WEIGHT_KS = (1, 2, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096)
WEIGHT_BETAS = (0.4, 1.0, 2.5)
WEIGHT_EPS = (0.01, 0.3, 1e4)
DIRECT_STEPSIZE = 0.5
# K -> seed, found by first_good_weight_seed(); "floor" -> the floor case
WEIGHT_SEEDS = {2: 0, 64: 3, 65: 0, 128: 0, 129: 0, 256: 0, 257: 3, 512: 0, 513: 0, 1024: 1, 1025: 2, 4096: 2, "floor": 0}
FLOOR_K = 129
FLOOR_EPS = (0.3, 1e4)        # (at eps = 0.01 eta is in the thousands and nothing reaches the floor)


def weight_inputs(k, seed=None, floor=False):
    """-> (normalised log weights, expected log ratios), both fp32-representable.  ``floor``: a tenth of the components has a
    hopeless reward, which the update puts on the -69.07 floor."""
    if seed is None:
        seed = WEIGHT_SEEDS.get("floor" if floor else k, 0)
    rng = np.random.default_rng([seed, k])
    lw = np.log(rng.dirichlet(np.ones(k)))
    lw = f32(lw - logsumexp(lw))
    elr = rng.normal(size=k) * 3
    if floor:
        elr[rng.permutation(k)[: k // 10]] -= 3000.0
    return lw, f32(elr)


def replay_weight_search(lw, elr, kl_bound, temperature):
    """weights.weights_bracketing_search step by step (same probes through weights.weights_kl) -> (kl, eta, new log weights,
    kl_margin, width_margin, number of entries on the floor before the final renormalisation of the returned weights)."""
    lb, ub = -45.0, 45.0
    log_eta = 0.5 * (ub + lb)
    ub_ok = False
    kl, eta, nl = -1.0, -1.0, lw
    kl_margin = width_margin = np.inf
    for _ in range(50):
        eta = np.exp(log_eta)
        width = abs(np.exp(ub) - np.exp(lb))
        width_margin = min(width_margin, abs(width - 1e-1))
        if width < 1e-1:
            break
        kl, nl = oweights.weights_kl(eta, lw, elr, temperature)
        kl_margin = min(kl_margin, min(abs(kl - t * kl_bound) for t in KL_THRESHOLDS) / kl_bound)
        if abs(kl_bound - kl) < 1e-1 * kl_bound:
            lb = ub
            break
        if kl_bound > kl:
            ub, ub_ok = log_eta, True
        else:
            lb = log_eta
        log_eta = 0.5 * (ub + lb)
    if lb != ub:
        if ub_ok:
            eta = np.exp(ub)
            kl, nl = oweights.weights_kl(eta, lw, elr, temperature)
        else:
            return -1.0, -1.0, lw, kl_margin, width_margin, 0
    u = (eta + 1) / (temperature + eta) * lw + 1.0 / (temperature + eta) * elr
    on_floor = int(np.sum(u - logsumexp(u) < LOG_WEIGHT_FLOOR))
    return kl, eta, nl, kl_margin, width_margin, on_floor


def weight_case_holds(k, seed=None, floor=False, margin=PROBE_MARGIN):
    lw, elr = weight_inputs(k, seed, floor)
    for beta in WEIGHT_BETAS:
        for eps in WEIGHT_EPS:
            _, _, _, a, b, nf = replay_weight_search(lw, elr, eps, beta)
            if a < margin or b < margin or (floor and eps in FLOOR_EPS and not 0 < nf < k):
                return False
    return True


def first_good_weight_seed(k, floor=False, tries=200):
    for seed in range(tries):
        if weight_case_holds(k, seed, floor, SEED_SEARCH_MARGIN):
            return seed
    raise AssertionError((k, floor))


def direct_floor_count(lw, elr, stepsize, temperature):
    u = lw + stepsize / temperature * elr
    return int(np.sum(u - logsumexp(u) < LOG_WEIGHT_FLOOR))


# ---- expected log ratios ----------------------------------------------------------------------------------------------------
def elr_formula(ld, bg, tlp, logq, beta, logw, snis, dtype=np.float64):
    """weight_updater.py:56-75 in ``dtype`` arithmetic -> (E [K], reward [K], ess [K]): the importance weights
    exp(ld - bg) against their row maximum, E = sum w rho / sum w (self-normalised) or sum w rho exp(max) / N."""
    ld, bg, tlp, logq, logw = (np.asarray(a, np.float64).astype(dtype) for a in (ld, bg, tlp, logq, logw))
    beta = dtype(beta)
    with np.errstate(invalid="ignore", over="ignore"):
        rho = tlp - beta * logq
        a = ld - bg[None, :]
        m = a.max(axis=1, keepdims=True)
        w = np.exp(a - m)
        s = w.sum(axis=1, dtype=dtype)
        se = (w * rho[None, :]).sum(axis=1, dtype=dtype)
        e = se / s if snis else se * np.exp(m[:, 0]) / dtype(ld.shape[1])
        ess = s * s / (w * w).sum(axis=1, dtype=dtype)
        return e, beta * logw + e, ess


def elr_benign_inputs(rng, k, n):
    """(the law of test_hip_kernels.py: test_expected_log_ratios) -> fp32-representable (ld, bg, tlp, logq, logw)."""
    ld = rng.normal(size=(k, n)) * 3 - 10
    bg = logsumexp(ld, axis=0) - np.log(k) + rng.normal(size=n) * 0.1
    tlp = rng.normal(size=n) * 5 - 20
    logq = logsumexp(ld - np.log(k), axis=0)
    logw = np.log(rng.dirichlet(np.ones(k)))
    return tuple(f32(a) for a in (ld, bg, tlp, logq, logw))


ELR_WIDE_N = 9000


def elr_wide_inputs(rng):
    """Three rows over N = 9000 (three rounds of 1024 x 4 samples, the last one ragged) whose ld - bg spans 150 nats:
    row 0 rises to its maximum at the very last sample (the clamped tail of the last round), row 1 is dominated by one sample
    in the second round, row 2 is spread evenly over the range."""
    n, k = ELR_WIDE_N, 3
    bg = rng.normal(size=n) * 2 - 12
    a = np.empty((k, n))
    a[0] = np.linspace(-150.0, 0.0, n) + rng.normal(size=n) * 0.5
    a[0, n - 1] = 3.0
    a[1] = rng.uniform(-150.0, -40.0, size=n)
    a[1, 5000] = 0.0
    a[2] = rng.uniform(-150.0, 0.0, size=n)
    ld = f32(a + bg[None, :])
    bg = f32(bg)
    tlp = f32(rng.normal(size=n) * 5 - 20)
    logq = f32(rng.normal(size=n) * 3 - 12)
    logw = f32(np.log(rng.dirichlet(np.ones(k))))
    return ld, bg, tlp, logq, logw


def split_log_values(rng, logq, r, dead_rows=1):
    """[r, N] fp32-representable partial rows; ``dead_rows`` of them are -inf on a third of the samples (a chunk of components
    whose densities all underflowed there).  The merged value is logsumexp over r of what is returned, not ``logq``."""
    n = logq.shape[0]
    frac = rng.dirichlet(np.ones(r), size=n).T
    parts = logq[None, :] + np.log(frac) + rng.normal(size=(r, n)) * 0.5
    for j in range(dead_rows):
        parts[(j * 3 + 1) % r, rng.random(n) < 1 / 3] = -np.inf
    return f32(parts)
