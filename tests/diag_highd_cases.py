"""Inputs and fp64 reference figures shared by test_hip_diag_highd.py (GPU) and test_diag_highd_cpu.py: diagonal mixtures
above D = 512.  Nothing here touches the device."""
import numpy as np

from oracle import gmm as ogmm, updaters as oupd

KL_CASES = [(3, 513), (4, 1024), (2, 8192), (2, 101770)]
ESS_CASE = (5, 20000, 512)

# worst relative difference of last_eta between the fp64 oracle and the oracle in fp32 mode over eta_tolerance_cases() (D = 512,
# where the one-wavefront kernel is trusted): 1.04e-7.  The device may differ from the fp64 oracle by four times that above 512.
ETA_RTOL_D512 = 1.04e-7


def random_diag_gmm(rng, k, d, dtype=np.float64):
    """(copy of tests/test_hip_diag_mmd.py: random_diag_gmm)"""
    means = rng.normal(size=(k, d)) * 3.0
    var = rng.uniform(0.3, 3.0, size=(k, d))
    w = rng.random(k) + 0.1
    return ogmm.DiagonalGMM(w / w.sum(), means, var, dtype=dtype)


def update_scale(d):
    """The inputs of test_hip_diag_mmd.py: _diag_update_inputs are of unit size per dimension, so the KL of a step at fixed eta
    grows like D.  Scaling them by sqrt(512 / D) above 512 keeps the accepted eta where it lies at D = 512 (33 ... 150 for the
    stepsizes 0.05 ... 0.5): the step is neither rejected nor trivial (accepted KL between 0.05 and 1.09 of the bound)."""
    return np.sqrt(512.0 / d) if d > 512 else 1.0


def diag_update_inputs(rng, k, d):
    """-> (fp64 DiagonalGMM with fp32-representable parameters, H_neg [k, d], g_neg [k, d], stepsizes [k]); the estimates are
    fp32-representable too, so that the device and the fp64 oracle read the same numbers."""
    m = random_diag_gmm(rng, k, d)
    hs = ((rng.normal(size=(k, d)) * 0.5 + 0.3) * update_scale(d)).astype(np.float32)   # mixed signs: negative precisions at small eta
    gs = (rng.normal(size=(k, d)) * update_scale(d)).astype(np.float32)
    m32 = ogmm.DiagonalGMM(m.weights, m.means.astype(np.float32), m.covs.astype(np.float32))
    return m32, hs, gs, np.linspace(0.05, 0.5, k)


def diag_kl_fp64(mean_new, sigma_new, mean_old, sigma_old):
    """KL(new || old) of two diagonal Gaussians, fp64, per-dimension terms."""
    mean_new, sigma_new, mean_old, sigma_old = (np.asarray(a, np.float64) for a in (mean_new, sigma_new, mean_old, sigma_old))
    r = np.square(sigma_new / sigma_old)
    return 0.5 * float(np.sum(r - 1.0 - np.log(r)) + np.sum(np.square((mean_new - mean_old) / sigma_old)))


def eta_tolerance_cases():
    """Worst relative last_eta difference, fp64 oracle against the oracle in fp32 mode, two rounds each at D = 512."""
    worst = 0.0
    for k in (2, 3, 4, 8):
        m, hs, gs, steps = diag_update_inputs(np.random.default_rng(1234), k, 512)
        m32 = ogmm.DiagonalGMM(m.weights, m.means.astype(np.float32), m.covs.astype(np.float32), dtype=np.float32)
        w64, w32 = ogmm.GmmWrapper(m, 0.1, 1e-12, 4), ogmm.GmmWrapper(m32, 0.1, 1e-12, 4)
        for _ in range(2):
            _, e64, _, _ = oupd.apply_ng_update_kl(w64, hs.astype(np.float64), gs.astype(np.float64), steps, 1.0, traces=[])
            _, e32, _, _ = oupd.apply_ng_update_kl(w32, hs, gs, steps.astype(np.float32), np.float32(1.0), traces=[])
            worst = max(worst, float(np.max(np.abs(e32.astype(np.float64) - e64) / np.abs(e64))))
    return worst


def ess(ld, bg):
    """Effective sample size per component of the self-normalised importance weights softmax_n(ld[k, n] - bg[n]), fp64."""
    lw = np.asarray(ld, np.float64) - np.asarray(bg, np.float64)[None, :]
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    return 1.0 / np.sum(w * w, axis=1)


def ess_case(rng):
    """-> (model, x fp32 [N, D], fp64 ld [K, N], fp64 bg [N], ESS of the fp64 values, worst relative ESS deviation that rounding
    ld and bg to fp32 alone produces)."""
    k, d, n = ESS_CASE
    m = random_diag_gmm(rng, k, d)
    m = ogmm.DiagonalGMM(m.weights, m.means.astype(np.float32), m.covs.astype(np.float32))
    n_k = np.full(k, n // k)
    n_k[: n - n_k.sum()] += 1
    x, _ = m.sample_from_components_no_shuffle(n_k, rng.normal(size=(n, d)))
    x = x.astype(np.float32)
    bg, ld = m.log_densities_also_individual(x.astype(np.float64))
    e64 = ess(ld, bg)
    e32 = ess(ld.astype(np.float32), bg.astype(np.float32))
    return m, x, ld, bg, e64, float(np.max(np.abs(e32 - e64) / e64))


def ulps_off(got, want):
    """|got - want| in units of the fp32 spacing at |want|."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
