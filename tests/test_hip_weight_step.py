"""GPU parity of the weight step (csrc/weights.hip) against fp64 at temperature != 1 and at the seams of its kernels: the
expected log ratios over several rounds of 1024 x 4 samples and over chunk partials, the categorical weight update at the
K where its register forms change, and the two stepsize rules beyond one wavefront / one workgroup.  The inputs come from
weight_step_cases.py; test_weight_step_cpu.py shows on the oracle alone that fp32 and fp64 take the same bisection path."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import weights as oweights, stepsizes as osteps
import weight_step_cases as cases
from test_hip_kernels import assert_parity

pytestmark = pytest.mark.gpu

BETAS = (0.4, 1.0, 2.5)
# ld - bg spanning 150 nats (elr_wide_inputs): the kernel's worst error against fp64 may be this multiple of the worst error of
# the same formula evaluated in fp32 NumPy (another summation order, exp / log of the fast kind) -- test_hip_bnn_classifier.py
ELR_WIDE_FACTOR = 16.0


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def ops():
    from gmmvi_amd import hip_ops
    return hip_ops


def _elr(ctx, ld, bg, tlp, logq, beta, logw, snis, parts=None):
    reward = ctx.empty((ld.shape[0],))
    e, ess = ops().expected_log_ratios(ctx, ctx.asarray(ld), ctx.asarray(bg), ctx.asarray(tlp),
                                       None if parts is not None else ctx.asarray(logq), beta, ctx.asarray(logw), snis,
                                       reward_out=reward, want_ess=True,
                                       logq_parts=None if parts is None else ctx.asarray(parts))
    return e.numpy(), reward.numpy(), ess.numpy()


def _assert_elr(got, ref, what):
    for g, r, name in zip(got, ref, ("E", "reward", "ess")):
        assert_parity(g, r, 1e-4, 1e-5, f"{name} {what}")


@pytest.mark.parametrize("k,n", [(k, n) for n in (1, 63, 1023, 1024, 1025, 4096, 4097, 9000) for k in (1, 3)] + [(300, 1025)])
def test_expected_log_ratios_rounds_and_temperature(ctx, rng, k, n):
    """One to three rounds of 1024 x 4 samples per thread with ragged (clamped) tails, K = 1 ... 300 workgroups, beta on both
    sides of 1, both importance-weight modes, rewards and effective sample sizes: rtol 1e-4 / atol 1e-5."""
    ld, bg, tlp, logq, logw = cases.elr_benign_inputs(rng, k, n)
    for beta in BETAS:
        for snis in (True, False):
            got = _elr(ctx, ld, bg, tlp, logq, beta, logw, snis)
            _assert_elr(got, cases.elr_formula(ld, bg, tlp, logq, beta, logw, snis), f"K={k} N={n} beta={beta} snis={snis}")


@pytest.mark.parametrize("n", [63, 4097, 9000])
def test_expected_log_ratios_minus_infinity_target(ctx, rng, n):
    """tlp = -inf on samples that carry weight (first, last and, from the second round on, one in a later round): the fp64
    value is -inf (or NaN); the kernel returns the same class, for E and for the reward, and a finite ESS."""
    k = 3
    ld, bg, tlp, logq, logw = cases.elr_benign_inputs(rng, k, n)
    tlp = tlp.copy()
    tlp[[0, n - 1, min(n - 1, 4096 + 17)]] = -np.inf
    for beta in (0.4, 2.5):
        for snis in (True, False):
            e, reward, ess = _elr(ctx, ld, bg, tlp, logq, beta, logw, snis)
            re, rr, ress = cases.elr_formula(ld, bg, tlp, logq, beta, logw, snis)
            assert np.all(np.isneginf(re) | np.isnan(re))
            for g, r in ((e, re), (reward, rr)):
                np.testing.assert_array_equal(np.isneginf(g), np.isneginf(r))
                np.testing.assert_array_equal(np.isnan(g), np.isnan(r))
            assert_parity(ess, ress, 1e-4, 1e-5, "ess")


def test_expected_log_ratios_wide_range(ctx, rng):
    """ld - bg over 150 nats, a maximum in the clamped tail of the last round, a row carried by one sample.  The bound is not
    guessed: the kernel's worst error against fp64, relative to max(1, max |fp64|) per quantity, stays below ELR_WIDE_FACTOR
    times that of the fp32 NumPy evaluation of the same formula (DESIGN.md section 4 records both figures)."""
    ld, bg, tlp, logq, logw = cases.elr_wide_inputs(rng)
    worst_kernel, worst_f32 = {}, {}
    for beta in BETAS:
        for snis in (True, False):
            ref = cases.elr_formula(ld, bg, tlp, logq, beta, logw, snis)
            f32 = cases.elr_formula(ld, bg, tlp, logq, beta, logw, snis, dtype=np.float32)
            got = _elr(ctx, ld, bg, tlp, logq, beta, logw, snis)
            for g, f, r, name in zip(got, f32, ref, ("E", "reward", "ess")):
                assert np.all(np.isfinite(g)), (name, beta, snis)
                scale = max(1.0, float(np.max(np.abs(r))))
                worst_kernel[name] = max(worst_kernel.get(name, 0.0), float(np.max(np.abs(g - r))) / scale)
                worst_f32[name] = max(worst_f32.get(name, 0.0), float(np.max(np.abs(f.astype(np.float64) - r))) / scale)
    for name in worst_kernel:
        print(f"elr wide range {name}: kernel {worst_kernel[name]:.3e}, fp32 NumPy {worst_f32[name]:.3e}, "
              f"ratio {worst_kernel[name] / worst_f32[name]:.2f}")
    for name in worst_kernel:
        assert worst_kernel[name] <= ELR_WIDE_FACTOR * worst_f32[name], name


@pytest.mark.parametrize("r", [2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 9, 20])
def test_expected_log_ratios_over_chunk_partials(ctx, rng, r):
    """logq handed over as the R chunk partials of a component-split sweep, merged while read (elr_accumulate<2..16> and, for
    R = 9 and 20, the run-time loop), one partial row -inf on a third of the samples: against fp64 logsumexp over R fed to the
    same formula, N = 4097 (second round, one sample), beta = 2.5."""
    k, n, beta = 3, 4097, 2.5
    ld, bg, tlp, logq, logw = cases.elr_benign_inputs(rng, k, n)
    parts = cases.split_log_values(rng, logq, r)
    assert np.isneginf(parts).any() and not np.isneginf(parts).all(axis=0).any()
    merged = logsumexp(parts, axis=0)
    for snis in (True, False):
        got = _elr(ctx, ld, bg, tlp, None, beta, logw, snis, parts=parts)
        _assert_elr(got, cases.elr_formula(ld, bg, tlp, merged, beta, logw, snis), f"R={r} snis={snis}")


def test_expected_log_ratios_parts_argument_checks(ctx, rng):
    ld, bg, tlp, logq, logw = cases.elr_benign_inputs(rng, 2, 70)
    d = [ctx.asarray(a) for a in (ld, bg, tlp, logq, logw)]
    with pytest.raises(ValueError):
        ops().expected_log_ratios(ctx, d[0], d[1], d[2], d[3], 1.0, d[4], logq_parts=ctx.asarray(np.stack([logq, logq])))
    with pytest.raises(ValueError):
        ops().expected_log_ratios(ctx, d[0], d[1], d[2], None, 1.0, d[4], logq_parts=ctx.asarray(logq[None, :]))
    e = ctx.empty((2,))
    rc = ctx.lib.gmmvi_expected_log_ratios_parts(ctx.handle, 2, 70, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, 1, 1.0, d[4].ptr, 1,
                                                 e.ptr, None, None)
    assert rc == -2                                                      # GMMVI_ERR_ARG: fewer than two partial rows


def _check_weight_update(ctx, lw, elr, beta, eps, what):
    logw = ctx.asarray(lw)
    info = ops().update_weights(ctx, "trust-region", logw, ctx.asarray(elr), ctx.asarray([eps]), beta, True).numpy()
    kl, eta, nl = oweights.weights_bracketing_search(lw, elr, eps, beta)
    nl = nl - logsumexp(nl)
    np.testing.assert_allclose(info[1], eta, rtol=1e-4, err_msg=f"eta {what}")
    np.testing.assert_allclose(info[0], kl, rtol=5e-3, atol=1e-5, err_msg=f"kl {what}")
    np.testing.assert_allclose(logw.numpy(), nl, rtol=1e-4, atol=2e-4, err_msg=f"log weights {what}")
    return logw.numpy()


def _check_direct_update(ctx, lw, elr, beta, what):
    class W:
        num_components = lw.shape[0]
        log_weights = lw

        def replace_weights(self, nl):
            self.new = nl - logsumexp(nl)
    w = W()
    oweights.direct_update(w, elr, cases.DIRECT_STEPSIZE, beta)
    logw = ctx.asarray(lw)
    ops().update_weights(ctx, "direct", logw, ctx.asarray(elr), ctx.asarray([cases.DIRECT_STEPSIZE]), beta)
    np.testing.assert_allclose(logw.numpy(), w.new, rtol=1e-4, atol=2e-4, err_msg=f"direct {what}")
    return logw.numpy()


@pytest.mark.parametrize("k", cases.WEIGHT_KS[1:])
def test_update_weights_at_the_seams_and_temperatures(ctx, k):
    """Both sides of every register form (K <= 128 | 256 | 512 | 1024 | LDS loop up to 4096) and of a wavefront, beta on both
    sides of 1, a tight, an ordinary and a never-binding bound: eta, KL and the new log weights against the oracle's search."""
    lw, elr = cases.weight_inputs(k)
    for beta in cases.WEIGHT_BETAS:
        for eps in cases.WEIGHT_EPS:
            _check_weight_update(ctx, lw, elr, beta, eps, f"K={k} beta={beta} eps={eps}")
        _check_direct_update(ctx, lw, elr, beta, f"K={k} beta={beta}")


def test_update_weights_single_component_and_range(ctx):
    """K = 1: the weight stays, kl = eta = -1 (weight_updater.py:275); K > 4096 is refused with GMMVI_ERR_ARG."""
    for beta in cases.WEIGHT_BETAS:
        logw = ctx.asarray(np.zeros(1))
        info = ops().update_weights(ctx, "trust-region", logw, ctx.asarray([3.0]), ctx.asarray([0.3]), beta, True)
        np.testing.assert_array_equal(info.numpy(), [-1.0, -1.0])
        np.testing.assert_array_equal(logw.numpy(), [0.0])
        ops().update_weights(ctx, "direct", logw, ctx.asarray([3.0]), ctx.asarray([0.3]), beta)
        np.testing.assert_array_equal(logw.numpy(), [0.0])
    k = 4097
    logw, e, step, info = ctx.asarray(np.full(k, -np.log(k))), ctx.zeros((k,)), ctx.asarray([0.3]), ctx.empty((2,))
    assert ctx.lib.gmmvi_update_weights_kl(ctx.handle, k, logw.ptr, e.ptr, step.ptr, 1.0, info.ptr) == -2
    assert ctx.lib.gmmvi_update_weights_direct(ctx.handle, k, logw.ptr, e.ptr, step.ptr, 1.0) == -2
    np.testing.assert_array_equal(logw.numpy(), np.full(k, -np.log(k), np.float32))


def test_update_weights_floor(ctx):
    """A tenth of the components on the -69.07 floor before the final renormalisation (test_weight_step_cpu.py), the others
    not: the floored weights come out equal, at the oracle's value."""
    k = cases.FLOOR_K
    lw, elr = cases.weight_inputs(k, floor=True)
    hopeless = elr < -1000
    assert 0 < hopeless.sum() < k
    for beta in cases.WEIGHT_BETAS:
        for eps in cases.FLOOR_EPS:
            new = _check_weight_update(ctx, lw, elr, beta, eps, f"floor beta={beta} eps={eps}")
            assert np.all(new[hopeless] == new[hopeless][0]) and abs(new[hopeless][0] - cases.LOG_WEIGHT_FLOOR) < 1e-4
            assert np.all(new[~hopeless] > cases.LOG_WEIGHT_FLOOR + 1.0)
        new = _check_direct_update(ctx, lw, elr, beta, f"floor beta={beta}")
        assert np.all(new[hopeless] == new[hopeless][0]) and abs(new[hopeless][0] - cases.LOG_WEIGHT_FLOOR) < 1e-4


@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 1000])
def test_stepsize_kernels_beyond_one_wavefront(ctx, rng, k):
    """component rule: second workgroup (K > 128), ties prev == last (a decrease, :177), steps clamped at min_stepsize and
    max_stepsize, float32.min sentinel rows.  weight rule: the lane-strided loop (K > 64) on non-uniform weights over five
    calls, one of them a tie with the call before."""
    mn, mx, inc, dec = 0.001, 1.0, 1.15, 0.85
    steps = (rng.random(k) * 0.9 + 0.002).astype(np.float32)
    prev, last = rng.normal(size=k).astype(np.float32), rng.normal(size=k).astype(np.float32)
    sentinel = np.finfo(np.float32).min
    idx = rng.permutation(k)
    tie, lowest, highest, fresh, half_fresh = (idx[i::5] for i in range(5))
    last[tie] = prev[tie]
    steps[lowest] = 0.00105; prev[lowest] = 1.0; last[lowest] = 0.0              # 0.85 x 0.00105 < min_stepsize
    steps[highest] = 0.95; prev[highest] = 0.0; last[highest] = 1.0              # 1.15 x 0.95 > max_stepsize
    prev[fresh] = last[fresh] = sentinel
    prev[half_fresh] = sentinel
    s = ctx.asarray(steps)
    ops().component_stepsize_improvement(ctx, s, ctx.asarray(prev), ctx.asarray(last), mn, mx, inc, dec)
    ref = osteps.component_stepsize_improvement(steps, np.stack([prev, last], 1), mn, mx, inc, dec)
    got = s.numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-6)
    assert np.all(got[lowest] == np.float32(mn)) and np.all(got[highest] == np.float32(mx))
    np.testing.assert_allclose(got[tie], np.maximum(np.float32(dec) * steps[tie], np.float32(mn)), rtol=1e-6)
    assert np.all(got[fresh] < steps[fresh]) and np.all(got[half_fresh] >= steps[half_fresh])

    class W:
        pass
    w = W()
    w.log_weights = cases.f32(np.log(rng.dirichlet(np.ones(k))))
    w.weights = np.exp(w.log_weights)
    a = osteps.WeightStepsizeImprovement(1.0, 1e-4, 1.0, 1.15, 0.85)
    state = ctx.asarray([1.0, sentinel])
    r1 = cases.f32(rng.normal(size=k) - 5)
    seen = []
    for rewards in [np.full(k, float(sentinel)), r1, r1, cases.f32(rng.normal(size=k) - 50), cases.f32(rng.normal(size=k))]:
        w.reward_history = np.stack([rewards, rewards], 1)
        ops().weight_stepsize_improvement(ctx, ctx.asarray(w.log_weights), ctx.asarray(rewards), state, 1e-4, 1.0, 1.15, 0.85)
        ref = a.update_stepsize(w)
        np.testing.assert_allclose(state.numpy()[0], ref, rtol=1e-6)
        np.testing.assert_allclose(state.numpy()[1], a.elbo_history[-1], rtol=1e-6)
        seen.append(ref)
    assert seen[0] < 1.0 and seen[1] > seen[0] and seen[2] < seen[1] and seen[3] < seen[2] and seen[4] > seen[3]
