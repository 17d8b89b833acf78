"""GPU parity of gmmvi_more_diag (csrc/more_diag.hip: the gradient-free MORE estimate for diagonal-covariance mixtures,
features [z^2, z, 1]) against the fp64 restatement tests/more_diag_ref.py, through the C ABI
(gmmvi_amd.hip_ops), and the end-to-end run of a target that implements log_density only.

Bound.  The project's MORE bound (test_hip_kernels.py, test_hip_more_blocked.py), unchanged: |device - reference| <= 1e-2 of
the component's largest |reference| entry + 1e-5, for H and g.  Every test prints the measured deviation before it asserts;
the figures measured on an MI355X are in DESIGN.md section 4b and next to each bound."""
import functools

import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import philox, gmm as ogmm, targets as otargets
from helpers import samtron_config
import more_diag_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-2


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def ops():
    from gmmvi_amd import hip_ops
    return hip_ops


def random_diag_gmm(rng, k, d, spread=3.0):
    w = rng.random(k) + 0.1
    return ogmm.DiagonalGMM(w / w.sum(), rng.normal(size=(k, d)) * spread, rng.random((k, d)) * 1.5 + 0.3)


def _inputs(rng, k, d, n, n_k=None):
    """The input pattern of test_hip_more_blocked.py on a diagonal model: samples of the model's own components, a GMM
    target, background densities of the count-weighted mixture that drew the samples."""
    m = random_diag_gmm(rng, k, d)
    n_k = rng.multinomial(n, np.ones(k) / k) if n_k is None else np.asarray(n_k)
    x, mapping = m.sample_from_components_no_shuffle(n_k, philox.normals(5, 0, n, d))
    x = x.astype(np.float32).astype(np.float64)
    tgt = otargets.make_gmm_target(d, rng, 3)
    tlp, _ = tgt.log_density_and_grad(x)
    cnt = np.maximum(n_k, 1e-9)
    bg = logsumexp(m.component_log_densities(x) + np.log(cnt / cnt.sum())[:, None], axis=0)
    return m, x, mapping, tlp, bg


@functools.lru_cache(maxsize=None)
def _case(k, d, n):
    """Inputs of one parity shape, built once and shared by both weightings (never modified)."""
    return _inputs(np.random.default_rng(4000 + 7 * d + k), k, d, n)


@functools.lru_cache(maxsize=None)
def _case_reference(k, d, n, snis):
    m, x, mapping, tlp, bg = _case(k, d, n)
    return ref.get_expected_hessian_and_grad(m, np.full(k, 1e-6), x, mapping, bg, tlp, False, snis)


def _device_inputs(ctx, m, x, d):
    packed = ops().diag_pack(ctx, ctx.asarray(m.means), ctx.asarray(m.chol_cov))
    xd = ctx.asarray(x)
    ld, lp, _ = ops().diag_mixture_eval(ctx, packed, ctx.asarray(m.log_weights), xd, d, want_ld=True, want_lp=True)
    return packed, xd, ld, lp


def _assert_bound(h, g, rh, rg, what, rows=None):
    """|device - reference| <= BOUND * (largest |reference| entry of the component) + 1e-5 for H and g."""
    rows = range(rh.shape[0]) if rows is None else rows
    h, g, rh, rg = (np.asarray(a, np.float64)[list(rows)] for a in (h, g, rh, rg))
    assert h.shape == rh.shape and g.shape == rg.shape
    assert np.all(np.isfinite(rh)) and np.all(np.isfinite(rg)), what
    scale_h = np.abs(rh).max(axis=1, keepdims=True)
    scale_g = np.abs(rg).max(axis=1, keepdims=True)
    dev_h = (np.abs(h - rh) / scale_h).max() if np.all(np.isfinite(h)) else np.inf
    dev_g = (np.abs(g - rg) / scale_g).max() if np.all(np.isfinite(g)) else np.inf
    print(f"\n[more_diag] {what}: deviation H {dev_h:.3e}  g {dev_g:.3e}  (bound {BOUND:.1e})")
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(g)), what
    assert np.all(np.abs(h - rh) <= BOUND * scale_h + 1e-5), (what, dev_h)
    assert np.all(np.abs(g - rg) <= BOUND * scale_g + 1e-5), (what, dev_g)


# (k, d, n), N about 3 F with F = 2 d + 1: F = 3 below one 64-sample tile; a ragged second tile; a register-path dimension
# (F = 41); F + 1 = 128, 130, 132: exactly one 128-column panel, then the bias row and the right-hand side crossing into a
# second panel; the C5 dimension; the cap (17 panels).  The fp64 reference at F = 2 049, N = 6 200 takes about a second.
PARITY_SHAPES = [(1, 1, 40), (3, 3, 70), (2, 20, 130), (2, 63, 400), (2, 64, 400), (1, 65, 420), (1, 300, 1850),
                 (1, 1024, 6200)]


@pytest.mark.parametrize("k,d,n", PARITY_SHAPES)
@pytest.mark.parametrize("snis", [True, False])
def test_more_diag_matches_the_reference(ctx, k, d, n, snis):
    """Every seam of the route, both weightings, ridge 1e-6, well-posed regime (N about 3 F).  Bound: 1e-2 of the
    per-component magnitude (+ 1e-5), the project's MORE bound, unchanged.
    Measured on an MI355X (H / g, the larger of the two weightings): d = 1 5.6e-7 / 2.4e-7, d = 3 2.3e-5 / 7.6e-7,
    d = 20 1.9e-5 / 1.8e-6, d = 63 1.0e-5 / 3.2e-6, d = 64 9.4e-6 / 2.6e-6, d = 65 3.2e-6 / 1.6e-6, d = 300 1.1e-5 / 4.5e-6,
    d = 1024 1.6e-5 / 4.6e-4 (there the largest |g| entry is 0.058: 2.7e-5 absolute)."""
    m, x, mapping, tlp, bg = _case(k, d, n)
    packed, xd, ld, lp = _device_inputs(ctx, m, x, d)
    h, g = ops().more_diag(ctx, packed, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(np.full(k, 1e-6)), d,
                           self_normalized=snis)
    assert h.shape == (k, d) and g.shape == (k, d)
    rh, rg = _case_reference(k, d, n, snis)
    _assert_bound(h.numpy(), g.numpy(), rh, rg, f"k={k} d={d} n={n} snis={snis}")


def test_more_diag_own_samples_and_shifted_mapping(ctx, rng):
    """only_use_own_samples with data-base style mapping values (shifted by 5, map_offset brings the newest to K - 1): every
    component regresses on its own about 3 F samples with plain weights.  Measured: H 2.9e-6, g 1.7e-6."""
    k, d, n = 2, 64, 800
    m, x, mapping, tlp, bg = _inputs(rng, k, d, n)
    packed, xd, ld, lp = _device_inputs(ctx, m, x, d)
    mp = mapping + 5
    l2 = np.full(k, 1e-6)
    h, g = ops().more_diag(ctx, packed, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(l2), d,
                           mapping=ctx.asarray(mp, np.int32), map_offset=k - 1 - int(mp.max()), own_samples_only=True)
    rh, rg = ref.get_expected_hessian_and_grad(m, l2, x, mp, bg, tlp, True, True)
    _assert_bound(h.numpy(), g.numpy(), rh, rg, f"own samples k={k} d={d} n={n}")


def test_more_diag_gaussian_target_closed_form(ctx, rng):
    """K = 1, target N(m, diag s^2): the reward is exactly a diagonal quadratic, so whatever the weights the estimate is
    G_i = 1 / s_i^2 - 1 / sigma_i^2, g_i = (mu_i - m_i) / s_i^2 (test_more_diag_cpu.py derives it); ridge 1e-10, same bound.
    Measured: H 3.9e-6, g 2.2e-7."""
    k, d, n = 1, 64, 400
    model = random_diag_gmm(rng, k, d)
    mu, sigma = model.means[0], model.chol_cov[0]
    tm, ts = rng.normal(size=d) * 2.0, rng.random(d) + 0.5
    x, _ = model.sample_from_components_no_shuffle([n], philox.normals(9, 0, n, d))
    x = x.astype(np.float32).astype(np.float64)
    tlp = ogmm.DiagonalGMM.diagonal_gaussian_log_pdf(d, tm, ts, x)
    bg = model.component_log_densities(x)[0] + 0.5 * rng.normal(size=n)      # any weights
    packed, xd, ld, lp = _device_inputs(ctx, model, x, d)
    h, g = ops().more_diag(ctx, packed, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(np.full(k, 1e-10)), d)
    want_h = (1.0 / ts ** 2 - 1.0 / sigma ** 2)[None]
    want_g = ((mu - tm) / ts ** 2)[None]
    _assert_bound(h.numpy(), g.numpy(), want_h, want_g, f"closed form k={k} d={d} n={n}")


def test_more_diag_result_does_not_depend_on_the_group_size(ctx, rng, monkeypatch):
    """GMMVI_MORE_WS_GB (read per call) so small that every component is its own group gives bit-identical H, g."""
    k, d, n = 3, 64, 400
    m, x, mapping, tlp, bg = _inputs(rng, k, d, n)
    packed, xd, ld, lp = _device_inputs(ctx, m, x, d)
    args = (ctx, packed, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(np.full(k, 1e-6)), d)
    monkeypatch.delenv("GMMVI_MORE_WS_GB", raising=False)
    h0, g0 = (a.numpy() for a in ops().more_diag(*args))
    monkeypatch.setenv("GMMVI_MORE_WS_GB", "0.0001")                     # 107 KB: below one component's 524 KB Gram matrix
    h1, g1 = (a.numpy() for a in ops().more_diag(*args))
    assert np.all(np.isfinite(h0)) and np.all(np.isfinite(g0))
    np.testing.assert_array_equal(h0, h1)
    np.testing.assert_array_equal(g0, g1)


def test_more_diag_refuses_dimensions_above_the_cap(ctx):
    """D = 1025: ValueError from hip_ops; the C call returns GMMVI_ERR_ARG (-2) before any launch and gmmvi_last_error names
    the limit."""
    k, d, n = 1, 1025, 8
    packed = ops().diag_pack(ctx, ctx.zeros((k, d)), ctx.full((k, d), 1.0))
    xd = ctx.zeros((n, d))
    ld, v, l2 = ctx.zeros((k, n)), ctx.zeros((n,)), ctx.full((k,), 1e-6)
    with pytest.raises(ValueError, match="1024"):
        ops().more_diag(ctx, packed, xd, ld, v, v, v, l2, d)
    hh, gg = ctx.empty((k, d)), ctx.empty((k, d))
    rc = ctx.lib.gmmvi_more_diag(ctx.handle, k, d, packed.ptr, xd.ptr, n, ld.ptr, v.ptr, v.ptr, v.ptr, None, 0, 1, l2.ptr,
                                 hh.ptr, gg.ptr)
    assert rc == -2                                                      # GMMVI_ERR_ARG (include/gmmvi_hip.h)
    assert "1024" in ctx.lib.gmmvi_last_error(ctx.handle).decode()


def test_more_diag_component_without_samples_is_nan(ctx, rng):
    """own samples only, ridge 0, a component that drew nothing: its Gram matrix is zero, the first pivot fails (a flag, no
    fault) and both outputs of THAT component are NaN; the others stay within the bound.  The diagonal updaters reject a NaN
    row and leave the component untouched (test_hip_diag_mmd.py::test_diag_update_kl_failure, ::test_diag_update_iblr).
    Measured on the two components with samples: H 3.3e-5, g 4.7e-7."""
    k, d = 3, 5
    n_k = [40, 0, 45]
    m, x, mapping, tlp, bg = _inputs(rng, k, d, sum(n_k), n_k=n_k)
    packed, xd, ld, lp = _device_inputs(ctx, m, x, d)
    l2 = np.zeros(k)
    h, g = ops().more_diag(ctx, packed, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(l2), d,
                           mapping=ctx.asarray(mapping, np.int32), map_offset=k - 1 - int(mapping.max()),
                           own_samples_only=True)
    h, g = h.numpy(), g.numpy()
    assert np.all(np.isnan(h[1])) and np.all(np.isnan(g[1]))
    rh, rg = ref.get_expected_hessian_and_grad(m, l2, x, mapping, bg, tlp, True, True)
    assert np.all(np.isnan(rh[1]))
    _assert_bound(h, g, rh, rg, "no own samples: the other components", rows=[0, 2])


# ---- end to end: a target that implements log_density only ---------------------------------------------------------------
E2E_D, E2E_ITERS, E2E_SAMPLES = 6, 30, 60
E2E_MEAN = np.array([1.5, -1.0, 0.5, 2.0, -2.0, 0.25])
E2E_STD = np.array([0.6, 1.4, 0.9, 0.5, 1.2, 0.8])


def _user_targets():
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF

    class BlackBoxGaussian(LNPDF):
        """A user target as the issue describes it: log_density (NumPy, on the host) and get_num_dimensions, nothing else."""

        def get_num_dimensions(self):
            return E2E_D

        def log_density(self, x):
            xh = np.asarray(x.numpy() if hasattr(x, "numpy") else x, np.float64)
            return (-0.5 * np.sum(np.square((xh - E2E_MEAN) / E2E_STD), axis=1) - np.sum(np.log(E2E_STD))
                    - 0.5 * E2E_D * np.log(2 * np.pi)).astype(np.float32)

    class GaussianWithGradient(BlackBoxGaussian):
        def log_density_and_grad(self, x):
            xh = np.asarray(x.numpy() if hasattr(x, "numpy") else x, np.float64)
            return self.log_density(x), (-(xh - E2E_MEAN) / np.square(E2E_STD)).astype(np.float32)

    return BlackBoxGaussian, GaussianWithGradient


def _build(target, estimator):
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    cfg = samtron_config(E2E_SAMPLES, reuse_ratio=0.0, estimator=estimator, diag=True)
    model = DiagonalGMM(np.ones(1), np.zeros((1, E2E_D), np.float32), np.ones((1, E2E_D), np.float32))
    model.seed = 3
    wrapper = GmmWrapper(model, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
    return GMMVI.build_from_config(cfg, target, wrapper)


def _kl_to_target(g):
    """Closed-form KL(q || p) of the one-component diagonal model against N(E2E_MEAN, diag E2E_STD^2)."""
    mu = g.model.means.numpy()[0].astype(np.float64)
    sg = g.model.chol_cov.numpy()[0].astype(np.float64)
    return 0.5 * np.sum(np.square(sg / E2E_STD) + np.square((mu - E2E_MEAN) / E2E_STD) - 1.0
                        + 2.0 * np.log(E2E_STD / sg))


def _fixed_point_deviation(g):
    """(means, factors): largest distance from the fixed point mu = E2E_MEAN, sigma = E2E_STD relative to the parameter scale,
    as test_hip_long_horizon.py measures its final parameters."""
    mu = g.model.means.numpy()[0].astype(np.float64)
    sg = g.model.chol_cov.numpy()[0].astype(np.float64)
    return (np.abs(mu - E2E_MEAN).max() / np.abs(E2E_MEAN).max(), np.abs(sg - E2E_STD).max() / np.abs(E2E_STD).max())


def test_gradient_free_target_trains_with_diagonal_more(monkeypatch):
    """30 iterations (KL updater, 60 samples per component, reuse ratio 0) on a D = 6 Gaussian target that implements
    log_density only, one diagonal component: build_from_config yields a DiagonalMoreNgEstimator, log_density_and_grad is never
    called, and the closed-form KL(q || p) decreases.  The same black-box class under Stein still raises NotImplementedError.
    Final state.  A Stein run of the same configuration on a subclass that adds the analytic gradient was to give the scale
    (KL_MORE <= 10 KL_Stein); measured on an MI355X: KL start 14.35, KL_MORE 4.8e-14, KL_Stein 3.0e-14.  Both are at the
    rounding level of the fp32 parameters (a relative error of 1e-7 in mu and sigma is a KL of about 1e-14), so their ratio
    says nothing; the run is instead held to the closed-form fixed point mu = m, sigma = s with the tolerances of
    test_hip_long_horizon.py: means and factors within 2 % of the parameter scale.  The Stein run stays, held to the same
    fixed point, and both KL values are printed."""
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import DiagonalMoreNgEstimator, SteinNgEstimator
    BlackBoxGaussian, GaussianWithGradient = _user_targets()

    with pytest.raises(NotImplementedError):
        _build(BlackBoxGaussian(), "Stein").train_iter()

    calls = []
    original = LNPDF.log_density_and_grad

    def counting(self, x):
        calls.append(type(self).__name__)
        return original(self, x)

    monkeypatch.setattr(LNPDF, "log_density_and_grad", counting)
    g = _build(BlackBoxGaussian(), "MORE")
    assert type(g.ng_estimator) is DiagonalMoreNgEstimator and g.ng_estimator.uses_target_gradients is False
    assert not g._fast_path.eligible()
    kl_start = _kl_to_target(g)
    for _ in range(E2E_ITERS):
        g.train_iter()
    kl_more = _kl_to_target(g)
    assert calls == []
    assert int(g.sample_db.num_samples_written) == E2E_ITERS * E2E_SAMPLES
    monkeypatch.undo()

    s = _build(GaussianWithGradient(), "Stein")
    assert type(s.ng_estimator) is SteinNgEstimator and s.ng_estimator.uses_target_gradients is True
    for _ in range(E2E_ITERS):
        s.train_iter()
    kl_stein = _kl_to_target(s)
    dev_more, dev_stein = _fixed_point_deviation(g), _fixed_point_deviation(s)
    print(f"\n[more_diag] end to end, {E2E_ITERS} iterations: KL start {kl_start:.4e}  KL_MORE {kl_more:.4e}  "
          f"KL_Stein {kl_stein:.4e};  MORE means {dev_more[0]:.2e} factors {dev_more[1]:.2e}, Stein means "
          f"{dev_stein[0]:.2e} factors {dev_stein[1]:.2e}  (bound 2.0e-02 of the parameter scale)")
    assert np.isfinite(kl_more) and np.isfinite(kl_stein)
    assert kl_more < kl_start
    assert max(dev_more) <= 2e-2, dev_more
    assert max(dev_stein) <= 2e-2, dev_stein
