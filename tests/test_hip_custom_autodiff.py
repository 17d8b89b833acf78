"""GPU tests of differentiated user-defined device targets (csrc/custom_target_autodiff.inc, DeviceAutodiffLNPDF): the
gradient of the dual-number passes and both value calls against fp64 at the seams of the pass width, of the 64-sample tile and
of the staged route's cap; the cap of the gradient call; the module cache with the mode in its key; and the target in the
modular and the single-call iteration and under a gradient-free estimator.

Kernel bound: the rule of tests/test_hip_custom_target.py, unchanged (its _bound): the device's largest error against the fp64
NumPy restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|; for lp and the gradient of the gradient call and for lp of the value call.  Every case prints its
ratios before it asserts."""

import numpy as np
import pytest

import custom_autodiff_cases as cases
import test_hip_custom_target as hand
from gmmvi_amd import _lib
from helpers import samtron_config

pytestmark = pytest.mark.gpu

ERR_ARG = -2
W = _lib.CUSTOM_AUTODIFF_TANGENTS


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name):
    from gmmvi_amd import hip_ops
    if name not in _handles:
        _handles[name] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], autodiff=True)
    return _handles[name]


_refs = {}


def _reference(name, d, n):
    key = (name, d, n)
    if key not in _refs:
        tgt, x = cases.build_case(name, d, n)
        lp64, g64 = tgt.log_density_and_grad(x.astype(np.float64))
        lp32, g32 = cases.fp32_twin(tgt).log_density_and_grad(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _refs[key] = (tgt, x, lp64, g64, lp32, g32)
    return _refs[key]


@pytest.mark.parametrize("name,d,n,routes", cases.kernel_cases(W), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_matches_fp64_reference(ctx, name, d, n, routes):
    tgt, x, lp64, g64, lp32, g32 = _reference(name, d, n)
    handle = _handle(ctx, name)
    params = tgt.params()
    for route in routes:
        rc, lp, g = hand._launch(ctx, handle, params, x, True, route)          # 64 canary rows behind both outputs
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
        e_lp, b_lp, r_lp = hand._bound(lp, lp64, lp32)
        e_g, b_g, r_g = hand._bound(g, g64, g32)
        print(f"\n[custom_autodiff] {name} D={d} N={n} route={route}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, "
              f"ratio to fp32 NumPy {r_lp:.2f}), gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})")
        assert e_lp <= b_lp, f"route {route}: lp error {e_lp:.3e} > {b_lp:.3e}"
        assert e_g <= b_g, f"route {route}: gradient error {e_g:.3e} > {b_g:.3e}"
        rc, lp_v, g_v = hand._launch(ctx, handle, params, x, False, route)
        assert rc == 0 and g_v is None
        e_v, b_v, r_v = hand._bound(lp_v, lp64, lp32)
        print(f"[custom_autodiff] {name} D={d} N={n} route={route} values only: lp error {e_v:.3e} (bound {b_v:.3e}, "
              f"{e_v / b_v:.3f} of it, ratio {r_v:.2f})")
        assert e_v <= b_v, f"route {route}, values only: lp error {e_v:.3e} > {b_v:.3e}"


def test_gradient_call_is_capped_and_the_value_call_is_not(ctx):
    lib = ctx.lib
    d, n = _lib.CUSTOM_AUTODIFF_MAX_DIM + 1, 8
    tgt, x = cases.build_case("quartic", d, n)
    handle = _handle(ctx, "quartic")
    rc, _, _ = hand._launch(ctx, handle, tgt.params(), x, True, 0)
    assert rc == ERR_ARG
    message = lib.gmmvi_last_error(ctx.handle).decode()
    assert "512" in message and "513" in message
    # nothing was launched: the outputs of a refused call are untouched
    xd, pd = ctx.asarray(x), ctx.asarray(tgt.params())
    lp, grad = ctx.full((n,), hand.SENTINEL), ctx.full((n, d), hand.SENTINEL)
    assert lib.gmmvi_target_custom(ctx.handle, handle.handle, d, pd.ptr, xd.ptr, n, lp.ptr, grad.ptr, 2) == ERR_ARG
    ctx.check(lib.gmmvi_sync(ctx.handle))
    assert np.all(lp.numpy() == hand.SENTINEL) and np.all(grad.numpy() == hand.SENTINEL)
    # the same call without a gradient pointer runs
    rc, lp_v, _ = hand._launch(ctx, handle, tgt.params(), x, False, 0)
    assert rc == 0
    lp64 = tgt.log_density(x.astype(np.float64))
    e, b, _ = hand._bound(lp_v, lp64, cases.fp32_twin(tgt).log_density(x))
    assert e <= b
    # a hand-written gradient has no such cap, and the context works afterwards
    rc, _, g_hand = hand._launch(ctx, hand._handle(ctx, "quartic"), tgt.params(), x, True, 0)
    assert rc == 0 and np.all(np.isfinite(g_hand))
    t, xs, lp64, g64, lp32, g32 = _reference("rosenbrock", 2, 65)
    rc, lp_ok, g_ok = hand._launch(ctx, _handle(ctx, "rosenbrock"), t.params(), xs, True, 0)
    assert rc == 0
    assert hand._bound(lp_ok, lp64, lp32)[0] <= hand._bound(lp_ok, lp64, lp32)[1]
    assert hand._bound(g_ok, g64, g32)[0] <= hand._bound(g_ok, g64, g32)[1]


def test_module_cache_keeps_the_mode_in_its_key(ctx):
    from gmmvi_amd import hip_ops
    h1 = _handle(ctx, "quartic")
    h2 = hip_ops.custom_target_compile(ctx, cases.QUARTIC_SRC, autodiff=True)
    assert h1.ptr == h2.ptr
    other = hip_ops.custom_target_compile(ctx, cases.QUARTIC_SRC + "\n// another text\n", autodiff=True)
    assert other.ptr != h1.ptr
    # the hand-written-gradient mode keeps its own handles: the key holds the mode
    assert hand._handle(ctx, "quartic").ptr not in (h1.ptr, other.ptr)


def test_same_text_compiled_both_ways_gives_two_handles(ctx):
    """A text that defines both functions is valid in both modes: the handles differ, the hand-written one returns its own
    (deliberately different) gradient, the differentiated one the derivative of the density."""
    from gmmvi_amd import hip_ops
    text = ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
            "    T s = 0.f; for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i]; return s; }\n"
            "#ifndef GMMVI_CUSTOM_AUTODIFF_TANGENTS\n"
            "__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {\n"
            "    if (grad) for (int i = 0; i < D; ++i) grad[i] = 7.f;\n"
            "    return gmmvi_user_density<float, const float*>(x, D, params); }\n"
            "#endif\n")
    ad = hip_ops.custom_target_compile(ctx, text, autodiff=True)
    hw = hip_ops.custom_target_compile(ctx, text, autodiff=False)
    assert ad.ptr != hw.ptr
    x = ctx.asarray(np.random.default_rng(1).normal(size=(65, 3)).astype(np.float32))
    lp_a, g_a = hip_ops.target_custom(ctx, ad, None, x, True)
    lp_h, g_h = hip_ops.target_custom(ctx, hw, None, x, True)
    np.testing.assert_array_equal(lp_a.numpy(), lp_h.numpy())
    np.testing.assert_array_equal(g_a.numpy(), -x.numpy())
    np.testing.assert_array_equal(g_h.numpy(), np.full((65, 3), 7.0, np.float32))


# ---- the iteration -----------------------------------------------------------------------------------------------------
def test_modular_path_rosenbrock_against_the_oracle(ctx, monkeypatch):
    """The setup of test_modular_path_rosenbrock_against_the_oracle (tests/test_hip_custom_target.py) with the density alone:
    SAMTRUX defaults, one initial component, 60 samples, five iterations on the modular path against the fp64 oracle, same
    Philox stream.  Five device calls, no host log_density*, no sample download."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.configs import get_default_algorithm_config, update_config
    from gmmvi_amd.device import DeviceArray
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceAutodiffLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    s, seed = 60, 11
    cfg = update_config(get_default_algorithm_config("SAMTRUX"), {
        "model_initialization": {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0., "prior_scale": 1.,
                                 "initial_cov": 1.},
        "use_sample_database": True, "max_database_size": int(1e6), "temperature": 1., "seed": 0,
        "sample_selector_config": {"desired_samples_per_component": s, "ratio_reused_samples_to_desired": 0.0}})
    ref = cases.Rosenbrock()
    o = hand._oracle(ref, 2, 1, seed, cfg, 1.0, 1.0)
    target = DeviceAutodiffLNPDF(cases.ROSENBROCK_SRC, 2, params=ref.params())
    g = hand._device(target, o, seed, cfg, 1.0)

    counts = {"device": 0, "host": 0, "downloads": 0}
    real = hip_ops.target_custom

    def counting_kernel(c, handle, params, x, want_grad=True, route=0):
        assert isinstance(x, DeviceArray)
        counts["device"] += 1
        return real(c, handle, params, x, want_grad, route)

    def host_call(self, x):
        counts["host"] += 1
        raise AssertionError("a host log_density* was called")

    real_numpy = DeviceArray.numpy

    def counting_numpy(self):
        if self.shape == (s, 2):
            counts["downloads"] += 1
        return real_numpy(self)

    monkeypatch.setattr(hip_ops, "target_custom", counting_kernel)
    monkeypatch.setattr(LNPDF, "log_density", host_call)
    monkeypatch.setattr(LNPDF, "log_density_and_grad", host_call)
    monkeypatch.setattr(DeviceArray, "numpy", counting_numpy)
    hand._run_pair(monkeypatch, o, g, 5, fused=False)
    assert counts == {"device": 5, "host": 0, "downloads": 0}, counts


def _autodiff_lnpdf(ref):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceAutodiffLNPDF
    return DeviceAutodiffLNPDF(cases.QUARTIC_SRC, ref.get_num_dimensions(), params=ref.params())


def test_single_call_iteration(ctx, monkeypatch):
    """The quartic target with c = 0 (a Gaussian) at D = W + 1 (two passes, the second a partial one), K = 3, 50 samples per
    component, 4 iterations: eligible for the single-call iteration, which is bit-identical to the modular path with the
    estimate materialised, follows the fp64 oracle within run_pair's criterion, and tracks the run of the hand-written-gradient
    DeviceLNPDF of the same target within the tolerances of test_single_call_iteration (tests/test_hip_custom_target.py)."""
    d, k, s, seed, iters = W + 1, 3, 50, 23, 4
    cfg = samtron_config(s)
    ref, o, device = hand._gauss_pair(d, k, s, seed, cfg, _autodiff_lnpdf)
    fast, slow = device(), device()
    slow._fast_path.enabled = False
    assert fast._fast_path.eligible() and not slow._fast_path.eligible()
    spec = fast.sample_selector.target_distribution._fast_path_target()
    assert spec.kind == 5 and spec.custom == fast.sample_selector.target_distribution._handle.ptr
    fast._fast_path.explicit_estimate = True
    for it in range(iters):
        fast.train_iter()
        slow.train_iter()
        for name in ("means", "chol_cov", "log_weights", "stepsizes", "last_log_etas", "l2_regularizers", "num_received_updates"):
            np.testing.assert_array_equal(getattr(fast.model, name).numpy(), getattr(slow.model, name).numpy(),
                                          err_msg=f"iteration {it}: {name}")
        np.testing.assert_array_equal(fast.model.reward_slot(0).numpy(), slow.model.reward_slot(0).numpy())
    np.testing.assert_array_equal(fast.sample_db.samples.numpy(), slow.sample_db.samples.numpy())
    np.testing.assert_array_equal(fast.sample_db.target_grads.numpy(), slow.sample_db.target_grads.numpy())
    np.testing.assert_array_equal(fast.sample_db.target_lnpdfs.numpy(), slow.sample_db.target_lnpdfs.numpy())

    # against the fp64 oracle on the fp64 restatement (run_pair, single-call path) ...
    user = device()
    hand._run_pair(monkeypatch, o, user, iters, fused=True)
    # ... and against the hand-written gradient of the same target, iteration by iteration (both from an untouched oracle's
    # initial mixture: run_pair has advanced `o`)
    fresh = hand._oracle(ref, d, k, seed, cfg, 5.0, 10.0)
    auto = hand._device(_autodiff_lnpdf(ref), fresh, seed, cfg, 10.0)
    written = hand._device(hand._device_lnpdf(ref), fresh, seed, cfg, 10.0)
    assert auto._fast_path.eligible() and written._fast_path.eligible()
    for it in range(iters):
        auto.train_iter()
        written.train_iter()
        tol = 5e-4 if it < 2 else 2e-3 * (1 + it)
        a, b = auto.model, written.model
        dev = {"means": np.abs(a.means.numpy() - b.means.numpy()).max() / max(1.0, np.abs(b.means.numpy()).max()),
               "chols": np.abs(a.chol_cov.numpy() - b.chol_cov.numpy()).max() / np.abs(b.chol_cov.numpy()).max(),
               "logw": np.abs(np.exp(a.log_weights.numpy()) - np.exp(b.log_weights.numpy())).max(),
               "stepsizes": np.abs(a.stepsizes.numpy() - b.stepsizes.numpy()).max()}
        print(f"[custom_autodiff] iteration {it}: deviation from the hand-written gradient's run {dev} (tolerance {tol:.1e})")
        for key, v in dev.items():
            assert v <= tol, f"iteration {it}: {key} deviates from the hand-written gradient's run by {v:.3e} (> {tol:.1e})"


def test_gradient_free_estimator_evaluates_values_only(ctx, monkeypatch):
    """Under MoreNgEstimator the differentiated target is asked for values alone: no call pays for the dual passes."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import MoreNgEstimator
    ref = hand._gaussian(3, 7)
    target = _autodiff_lnpdf(ref)
    wanted = []
    real = hip_ops.target_custom

    def recording(c, handle, params, x, want_grad=True, route=0):
        wanted.append(bool(want_grad))
        return real(c, handle, params, x, want_grad, route)

    monkeypatch.setattr(hip_ops, "target_custom", recording)
    g = hand._build_one_component(target, 3, "MORE", False)
    assert type(g.ng_estimator) is MoreNgEstimator and g.ng_estimator.uses_target_gradients is False
    for _ in range(3):
        g.train_iter()
    assert len(wanted) == 3 and not any(wanted), wanted
    assert int(g.sample_db.num_samples_written) == 3 * hand.E2E_SAMPLES
    tlp = g.sample_db.target_lnpdfs.numpy()
    np.testing.assert_allclose(tlp, ref.log_density(g.sample_db.samples.numpy().astype(np.float64)), rtol=1e-4,
                               atol=1e-4 * np.abs(tlp).max())
