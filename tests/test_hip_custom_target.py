"""GPU tests of user-defined device targets (csrc/custom_target.hip, DeviceLNPDF): the wrapper kernels against fp64 on the
tile seams and on both sides of the staged route's cap, the argument and compile errors, and the target in the modular, the
single-call and the sharded iteration and under the gradient-free estimators.

Kernel bound (the project's rule for targets, tests/test_hip_bnn_mlp.py): the device's largest error against the fp64 NumPy
restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs, plus a floor of
4 * eps32 * max|reference| so that a case the fp32 restatement gets exact does not demand exactness; for lp and for the
gradient.  Every case prints its ratios before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_target_cases as cases
from helpers import samtron_config
from oracle import train as otrain

pytestmark = pytest.mark.gpu

E32_FACTOR = 16.0
EPS32 = float(np.finfo(np.float32).eps)
SENTINEL = np.float32(-12345.678)
CANARY_ROWS = 64
ERR_ARG = -2


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name):
    from gmmvi_amd import hip_ops
    if name not in _handles:
        _handles[name] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name])
    return _handles[name]


def _launch(ctx, handle, params, x, want_grad, route):
    """gmmvi_target_custom on outputs with CANARY_ROWS extra rows of SENTINEL behind them -> (rc, lp, grad | None); the extra
    rows are checked here: bit-unchanged."""
    n, d = x.shape
    xd = ctx.asarray(x)
    pd = ctx.asarray(params)
    lp = ctx.full((n + CANARY_ROWS,), SENTINEL)
    grad = ctx.full((n + CANARY_ROWS, d), SENTINEL) if want_grad else None
    rc = ctx.lib.gmmvi_target_custom(ctx.handle, handle.handle, d, pd.ptr, xd.ptr, n, lp.ptr,
                                     None if grad is None else grad.ptr, route)
    if rc != 0:
        return rc, None, None
    lp_h = lp.numpy()
    assert np.all(lp_h[n:].view(np.uint32) == np.array(SENTINEL).view(np.uint32)), "lp written past N"
    g_h = None
    if want_grad:
        g_h = grad.numpy()
        assert np.all(g_h[n:].view(np.uint32) == np.array(SENTINEL).view(np.uint32)), "gradient written past N"
        g_h = g_h[:n]
    return rc, lp_h[:n], g_h


def _bound(dev, ref64, ref32):
    """-> (device error, bound, ratio to the fp32 restatement's error)."""
    e_dev = float(np.abs(dev.astype(np.float64) - ref64).max())
    e_32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    floor = 4.0 * EPS32 * float(np.abs(ref64).max())
    return e_dev, E32_FACTOR * e_32 + floor, e_dev / max(e_32, 1e-300)


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


@pytest.mark.parametrize("name,d,n,routes", cases.KERNEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_matches_fp64_reference(ctx, name, d, n, routes):
    tgt, x, lp64, g64, lp32, g32 = _reference(name, d, n)
    handle = _handle(ctx, name)
    params = tgt.params()
    for route in routes:
        rc, lp, g = _launch(ctx, handle, params, x, True, route)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
        e_lp, b_lp, r_lp = _bound(lp, lp64, lp32)
        e_g, b_g, r_g = _bound(g, g64, g32)
        print(f"\n[custom_target] {name} D={d} N={n} route={route}: lp error {e_lp:.3e} (bound {b_lp:.3e}, ratio to fp32 NumPy "
              f"{r_lp:.2f}), gradient error {e_g:.3e} (bound {b_g:.3e}, ratio {r_g:.2f})")
        assert e_lp <= b_lp, f"route {route}: lp error {e_lp:.3e} > {b_lp:.3e}"
        assert e_g <= b_g, f"route {route}: gradient error {e_g:.3e} > {b_g:.3e}"
        # values only: the same rule
        rc, lp_v, g_v = _launch(ctx, handle, params, x, False, route)
        assert rc == 0 and g_v is None
        e_v, b_v, r_v = _bound(lp_v, lp64, lp32)
        print(f"[custom_target] {name} D={d} N={n} route={route} values only: lp error {e_v:.3e} (bound {b_v:.3e}, ratio {r_v:.2f})")
        assert e_v <= b_v, f"route {route}, values only: lp error {e_v:.3e} > {b_v:.3e}"


def test_python_wrapper_and_module_cache(ctx):
    """hip_ops.target_custom / DeviceLNPDF give what the C call gives; the same source compiles to the same handle."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    tgt, x, lp64, g64, lp32, g32 = _reference("quartic", 3, 70)
    h1 = _handle(ctx, "quartic")
    h2 = hip_ops.custom_target_compile(ctx, cases.QUARTIC_SRC)
    assert h1.ptr == h2.ptr
    other = hip_ops.custom_target_compile(ctx, cases.QUARTIC_SRC + "\n// another text\n")
    assert other.ptr != h1.ptr
    _, lp_c, g_c = _launch(ctx, h1, tgt.params(), x, True, 0)
    t = DeviceLNPDF(cases.QUARTIC_SRC, 3, params=tgt.params())
    assert t.get_num_dimensions() == 3 and t.use_log_density_and_grad
    lp, g = t.log_density_and_grad(x)
    np.testing.assert_array_equal(lp.numpy(), lp_c)
    np.testing.assert_array_equal(g.numpy(), g_c)
    e, b, _ = _bound(t.log_density(ctx.asarray(x)).numpy(), lp64, lp32)
    assert e <= b
    spec = t._fast_path_target()
    assert spec.kind == 5 and spec.custom == t._handle.ptr and spec.custom_params == t._params_dev.ptr
    with pytest.raises(ValueError):
        t.log_density(np.zeros((4, 5), np.float32))
    # a target without parameters gets a null pointer
    const = DeviceLNPDF("__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {\n"
                        "    if (grad) for (int i = 0; i < D; ++i) grad[i] = params ? 1.f : -x[i];\n"
                        "    float s = 0.f; for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i]; return s; }\n", 3)
    lp, g = const.log_density_and_grad(x)
    np.testing.assert_array_equal(g.numpy(), -x)
    np.testing.assert_allclose(lp.numpy(), -0.5 * np.sum(x.astype(np.float64) ** 2, axis=1), rtol=1e-6)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_argument_and_compile_errors_leave_the_context_usable(ctx):
    from gmmvi_amd import _lib
    from gmmvi_amd.optimization.fused import SamtronPlan
    from gmmvi_amd.sharded import ShardedPlan
    lib = ctx.lib

    def last():
        return lib.gmmvi_last_error(ctx.handle).decode()

    # kind 5 with a null handle, both plans
    p = ShardedPlan()
    p.target.kind = 5
    assert lib.gmmvi_train_iter_sharded_phase(ctx.handle, C.byref(p), 1) == ERR_ARG
    assert "target_kind 5" in last()
    q = SamtronPlan()
    q.target.kind = 5
    assert lib.gmmvi_train_iter_samtron(ctx.handle, C.byref(q)) == ERR_ARG
    assert "target_kind 5" in last()
    # route 1 above the cap; bad shapes and pointers
    handle = _handle(ctx, "quartic")
    tgt, x = cases.build_case("quartic", 121, 8)
    rc, _, _ = _launch(ctx, handle, tgt.params(), x, True, 1)
    assert rc == ERR_ARG and "121" in last()
    xd, pd, lp = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.empty((8,))
    for d, n, xp, lpp, route in ((0, 8, xd.ptr, lp.ptr, 0), (121, 0, xd.ptr, lp.ptr, 0), (121, 8, None, lp.ptr, 0),
                                 (121, 8, xd.ptr, None, 0), (121, 8, xd.ptr, lp.ptr, 3), (_lib.MAX_DIM_DIAG + 1, 8, xd.ptr, lp.ptr, 2)):
        assert lib.gmmvi_target_custom(ctx.handle, handle.handle, d, pd.ptr, xp, n, lpp, None, route) == ERR_ARG
    assert lib.gmmvi_target_custom(ctx.handle, None, 121, pd.ptr, xd.ptr, 8, lp.ptr, None, 0) == ERR_ARG
    # a compile error through the context: the compiler log is the context's last error
    h = C.c_void_p()
    bad = cases.ROSENBROCK_SRC.replace("const float u = a - x[0];", "const float u = a - ;")
    assert lib.gmmvi_custom_target_compile(ctx.handle, bad.encode(), C.byref(h)) == ERR_ARG
    assert not h.value and "error" in last() and "gmmvi_user_target.hip:" in last()
    assert lib.gmmvi_custom_target_compile(ctx.handle, b"__device__ float f(float x) { return x; }", C.byref(h)) == ERR_ARG
    assert "gmmvi_user_target" in last()
    # the context works afterwards
    t, xs, lp64, g64, lp32, g32 = _reference("rosenbrock", 2, 65)
    rc, lp_ok, _ = _launch(ctx, _handle(ctx, "rosenbrock"), t.params(), xs, True, 0)
    assert rc == 0
    e, b, _ = _bound(lp_ok, lp64, lp32)
    assert e <= b


# ---- the iteration -----------------------------------------------------------------------------------------------------
def _oracle(target, d, k, seed, cfg, prior_scale, initial_cov):
    model = otrain.construct_initial_mixture(d, k, 0.0, prior_scale, initial_cov, np.random.default_rng(seed + 1))
    adaptive = cfg["num_component_adapter_type"] == "adaptive"
    return otrain.OracleGMMVI(
        target, model, temperature=cfg["temperature"], seed=seed,
        desired_samples_per_component=cfg["sample_selector_config"]["desired_samples_per_component"],
        ratio_reused_samples_to_desired=cfg["sample_selector_config"]["ratio_reused_samples_to_desired"],
        ng_estimator=cfg["ng_estimator_type"], only_use_own_samples=cfg["ng_estimator_config"]["only_use_own_samples"],
        use_self_normalized_importance_weights=cfg["ng_estimator_config"]["use_self_normalized_importance_weights"],
        updater=cfg["ng_based_updater_type"], component_stepsize_config=cfg["component_stepsize_adapter_config"],
        weight_updater=cfg["weight_updater_type"],
        weight_stepsize="fixed" if cfg["weight_stepsize_adapter_type"] == "fixed" else "improvement_based",
        weight_stepsize_config=cfg["weight_stepsize_adapter_config"],
        adaptive=(dict(cfg["num_component_adapter_config"], prior_mean=0.0, initial_cov=initial_cov) if adaptive else None),
        max_reward_history_length=400, sample_selector=cfg["sample_selector_type"],
        max_database_size=cfg["max_database_size"], host_rng=np.random.default_rng(seed))


def _device(target, o, seed, cfg, initial_cov):
    """Device GMMVI on ``target`` with the oracle's initial mixture and seed."""
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    om = o.model.model
    m = FullCovGMM(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
    m.seed = seed
    wrapper = GmmWrapper(m, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
    c = dict(cfg)
    c["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=initial_cov)
    g = GMMVI.build_from_config(c, target, wrapper)
    if cfg["num_component_adapter_type"] == "adaptive":
        g.num_component_adapter.rng = np.random.default_rng(seed)
    return g


def _run_pair(monkeypatch, o, g, iters, fused):
    """run_pair of tests/test_hip_train_iter.py (its per-iteration criterion, unchanged) on a pair built here."""
    import test_hip_train_iter as tti
    monkeypatch.setattr(tti, "make_oracle", lambda *a, **kw: o)
    monkeypatch.setattr(tti, "make_device", lambda *a, **kw: g)
    return tti.run_pair(None, None, None, None, seed=None, iters=iters, cfg=None, fused=fused)


def test_modular_path_rosenbrock_against_the_oracle(ctx, monkeypatch):
    """DeviceLNPDF Rosenbrock under the SAMTRUX defaults of upstream's example 4 (one initial component, prior scale 1, initial
    covariance 1), 60 samples per component, reuse ratio 0, five iterations on the modular path against the fp64 oracle on the
    fp64 NumPy Rosenbrock, same Philox stream.  No host log_density* runs, and no sample or gradient array is downloaded."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.configs import get_default_algorithm_config, update_config
    from gmmvi_amd.device import DeviceArray
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    s, seed = 60, 11
    cfg = update_config(get_default_algorithm_config("SAMTRUX"), {
        "model_initialization": {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0., "prior_scale": 1.,
                                 "initial_cov": 1.},
        "use_sample_database": True, "max_database_size": int(1e6), "temperature": 1., "seed": 0,
        "sample_selector_config": {"desired_samples_per_component": s, "ratio_reused_samples_to_desired": 0.0}})
    ref = cases.Rosenbrock()
    o = _oracle(ref, 2, 1, seed, cfg, 1.0, 1.0)
    target = DeviceLNPDF(cases.ROSENBROCK_SRC, 2, params=ref.params())
    g = _device(target, o, seed, cfg, 1.0)

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
    _run_pair(monkeypatch, o, g, 5, fused=False)
    assert counts == {"device": 5, "host": 0, "downloads": 0}, counts


def _gaussian(d, seed):
    """The quartic target with c = 0: log N(x; m, P^-1) up to its constant."""
    return cases.Quartic.random(d, 0.0, seed)


def _gauss_pair(d, k, s, seed, cfg, target_of):
    ref = _gaussian(d, seed)
    o = _oracle(ref, d, k, seed, cfg, 5.0, 10.0)
    return ref, o, (lambda: _device(target_of(ref), o, seed, cfg, 10.0))


def _device_lnpdf(ref):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    return DeviceLNPDF(cases.QUARTIC_SRC, ref.get_num_dimensions(), params=ref.params())


def test_single_call_iteration(ctx, monkeypatch):
    """D = 8, K = 3, 50 samples per component: the target is eligible for the single-call iteration, which is bit-identical to
    the modular path with the estimate materialised, follows the fp64 oracle within run_pair's criterion, and tracks the run on
    the built-in GMM_LNPDF of the same Gaussian within that criterion's tolerances."""
    from gmmvi_amd.experiments.target_distributions.gmm import GMM_LNPDF
    d, k, s, seed, iters = 8, 3, 50, 23, 4
    cfg = samtron_config(s)
    ref, o, device = _gauss_pair(d, k, s, seed, cfg, _device_lnpdf)
    fast, slow = device(), device()
    slow._fast_path.enabled = False
    assert fast._fast_path.eligible() and not slow._fast_path.eligible()
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
    _run_pair(monkeypatch, o, user, iters, fused=True)
    # ... and against the built-in mixture target of the same Gaussian, iteration by iteration
    cov = np.linalg.inv(ref.P)
    # (both from an untouched oracle's initial mixture: run_pair has advanced `o`)
    fresh = _oracle(ref, d, k, seed, cfg, 5.0, 10.0)
    user = _device(_device_lnpdf(ref), fresh, seed, cfg, 10.0)
    builtin = _device(GMM_LNPDF(np.ones(1), ref.m[None], cov[None]), fresh, seed, cfg, 10.0)
    assert user._fast_path.eligible() and builtin._fast_path.eligible()
    for it in range(iters):
        user.train_iter()
        builtin.train_iter()
        tol = 5e-4 if it < 2 else 2e-3 * (1 + it)
        a, b = user.model, builtin.model
        dev = {"means": np.abs(a.means.numpy() - b.means.numpy()).max() / max(1.0, np.abs(b.means.numpy()).max()),
               "chols": np.abs(a.chol_cov.numpy() - b.chol_cov.numpy()).max() / np.abs(b.chol_cov.numpy()).max(),
               "logw": np.abs(np.exp(a.log_weights.numpy()) - np.exp(b.log_weights.numpy())).max(),
               "stepsizes": np.abs(a.stepsizes.numpy() - b.stepsizes.numpy()).max()}
        for key, v in dev.items():
            assert v <= tol, f"iteration {it}: {key} deviates from the built-in target's run by {v:.3e} (> {tol:.1e})"


def test_blocked_path_dimension_runs_modular(ctx):
    """D = 64 is a blocked-path dimension: not eligible for the single-call iteration, the modular path runs it."""
    d, k, s, seed = 64, 2, 80, 29
    cfg = samtron_config(s)
    ref, o, device = _gauss_pair(d, k, s, seed, cfg, _device_lnpdf)
    g = device()
    assert hasattr(g.sample_selector.target_distribution, "_fast_path_target")
    assert not g._fast_path.eligible()
    for _ in range(2):
        g.train_iter()
    assert int(g.sample_db.num_samples_written) == 2 * k * s
    assert np.all(np.isfinite(g.model.means.numpy())) and np.all(np.isfinite(g.model.chol_cov.numpy()))
    tlp = g.sample_db.target_lnpdfs.numpy()
    np.testing.assert_allclose(tlp, ref.log_density(g.sample_db.samples.numpy().astype(np.float64)), rtol=1e-4,
                               atol=1e-4 * np.abs(tlp).max())


@pytest.mark.parametrize("phased", [True, False])
def test_single_rank_sharded_equals_modular_gmmvi(ctx, phased, monkeypatch):
    """The arrangement and tolerances of the sharded test of tests/test_hip_logreg.py on the D = 8 target."""
    from gmmvi_amd.sharded import ShardedGMMVI, HipOps, LocalExchange
    d, k, s, seed = 8, 3, 60, 17
    cfg = samtron_config(s)
    _, _, device = _gauss_pair(d, k, s, seed, cfg, _device_lnpdf)
    g = device()
    if not phased:
        monkeypatch.setenv("GMMVI_FAST_PATH", "0")
    sh = ShardedGMMVI(HipOps(ctx, g.sample_selector.target_distribution), LocalExchange(), d, k,
                      g.model.means.numpy(), g.model.chol_cov.numpy(), s, seed, cfg)
    assert (sh._fast is not None) == phased
    for _ in range(6):
        g.train_iter()
        sh.train_iter()
    sh.flush()
    np.testing.assert_allclose(sh.means.numpy(), g.model.means.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(sh.chols.numpy(), g.model.chol_cov.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(sh.log_weights.numpy(), g.model.log_weights.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(sh.stepsizes.numpy(), g.model.stepsizes.numpy(), rtol=1e-6)


# ---- values only ---------------------------------------------------------------------------------------------------------
E2E_ITERS, E2E_SAMPLES = 30, 60


def _values_only(ref):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    return DeviceLNPDF(cases.QUARTIC_SRC, ref.get_num_dimensions(), params=ref.params(), has_gradient=False)


def _build_one_component(target, d, estimator, diag):
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    cfg = samtron_config(E2E_SAMPLES, reuse_ratio=0.0, estimator=estimator, diag=diag)
    if diag:
        model = DiagonalGMM(np.ones(1), np.zeros((1, d), np.float32), np.ones((1, d), np.float32))
    else:
        model = FullCovGMM(np.ones(1), np.zeros((1, d), np.float32), np.eye(d, dtype=np.float32)[None])
    model.seed = 3
    wrapper = GmmWrapper(model, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
    return GMMVI.build_from_config(cfg, target, wrapper)


@pytest.mark.parametrize("d,diag", [(6, True), (3, False)], ids=["diagonal_more_d6", "full_more_d3"])
def test_values_only_target_reaches_the_fixed_point(ctx, d, diag, monkeypatch):
    """has_gradient=False Gaussian under the gradient-free estimators (KL updater, 60 samples, reuse ratio 0, 30 iterations, the
    configuration of test_gradient_free_target_trains_with_diagonal_more): mu = m and Sigma = P^-1 within 2 % of the parameter
    scale; log_density_and_grad is never called; under Stein the same object raises NotImplementedError."""
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import DiagonalMoreNgEstimator, MoreNgEstimator
    if diag:
        std = np.array([0.6, 1.4, 0.9, 0.5, 1.2, 0.8])
        ref = cases.Quartic(np.array([1.5, -1.0, 0.5, 2.0, -2.0, 0.25], np.float32), np.diag(1.0 / std ** 2).astype(np.float32), 0.0)
    else:
        ref = _gaussian(3, 7)
    target = _values_only(ref)
    assert not hasattr(target, "_fast_path_target")

    with pytest.raises(NotImplementedError):
        _build_one_component(target, d, "Stein", diag).train_iter()

    calls = []
    original = LNPDF.log_density_and_grad
    monkeypatch.setattr(LNPDF, "log_density_and_grad", lambda self, x: (calls.append(1), original(self, x))[1])
    g = _build_one_component(target, d, "MORE", diag)
    assert type(g.ng_estimator) is (DiagonalMoreNgEstimator if diag else MoreNgEstimator)
    assert g.ng_estimator.uses_target_gradients is False and not g._fast_path.eligible()
    for _ in range(E2E_ITERS):
        g.train_iter()
    assert calls == []
    assert int(g.sample_db.num_samples_written) == E2E_ITERS * E2E_SAMPLES
    mu = g.model.means.numpy()[0].astype(np.float64)
    cov_ref = np.linalg.inv(ref.P)
    if diag:
        sg = g.model.chol_cov.numpy()[0].astype(np.float64)
        dev = (np.abs(mu - ref.m).max() / np.abs(ref.m).max(), np.abs(sg - std).max() / np.abs(std).max())
    else:
        L = g.model.chol_cov.numpy()[0].astype(np.float64)
        L_ref = np.linalg.cholesky(cov_ref)
        dev = (np.abs(mu - ref.m).max() / np.abs(ref.m).max(), np.abs(L - L_ref).max() / np.abs(L_ref).max())
    print(f"\n[custom_target] values only, D = {d}: means {dev[0]:.2e} factors {dev[1]:.2e} (bound 2.0e-02 of the parameter scale)")
    assert max(dev) <= 2e-2, dev
