"""GPU tests of user-defined device targets differentiated on a tape (csrc/custom_target_tape.inc, DeviceTapeLNPDF): the
gradient of the recorded evaluation and its backward sweep, and both value calls, against fp64 at the seams of the 64-lane wave,
at the dimensions of the forward mode's tests, above its cap and at the largest diagonal dimension; capacity growth, slabs, the
scratch budget, determinism and the mode refusals; and the target in the modular iteration (full covariance and diagonal) and
under a gradient-free estimator.

Kernel bound: the rule of tests/test_hip_custom_target.py, unchanged (its _bound): the device's largest error against the fp64
NumPy restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|; for lp and the gradient of the gradient call and for lp of the value call.  Every case prints its
ratios before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_tape_cases as cases
import test_hip_custom_autodiff as forward
import test_hip_custom_target as hand
from gmmvi_amd import _lib
from helpers import samtron_config
from oracle import train as otrain

pytestmark = pytest.mark.gpu

ERR_ARG = -2
RECORD_BYTES = _lib.CUSTOM_TAPE_RECORD_BYTES


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name):
    from gmmvi_amd import hip_ops
    if name not in _handles:
        _handles[name] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode="tape")
    return _handles[name]


def _launch(ctx, handle, params, x, want_grad, capacity=0, scratch=0):
    """gmmvi_target_custom_tape on outputs with hand.CANARY_ROWS extra rows of SENTINEL behind them -> (rc, lp, grad | None);
    the extra rows are checked here: bit-unchanged (hand._launch for this entry point)."""
    n, d = x.shape
    xd, pd = ctx.asarray(x), ctx.asarray(params)
    lp = ctx.full((n + hand.CANARY_ROWS,), hand.SENTINEL)
    grad = ctx.full((n + hand.CANARY_ROWS, d), hand.SENTINEL) if want_grad else None
    rc = ctx.lib.gmmvi_target_custom_tape(ctx.handle, handle.handle, d, pd.ptr, xd.ptr, n, lp.ptr,
                                          None if grad is None else grad.ptr, capacity, scratch)
    if rc != 0:
        return rc, None, None
    sentinel = np.array(hand.SENTINEL).view(np.uint32)
    lp_h = lp.numpy()
    assert np.all(lp_h[n:].view(np.uint32) == sentinel), "lp written past N"
    g_h = None
    if want_grad:
        g_h = grad.numpy()
        assert np.all(g_h[n:].view(np.uint32) == sentinel), "gradient written past N"
        g_h = g_h[:n]
    return rc, lp_h[:n], g_h


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


def _tape_launches(ctx, call):
    """-> (result of call(), launches with the profiling tag target_custom_tape it made)."""
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 1))
    try:
        out = call()
    finally:
        buf = C.create_string_buffer(1 << 16)
        ctx.check(ctx.lib.gmmvi_profile_report(ctx.handle, buf, len(buf)))
        ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 0))
    count = 0
    for line in buf.value.decode().splitlines():
        fields = line.split()
        if fields and fields[0] == "target_custom_tape":
            count += int(fields[1])
    return out, count


def _check_case(ctx, name, d, n, scratch=0):
    tgt, x, lp64, g64, lp32, g32 = _reference(name, d, n)
    handle = _handle(ctx, name)
    params = tgt.params()
    rc, lp, g = _launch(ctx, handle, params, x, True, 0, scratch)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    e_lp, b_lp, r_lp = hand._bound(lp, lp64, lp32)
    e_g, b_g, r_g = hand._bound(g, g64, g32)
    from gmmvi_amd import hip_ops
    print(f"\n[custom_tape] {name} D={d} N={n}: tape length {hip_ops.custom_tape_length(ctx, handle, d)}, lp error {e_lp:.3e} "
          f"(bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f}), gradient error {e_g:.3e} (bound {b_g:.3e}, "
          f"{e_g / b_g:.3f} of it, ratio {r_g:.2f})")
    assert e_lp <= b_lp, f"lp error {e_lp:.3e} > {b_lp:.3e}"
    assert e_g <= b_g, f"gradient error {e_g:.3e} > {b_g:.3e}"
    rc, lp_v, g_v = _launch(ctx, handle, params, x, False)
    assert rc == 0 and g_v is None
    e_v, b_v, r_v = hand._bound(lp_v, lp64, lp32)
    print(f"[custom_tape] {name} D={d} N={n} values only: lp error {e_v:.3e} (bound {b_v:.3e}, {e_v / b_v:.3f} of it, ratio {r_v:.2f})")
    assert e_v <= b_v, f"values only: lp error {e_v:.3e} > {b_v:.3e}"


@pytest.mark.parametrize("name,d,n", cases.KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_matches_fp64_reference(ctx, name, d, n):
    _check_case(ctx, name, d, n)


def test_kernel_at_the_largest_dimension(ctx):
    """chain at D = GMMVI_MAX_DIM_DIAG, two samples, an explicit scratch budget of 1 GiB (the tape of one wave takes 5 D records
    of 1280 bytes: 0.8 GiB)."""
    name, d, n = cases.MAX_DIM_CASE
    assert d == _lib.MAX_DIM_DIAG
    _check_case(ctx, name, d, n, scratch=1 << 30)


@pytest.mark.parametrize("name,d,n", [("quartic", 17, 70), ("allops", 6, 200)])
def test_forward_mode_and_tape_agree(ctx, name, d, n):
    """The same text through both modes: each gradient within its own bound of fp64, and the value calls, both the float
    instantiation of the same function, bit-equal."""
    tgt, x, lp64, g64, lp32, g32 = _reference(name, d, n)
    params = tgt.params()
    rc, lp_t, g_t = _launch(ctx, _handle(ctx, name), params, x, True)
    assert rc == 0
    rc, lp_f, g_f = hand._launch(ctx, forward._handle(ctx, name), params, x, True, 0)
    assert rc == 0
    for label, lp, g in (("tape", lp_t, g_t), ("forward", lp_f, g_f)):
        e_lp, b_lp, _ = hand._bound(lp, lp64, lp32)
        e_g, b_g, _ = hand._bound(g, g64, g32)
        print(f"\n[custom_tape] {name} D={d} {label}: lp {e_lp / b_lp:.3f} of its bound, gradient {e_g / b_g:.3f} of its bound")
        assert e_lp <= b_lp and e_g <= b_g, label
    _, v_t, _ = _launch(ctx, _handle(ctx, name), params, x, False)
    _, v_f, _ = hand._launch(ctx, forward._handle(ctx, name), params, x, False, 2)
    np.testing.assert_array_equal(v_t.view(np.uint32), v_f.view(np.uint32))


def test_capacity_growth_and_the_remembered_length(ctx):
    """quartic at D = 17 from a capacity of 8 records: the launch reports the needed length, the call repeats it once, and the
    result is bit-identical to a run with ample capacity; the handle then knows the length, and a call with capacity 0 launches
    once."""
    from gmmvi_amd import hip_ops
    tgt, x, *_ = _reference("quartic", 17, 70)
    text = cases.SOURCES["quartic"] + "\n// capacity growth\n"                # a handle of its own: nothing remembered yet
    handle = hip_ops.custom_target_compile(ctx, text, mode="tape")
    assert hip_ops.custom_tape_length(ctx, handle, 17) == 0
    (rc, lp_small, g_small), launches = _tape_launches(ctx, lambda: _launch(ctx, handle, tgt.params(), x, True, 8))
    assert rc == 0 and launches == 2
    needed = hip_ops.custom_tape_length(ctx, handle, 17)
    assert needed > 8 and hip_ops.custom_tape_length(ctx, handle, 16) == 0
    (rc, lp_auto, g_auto), launches = _tape_launches(ctx, lambda: _launch(ctx, handle, tgt.params(), x, True, 0))
    assert rc == 0 and launches == 1
    (rc, lp_big, g_big), launches = _tape_launches(ctx, lambda: _launch(ctx, handle, tgt.params(), x, True, 4 * needed))
    assert rc == 0 and launches == 1
    assert hip_ops.custom_tape_length(ctx, handle, 17) == needed
    for lp, g in ((lp_small, g_small), (lp_auto, g_auto)):
        np.testing.assert_array_equal(lp.view(np.uint32), lp_big.view(np.uint32))
        np.testing.assert_array_equal(g.view(np.uint32), g_big.view(np.uint32))
    # a capacity of exactly the needed length is enough, one record less is not
    (rc, _, g_exact), launches = _tape_launches(ctx, lambda: _launch(ctx, handle, tgt.params(), x, True, needed))
    assert rc == 0 and launches == 1
    np.testing.assert_array_equal(g_exact.view(np.uint32), g_big.view(np.uint32))
    (rc, _, g_less), launches = _tape_launches(ctx, lambda: _launch(ctx, handle, tgt.params(), x, True, needed - 1))
    assert rc == 0 and launches == 2
    np.testing.assert_array_equal(g_less.view(np.uint32), g_big.view(np.uint32))


def test_slabs_budget_refusal_and_determinism(ctx):
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = _reference("quartic", 17, 200)
    handle = _handle(ctx, "quartic")
    rc, lp_one, g_one = _launch(ctx, handle, tgt.params(), x, True)
    assert rc == 0
    needed = hip_ops.custom_tape_length(ctx, handle, 17)
    assert hip_ops.custom_tape_plan(200, needed) == (1, 256)
    # two identical calls: the same bits
    rc, lp_again, g_again = _launch(ctx, handle, tgt.params(), x, True)
    np.testing.assert_array_equal(lp_again.view(np.uint32), lp_one.view(np.uint32))
    np.testing.assert_array_equal(g_again.view(np.uint32), g_one.view(np.uint32))
    # a budget of one wave's tape: four slabs of 64 lanes, the same bits
    budget = 64 * needed * RECORD_BYTES
    assert hip_ops.custom_tape_plan(200, needed, budget) == (4, 64)
    (rc, lp_slabs, g_slabs), launches = _tape_launches(ctx, lambda: _launch(ctx, handle, tgt.params(), x, True, 0, budget))
    assert rc == 0 and launches == 4
    np.testing.assert_array_equal(lp_slabs.view(np.uint32), lp_one.view(np.uint32))
    np.testing.assert_array_equal(g_slabs.view(np.uint32), g_one.view(np.uint32))
    # one byte less holds no wave of the needed length: refused, the message names the length and its bytes
    rc, _, _ = _launch(ctx, handle, tgt.params(), x, True, 0, budget - 1)
    assert rc == ERR_ARG
    message = ctx.lib.gmmvi_last_error(ctx.handle).decode()
    assert str(needed) in message and str(budget) in message and str(budget - 1) in message, message
    # the value call needs no tape, and the next gradient call on the context works
    rc, lp_v, _ = _launch(ctx, handle, tgt.params(), x, False, 0, 1)
    assert rc == 0
    rc, lp_ok, g_ok = _launch(ctx, handle, tgt.params(), x, True)
    assert rc == 0
    np.testing.assert_array_equal(g_ok.view(np.uint32), g_one.view(np.uint32))
    assert hand._bound(g_ok, g64, g32)[0] <= hand._bound(g_ok, g64, g32)[1]


def test_mode_refusals_and_the_module_cache(ctx):
    from gmmvi_amd import hip_ops
    lib = ctx.lib
    tgt, x, *_ = _reference("quartic", 17, 70)
    n, d = x.shape
    tape, auto, written = _handle(ctx, "quartic"), forward._handle(ctx, "quartic"), hand._handle(ctx, "quartic")
    # the key holds the mode: the same text gives one handle per mode, and the same handle again within a mode
    assert len({tape.ptr, auto.ptr, written.ptr}) == 3
    assert hip_ops.custom_target_compile(ctx, cases.SOURCES["quartic"], mode="tape").ptr == tape.ptr
    assert hip_ops.custom_target_compile(ctx, cases.SOURCES["quartic"], mode="autodiff").ptr == auto.ptr
    xd, pd = ctx.asarray(x), ctx.asarray(tgt.params())
    lp, grad = ctx.full((n,), hand.SENTINEL), ctx.full((n, d), hand.SENTINEL)

    def untouched():
        ctx.check(lib.gmmvi_sync(ctx.handle))
        return np.all(lp.numpy() == hand.SENTINEL) and np.all(grad.numpy() == hand.SENTINEL)

    for route in (0, 1, 2):
        assert lib.gmmvi_target_custom(ctx.handle, tape.handle, d, pd.ptr, xd.ptr, n, lp.ptr, grad.ptr, route) == ERR_ARG
        assert "gmmvi_target_custom_tape" in lib.gmmvi_last_error(ctx.handle).decode()
    assert lib.gmmvi_target_custom(ctx.handle, tape.handle, d, pd.ptr, xd.ptr, n, lp.ptr, None, 0) == ERR_ARG
    assert untouched()
    for other in (auto, written):
        for g in (grad.ptr, None):
            assert lib.gmmvi_target_custom_tape(ctx.handle, other.handle, d, pd.ptr, xd.ptr, n, lp.ptr, g, 0, 0) == ERR_ARG
            message = lib.gmmvi_last_error(ctx.handle).decode()
            assert "gmmvi_custom_target_compile_tape" in message and "gmmvi_target_custom" in message
    assert untouched()
    # bad shapes and pointers
    for dd, nn, xp, lpp, cap in ((0, n, xd.ptr, lp.ptr, 0), (d, 0, xd.ptr, lp.ptr, 0), (d, n, None, lp.ptr, 0), (d, n, xd.ptr, None, 0),
                                 (d, n, xd.ptr, lp.ptr, -1), (_lib.MAX_DIM_DIAG + 1, n, xd.ptr, lp.ptr, 0)):
        assert lib.gmmvi_target_custom_tape(ctx.handle, tape.handle, dd, pd.ptr, xp, nn, lpp, grad.ptr, cap, 0) == ERR_ARG
    assert lib.gmmvi_target_custom_tape(ctx.handle, None, d, pd.ptr, xd.ptr, n, lp.ptr, grad.ptr, 0, 0) == ERR_ARG
    assert untouched()
    # the python wrapper and the class give what the C call gives
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceTapeLNPDF
    rc, lp_c, g_c = _launch(ctx, tape, tgt.params(), x, True)
    t = DeviceTapeLNPDF(cases.SOURCES["quartic"], d, params=tgt.params(), tape_capacity=16)
    assert t._handle.ptr == tape.ptr and t.get_num_dimensions() == d and t.use_log_density_and_grad
    lp_p, g_p = t.log_density_and_grad(x)
    np.testing.assert_array_equal(lp_p.numpy(), lp_c)
    np.testing.assert_array_equal(g_p.numpy(), g_c)
    np.testing.assert_array_equal(t.log_density(ctx.asarray(x)).numpy(), _launch(ctx, tape, tgt.params(), x, False)[1])
    with pytest.raises(ValueError):
        t.log_density(np.zeros((4, d + 1), np.float32))


def test_output_that_is_an_input_or_a_constant(ctx):
    from gmmvi_amd import hip_ops
    text = ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
            "    if (x[0] > 1.f) return x[1];\n"                      # an input
            "    if (x[0] < -1.f) return 3.f;\n"                      # a constant
            "    const T unused = x[0] * x[1];\n"                     # a record behind which the output does not stand
            "    return x[2] * 2.f + gmmvi_value(unused) * 0.f;\n}\n")
    handle = hip_ops.custom_target_compile(ctx, text, mode="tape")
    x = np.random.default_rng(3).normal(size=(130, 3)).astype(np.float32) * 2
    rc, lp, g = _launch(ctx, handle, np.zeros(1, np.float32), x, True)
    assert rc == 0
    want_lp = np.where(x[:, 0] > 1, x[:, 1], np.where(x[:, 0] < -1, np.float32(3), x[:, 2] * np.float32(2)))
    want_g = np.zeros_like(x)
    want_g[x[:, 0] > 1, 1] = 1
    want_g[np.abs(x[:, 0]) <= 1, 2] = 2
    assert (x[:, 0] > 1).any() and (x[:, 0] < -1).any() and (np.abs(x[:, 0]) <= 1).any()
    np.testing.assert_array_equal(lp, want_lp.astype(np.float32))
    np.testing.assert_array_equal(g, want_g)


# ---- the iteration -----------------------------------------------------------------------------------------------------
def test_modular_path_rosenbrock_against_the_oracle(ctx, monkeypatch):
    """The set-up of test_modular_path_rosenbrock_against_the_oracle (tests/test_hip_custom_autodiff.py) with the tape class:
    SAMTRUX defaults, one initial component, 60 samples, five iterations on the modular path against the fp64 oracle, same Philox
    stream and bounds.  Five device gradient calls, no host log_density*, no sample download; the single-call iteration is not
    eligible."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.configs import get_default_algorithm_config, update_config
    from gmmvi_amd.device import DeviceArray
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceTapeLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    s, seed = 60, 11
    cfg = update_config(get_default_algorithm_config("SAMTRUX"), {
        "model_initialization": {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0., "prior_scale": 1.,
                                 "initial_cov": 1.},
        "use_sample_database": True, "max_database_size": int(1e6), "temperature": 1., "seed": 0,
        "sample_selector_config": {"desired_samples_per_component": s, "ratio_reused_samples_to_desired": 0.0}})
    ref = cases.Rosenbrock()
    o = hand._oracle(ref, 2, 1, seed, cfg, 1.0, 1.0)
    target = DeviceTapeLNPDF(cases.SOURCES["rosenbrock"], 2, params=ref.params())
    g = hand._device(target, o, seed, cfg, 1.0)
    assert not hasattr(target, "_fast_path_target") and not g._fast_path.eligible()

    counts = {"device": 0, "host": 0, "downloads": 0}
    real = hip_ops.target_custom_tape

    def counting_kernel(c, handle, params, x, want_grad=True, **kw):
        assert isinstance(x, DeviceArray) and want_grad
        counts["device"] += 1
        return real(c, handle, params, x, want_grad, **kw)

    def host_call(self, x):
        counts["host"] += 1
        raise AssertionError("a host log_density* was called")

    real_numpy = DeviceArray.numpy

    def counting_numpy(self):
        if self.shape == (s, 2):
            counts["downloads"] += 1
        return real_numpy(self)

    monkeypatch.setattr(hip_ops, "target_custom_tape", counting_kernel)
    monkeypatch.setattr(LNPDF, "log_density", host_call)
    monkeypatch.setattr(LNPDF, "log_density_and_grad", host_call)
    monkeypatch.setattr(DeviceArray, "numpy", counting_numpy)
    hand._run_pair(monkeypatch, o, g, 5, fused=False)
    assert counts == {"device": 5, "host": 0, "downloads": 0}, counts


def test_diagonal_stein_iteration_on_the_chain_above_the_forward_cap():
    """chain at D = 600 (the forward mode stops at 512) under a diagonal-covariance model with the Stein estimator and the KL trust
    region, K = 3, 40 samples per component, three iterations against the fp64 oracle on the NumPy restatement, identical draws;
    the criteria of _run_pair in tests/test_hip_diag_highd.py."""
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceTapeLNPDF
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    d, k, s, seed, iters = 600, 3, 40, 11, 3
    cfg = samtron_config(s, diag=True)
    ref = cases.Chain(d)
    prior_scale, initial_cov = 0.5, 0.25
    model = otrain.construct_initial_mixture(d, k, 0.0, prior_scale, initial_cov, np.random.default_rng(seed + 1),
                                             use_diagonal_covs=True)
    o = otrain.OracleGMMVI(
        ref, model, temperature=cfg["temperature"], seed=seed, desired_samples_per_component=s, ratio_reused_samples_to_desired=0.0,
        ng_estimator="Stein", only_use_own_samples=cfg["ng_estimator_config"]["only_use_own_samples"],
        use_self_normalized_importance_weights=cfg["ng_estimator_config"]["use_self_normalized_importance_weights"],
        updater=cfg["ng_based_updater_type"], component_stepsize_config=cfg["component_stepsize_adapter_config"],
        weight_updater=cfg["weight_updater_type"], weight_stepsize_config=cfg["weight_stepsize_adapter_config"], adaptive=None,
        max_reward_history_length=400, sample_selector=cfg["sample_selector_type"], max_database_size=cfg["max_database_size"],
        host_rng=np.random.default_rng(seed))
    om = o.model.model
    m = DiagonalGMM(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
    m.seed = seed
    wrapper = GmmWrapper(m, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
    c = dict(cfg)
    c["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=initial_cov)
    g = GMMVI.build_from_config(c, DeviceTapeLNPDF(cases.CHAIN_SRC, d, params=ref.params()), wrapper)
    assert g.model.diagonal_covs and g.sample_db.diagonal_covariances and not g._fast_path.eligible()
    for it in range(iters):
        info = o.train_iter()
        g.train_iter()
        gm = g.model
        assert gm.num_components == o.model.num_components
        tol = 2e-3 * (1 + it)
        dm = np.abs(gm.means.numpy() - o.model.means).max() / max(1.0, np.abs(o.model.means).max())
        dc = np.abs(gm.chol_cov.numpy() - o.model.chol_cov).max() / np.abs(o.model.chol_cov).max()
        dw = np.abs(np.exp(gm.log_weights.numpy()) - o.model.weights).max()
        print(f"\n[custom_tape] chain D={d} iteration {it}: means {dm:.2e} sigma {dc:.2e} weights {dw:.2e} (tolerance {tol:.1e})")
        assert dm <= tol, it
        assert dc <= tol, it
        assert dw <= tol, it
        if "success" in info and g.ng_based_updater.last_success is not None:
            np.testing.assert_array_equal(g.ng_based_updater.last_success.numpy().astype(bool), info["success"])
        np.testing.assert_allclose(gm.num_received_updates.numpy(), o.model.num_received_updates)
    assert int(g.sample_db.num_samples_written) == iters * k * s


def test_gradient_free_estimator_evaluates_values_only(ctx, monkeypatch):
    """Under DiagonalMoreNgEstimator the tape class is asked for values alone: no call records a tape."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceTapeLNPDF
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import DiagonalMoreNgEstimator
    d = 6
    ref = cases.Chain(d)
    target = DeviceTapeLNPDF(cases.CHAIN_SRC, d, params=ref.params())
    wanted = []
    real = hip_ops.target_custom_tape

    def recording(c, handle, params, x, want_grad=True, **kw):
        wanted.append(bool(want_grad))
        return real(c, handle, params, x, want_grad, **kw)

    monkeypatch.setattr(hip_ops, "target_custom_tape", recording)
    g = hand._build_one_component(target, d, "MORE", True)
    assert type(g.ng_estimator) is DiagonalMoreNgEstimator and g.ng_estimator.uses_target_gradients is False
    (_, launches) = _tape_launches(ctx, lambda: [g.train_iter() for _ in range(3)])
    assert len(wanted) == 3 and not any(wanted), wanted
    assert launches == 3
    assert int(g.sample_db.num_samples_written) == 3 * hand.E2E_SAMPLES
    tlp = g.sample_db.target_lnpdfs.numpy()
    np.testing.assert_allclose(tlp, ref.log_density(g.sample_db.samples.numpy().astype(np.float64)), rtol=1e-4,
                               atol=1e-4 * np.abs(tlp).max())
