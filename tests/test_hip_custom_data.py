"""GPU tests of user-defined device targets summed over a data set (csrc/custom_target_data.inc, DeviceDataLNPDF): the kernels
against fp64 at the seams of the 64-sample tile, of the pass width, of the staged route's cap, of the four waves and of the row
chunks, in full-data and in minibatch mode; determinism; agreement across chunk counts; the refused arguments; the module cache
with the mode in its key; a cross-check against the built-in logistic regression; and the target in the modular iteration, with
and without minibatches, and under a gradient-free estimator.

Kernel bound: the rule of tests/test_hip_custom_target.py, unchanged (its _bound): the device's largest error against the fp64
NumPy restatement is at most 16 times the largest error of the fp32 NumPy restatement (row sum sequential in row-list order) on
the same inputs plus 4 * eps32 * max|reference|; for lp and the gradient of the gradient call and for lp of the value call.
Every case prints its ratios before it asserts.  tests/test_custom_data_host.py shows what that bound can see."""
import ctypes as C

import numpy as np
import pytest

import custom_data_cases as cases
import test_hip_custom_target as hand
from gmmvi_amd import _lib
from test_hip_custom_target import SENTINEL, _bound

pytestmark = pytest.mark.gpu

ERR_ARG = -2
W = _lib.CUSTOM_AUTODIFF_TANGENTS
KERNEL_CASES = cases.kernel_cases(W, _lib.CUSTOM_STAGED_MAX_DIM)


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name):
    from gmmvi_amd import hip_ops
    if name not in _handles:
        _handles[name] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode="data")
    return _handles[name]


def _launch(ctx, handle, tgt, x, want_grad, chunks=0):
    """gmmvi_target_custom_data for the restatement ``tgt`` (its data, params, batch, seed and current call) on outputs with
    CANARY_ROWS extra rows of SENTINEL behind them, in the manner of _launch of tests/test_hip_custom_target.py -> (rc, lp,
    grad | None); the extra rows are checked here: bit-unchanged."""
    n, d = x.shape
    t, c = tgt.data.shape
    xd, pd, dd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    lp = ctx.full((n + hand.CANARY_ROWS,), SENTINEL)
    grad = ctx.full((n + hand.CANARY_ROWS, d), SENTINEL) if want_grad else None
    mini = tgt.batch_size is not None
    rc = ctx.lib.gmmvi_target_custom_data(ctx.handle, handle.handle, d, pd.ptr, dd.ptr, t, c, int(mini), tgt.batch_size if mini else t,
                                          tgt.seed, tgt.call_count, xd.ptr, n, lp.ptr, None if grad is None else grad.ptr, chunks)
    if rc != 0:
        return rc, None, None
    sentinel_bits = np.array(SENTINEL).view(np.uint32)
    lp_h = lp.numpy()
    assert np.all(lp_h[n:].view(np.uint32) == sentinel_bits), "lp written past N"
    g_h = None
    if want_grad:
        g_h = grad.numpy()
        assert np.all(g_h[n:].view(np.uint32) == sentinel_bits), "gradient written past N"
        g_h = g_h[:n]
    return rc, lp_h[:n], g_h


def _check(tag, lp, g, lp64, g64, lp32, g32):
    e_lp, b_lp, r_lp = _bound(lp, lp64, lp32)
    line = f"[custom_data] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
    if g is not None:
        e_g, b_g, r_g = _bound(g, g64, g32)
        line += f", gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})"
    print("\n" + line)
    assert np.all(np.isfinite(lp)) and (g is None or np.all(np.isfinite(g)))
    assert e_lp <= b_lp, f"{tag}: lp error {e_lp:.3e} > {b_lp:.3e}"
    if g is not None:
        assert e_g <= b_g, f"{tag}: gradient error {e_g:.3e} > {b_g:.3e}"


@pytest.mark.parametrize("c", KERNEL_CASES, ids=cases.case_id)
def test_kernel_matches_fp64_reference(ctx, c):
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, c.name)
    rc, lp, g = _launch(ctx, handle, tgt, x, True, c.chunks)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    _check(cases.case_id(c), lp, g, lp64, g64, lp32, g32)
    rc, lp_v, g_v = _launch(ctx, handle, tgt, x, False, c.chunks)
    assert rc == 0 and g_v is None
    _check(cases.case_id(c) + " values only", lp_v, None, lp64, g64, lp32, g32)


SEAM_CASE = cases.Case("logit", W + 1, 65, 67, 0, None, 0)
SEAM_MINIBATCH = cases.Case("student", 5, 65, 257, 0, 257, 3)


@pytest.mark.parametrize("c", [SEAM_CASE, SEAM_MINIBATCH], ids=cases.case_id)
def test_same_call_twice_gives_the_same_bits(ctx, c):
    tgt, x = cases.reference(c)[:2]
    handle = _handle(ctx, c.name)
    for chunks in (1, 3):
        for want_grad in (True, False):
            _, lp_a, g_a = _launch(ctx, handle, tgt, x, want_grad, chunks)
            _, lp_b, g_b = _launch(ctx, handle, tgt, x, want_grad, chunks)
            np.testing.assert_array_equal(lp_a.view(np.uint32), lp_b.view(np.uint32))
            if want_grad:
                np.testing.assert_array_equal(g_a.view(np.uint32), g_b.view(np.uint32))


@pytest.mark.parametrize("c", [SEAM_CASE, SEAM_MINIBATCH], ids=cases.case_id)
def test_chunk_counts_agree_within_the_bound(ctx, c):
    """chunks = 1, 2, 3 each meet the kernel bound and differ from each other by no more than it.  They need not agree bitwise:
    another chunk count adds the same terms in another order."""
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, c.name)
    out = {}
    for chunks in (1, 2, 3):
        rc, lp, g = _launch(ctx, handle, tgt, x, True, chunks)
        assert rc == 0
        _check(f"{cases.case_id(c)} forced to {chunks} chunk(s)", lp, g, lp64, g64, lp32, g32)
        out[chunks] = (lp, g)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    for a, b in ((1, 2), (1, 3), (2, 3)):
        d_lp = float(np.abs(out[a][0].astype(np.float64) - out[b][0]).max())
        d_g = float(np.abs(out[a][1].astype(np.float64) - out[b][1]).max())
        print(f"[custom_data] chunks {a} against {b}: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), the gradient by "
              f"{d_g:.3e} ({d_g / b_g:.3f})")
        assert d_lp <= b_lp and d_g <= b_g


def test_python_wrapper_gives_what_the_c_call_gives(ctx):
    from gmmvi_amd import hip_ops
    for c in (SEAM_CASE, SEAM_MINIBATCH):
        tgt, x = cases.reference(c)[:2]
        handle = _handle(ctx, c.name)
        _, lp_c, g_c = _launch(ctx, handle, tgt, x, True, 0)
        lp, g = hip_ops.target_custom_data(ctx, handle, ctx.asarray(tgt.params()), ctx.asarray(tgt.data), ctx.asarray(x), True,
                                           batch_size=tgt.batch_size, seed=tgt.seed, call=tgt.call_count)
        np.testing.assert_array_equal(lp.numpy(), lp_c)
        np.testing.assert_array_equal(g.numpy(), g_c)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_outputs_and_the_context_alone(ctx):
    lib = ctx.lib
    c = cases.Case("logit", 5, 8, 9, 0, 5, 0)
    tgt, x = cases.build_case(c)
    handle = _handle(ctx, "logit")
    n, d, t, cols = 8, 5, 9, 6
    xd, pd, dd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    lp, grad = ctx.full((n,), SENTINEL), ctx.full((n, d), SENTINEL)

    def call(D=d, data=dd.ptr, T=t, Cc=cols, mini=1, B=5, X=xd.ptr, N=n, out=lp.ptr, g=grad.ptr, h=handle.handle, chunks=0):
        return lib.gmmvi_target_custom_data(ctx.handle, h, D, pd.ptr, data, T, Cc, mini, B, 9, 0, X, N, out, g, chunks)

    def last():
        return lib.gmmvi_last_error(ctx.handle).decode()

    assert call(B=0) == ERR_ARG and "B = 0" in last()
    assert call(B=10) == ERR_ARG and "B = 10" in last() and "T = 9" in last()
    assert call(mini=0, B=10) == ERR_ARG
    assert call(Cc=0) == ERR_ARG and "C = 0" in last()
    assert call(data=None) == ERR_ARG
    assert call(T=0) == ERR_ARG and "T = 0" in last()
    assert call(T=2 ** 31) == ERR_ARG and "2^31" in last()
    for kw in (dict(N=0), dict(X=None), dict(out=None), dict(D=0), dict(mini=2), dict(chunks=-1), dict(h=None)):
        assert call(**kw) == ERR_ARG, kw
    # a handle of another mode
    assert call(h=hand._handle(ctx, "rosenbrock").handle) == ERR_ARG and "gmmvi_custom_target_compile_data" in last()
    # a gradient pointer above the cap of the dual passes; the outputs are as large as that call needs
    big = _lib.CUSTOM_AUTODIFF_MAX_DIM + 1
    cb = cases.Case("logit", big, n, 3, 0, None, 0)
    tgt_b, x_b, lp64, g64, lp32, g32 = cases.reference(cb)
    xb, db = ctx.asarray(x_b), ctx.asarray(tgt_b.data)
    grad_b = ctx.full((n, big), SENTINEL)
    rc = lib.gmmvi_target_custom_data(ctx.handle, handle.handle, big, pd.ptr, db.ptr, 3, big + 1, 0, 3, 0, 0, xb.ptr, n, lp.ptr, grad_b.ptr, 0)
    assert rc == ERR_ARG and "512" in last() and "513" in last()
    ctx.check(lib.gmmvi_sync(ctx.handle))
    bits = np.array(SENTINEL).view(np.uint32)
    assert np.all(lp.numpy().view(np.uint32) == bits) and np.all(grad.numpy().view(np.uint32) == bits)
    assert np.all(grad_b.numpy().view(np.uint32) == bits)
    # the same call without a gradient pointer runs
    rc, lp_v, _ = _launch(ctx, handle, tgt_b, x_b, False)
    assert rc == 0
    _check("D = 513, values only", lp_v, None, lp64, g64, lp32, g32)
    # the context works afterwards
    tgt_s, x_s, lp64, g64, lp32, g32 = cases.reference(SEAM_CASE)
    rc, lp_ok, g_ok = _launch(ctx, handle, tgt_s, x_s, True)
    assert rc == 0
    _check("after the refusals", lp_ok, g_ok, lp64, g64, lp32, g32)


BOTH_MODES_SRC = ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
                  "    T s = 0.f; for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i]; return s; }\n"
                  "template <class T, class X> __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {\n"
                  "    return row[0] * x[0]; }\n"
                  "template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params) {\n"
                  "    return gmmvi_user_density<T, X>(x, D, params); }\n")


def test_handle_modes(ctx):
    from gmmvi_amd import hip_ops
    lib = ctx.lib
    h1 = _handle(ctx, "logit")
    h2 = hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data")
    assert h1.ptr == h2.ptr
    assert hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC + "\n// another text\n", mode="data").ptr != h1.ptr
    # gmmvi_target_custom (and so target kind 5) refuses a data-mode handle and names the entry point that takes it
    x = ctx.asarray(np.zeros((4, 5), np.float32))
    lp = ctx.full((4,), SENTINEL)
    assert lib.gmmvi_target_custom(ctx.handle, h1.handle, 5, None, x.ptr, 4, lp.ptr, None, 0) == ERR_ARG
    assert "gmmvi_target_custom_data" in lib.gmmvi_last_error(ctx.handle).decode()
    ctx.check(lib.gmmvi_sync(ctx.handle))
    assert np.all(lp.numpy() == SENTINEL)
    with pytest.raises(_lib.GmmviError, match="gmmvi_target_custom_data"):
        hip_ops.target_custom(ctx, h1, None, x, want_grad=False)
    # a text valid in two modes: the mode is part of the key
    data_mode = hip_ops.custom_target_compile(ctx, BOTH_MODES_SRC, mode="data")
    autodiff = hip_ops.custom_target_compile(ctx, BOTH_MODES_SRC, mode="autodiff")
    assert data_mode.ptr != autodiff.ptr
    xs = np.random.default_rng(1).normal(size=(65, 3)).astype(np.float32)
    rows = np.array([[2.0], [-0.5]], np.float32)
    lp_d, g_d = hip_ops.target_custom_data(ctx, data_mode, None, ctx.asarray(rows), ctx.asarray(xs), True)
    lp_a, g_a = hip_ops.target_custom(ctx, autodiff, None, ctx.asarray(xs), True)
    want = np.zeros_like(xs)
    want[:, 0] = 1.5
    np.testing.assert_array_equal(g_d.numpy()[:, 1:], g_a.numpy()[:, 1:])
    np.testing.assert_allclose(g_d.numpy() - g_a.numpy(), want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(lp_d.numpy() - lp_a.numpy(), 1.5 * xs[:, 0], rtol=0, atol=4e-6)
    with pytest.raises(ValueError, match="mode"):
        hip_ops.custom_target_compile(ctx, BOTH_MODES_SRC, mode="reverse")


# ---- the built-in logistic regression on the same data ---------------------------------------------------------------------
def _breast_cancer_rows():
    """-> (rows [569, 32] = [X~ (31, bias first) | s], A [569, 31] = diag(s) X~) of the committed fixture, fp32."""
    import logreg_ref
    from gmmvi_amd.experiments.target_distributions import logistic_regression as lr
    table = logreg_ref.load_tables()["breast_cancer"]
    A, _ = lr.preprocess(table, "breast_cancer")
    s = np.where(lr.split_table(table, "breast_cancer")[1] == 1, -1.0, 1.0).astype(np.float32)
    return np.concatenate([A * s[:, None], s[:, None]], axis=1).astype(np.float32), A


def test_logit_text_against_the_built_in_logistic_regression(ctx):
    import logreg_ref
    from gmmvi_amd import hip_ops
    from gmmvi_amd.experiments.target_distributions import logistic_regression as lr
    rows, A = _breast_cancer_rows()
    n, d = 130, A.shape[1]
    x = (np.random.default_rng(3).normal(size=(n, d)) * 0.3).astype(np.float32)
    ref = logreg_ref.LogRegRef(A, lr.PRIOR_MEAN, lr.PRIOR_STD)
    lp64, g64 = ref.log_density_and_grad(x.astype(np.float64))
    tgt = cases.Logit(rows, [lr.PRIOR_MEAN, lr.PRIOR_STD])
    mine64 = tgt.evaluate(x.astype(np.float64))
    np.testing.assert_allclose(mine64[0], lp64, rtol=1e-12)                 # the restatement is that posterior
    np.testing.assert_allclose(mine64[1], g64, rtol=1e-9, atol=1e-12)
    lp32, g32 = cases.fp32_twin(tgt).evaluate(x)
    rc, lp, g = _launch(ctx, _handle(ctx, "logit"), tgt, x, True)
    assert rc == 0
    _check("logit text on breast_cancer", lp, g, lp64, g64, lp32, g32)
    built_in = lr.LogisticRegression(X=rows[:, :-1].astype(np.float64) * rows[:, -1:], labels=np.zeros(len(rows)))
    lp_b, g_b = built_in.log_density_and_grad(ctx.asarray(x))
    _check("built-in LogisticRegression", lp_b.numpy(), g_b.numpy(), lp64, g64, lp32, g32)
    print(f"[custom_data] logit text against the built-in kernel: lp differs by {np.abs(lp - lp_b.numpy()).max():.3e}, the gradient "
          f"by {np.abs(g - g_b.numpy()).max():.3e}")


# ---- the iteration -----------------------------------------------------------------------------------------------------
ITER_SAMPLES, ITER_SEED = 60, 11


def _iteration_setup(batch_size):
    from gmmvi_amd.configs import get_default_algorithm_config, update_config
    from gmmvi_amd.experiments.target_distributions import logistic_regression as lr
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF
    cfg = update_config(get_default_algorithm_config("SAMTRUX"), {
        "model_initialization": {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0., "prior_scale": 1.,
                                 "initial_cov": 1.},
        "use_sample_database": True, "max_database_size": int(1e6), "temperature": 1., "seed": 0,
        "sample_selector_config": {"desired_samples_per_component": ITER_SAMPLES, "ratio_reused_samples_to_desired": 0.0}})
    rows = _breast_cancer_rows()[0]
    data = np.concatenate([rows[:40, :6], rows[:40, -1:]], axis=1)           # the bias, five features, the sign
    params = [lr.PRIOR_MEAN, lr.PRIOR_STD]
    ref = cases.Logit(data, params, batch_size=batch_size, seed=9)
    target = DeviceDataLNPDF(cases.LOGIT_SRC, 6, data, params=params, batch_size=batch_size, seed=9)
    o = hand._oracle(ref, 6, 1, ITER_SEED, cfg, 1.0, 1.0)
    g = hand._device(target, o, ITER_SEED, cfg, 1.0)
    return ref, target, o, g


def _count_calls(monkeypatch):
    from gmmvi_amd import hip_ops
    from gmmvi_amd.device import DeviceArray
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    counts = {"device": 0, "host": 0, "downloads": 0, "grads": []}
    real = hip_ops.target_custom_data

    def counting_kernel(c, handle, params, data, x, want_grad=True, **kw):
        assert isinstance(x, DeviceArray)
        counts["device"] += 1
        counts["grads"].append(bool(want_grad))
        return real(c, handle, params, data, x, want_grad, **kw)

    def host_call(self, x):
        counts["host"] += 1
        raise AssertionError("a host log_density* was called")

    real_numpy = DeviceArray.numpy

    def counting_numpy(self):
        if self.shape == (ITER_SAMPLES, 6):
            counts["downloads"] += 1
        return real_numpy(self)

    monkeypatch.setattr(hip_ops, "target_custom_data", counting_kernel)
    monkeypatch.setattr(LNPDF, "log_density", host_call)
    monkeypatch.setattr(LNPDF, "log_density_and_grad", host_call)
    monkeypatch.setattr(DeviceArray, "numpy", counting_numpy)
    return counts


def test_modular_iteration_full_data_against_the_oracle(ctx, monkeypatch):
    """logit on 40 rows of the breast-cancer fixture (bias + five features, D = 6), SAMTRUX defaults, one initial component, 60
    samples, five iterations on the modular path against the fp64 oracle on the fp64 restatement, same Philox stream.  Five
    device calls, no host log_density*, no sample download; the single-call iteration is not eligible."""
    ref, target, o, g = _iteration_setup(None)
    assert not hasattr(target, "_fast_path_target") and not g._fast_path.eligible()
    counts = _count_calls(monkeypatch)
    hand._run_pair(monkeypatch, o, g, 5, fused=False)
    assert (counts["device"], counts["host"], counts["downloads"]) == (5, 0, 0), counts
    assert all(counts["grads"])
    assert target.call_count == 0                                              # full data: no stream, no counter


def test_modular_iteration_minibatch_against_the_oracle(ctx, monkeypatch):
    """The same with batch_size = 8, seed = 9: the oracle's target is the restatement following the same call counter."""
    ref, target, o, g = _iteration_setup(8)
    assert not g._fast_path.eligible()
    counts = _count_calls(monkeypatch)
    hand._run_pair(monkeypatch, o, g, 5, fused=False)
    assert (counts["device"], counts["host"], counts["downloads"]) == (5, 0, 0), counts
    assert target.call_count == 5 and ref.call_count == 5
    monkeypatch.undo()
    # log_density_full: the full-data object's log_density by the kernel rule, and the counter stays
    full_ref = ref.full()
    x = (np.random.default_rng(4).normal(size=(65, 6)) * 0.5).astype(np.float32)
    lp64, g64 = full_ref.evaluate(x.astype(np.float64))
    lp32, g32 = cases.fp32_twin(full_ref).evaluate(x)
    lp_full = target.log_density_full(x).numpy()
    _check("log_density_full", lp_full, None, lp64, g64, lp32, g32)
    assert target.call_count == 5
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF
    same = DeviceDataLNPDF(cases.LOGIT_SRC, 6, ref.data, params=ref.params())
    np.testing.assert_array_equal(same.log_density(x).numpy(), lp_full)
    assert same.call_count == 0
    # an empty evaluation leaves the counter alone
    target.log_density(np.zeros((0, 6), np.float32))
    assert target.call_count == 5


def test_gradient_free_estimator_evaluates_values_only(ctx, monkeypatch):
    """Under MoreNgEstimator the target is asked for values alone: no call pays for the dual passes."""
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import MoreNgEstimator
    ref, target, _, _ = _iteration_setup(8)
    counts = _count_calls(monkeypatch)
    g = hand._build_one_component(target, 6, "MORE", False)
    assert type(g.ng_estimator) is MoreNgEstimator and g.ng_estimator.uses_target_gradients is False
    for _ in range(3):
        g.train_iter()
    assert counts["device"] == 3 and not any(counts["grads"]), counts
    assert target.call_count == 3
    assert int(g.sample_db.num_samples_written) == 3 * hand.E2E_SAMPLES
