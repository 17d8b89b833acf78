"""GPU tests of the predictive density of data-set device targets (the predictive kernels of csrc/custom_target_data.inc,
gmmvi_custom_data_predictive, ``log_predictive`` / ``waic`` / ``expensive_metrics`` of DeviceDataLNPDF and DeviceDataTapeLNPDF):
the kernels against fp64 at the seams of the 64-sample tile (the in-place finish against the merge kernel), of the four waves,
of the row chunks and of the staged route's cap; the edge values of include/gmmvi_hip.h; determinism, also across chunk requests;
both data modes; NULL outputs; the refused arguments; the classes; and the metrics in a GmmviRunner run.

Kernel bound: _bound of tests/test_hip_custom_target.py, unchanged: the device's largest error against the fp64 reference is at
most 16 times the largest error of the fp32 twin (tests/custom_predictive_cases.py) plus 4 eps32 max|reference|, for each of lpd,
mean and var over the entries whose reference is finite; entries with a non-finite reference are compared exactly.  Every case
prints device error, bound and ratio before it asserts.  tests/test_custom_predictive_host.py shows what that bound can see."""
import numpy as np
import pytest

import custom_predictive_cases as cases
import test_hip_custom_target as hand
from gmmvi_amd import _lib
from test_hip_custom_target import SENTINEL, _bound

pytestmark = pytest.mark.gpu

ERR_ARG = -2
OUTPUTS = ("lpd", "mean", "var")
KERNEL_CASES = cases.kernel_cases(_lib.CUSTOM_STAGED_MAX_DIM)
DENSITY_SRC = ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
               "    T s = 0.f; for (int i = 0; i < D; ++i) s -= 0.5f * x[i] * x[i]; return s; }\n")


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name, mode="data"):
    from gmmvi_amd import hip_ops
    if (name, mode) not in _handles:
        _handles[(name, mode)] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode=mode)
    return _handles[(name, mode)]


def _launch(ctx, handle, params, rows, x, chunks=0, want=(True, True)):
    """gmmvi_custom_data_predictive on outputs with CANARY_ROWS extra entries of SENTINEL behind them, which are checked here:
    bit-unchanged.  want: whether mean / var get a pointer.  -> (rc, [lpd, mean | None, var | None])."""
    n, d = x.shape
    m, c = rows.shape
    xd, pd, rd = ctx.asarray(x), ctx.asarray(np.asarray(params, np.float32)), ctx.asarray(np.asarray(rows, np.float32))
    outs = [ctx.full((m + hand.CANARY_ROWS,), SENTINEL) if w else None for w in (True,) + tuple(want)]
    rc = ctx.lib.gmmvi_custom_data_predictive(ctx.handle, handle.handle, d, pd.ptr, rd.ptr, m, c, xd.ptr, n,
                                              *[None if o is None else o.ptr for o in outs], chunks)
    if rc != 0:
        return rc, None
    bits = np.array(SENTINEL).view(np.uint32)
    host = []
    for o, name in zip(outs, OUTPUTS):
        if o is None:
            host.append(None)
            continue
        h = o.numpy()
        assert np.all(h[m:].view(np.uint32) == bits), f"{name} written past M"
        host.append(h[:m])
    return rc, host


def _check(tag, out, ref, twin, columns=None):
    for k, name in enumerate(OUTPUTS):
        if out[k] is None:
            continue
        pick = slice(None) if columns is None or k == 0 else columns
        e, b, r, exact = cases.compare(_bound, out[k][pick], ref[k][pick], twin[k][pick])
        print(f"\n[custom_predictive] {tag}: {name} error {e:.3e} (bound {b:.3e}, {e / b if b else 0:.3f} of it, ratio to the fp32 twin "
              f"{r:.2f})", end="")
        assert exact, f"{tag}: {name} differs where the reference is not finite"
        assert cases.within(e, b), f"{tag}: {name} error {e:.3e} > {b:.3e}"
    print()


@pytest.mark.parametrize("c", KERNEL_CASES, ids=cases.case_id)
def test_kernel_matches_fp64_reference(ctx, c):
    tgt, x = cases.build_case(c)
    _, _, ref, twin = cases.reference(c, tgt, x)
    rc, out = _launch(ctx, _handle(ctx, c.name), tgt.params(), tgt.data, x, c.chunks)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    assert all(np.all(np.isfinite(o)) for o in out)
    _check(cases.case_id(c), out, ref, twin)
    if c.n == 1:
        np.testing.assert_array_equal(out[2], np.zeros(c.m, np.float32))


def test_fault_table_cases_on_the_device(ctx):
    """The affine cases of the planted-fault table (l = 30 x0 - 300: the shift; l = 0.1 x0 - 1000: the centred variance)."""
    for tag, tgt, x in cases.fault_cases()[2:]:
        _, _, ref, twin = cases.reference(tag, tgt, x)
        rc, out = _launch(ctx, _handle(ctx, "affine"), tgt.params(), tgt.data, x)
        assert rc == 0
        _check(tag, out, ref, twin)


@pytest.mark.parametrize("e", cases.edge_cases(65), ids=lambda e: e.name)
def test_edge_values(ctx, e):
    x = np.zeros((len(e.x0), 2), np.float32)
    x[:, 0] = e.x0
    l64, l32 = cases.edge_matrix(e, np.float64), cases.edge_matrix(e, np.float32)
    ref, twin = cases.reference64(l64), cases.twin32(l32)
    rc, out = _launch(ctx, _handle(ctx, "affine"), [0.0], np.asarray(e.rows, np.float32), x)
    assert rc == 0
    for m, want in enumerate(e.lpd):
        if want is None:
            assert np.isfinite(out[0][m])
        elif np.isnan(want):
            assert np.isnan(out[0][m])
        else:
            assert out[0][m] == want
    # mean and var are promised only for columns of finite values
    _check(f"edge '{e.name}'", out, ref, twin, columns=np.all(np.isfinite(l64), axis=0))


SEAM = cases.Case("logit", 5, 130, 67, 0)


def test_same_call_twice_and_every_chunk_request_give_the_same_bits(ctx):
    tgt, x = cases.build_case(SEAM)
    handle = _handle(ctx, "logit")
    _, first = _launch(ctx, handle, tgt.params(), tgt.data, x, 1)
    for chunks in (1, 2, 3, 0):
        _, again = _launch(ctx, handle, tgt.params(), tgt.data, x, chunks)
        for a, b, name in zip(first, again, OUTPUTS):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{name}, chunk request {chunks}")


@pytest.mark.parametrize("c", [SEAM, cases.Case("student", 3, 64, 5, 0)], ids=cases.case_id)
def test_data_and_data_tape_handles_give_the_same_bits(ctx, c):
    tgt, x = cases.build_case(c)
    _, a = _launch(ctx, _handle(ctx, c.name, "data"), tgt.params(), tgt.data, x)
    rc, b = _launch(ctx, _handle(ctx, c.name, "data_tape"), tgt.params(), tgt.data, x)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("c", [SEAM, cases.Case("logit", 5, 63, 5, 0)], ids=cases.case_id)
def test_null_mean_and_var_leave_lpd_unchanged(ctx, c):
    tgt, x = cases.build_case(c)
    handle = _handle(ctx, c.name)
    _, full = _launch(ctx, handle, tgt.params(), tgt.data, x)
    for want in ((False, False), (True, False), (False, True)):
        rc, out = _launch(ctx, handle, tgt.params(), tgt.data, x, want=want)
        assert rc == 0
        for a, b in zip(full, out):
            if b is not None:
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_python_wrapper_gives_what_the_c_call_gives(ctx):
    from gmmvi_amd import hip_ops
    tgt, x = cases.build_case(SEAM)
    handle = _handle(ctx, "logit")
    _, want = _launch(ctx, handle, tgt.params(), tgt.data, x)
    got = hip_ops.custom_data_predictive(ctx, handle, ctx.asarray(tgt.params()), ctx.asarray(tgt.data), ctx.asarray(x))
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b.numpy())
    with pytest.raises(ValueError):
        hip_ops.custom_data_predictive(ctx, handle, None, ctx.asarray(tgt.data), ctx.asarray(x[:0]))


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_outputs_and_the_context_alone(ctx):
    from gmmvi_amd import hip_ops
    lib = ctx.lib
    c = cases.Case("logit", 5, 8, 9, 0)
    tgt, x = cases.build_case(c)
    handle = _handle(ctx, "logit")
    n, d, m, cols = 8, 5, 9, 6
    xd, pd, rd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    outs = [ctx.full((m,), SENTINEL) for _ in range(3)]

    def call(D=d, rows=rd.ptr, M=m, Cc=cols, X=xd.ptr, N=n, lpd=outs[0].ptr, h=handle.handle, chunks=0):
        return lib.gmmvi_custom_data_predictive(ctx.handle, h, D, pd.ptr, rows, M, Cc, X, N, lpd, outs[1].ptr, outs[2].ptr, chunks)

    def last():
        return lib.gmmvi_last_error(ctx.handle).decode()

    assert call(N=0) == ERR_ARG and "N = 0" in last()
    assert call(M=0) == ERR_ARG and "M = 0" in last()
    assert call(M=2 ** 31) == ERR_ARG and "2^31" in last()
    assert call(Cc=0) == ERR_ARG and "C = 0" in last()
    assert call(D=0) == ERR_ARG and "D = 0" in last()
    assert call(D=_lib.MAX_DIM_DIAG + 1) == ERR_ARG and str(_lib.MAX_DIM_DIAG) in last()
    for kw in (dict(rows=None), dict(X=None), dict(lpd=None), dict(h=None), dict(chunks=-1)):
        assert call(**kw) == ERR_ARG and last(), kw
    others = {"hand": hand._handle(ctx, "rosenbrock"),
              "autodiff": hip_ops.custom_target_compile(ctx, DENSITY_SRC, mode="autodiff"),
              "tape": hip_ops.custom_target_compile(ctx, DENSITY_SRC, mode="tape")}
    for mode, other in others.items():
        assert call(h=other.handle) == ERR_ARG and "gmmvi_custom_target_compile_data" in last(), mode
    ctx.check(lib.gmmvi_sync(ctx.handle))
    bits = np.array(SENTINEL).view(np.uint32)
    assert all(np.all(o.numpy().view(np.uint32) == bits) for o in outs)
    # the context works afterwards
    _, _, ref, twin = cases.reference(c, tgt, x)
    rc, out = _launch(ctx, handle, tgt.params(), tgt.data, x)
    assert rc == 0
    _check("after the refusals", out, ref, twin)


# ---- the classes -----------------------------------------------------------------------------------------------------------
T_ROWS, TEST_ROWS = 40, 7


def _class_setup(cls_name, batch_size=None, kw=lambda test: {}):
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    rng = np.random.default_rng(31)
    d = 5
    rows = np.concatenate([rng.normal(size=(T_ROWS + TEST_ROWS, d)) / np.sqrt(d),
                           rng.choice([-1.0, 1.0], size=(T_ROWS + TEST_ROWS, 1))], axis=1).astype(np.float32)
    train, test = rows[:T_ROWS], rows[T_ROWS:]
    params = [0.25, 2.0]
    target = getattr(device_lnpdf, cls_name)(cases.SOURCES["logit"], d, train, params=params, batch_size=batch_size, seed=9, **kw(test))
    x = (rng.normal(size=(130, d)) * 0.7).astype(np.float32)
    return target, cases.CLASSES["logit"](train, params), test, x


@pytest.mark.parametrize("cls_name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_class_methods_and_metrics(ctx, cls_name):
    from gmmvi_amd import hip_ops
    target, ref_tgt, test, x = _class_setup(cls_name, batch_size=8, kw=lambda t: dict(eval_sets={"test": t}, report_waic=True))
    assert target.call_count == 0
    twin_tgt = cases.data_cases.fp32_twin(ref_tgt)
    l64, l32 = cases.row_terms(ref_tgt, x.astype(np.float64)), cases.row_terms(twin_tgt, x)
    ref, twin = cases.reference64(l64), cases.twin32(l32)
    # rows=None is the training data on the device
    none = [o.numpy() for o in target.log_predictive(x)]
    given = [o.numpy() for o in target.log_predictive(x, ref_tgt.data)]
    for a, b in zip(none, given):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    _check(f"{cls_name}.log_predictive", none, ref, twin)
    # WAIC: the fp64 sums, within the per-row bound scaled by T
    waic = target.waic(x)
    assert set(waic) == {"lppd", "p_waic", "elpd_waic"}
    b_lpd = cases.compare(_bound, twin[0], ref[0], twin[0])[1]
    b_var = cases.compare(_bound, twin[2], ref[2], twin[2])[1]
    want = {"lppd": ref[0].sum(), "p_waic": ref[2].sum()}
    want["elpd_waic"] = want["lppd"] - want["p_waic"]
    bounds = {"lppd": T_ROWS * b_lpd, "p_waic": T_ROWS * b_var, "elpd_waic": T_ROWS * (b_lpd + b_var)}
    for key in want:
        err = abs(waic[key] - want[key])
        print(f"[custom_predictive] {cls_name}.waic {key}: {waic[key]:.6f}, fp64 {want[key]:.6f}, error {err:.3e} (bound {bounds[key]:.3e})")
        assert err <= bounds[key]
    # the metrics: exactly the five keys
    t64, t32 = cases.row_terms(ref_tgt, x.astype(np.float64), test), cases.row_terms(twin_tgt, x, test)
    t_ref, t_twin = cases.reference64(t64), cases.twin32(t32)
    metrics = target.expensive_metrics(None, ctx.asarray(x))
    assert set(metrics) == {"test_lpd", "test_mean_ll", "lppd", "p_waic", "elpd_waic"}
    for key, k in (("test_lpd", 0), ("test_mean_ll", 1)):
        bound = cases.compare(_bound, t_twin[k], t_ref[k], t_twin[k])[1]
        err = abs(metrics[key] - t_ref[k].mean())
        print(f"[custom_predictive] {cls_name} {key}: {metrics[key]:.6f}, fp64 {t_ref[k].mean():.6f}, error {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    for key in want:
        assert metrics[key] == waic[key]
    lpd_test = target.log_predictive(x, test)[0].numpy()
    assert metrics["test_lpd"] == float(np.mean(lpd_test, dtype=np.float64))
    assert target.call_count == 0                          # none of this advanced the minibatch stream
    target.log_density(x)
    assert target.call_count == 1
    for bad in (np.zeros(6), np.zeros((3, 5)), np.zeros((0, 6))):
        with pytest.raises(ValueError, match="rows"):
            target.log_predictive(x, bad)


def test_target_without_the_keywords_reports_nothing(ctx):
    target, _, _, x = _class_setup("DeviceDataLNPDF", kw=lambda t: {})
    assert target.expensive_metrics(None, ctx.asarray(x)) == {}


def test_runner_logs_the_held_out_density(ctx):
    """GmmviRunner, diagonal model, Stein estimator, the logit target with a test set, 2 iterations, metrics at every one."""
    from gmmvi_amd.configs import get_default_algorithm_config, update_config
    from gmmvi_amd.gmmvi_runner import GmmviRunner
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import SteinNgEstimator
    target, _, _, _ = _class_setup("DeviceDataLNPDF", kw=lambda t: dict(eval_sets={"test": t}))
    cfg = update_config(get_default_algorithm_config("SAMTRON"), {
        "start_seed": 3, "temperature": 1., "use_sample_database": True, "max_database_size": 100000,
        "model_initialization": {"use_diagonal_covs": True, "num_initial_components": 2, "prior_mean": 0., "prior_scale": 1.,
                                 "initial_cov": 1.},
        "sample_selector_config": {"desired_samples_per_component": 40},
        "gmmvi_runner_config": {"log_metrics_interval": 1}})
    cfg["target_fn"] = target
    runner = GmmviRunner.build_from_config(cfg)
    assert runner.gmmvi.sample_selector.target_distribution is target and runner.gmmvi.model.diagonal_covs
    assert isinstance(runner.gmmvi.ng_estimator, SteinNgEstimator)
    for n in range(2):
        metrics = runner.iterate_and_log(n)
        assert "test_lpd" in metrics and "test_mean_ll" in metrics, sorted(metrics)
        assert np.isfinite(metrics["test_lpd"]) and np.isfinite(metrics["test_mean_ll"])
        assert metrics["test_lpd"] >= metrics["test_mean_ll"]             # Jensen
        assert "lppd" not in metrics
    runner.finalize()
