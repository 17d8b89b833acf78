"""GPU tests of the special functions of user-defined device targets (csrc/custom_target_special.inc and their rules in
csrc/custom_target_autodiff.inc and csrc/custom_target_tape.inc): every function pointwise through DeviceAutodiffLNPDF's and
DeviceTapeLNPDF's kernels on the grid of tests/test_custom_special_host.py against SciPy in fp64; the ``specials`` density at the
seams of the 64-sample tile in both modes; ``negbin`` and ``erfmix`` through both data classes at the seams of the tile, the row
chunks and the minibatch stream, and with own batches; and ``negbin`` in the modular iteration with its held-out predictive
density.  Every launch goes through the _launch helpers of the existing test files, which check that nothing is written past N.

Pointwise bound: twice the host bound of the same function (value_bound and partial_bound of tests/test_custom_special_host.py):
the device's expf, log1pf, erfcf and lgammaf are ROCm's, which are specified more loosely than glibc's.  ROCm's own lgammaf, erff
and erfcf are evaluated on the same grid by a hand-written-mode target; where one of them alone exceeds that bound, the
function's value bound is ROCM_VALUE_ULPS ulp, twice the worst error measured on ROCm's own function.
Kernel bound of the densities: the rule of tests/test_hip_custom_target.py, unchanged (its _bound).  Every case prints its
figures before it asserts."""
import numpy as np
import pytest

import custom_predictive_cases as pred
import custom_special_cases as cases
import test_custom_autodiff_host as fwd
import test_custom_special_host as host
import test_hip_custom_data as data_mode
import test_hip_custom_data_own as own_mode
import test_hip_custom_data_tape as tape_mode
import test_hip_custom_predictive as pred_mode
import test_hip_custom_tape as tape
import test_hip_custom_target as hand
from custom_data_own_cases import OwnBatches
from gmmvi_amd import _lib
from helpers import samtron_config
from oracle import train as otrain
from test_hip_custom_target import _bound

pytestmark = pytest.mark.gpu

f32 = np.float32
NO_PARAMS = np.zeros(1, np.float32)
# function -> the value bound in ulp where ROCm's own float function alone exceeds twice the host bound (none measured so far)
ROCM_VALUE_ULPS = {}


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


# ---- 1. pointwise -----------------------------------------------------------------------------------------------------------------
def _density_source(op):
    rule, form = cases.split(op)
    name = cases.source_name(op[:-3] if form != "tt" else op)
    args = {"tt": "x[0], x[1]", "tf": "x[0], gmmvi_value(x[1])", "ft": "gmmvi_value(x[0]), x[1]"}[form] if rule == "logaddexp" else "x[0]"
    return ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
            f"    return {name}({args});\n}}\n")


def _float_source(fn):
    """A hand-written-mode target that calls the float function directly."""
    return ("__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {\n"
            f"    if (grad) grad[0] = 0.f;\n    return {fn}(x[0]);\n}}\n")


def _grid(op):
    """-> x [N, 1 or 2] fp32: the grid of the host test; N crosses the 64-sample tile."""
    rule, _ = cases.split(op)
    pairs = host._operands(op)
    x = np.array([[a, b] for a, b in pairs] if rule == "logaddexp" else [[a] for a, _ in pairs], np.float32)
    assert x.shape[0] > 64
    return x


def _value_bounds(op, x, want):
    rule, _ = cases.split(op)
    out = np.empty(len(want))
    for i, w in enumerate(want):
        b = host.value_bound(op, w, x[i, 0], x[i, -1])
        if b is not None and rule in ROCM_VALUE_ULPS:
            b = ROCM_VALUE_ULPS[rule] * float(np.spacing(np.abs(f32(w))))
        out[i] = np.inf if b is None else (b if rule in ROCM_VALUE_ULPS else 2.0 * b)
    return out


POINTWISE_OPS = [op for op in _lib.SPECIAL_OPS if op != "trigamma"]


@pytest.mark.parametrize("op", POINTWISE_OPS)
def test_pointwise_against_fp64(ctx, op):
    from gmmvi_amd import hip_ops
    rule, form = cases.split(op)
    x = _grid(op)
    n, d = x.shape
    wants = [host._want(op, x[i, 0], x[i, -1]) for i in range(n)]
    want = np.array([w[0] for w in wants])
    want_p = np.array([[w[1], w[2]][:d] for w in wants])
    vb = _value_bounds(op, x, want)
    pb = 2.0 * np.array([[host.partial_bound(op, p) for p in row] for row in want_p])
    source = _density_source(op)
    values = {}
    for mode, launch in (("autodiff", lambda h, g: hand._launch(ctx, h, NO_PARAMS, x, g, 0)),
                         ("tape", lambda h, g: tape._launch(ctx, h, NO_PARAMS, x, g))):
        handle = hip_ops.custom_target_compile(ctx, source, mode=mode)
        rc, lp, grad = launch(handle, True)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        rc, lp_v, _ = launch(handle, False)
        assert rc == 0
        e_v = np.abs(lp.astype(np.float64) - want)
        e_p = np.abs(grad.astype(np.float64) - want_p)
        with np.errstate(all="ignore"):
            r_v = np.where(np.isfinite(vb), e_v / np.where(vb > 0, vb, 1.0), 0.0)
            r_p = np.where(pb > 0, e_p / np.where(pb > 0, pb, 1.0), np.where(e_p == 0, 0.0, np.inf))
        print(f"\n[custom_special] {mode} {op}: worst value error {r_v.max():.3f} of its bound (at x = {x[r_v.argmax()]}), worst "
              f"gradient error {r_p.max():.3f} of its bound (at x = {x[r_p.max(axis=1).argmax()]})")
        at = int(r_v.argmax())
        assert r_v.max() <= 1.0, f"{mode} {op}({x[at]}): value {lp[at]!r}, SciPy fp64 {want[at]!r}, error {e_v[at]:.3e} > {vb[at]:.3e}"
        at = int(r_p.max(axis=1).argmax())
        assert r_p.max() <= 1.0, f"{mode} {op}({x[at]}): gradient {grad[at]!r}, closed form {want_p[at]!r}, bound {pb[at]!r}"
        # the value call (T = float) and the gradient call give the same bits
        np.testing.assert_array_equal(lp.view(np.uint32), lp_v.view(np.uint32))
        values[mode] = lp
    np.testing.assert_array_equal(values["autodiff"].view(np.uint32), values["tape"].view(np.uint32))
    if rule in ("lgamma", "erf", "erfc"):
        # ROCm's own float function on the same grid, by the hand-written mode: the same bits, and its own error
        rc, rocm, _ = hand._launch(ctx, hip_ops.custom_target_compile(ctx, _float_source(rule + "f")), NO_PARAMS, x, False, 0)
        assert rc == 0
        ulps = np.abs(rocm.astype(np.float64) - want) / np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
        print(f"[custom_special] ROCm's {rule}f alone: worst error {ulps.max():.2f} ulp (at x = {x[ulps.argmax(), 0]!r}; bound "
              f"{ROCM_VALUE_ULPS.get(rule, 8.0)} ulp)")
        np.testing.assert_array_equal(values["autodiff"].view(np.uint32), rocm.view(np.uint32))


def test_trigamma_pointwise_in_the_hand_written_mode(ctx):
    """gmmvi_trigamma is a float function only: a hand-written-mode target calls it, as it may call all six."""
    from gmmvi_amd import hip_ops
    x = _grid("trigamma")
    want = np.array([host._want("trigamma", a, 0.0)[0] for a in x[:, 0]])
    bound = 2.0 * np.array([host.value_bound("trigamma", w, 0.0, 0.0) for w in want])
    rc, lp, _ = hand._launch(ctx, hip_ops.custom_target_compile(ctx, _float_source("gmmvi_trigamma")), NO_PARAMS, x, False, 0)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    ratio = np.abs(lp.astype(np.float64) - want) / bound
    print(f"\n[custom_special] hand-written gmmvi_trigamma: worst value error {ratio.max():.3f} of its bound (at x = {x[ratio.argmax(), 0]!r})")
    assert ratio.max() <= 1.0


# ---- 2. specials ------------------------------------------------------------------------------------------------------------------------
_specials = {}


def _specials_reference(n):
    if n not in _specials:
        tgt, x = cases.build_specials(n)
        lp64, g64 = tgt.log_density_and_grad(x.astype(np.float64))
        lp32, g32 = tgt.as_dtype(np.float32).log_density_and_grad(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _specials[n] = (tgt, x, lp64, g64, lp32, g32)
    return _specials[n]


def _check(tag, lp, g, lp64, g64, lp32, g32):
    e_lp, b_lp, r_lp = _bound(lp, lp64, lp32)
    line = f"[custom_special] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
    if g is not None:
        e_g, b_g, r_g = _bound(g, g64, g32)
        line += f", gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})"
    print("\n" + line)
    assert np.all(np.isfinite(lp)) and (g is None or np.all(np.isfinite(g)))
    assert e_lp <= b_lp, f"{tag}: lp error {e_lp:.3e} > {b_lp:.3e}"
    if g is not None:
        assert e_g <= b_g, f"{tag}: gradient error {e_g:.3e} > {b_g:.3e}"


_density_handles = {}


@pytest.mark.parametrize("n", [1, 64, 65, 200])
@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_specials_density_matches_fp64_reference(ctx, mode, n):
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = _specials_reference(n)
    if mode not in _density_handles:
        _density_handles[mode] = hip_ops.custom_target_compile(ctx, cases.SPECIALS_SRC, mode=mode)
    handle = _density_handles[mode]
    for want_grad in (True, False):
        if mode == "autodiff":
            rc, lp, g = hand._launch(ctx, handle, tgt.params(), x, want_grad, 0)
        else:
            rc, lp, g = tape._launch(ctx, handle, tgt.params(), x, want_grad)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        _check(f"specials {mode} N={n}" + ("" if want_grad else " values only"), lp, g, lp64, g64, lp32, g32)


# ---- 3. negbin and erfmix -----------------------------------------------------------------------------------------------------------------
_data_handles = {}


def _data_handle(ctx, kind, name):
    from gmmvi_amd import hip_ops
    if (kind, name) not in _data_handles:
        _data_handles[(kind, name)] = hip_ops.custom_target_compile(ctx, cases.DATA_SOURCES[name],
                                                                    mode="data_tape" if kind == "tape" else "data")
    return _data_handles[(kind, name)]


@pytest.mark.parametrize("c", cases.data_kernel_cases(), ids=cases.case_id)
def test_data_kernels_match_fp64_reference(ctx, c):
    tgt, x, lp64, g64, lp32, g32 = cases.data_reference(c)
    out = {}
    for kind, mod in (("data", data_mode), ("tape", tape_mode)):
        handle = _data_handle(ctx, kind, c.name)
        rc, lp, g = mod._launch(ctx, handle, tgt, x, True, c.chunks)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        _check(f"{kind} {cases.case_id(c)}", lp, g, lp64, g64, lp32, g32)
        rc, lp_v, g_v = mod._launch(ctx, handle, tgt, x, False, c.chunks)
        assert rc == 0 and g_v is None
        _check(f"{kind} {cases.case_id(c)} values only", lp_v, None, lp64, g64, lp32, g32)
        out[kind] = (lp, g)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    d_lp = float(np.abs(out["data"][0].astype(np.float64) - out["tape"][0]).max())
    d_g = float(np.abs(out["data"][1].astype(np.float64) - out["tape"][1]).max())
    print(f"[custom_special] {cases.case_id(c)} forward against reverse: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), the "
          f"gradient by {d_g:.3e} ({d_g / b_g:.3f})")
    assert d_lp <= b_lp and d_g <= b_g


@pytest.mark.parametrize("name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_negbin_with_own_batches(ctx, name):
    """use_own_batch_per_sample=True at T = 67, B = 5 against the per-sample restatement of tests/custom_data_own_cases.py."""
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    c = cases.Case("negbin", 4, 65, 67, 0, 5, 0)
    tgt, x = cases.build_data_case(c)
    own = OwnBatches(tgt)
    lp64, g64 = own.evaluate(x.astype(np.float64))
    lp32, g32 = own.as_dtype(np.float32).evaluate(x)
    target = getattr(device_lnpdf, name)(cases.NEGBIN_SRC, c.d, tgt.data, params=tgt.params(), batch_size=5, seed=cases.MINIBATCH_SEED,
                                         use_own_batch_per_sample=True)
    lp, g = (a.numpy() for a in target.log_density_and_grad(x))
    _check(f"{name} negbin, own batches", lp, g, lp64, g64, lp32, g32)
    assert target.call_count == 1
    # and through the C entry, with the rows behind N checked
    kind = "tape" if name == "DeviceDataTapeLNPDF" else "data"
    rc, lp_c, g_c = own_mode._launch(ctx, kind, _data_handle(ctx, kind, "negbin"), own, x, True)
    assert rc == 0
    np.testing.assert_array_equal(lp_c.view(np.uint32), lp.view(np.uint32))
    np.testing.assert_array_equal(g_c.view(np.uint32), g.view(np.uint32))


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------------
T_ROWS, TEST_ROWS, E2E_D = 40, 5, 4


def _negbin_rows(rng, t, d):
    features = rng.normal(size=(t, d - 1)) / np.sqrt(d)
    return np.concatenate([features, rng.negative_binomial(2.0, 0.4, size=(t, 1))], axis=1).astype(np.float32)


def _diagonal_pair(name, rows, batch_size):
    """The set-up of _diagonal_pair of tests/test_hip_custom_data_tape.py (a diagonal-covariance model, the Stein estimator, the KL
    trust region, K = 3, 40 samples per component) on negbin over ``rows`` with the class ``name``."""
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    d, k, s, seed = E2E_D, 3, 40, 11
    cfg = samtron_config(s, diag=True)
    ref = cases.NegBin(rows, [0.25, 2.0], batch_size=batch_size, seed=9, d=d)
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
    target = getattr(device_lnpdf, name)(cases.NEGBIN_SRC, d, rows, params=ref.params(), batch_size=batch_size, seed=9)
    g = GMMVI.build_from_config(c, target, wrapper)
    assert g.model.diagonal_covs and g.sample_db.diagonal_covariances and not g._fast_path.eligible()
    return ref, target, o, g


@pytest.mark.parametrize("name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_diagonal_stein_iteration_on_negbin(ctx, name):
    """negbin at D = 4, T = 40, B = 8, K = 3: three iterations against the fp64 oracle on the restatement at the same calls, under the
    tolerance rule of tests/test_hip_custom_data_tape.py (its _follow); then log_predictive on 5 held-out rows."""
    rows = _negbin_rows(np.random.default_rng(17), T_ROWS + TEST_ROWS, E2E_D)
    train, test = rows[:T_ROWS], rows[T_ROWS:]
    ref, target, o, g = _diagonal_pair(name, train, 8)

    def each(it):
        assert target.call_count == it + 1 == ref.call_count

    tape_mode._follow(o, g, 3, E2E_D, each)
    x = (np.random.default_rng(4).normal(size=(130, E2E_D)) * 0.5).astype(np.float32)
    full = ref.full()
    l64, l32 = pred.row_terms(full, x.astype(np.float64), test), pred.row_terms(cases.fp32_twin(full), x, test)
    out = [a.numpy() for a in target.log_predictive(x, test)]
    assert out[0].shape == (TEST_ROWS,)
    pred_mode._check(f"{name}.log_predictive on negbin", out, pred.reference64(l64), pred.twin32(l32))
    assert target.call_count == 3
