"""GPU tests of gmmvi_erfcx, gmmvi_ndtr, gmmvi_log_ndtr and sinh, cosh, asin, acos of user-defined device targets
(csrc/custom_target_special.inc and their rules in csrc/custom_target_autodiff.inc and csrc/custom_target_tape.inc): every function
pointwise through DeviceAutodiffLNPDF's and DeviceTapeLNPDF's kernels on the grids of tests/custom_normal_cases.py against SciPy in
fp64; the ``normals`` density at the seams of the 64-sample tile in both modes; ``probit`` (with its planted row at a signed
predictor of -20) and ``tobit`` through both data classes at the seams of the tile, the row chunks and the minibatch stream; the
plain form log(erfc / 2) on the same probit data, which is not finite there; ``probit`` with own batches; and ``probit`` in the
modular iteration with its held-out predictive density.  Every launch goes through the _launch helpers of the existing test
files, which check that nothing is written past N.

Pointwise bound: twice the host bound of the same function (value_bound and partial_bound of tests/test_custom_normal_host.py):
the device's expf, logf, log1pf, sinhf, coshf, asinf and acosf are ROCm's, which are specified more loosely than glibc's.  ROCm's
own erfcf, expf, sinhf, coshf, asinf and acosf are evaluated alone on the same grids by a hand-written-mode target and printed;
where one of them alone exceeds twice the host bound, the value bound of the function built on it is ROCM_VALUE_ULPS ulp, twice the
worst error measured on ROCm's own function.  Kernel bound of the densities: the rule of
tests/test_hip_custom_target.py, unchanged (its _bound).  Every case prints its figures before it asserts."""
import numpy as np
import pytest
from scipy import special as sp

import custom_normal_cases as cases
import custom_predictive_cases as pred
import test_custom_normal_host as host
import test_hip_custom_data as data_mode
import test_hip_custom_data_own as own_mode
import test_hip_custom_data_tape as tape_mode
import test_hip_custom_predictive as pred_mode
import test_hip_custom_special as special_gpu
import test_hip_custom_tape as tape
import test_hip_custom_target as hand
from custom_data_own_cases import OwnBatches
from gmmvi_amd import _lib
from helpers import samtron_config
from oracle import train as otrain
from test_hip_custom_special import _check
from test_hip_custom_target import _bound

pytestmark = pytest.mark.gpu

f32 = np.float32
NO_PARAMS = np.zeros(1, np.float32)
# function -> the value bound in ulp where ROCm's own float function alone exceeds twice the host bound.  None does: measured on
# these grids, erfcf 1.35, expf 0.65, sinhf 0.54, coshf 0.51, asinf 1.90 and acosf 1.01 ulp (test_rocm_functions_alone prints them)
ROCM_VALUE_ULPS = {}
# ROCm's own functions: name -> (fp64 reference, grid)
ROCM_FUNCTIONS = {
    "erfcf": (sp.erfc, cases.ERFCX_GRID), "expf": (np.exp, cases.HYPERBOLIC_GRID), "sinhf": (np.sinh, cases.HYPERBOLIC_GRID),
    "coshf": (np.cosh, cases.HYPERBOLIC_GRID), "asinf": (np.arcsin, cases.ARC_GRID), "acosf": (np.arccos, cases.ARC_GRID),
}


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


# ---- 1. pointwise -----------------------------------------------------------------------------------------------------------------
def _density_source(op):
    return ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
            f"    return {cases.source_name(op)}(x[0]);\n}}\n")


def _ratios(got, want, bounds):
    return np.array([host.error_ratio(g, w, b) for g, w, b in zip(got, want, bounds)])


@pytest.mark.parametrize("op", _lib.EXTRA_OPS)
def test_pointwise_against_fp64(ctx, op):
    from gmmvi_amd import hip_ops
    rule = cases.rule_of(op)
    x = cases.unary_grid(rule).reshape(-1, 1)
    n = x.shape[0]
    assert n > 64
    wants = [host._want(op, a) for a in x[:, 0]]
    want, want_p = np.array([w[0] for w in wants]), np.array([w[1] for w in wants])
    vb = []
    for w in want:
        b = host.value_bound(op, w)
        if b is not None:
            b = ROCM_VALUE_ULPS[rule] / (8.0 if rule in cases.NORMAL_FAMILY else 4.0) * b if rule in ROCM_VALUE_ULPS else 2.0 * b
        vb.append(b)
    pb = [2.0 * host.partial_bound(op, p) for p in want_p]
    source = _density_source(op)
    values = {}
    for mode, launch in (("autodiff", lambda h, g: hand._launch(ctx, h, NO_PARAMS, x, g, 0)),
                         ("tape", lambda h, g: tape._launch(ctx, h, NO_PARAMS, x, g))):
        handle = hip_ops.custom_target_compile(ctx, source, mode=mode)
        rc, lp, grad = launch(handle, True)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        rc, lp_v, _ = launch(handle, False)
        assert rc == 0
        r_v, r_p = _ratios(lp, want, vb), _ratios(grad[:, 0], want_p, pb)
        shown = np.where(np.abs(want_p) >= host.NORMAL_CUT, r_p, 0.0)
        print(f"\n[custom_normal] {mode} {op}: worst value error {r_v.max():.3f} of its bound (at x = {x[r_v.argmax(), 0]!r}), worst "
              f"gradient error {shown.max():.3f} of its bound (at x = {x[shown.argmax(), 0]!r}; over partials of at least 1e-37)")
        at = int(r_v.argmax())
        assert r_v.max() <= 1.0, f"{mode} {op}({x[at, 0]!r}): value {lp[at]!r}, SciPy fp64 {want[at]!r}, bound {vb[at]!r}"
        at = int(r_p.argmax())
        assert r_p.max() <= 1.0, f"{mode} {op}({x[at, 0]!r}): gradient {grad[at, 0]!r}, closed form {want_p[at]!r}, bound {pb[at]!r}"
        # the value call (T = float) and the gradient call give the same bits
        np.testing.assert_array_equal(lp.view(np.uint32), lp_v.view(np.uint32))
        values[mode] = lp
    np.testing.assert_array_equal(values["autodiff"].view(np.uint32), values["tape"].view(np.uint32))
    if rule not in cases.NORMAL_FAMILY:
        # ROCm's own float function on the same grid, by the hand-written mode: the same bits
        rc, rocm, _ = hand._launch(ctx, hip_ops.custom_target_compile(ctx, special_gpu._float_source(rule + "f")), NO_PARAMS, x, False, 0)
        assert rc == 0
        np.testing.assert_array_equal(values["autodiff"].view(np.uint32), rocm.view(np.uint32))
    else:
        # the float function called by a hand-written target: the same bits
        rc, own, _ = hand._launch(ctx, hip_ops.custom_target_compile(ctx, special_gpu._float_source("gmmvi_" + rule)), NO_PARAMS, x, False, 0)
        assert rc == 0
        np.testing.assert_array_equal(values["autodiff"].view(np.uint32), own.view(np.uint32))


@pytest.mark.parametrize("fn", sorted(ROCM_FUNCTIONS))
def test_rocm_functions_alone(ctx, fn):
    """ROCm's own erfcf, expf, sinhf, coshf, asinf, acosf on the grids of the functions next to them, over results inside fp32's
    normal range: a measurement, printed for DESIGN.md section 6.  What is held to a bound is the library's functions
    (test_pointwise_against_fp64, which also finds sinhf, coshf, asinf and acosf bit for bit behind sinh, cosh, asin and acos);
    gmmvi_erfcx, gmmvi_ndtr and gmmvi_log_ndtr call expf, logf and log1pf only."""
    from gmmvi_amd import hip_ops
    reference, grid = ROCM_FUNCTIONS[fn]
    x = grid.reshape(-1, 1)
    rc, got, _ = hand._launch(ctx, hip_ops.custom_target_compile(ctx, special_gpu._float_source(fn)), NO_PARAMS, x, False, 0)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    with np.errstate(all="ignore"):
        want = reference(x[:, 0].astype(np.float64))
    inside = (np.abs(want) > host.NORMAL_CUT) & (np.abs(want) < host.FLT_MAX)
    assert inside.sum() > 64 and np.all(np.isfinite(got[inside]))
    ulps = np.abs(got.astype(np.float64) - want)[inside] / np.spacing(np.abs(want[inside].astype(np.float32))).astype(np.float64)
    print(f"\n[custom_normal] ROCm's {fn} alone: worst error {ulps.max():.2f} ulp (at x = {x[inside][ulps.argmax(), 0]!r}, over "
          f"{int(inside.sum())} results inside fp32's normal range)")


# ---- 2. normals ---------------------------------------------------------------------------------------------------------------------------
_normals = {}


def _normals_reference(n):
    if n not in _normals:
        tgt, x = cases.build_normals(n)
        lp64, g64 = tgt.log_density_and_grad(x.astype(np.float64))
        lp32, g32 = tgt.as_dtype(np.float32).log_density_and_grad(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        _normals[n] = (tgt, x, lp64, g64, lp32, g32)
    return _normals[n]


_density_handles = {}


@pytest.mark.parametrize("n", [1, 64, 65, 200])
@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_normals_density_matches_fp64_reference(ctx, mode, n):
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = _normals_reference(n)
    if mode not in _density_handles:
        _density_handles[mode] = hip_ops.custom_target_compile(ctx, cases.NORMALS_SRC, mode=mode)
    handle = _density_handles[mode]
    for want_grad in (True, False):
        if mode == "autodiff":
            rc, lp, g = hand._launch(ctx, handle, tgt.params(), x, want_grad, 0)
        else:
            rc, lp, g = tape._launch(ctx, handle, tgt.params(), x, want_grad)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        _check(f"normals {mode} N={n}" + ("" if want_grad else " values only"), lp, g, lp64, g64, lp32, g32)


# ---- 3. probit and tobit ------------------------------------------------------------------------------------------------------------------
_data_handles = {}


def _data_handle(ctx, kind, name, source=None):
    from gmmvi_amd import hip_ops
    if (kind, name) not in _data_handles:
        _data_handles[(kind, name)] = hip_ops.custom_target_compile(ctx, source or cases.DATA_SOURCES[name],
                                                                    mode="data_tape" if kind == "tape" else "data")
    return _data_handles[(kind, name)]


@pytest.mark.parametrize("c", cases.data_kernel_cases(), ids=cases.case_id)
def test_data_kernels_match_fp64_reference(ctx, c):
    tgt, x, lp64, g64, lp32, g32 = cases.data_reference(c)
    assert np.all(np.isfinite(lp64)) and np.all(np.isfinite(g64))
    out = {}
    for kind, mod in (("data", data_mode), ("tape", tape_mode)):
        handle = _data_handle(ctx, kind, c.name)
        rc, lp, g = mod._launch(ctx, handle, tgt, x, True, c.chunks)
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        _check(f"{kind} {cases.case_id(c)}", lp, g, lp64, g64, lp32, g32)                 # (finite, and within the bound)
        rc, lp_v, g_v = mod._launch(ctx, handle, tgt, x, False, c.chunks)
        assert rc == 0 and g_v is None
        _check(f"{kind} {cases.case_id(c)} values only", lp_v, None, lp64, g64, lp32, g32)
        out[kind] = (lp, g)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    d_lp = float(np.abs(out["data"][0].astype(np.float64) - out["tape"][0]).max())
    d_g = float(np.abs(out["data"][1].astype(np.float64) - out["tape"][1]).max())
    print(f"[custom_normal] {cases.case_id(c)} forward against reverse: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), the "
          f"gradient by {d_g:.3e} ({d_g / b_g:.3f})")
    assert d_lp <= b_lp and d_g <= b_g


def test_the_plain_form_is_not_finite_on_the_planted_row(ctx):
    """The full-data probit case N = 65, T = 67 with log(0.5f * erfc(...)) in place of gmmvi_log_ndtr: erfcf has underflowed at the
    planted row's predictor of -20, the logarithm is -inf and sample 0's density with it, where gmmvi_log_ndtr is within its bound
    (test_data_kernels_match_fp64_reference).  Only the evaluation is non-finite: the launch succeeds."""
    c = cases.Case("probit", 4, 65, 67, 3, None, 0)
    assert c in cases.data_kernel_cases()
    tgt, x, lp64, _, _, _ = cases.data_reference(c)
    assert abs(float(tgt.data[0, :-1].astype(np.float64) @ x[0].astype(np.float64)) - cases.PLANTED_ETA) < 1e-4
    rc, plain, g_plain = data_mode._launch(ctx, _data_handle(ctx, "data", "probit_plain", cases.PROBIT_PLAIN_SRC), tgt, x, True, c.chunks)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    rc, lp, g = data_mode._launch(ctx, _data_handle(ctx, "data", "probit"), tgt, x, True, c.chunks)
    assert rc == 0
    print(f"\n[custom_normal] probit sample 0: fp64 {lp64[0]!r}, gmmvi_log_ndtr {lp[0]!r}, log(0.5f * erfc(.)) {plain[0]!r} with gradient "
          f"{g_plain[0]!r}; samples with a non-finite plain form: {int((~np.isfinite(plain)).sum())} of {len(plain)}")
    assert not np.isfinite(plain[0])
    assert np.isfinite(lp[0]) and np.all(np.isfinite(g[0]))


@pytest.mark.parametrize("name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_probit_with_own_batches(ctx, name):
    """use_own_batch_per_sample=True at T = 67, B = 5 against the per-sample restatement of tests/custom_data_own_cases.py."""
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    c = cases.Case("probit", 4, 65, 67, 0, 5, 0)
    tgt, x = cases.build_data_case(c)
    own = OwnBatches(tgt)
    lp64, g64 = own.evaluate(x.astype(np.float64))
    lp32, g32 = own.as_dtype(np.float32).evaluate(x)
    target = getattr(device_lnpdf, name)(cases.PROBIT_SRC, c.d, tgt.data, params=tgt.params(), batch_size=5, seed=cases.MINIBATCH_SEED,
                                         use_own_batch_per_sample=True)
    lp, g = (a.numpy() for a in target.log_density_and_grad(x))
    _check(f"{name} probit, own batches", lp, g, lp64, g64, lp32, g32)
    assert target.call_count == 1
    # and through the C entry, with the rows behind N checked
    kind = "tape" if name == "DeviceDataTapeLNPDF" else "data"
    rc, lp_c, g_c = own_mode._launch(ctx, kind, _data_handle(ctx, kind, "probit"), own, x, True)
    assert rc == 0
    np.testing.assert_array_equal(lp_c.view(np.uint32), lp.view(np.uint32))
    np.testing.assert_array_equal(g_c.view(np.uint32), g.view(np.uint32))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
T_ROWS, TEST_ROWS, E2E_D = 40, 5, 4


def _probit_rows(rng, t, d):
    features = rng.normal(size=(t, d)) / np.sqrt(d)
    labels = (features @ np.array([1.5, -1.0, 0.5, 2.0])[:d] + rng.normal(size=t) > 0).astype(np.float64)
    return np.concatenate([features, labels[:, None]], axis=1).astype(np.float32)


def _diagonal_pair(name, rows, batch_size):
    """The set-up of _diagonal_pair of tests/test_hip_custom_special.py (a diagonal-covariance model, the Stein estimator, the KL
    trust region, K = 3, 40 samples per component) on probit over ``rows`` with the class ``name``."""
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    d, k, s, seed = E2E_D, 3, 40, 11
    cfg = samtron_config(s, diag=True)
    ref = cases.Probit(rows, [0.25, 2.0], batch_size=batch_size, seed=9, d=d)
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
    target = getattr(device_lnpdf, name)(cases.PROBIT_SRC, d, rows, params=ref.params(), batch_size=batch_size, seed=9)
    g = GMMVI.build_from_config(c, target, wrapper)
    assert g.model.diagonal_covs and g.sample_db.diagonal_covariances and not g._fast_path.eligible()
    return ref, target, o, g


@pytest.mark.parametrize("name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_diagonal_stein_iteration_on_probit(ctx, name):
    """probit at D = 4, T = 40, B = 8, K = 3: three iterations against the fp64 oracle on the restatement at the same calls, under the
    tolerance rule of tests/test_hip_custom_data_tape.py (its _follow); then log_predictive on 5 held-out rows."""
    rows = _probit_rows(np.random.default_rng(17), T_ROWS + TEST_ROWS, E2E_D)
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
    pred_mode._check(f"{name}.log_predictive on probit", out, pred.reference64(l64), pred.twin32(l32))
    assert target.call_count == 3
