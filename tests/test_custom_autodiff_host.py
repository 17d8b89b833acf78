"""Differentiated user-defined device targets, the part that needs no GPU: the run-time compiler builds source + dual-number
text + wrapper kernels for gfx950 without a device (gmmvi_custom_target_check_autodiff), compile errors come back as argument
errors with the user's own line numbers, every rule of the dual-number text is evaluated on the host through
gmmvi_autodiff_probe against NumPy, and DeviceAutodiffLNPDF rejects bad arguments before it touches the device.

Probe bounds.  Values: NumPy's fp32 function within 4 ulp.  Tangents: the fp64 closed form d f/d a * da + d f/d b * db at the
fp32 operands within 16 * eps32 * (|d f/d a * da| + |d f/d b * db|), the factor tests/test_hip_custom_target.py uses."""
import ctypes as C

import numpy as np
import pytest

import custom_autodiff_cases as cases
from helpers import use_host_context

ERR_ARG = -2
EPS32 = float(np.finfo(np.float32).eps)
f32 = np.float32


# ---- the compiler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_case_sources_compile_for_gfx950(name):
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_autodiff(cases.SOURCES[name], "gfx950")
    assert rc == 0, log


def test_syntax_error_is_an_argument_error_with_the_users_line():
    from gmmvi_amd import _lib, hip_ops
    lines = cases.ROSENBROCK_SRC.split("\n")
    bad_line = next(i for i, text in enumerate(lines) if "const T u" in text)
    lines[bad_line] = "    const T u = a - ;"
    rc, log = hip_ops.custom_target_check_autodiff("\n".join(lines), "gfx950")
    assert rc == ERR_ARG
    assert f":{bad_line + 1}:" in log, log                     # clang's file:line:column of the user's own text
    assert "error" in log
    assert log.strip() in _lib.load().gmmvi_last_error(None).decode()
    # an error on the user's FIRST line keeps its line number too
    rc, log = hip_ops.custom_target_check_autodiff("int broken = ;\n" + cases.ROSENBROCK_SRC, "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_target.hip:1:" in log, log


def test_source_without_the_function_names_it():
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_autodiff("__device__ float something_else(const float* x) { return x[0]; }\n", "gfx950")
    assert rc == ERR_ARG
    assert "gmmvi_user_density" in log
    # the hand-written-gradient contract is another mode: its source is not a density
    rc, log = hip_ops.custom_target_check_autodiff(cases.base.ROSENBROCK_SRC, "gfx950")
    assert rc == ERR_ARG and "does not define gmmvi_user_density" in log
    # and the other way round
    rc, log = hip_ops.custom_target_check(cases.ROSENBROCK_SRC, "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_target" in log


def test_function_outside_the_surface_is_a_compile_error():
    """A dual does not convert to float: lgammaf on a T does not compile, on a float it does."""
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_autodiff(cases.ROSENBROCK_SRC.replace("return -(", "return lgammaf(u) - ("), "gfx950")
    assert rc == ERR_ARG
    assert log.strip() and "lgammaf" in log
    rc, log = hip_ops.custom_target_check_autodiff(cases.ROSENBROCK_SRC.replace("return -(", "return lgammaf(a) - ("), "gfx950")
    assert rc == 0, log


def test_null_arguments_are_argument_errors():
    from gmmvi_amd import _lib
    lib = _lib.load()
    assert lib.gmmvi_custom_target_check_autodiff(None, b"gfx950", None, 0) == ERR_ARG
    assert lib.gmmvi_custom_target_check_autodiff(b"", None, None, 0) == ERR_ARG
    buf = C.create_string_buffer(b"\xff" * 16, 16)
    assert lib.gmmvi_custom_target_check_autodiff(b"nonsense", b"gfx950", buf, 16) == ERR_ARG
    assert len(buf.value) == 15
    v, t = C.c_float(), C.c_float()
    assert lib.gmmvi_autodiff_probe(0, 1.0, 1.0, 1.0, 1.0, None, C.byref(t)) == ERR_ARG
    assert lib.gmmvi_autodiff_probe(0, 1.0, 1.0, 1.0, 1.0, C.byref(v), None) == ERR_ARG


def test_constants_and_symbols():
    import os
    import re
    from gmmvi_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmmvi_hip.h")).read()
    assert int(re.search(r"#define GMMVI_CUSTOM_AUTODIFF_TANGENTS (\d+)", header).group(1)) == _lib.CUSTOM_AUTODIFF_TANGENTS
    assert int(re.search(r"#define GMMVI_CUSTOM_AUTODIFF_MAX_DIM (\d+)", header).group(1)) == _lib.CUSTOM_AUTODIFF_MAX_DIM == 512
    assert _lib.CUSTOM_AUTODIFF_MAX_DIM == _lib.MAX_DIM_BLOCKED
    for symbol in ("gmmvi_custom_target_check_autodiff", "gmmvi_custom_target_compile_autodiff", "gmmvi_autodiff_probe"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    # no new struct came with the feature
    assert [f[0] for f in _lib.TargetSpec._fields_][-2:] == ["custom", "custom_params"]


# ---- the probe -----------------------------------------------------------------------------------------------------------
def _probe(op, a, da=0.0, b=0.0, db=0.0):
    from gmmvi_amd import _lib
    v, t = C.c_float(), C.c_float()
    rc = _lib.load().gmmvi_autodiff_probe(_lib.AUTODIFF_OPS.index(op), a, da, b, db, C.byref(v), C.byref(t))
    assert rc == 0, op
    return f32(v.value), f32(t.value)


def _split(op):
    """'powf_tf' -> ('pow', 'tf'): the rule and which operands are duals ('tt', 'tf' or 'ft')."""
    form = "tt"
    for suffix in ("_tf", "_ft"):
        if op.endswith(suffix):
            op, form = op[:-3], suffix[1:]
    if op.endswith("_assign"):
        op = op[:-7]
    if op.endswith("f") and op[:-1] in RULES:
        op = op[:-1]
    return op, form


def _sech2(a):
    return 1.0 / np.cosh(a) ** 2


def _first_wins(cmp):
    """fmax / fmin: the first operand's tangent unless the second strictly wins."""
    return (lambda a, b: 0.0 if cmp(b, a) else 1.0), (lambda a, b: 1.0 if cmp(b, a) else 0.0)


# rule -> (value in the dtype of its operands, d/da in fp64, d/db in fp64 or None, domain)
RULES = {
    "add": (lambda a, b: a + b, lambda a, b: 1.0, lambda a, b: 1.0, None),
    "sub": (lambda a, b: a - b, lambda a, b: 1.0, lambda a, b: -1.0, None),
    "mul": (lambda a, b: a * b, lambda a, b: b, lambda a, b: a, None),
    "div": (lambda a, b: a / b, lambda a, b: 1.0 / b, lambda a, b: -a / (b * b), lambda a, b: abs(b) > 1e-7),
    "neg": (lambda a, b: -a, lambda a, b: -1.0, None, None),
    "exp": (lambda a, b: np.exp(a), lambda a, b: np.exp(a), None, None),
    "expm1": (lambda a, b: np.expm1(a), lambda a, b: np.exp(a), None, None),
    "log": (lambda a, b: np.log(a), lambda a, b: 1.0 / a, None, lambda a, b: a > 0),
    "log1p": (lambda a, b: np.log1p(a), lambda a, b: 1.0 / (1.0 + a), None, lambda a, b: a > -1),
    "sqrt": (lambda a, b: np.sqrt(a), lambda a, b: 0.5 / np.sqrt(a), None, lambda a, b: a > 0),
    "rsqrt": (lambda a, b: type(a)(1) / np.sqrt(a), lambda a, b: -0.5 / (a * np.sqrt(a)), None, lambda a, b: a > 1e-20),
    "sin": (lambda a, b: np.sin(a), lambda a, b: np.cos(a), None, None),
    "cos": (lambda a, b: np.cos(a), lambda a, b: -np.sin(a), None, None),
    "tan": (lambda a, b: np.tan(a), lambda a, b: 1.0 + np.tan(a) ** 2, None, None),
    "tanh": (lambda a, b: np.tanh(a), lambda a, b: _sech2(a), None, None),
    "atan": (lambda a, b: np.arctan(a), lambda a, b: 1.0 / (1.0 + a * a), None, None),
    "fabs": (lambda a, b: np.abs(a), lambda a, b: float(np.sign(a)), None, None),
    "fmax": (lambda a, b: np.maximum(a, b),) + _first_wins(lambda x, y: x > y) + (None,),
    "fmin": (lambda a, b: np.minimum(a, b),) + _first_wins(lambda x, y: x < y) + (None,),
    "pow": (lambda a, b: np.power(a, b), lambda a, b: 0.0 if b == 0 else b * np.power(a, b - 1.0),
            lambda a, b: np.power(a, b) * np.log(a), lambda a, b: a >= 0.25),
    "value": (lambda a, b: a, lambda a, b: 0.0, None, None),
}
COMPARISONS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}

# Domains keep every value AND every derivative inside fp32's range: the tangent of a / b at |b| <= 1e-7, of rsqrt at 1e-30 and
# of pow at a tiny base with the exponents +-7 overflows, and an overflow is not a rounding error.
# operands: ordinary numbers of both signs, and the seams: +-0 (fabs), |a| <= 1e-6 (log1p, expm1), 1e-30 (sqrt), the
# exponents 0, 1, 2, 0.5, -1.5 (pow); every a is also a b, so that fmax / fmin and the comparisons meet their ties
OPERANDS = [0.0, -0.0, 1e-6, -1e-6, 3e-7, 1e-30, 0.3, -0.3, 0.5, 1.0, -1.0, 1.25, -1.5, 2.0, 2.5, -2.5, 0.9, 7.0, -7.0]
TANGENTS = [(1.0, 1.0), (-0.75, 0.5), (0.0, 2.0), (1.5, 0.0)]


def _ulps(got, want):
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(f32(want)))) if np.isfinite(want) else (0.0 if got == want else np.inf)


def test_every_operation_has_a_rule_and_unknown_ops_are_refused():
    from gmmvi_amd import _lib
    lib = _lib.load()
    assert len(set(_lib.AUTODIFF_OPS)) == len(_lib.AUTODIFF_OPS)
    for op in _lib.AUTODIFF_OPS:
        rule, form = _split(op)
        assert rule in RULES or rule in COMPARISONS, op
    v, t = C.c_float(), C.c_float()
    for bad in (-1, len(_lib.AUTODIFF_OPS), 10 ** 6):
        assert lib.gmmvi_autodiff_probe(bad, 1.0, 1.0, 1.0, 1.0, C.byref(v), C.byref(t)) == ERR_ARG
        assert "unknown operation" in lib.gmmvi_last_error(None).decode()
    assert lib.gmmvi_autodiff_probe(len(_lib.AUTODIFF_OPS) - 1, 1.0, 1.0, 1.0, 1.0, C.byref(v), C.byref(t)) == 0
    # every function of the surface under both spellings, every operator in its three operand forms
    for fn in ("exp", "expm1", "log", "log1p", "sqrt", "rsqrt", "sin", "cos", "tan", "tanh", "atan", "fabs", "fmax", "fmin", "pow"):
        assert fn in _lib.AUTODIFF_OPS and fn + "f" in _lib.AUTODIFF_OPS
    for o in ("add", "sub", "mul", "div", "lt", "le", "gt", "ge", "eq", "ne"):
        assert {o, o + "_tf", o + "_ft"} <= set(_lib.AUTODIFF_OPS)


def _grid(op):
    """-> [(a, b, da, db)] of fp32 operands inside the rule's domain; a float operand has tangent 0."""
    rule, form = _split(op)
    domain = RULES[rule][3] if rule in RULES else None
    binary = rule in COMPARISONS or RULES[rule][2] is not None
    out = []
    for a in OPERANDS:
        for b in (OPERANDS if binary else [0.0]):
            if domain is not None and not domain(f32(a), f32(b)):
                continue
            for da, db in TANGENTS:
                out.append((a, b, da, db))
    assert out
    return out


def _all_ops():
    from gmmvi_amd import _lib
    return _lib.AUTODIFF_OPS


@pytest.mark.parametrize("op", _all_ops())
def test_probe_values_and_tangents(op):
    rule, form = _split(op)
    worst_ulp, worst_tan = 0.0, 0.0
    for a, b, da, db in _grid(op):
        v, t = _probe(op, a, da, b, db)
        a32, b32 = f32(a), f32(b)
        if rule in COMPARISONS:
            assert v == f32(COMPARISONS[rule](a32, b32)) and t == 0.0, (op, a, b)
            continue
        value, dfa, dfb, _ = RULES[rule]
        with np.errstate(all="ignore"):
            want = f32(value(a32, b32))
            ulps = _ulps(v, want)
            a64, b64 = np.float64(a32), np.float64(b32)
            term_a = 0.0 if form == "ft" else float(dfa(a64, b64)) * da
            term_b = 0.0 if form == "tf" or dfb is None else float(dfb(a64, b64)) * db
        worst_ulp = max(worst_ulp, ulps)
        assert ulps <= 4.0, f"{op}({a}, {b}): value {v!r}, NumPy fp32 {want!r}, {ulps:.1f} ulp"
        bound = 16.0 * EPS32 * (abs(term_a) + abs(term_b))
        err = abs(float(t) - (term_a + term_b))
        if bound > 0:
            worst_tan = max(worst_tan, err / bound)
        assert err <= bound, f"{op}({a}, {b}; {da}, {db}): tangent {t!r}, closed form {term_a + term_b!r}, error {err:.3e} > {bound:.3e}"
    print(f"\n[custom_autodiff] {op}: worst value error {worst_ulp:.2f} ulp (bound 4), worst tangent error {worst_tan:.3f} of its bound")


def test_probe_tie_rules_hold_exactly():
    for spelling in ("fabs", "fabsf"):
        for zero in (0.0, -0.0):
            v, t = _probe(spelling, zero, 3.0)
            assert v == 0.0 and not np.signbit(v) and t == 0.0
        assert _probe(spelling, 2.0, 3.0) == (2.0, 3.0) and _probe(spelling, -2.0, 3.0) == (2.0, -3.0)
    for name in ("fmax", "fmin", "fmaxf", "fminf"):
        for tie in (1.25, 0.0, -7.0):
            assert _probe(name, tie, 3.0, tie, -5.0) == (f32(tie), 3.0)           # the first operand's tangent
            assert _probe(name + "_tf", tie, 3.0, tie, -5.0) == (f32(tie), 3.0)   # first a dual, second a float
            assert _probe(name + "_ft", tie, 3.0, tie, -5.0) == (f32(tie), 0.0)   # first a float: a constant
    assert _probe("fmax", 1.0, 3.0, 2.0, -5.0) == (2.0, -5.0) and _probe("fmax", 2.0, 3.0, 1.0, -5.0) == (2.0, 3.0)
    assert _probe("fmin", 1.0, 3.0, 2.0, -5.0) == (1.0, 3.0) and _probe("fmin", 2.0, 3.0, 1.0, -5.0) == (1.0, -5.0)
    # comparisons look at the values alone, whatever the tangents are
    assert _probe("lt", 1.0, 9.0, 1.0, -9.0) == (0.0, 0.0) and _probe("le", 1.0, 9.0, 1.0, -9.0) == (1.0, 0.0)
    assert _probe("eq", 1.0, 9.0, 1.0, -9.0) == (1.0, 0.0) and _probe("ne", 1.0, 9.0, 1.0, -9.0) == (0.0, 0.0)
    # pow: exponent 0 has tangent 0 even at a = 0; a constant exponent keeps a negative base usable
    assert _probe("pow_tf", 0.0, 1.0, 0.0) == (1.0, 0.0)
    assert _probe("pow", -2.0, 1.0, 2.0, 0.0) == (4.0, -4.0)
    # gmmvi_value drops the tangent
    assert _probe("value", 1.5, 3.0) == (1.5, 0.0)


# ---- the references --------------------------------------------------------------------------------------------------------
def test_allops_restatement_agrees_with_finite_differences():
    """The rule of test_restatements_agree_with_finite_differences (tests/test_custom_target_host.py) on the allops density."""
    tgt, x = cases.build_case("allops", 6, 7)
    x = x.astype(np.float64)
    _, g = tgt.log_density_and_grad(x)
    h = 1e-6
    for i in range(6):
        e = np.zeros(6); e[i] = h
        fd = (tgt.log_density(x + e) - tgt.log_density(x - e)) / (2 * h)
        np.testing.assert_allclose(g[:, i], fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"allops coordinate {i}")


def test_kernel_cases_sit_on_the_seams_of_the_pass_width():
    from gmmvi_amd import _lib
    w = _lib.CUSTOM_AUTODIFF_TANGENTS
    dims = {d for name, d, n, routes in cases.kernel_cases(w) if name == "quartic"}
    assert {3, w - 1, w, w + 1, 2 * w, 2 * w + 1, 50, 120, 121, 300} <= dims


# ---- the class -------------------------------------------------------------------------------------------------------------
def test_device_autodiff_lnpdf_argument_errors(monkeypatch):
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    use_host_context(monkeypatch, device_lnpdf)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="num_dimensions"):
            device_lnpdf.DeviceAutodiffLNPDF(cases.ROSENBROCK_SRC, bad, params=[1.0, 100.0])
    with pytest.raises(ValueError, match="one-dimensional"):
        device_lnpdf.DeviceAutodiffLNPDF(cases.ROSENBROCK_SRC, 2, params=np.ones((2, 2)))
    for d in (513, 1024):
        with pytest.raises(ValueError, match="512") as info:
            device_lnpdf.DeviceAutodiffLNPDF(cases.QUARTIC_SRC, d)
        assert "DeviceLNPDF" in str(info.value) and "by hand" in str(info.value)


def test_class_facts():
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceAutodiffLNPDF, DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi.experiments.target_distributions.device_lnpdf import DeviceAutodiffLNPDF as Alias
    assert Alias is DeviceAutodiffLNPDF
    assert issubclass(DeviceAutodiffLNPDF, DeviceLNPDF)
    assert DeviceAutodiffLNPDF.log_density_and_grad is not LNPDF.log_density_and_grad
    assert hasattr(DeviceAutodiffLNPDF, "_fast_path_target")
    assert type(DeviceAutodiffLNPDF.__new__(DeviceAutodiffLNPDF, "", 2)) is DeviceAutodiffLNPDF


def test_device_lnpdf_is_what_it_was():
    """The facts of test_values_only_object_leaves_the_gradient_call_alone, with the new class beside it."""
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    assert DeviceLNPDF.log_density_and_grad is LNPDF.log_density_and_grad
    assert not hasattr(DeviceLNPDF, "_fast_path_target")
    with_grad = DeviceLNPDF.__new__(DeviceLNPDF, "", 2)
    values_only = DeviceLNPDF.__new__(DeviceLNPDF, "", 2, has_gradient=False)
    assert isinstance(with_grad, DeviceLNPDF) and type(values_only) is DeviceLNPDF
    assert type(with_grad).log_density_and_grad is not LNPDF.log_density_and_grad
    assert hasattr(with_grad, "_fast_path_target")
