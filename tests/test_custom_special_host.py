"""The special functions of user-defined device targets, the part that needs no GPU: every operation of _lib.SPECIAL_OPS through
gmmvi_autodiff_probe_special and gmmvi_tape_probe_special against SciPy in fp64, the exact edge rules, one source per mode that
calls every new function through that mode's run-time compilation for gfx950, and the restatements of the new test targets
against central differences.

Probe bounds (eps32 = np.finfo(float32).eps; the reference is SciPy's fp64 function at the fp32 operands).
  values of lgamma, erf, erfc, softplus, log_sigmoid, and of sigmoid over results above 1e-37: 4 ulp of the reference;
  values of logaddexp: 4 ulp of max(|want|, |a|, |b|): the result crosses zero at a = b = -ln 2;
  gmmvi_digamma values, and lgamma tangents per unit tangent: 16 eps32 max(|want|, 1): digamma crosses zero at 1.4616321;
  gmmvi_trigamma values: 16 eps32 |want|;
  every other tangent: 16 eps32 (|d f/d a da| + |d f/d b db|), the rule of tests/test_custom_autodiff_host.py.
That file keeps its operands where every derivative is inside fp32's range ("an overflow is not a rounding error"); the grids here
reach +-90, where sigmoid(-a) and exp(-a^2) lie below fp32's smallest normal number, and an underflow is no rounding error
either: a partial derivative whose fp64 value is below 1e-37 in magnitude, the cut-off of the sigmoid values, is allowed an
absolute error of that value itself (it may be stored as a subnormal number or as zero)."""
import ctypes as C

import numpy as np
import pytest

import custom_special_cases as cases
import test_custom_autodiff_host as fwd

ERR_ARG = -2
EPS32 = float(np.finfo(np.float32).eps)
f32 = np.float32
NORMAL_CUT = 1e-37


def _special_ops():
    from gmmvi_amd import _lib
    return _lib.SPECIAL_OPS


def _forward(op, a, da=0.0, b=0.0, db=0.0):
    from gmmvi_amd import _lib
    v, t = C.c_float(), C.c_float()
    rc = _lib.load().gmmvi_autodiff_probe_special(_lib.SPECIAL_OPS.index(op), a, da, b, db, C.byref(v), C.byref(t))
    assert rc == 0, op
    return f32(v.value), f32(t.value)


def _tape(op, a, b=0.0, a_const=False, b_const=False):
    from gmmvi_amd import _lib
    v, pa, pb, n = C.c_float(), C.c_float(), C.c_float(), C.c_int()
    rc = _lib.load().gmmvi_tape_probe_special(_lib.SPECIAL_OPS.index(op), a, b, int(a_const), int(b_const), C.byref(v), C.byref(pa),
                                              C.byref(pb), C.byref(n))
    assert rc == 0, op
    return f32(v.value), f32(pa.value), f32(pb.value), n.value


def _operands(op):
    """-> [(a, b)] fp32 operands of the operation."""
    rule, _ = cases.split(op)
    if rule != "logaddexp":
        return [(f32(a), f32(0)) for a in cases.unary_grid(rule)]
    both = [f32(v) for v in fwd.OPERANDS + cases.LOGADDEXP_EXTRA]
    return [(a, b) for a in both for b in both]


def _want(op, a32, b32):
    """-> (value, d/da, d/db) in fp64 at the fp32 operands; a float operand has the partial 0."""
    rule, form = cases.split(op)
    value, dfa, dfb = cases.RULES[rule]
    a, b = np.float64(a32), np.float64(b32)
    args = (a, b) if dfb is not None else (a,)
    with np.errstate(all="ignore"):
        return (float(value(*args)), 0.0 if form == "ft" else float(dfa(*args)),
                0.0 if form == "tf" or dfb is None else float(dfb(*args)))


def value_bound(op, want, a, b):
    """The absolute bound of the value, or None where the value is not checked (a sigmoid at or below 1e-37)."""
    rule, _ = cases.split(op)
    if rule == "digamma":
        return 16.0 * EPS32 * max(abs(want), 1.0)
    if rule == "trigamma":
        return 16.0 * EPS32 * abs(want)
    if rule == "logaddexp":
        return 4.0 * float(np.spacing(f32(max(abs(want), abs(float(a)), abs(float(b))))))
    if rule == "sigmoid" and want <= NORMAL_CUT:
        return None
    return 4.0 * float(np.spacing(np.abs(f32(want))))


def partial_bound(op, want_p):
    """The absolute bound of one partial derivative per unit tangent."""
    rule, _ = cases.split(op)
    if abs(want_p) < NORMAL_CUT:
        return abs(want_p)
    if rule == "lgamma":
        return 16.0 * EPS32 * max(abs(want_p), 1.0)
    return 16.0 * EPS32 * abs(want_p)


# ---- the lists and the refusals ------------------------------------------------------------------------------------------------------
def test_the_op_list_and_the_refusals():
    from gmmvi_amd import _lib
    lib = _lib.load()
    ops = _lib.SPECIAL_OPS
    assert len(set(ops)) == len(ops)
    for op in ops:
        assert cases.split(op)[0] in cases.RULES, op
    for fn in ("erf", "erfc"):
        assert fn in ops and fn + "f" in ops
    assert "lgamma" in ops and "lgammaf" not in ops               # lgammaf stays a float function: the existing tests say so
    assert {"digamma", "trigamma", "sigmoid", "softplus", "log_sigmoid", "logaddexp", "logaddexp_tf", "logaddexp_ft"} <= set(ops)
    for symbol in ("gmmvi_autodiff_probe_special", "gmmvi_tape_probe_special"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    v, t, pa, pb, n = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int()
    outs = [C.byref(v), C.byref(pa), C.byref(pb), C.byref(n)]
    for bad in (-1, len(ops), 10 ** 6):
        assert lib.gmmvi_autodiff_probe_special(bad, 1.0, 1.0, 1.0, 1.0, C.byref(v), C.byref(t)) == ERR_ARG
        assert "unknown operation" in lib.gmmvi_last_error(None).decode()
        assert lib.gmmvi_tape_probe_special(bad, 1.0, 1.0, 0, 0, *outs) == ERR_ARG
        assert "unknown operation" in lib.gmmvi_last_error(None).decode()
    assert lib.gmmvi_autodiff_probe_special(len(ops) - 1, 1.0, 1.0, 1.0, 1.0, C.byref(v), C.byref(t)) == 0
    assert lib.gmmvi_tape_probe_special(len(ops) - 1, 1.0, 1.0, 0, 0, *outs) == 0
    assert lib.gmmvi_autodiff_probe_special(0, 1.0, 1.0, 1.0, 1.0, None, C.byref(t)) == ERR_ARG
    assert lib.gmmvi_autodiff_probe_special(0, 1.0, 1.0, 1.0, 1.0, C.byref(v), None) == ERR_ARG
    for missing in range(4):
        args = list(outs)
        args[missing] = None
        assert lib.gmmvi_tape_probe_special(0, 1.0, 1.0, 0, 0, *args) == ERR_ARG


# ---- the probes over the grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", _special_ops())
def test_forward_probe_values_and_tangents(op):
    worst_v, worst_t = 0.0, 0.0
    for a, b in _operands(op):
        want, want_a, want_b = _want(op, a, b)
        vb = value_bound(op, want, a, b)
        for da, db in fwd.TANGENTS:
            v, t = _forward(op, a, da, b, db)
            if vb is not None:
                err = abs(float(v) - want)
                worst_v = max(worst_v, err / vb if vb > 0 else (0.0 if err == 0 else np.inf))
                assert err <= vb, f"{op}({a!r}, {b!r}): value {v!r}, SciPy fp64 {want!r}, error {err:.3e} > {vb:.3e}"
            bound = partial_bound(op, want_a) * abs(da) + partial_bound(op, want_b) * abs(db)
            err = abs(float(t) - (want_a * da + want_b * db))
            if bound > 0:
                worst_t = max(worst_t, err / bound)
            assert err <= bound, (f"{op}({a!r}, {b!r}; {da}, {db}): tangent {t!r}, closed form {want_a * da + want_b * db!r}, "
                                  f"error {err:.3e} > {bound:.3e}")
    print(f"\n[custom_special] forward {op}: worst value error {worst_v:.3f} of its bound, worst tangent error {worst_t:.3f} of its bound")


@pytest.mark.parametrize("op", _special_ops())
def test_tape_probe_values_partials_and_records(op):
    rule, form = cases.split(op)
    binary = cases.RULES[rule][2] is not None
    makes_records = rule != "trigamma"
    worst_v, worst_p = 0.0, 0.0
    for a, b in _operands(op):
        want, want_a, want_b = _want(op, a, b)
        v, pa, pb, n = _tape(op, a, b)
        assert n == (1 if makes_records else 0), (op, a, b, n)
        vb = value_bound(op, want, a, b)
        if vb is not None:
            err = abs(float(v) - want)
            worst_v = max(worst_v, err / vb if vb > 0 else (0.0 if err == 0 else np.inf))
            assert err <= vb, f"{op}({a!r}, {b!r}): value {v!r}, SciPy fp64 {want!r}, error {err:.3e} > {vb:.3e}"
        assert v == _forward(op, a, 1.0, b, 1.0)[0], (op, a, b)                     # the same float function
        for which, got, want_p in (("a", pa, want_a), ("b", pb, want_b)):
            bound = partial_bound(op, want_p)
            err = abs(float(got) - want_p)
            if bound > 0:
                worst_p = max(worst_p, err / bound)
            assert err <= bound, f"{op}({a!r}, {b!r}): partial by {which} {got!r}, closed form {want_p!r}, error {err:.3e} > {bound:.3e}"
    # a constant operand takes no partial; no record when every operand is a constant
    for a, b in _operands(op)[::11]:
        full = _tape(op, a, b)
        for a_const, b_const in ((True, False), (False, True), (True, True)):
            v, pa, pb, n = _tape(op, a, b, a_const, b_const)
            assert v == full[0] or (np.isnan(v) and np.isnan(full[0]))
            a_moves = not a_const and form != "ft"
            b_moves = not b_const and form != "tf" and binary
            assert n == (1 if makes_records and (a_moves or b_moves) else 0), (op, a, b, a_const, b_const, n)
            assert pa == (full[1] if a_moves and makes_records else 0.0), (op, a, b, a_const, b_const)
            assert pb == (full[2] if b_moves and makes_records else 0.0), (op, a, b, a_const, b_const)
    print(f"\n[custom_special] tape {op}: worst value error {worst_v:.3f} of its bound, worst partial error {worst_p:.3f} of its bound")


# ---- the exact rules --------------------------------------------------------------------------------------------------------------------
def test_gamma_family_outside_its_domain_is_nan():
    for bad in (0.0, -0.0, -1.0, -0.5, float("nan")):
        for op in ("digamma", "trigamma"):
            assert np.isnan(_forward(op, bad, 1.0)[0]) and np.isnan(_tape(op, bad)[0]), (op, bad)
        assert np.isnan(_forward("digamma", bad, 1.0)[1]) and np.isnan(_tape("digamma", bad)[1])
    # lgamma at -0.5: the value is libm's, the tangent is digamma's NaN
    for spelling in ("lgamma",):
        v, t = _forward(spelling, -0.5, 1.0)
        assert abs(float(v) - 1.2655121234846454) <= 4 * np.spacing(f32(1.2655121)) and np.isnan(t)
        v, pa, _, n = _tape(spelling, -0.5)
        assert abs(float(v) - 1.2655121234846454) <= 4 * np.spacing(f32(1.2655121)) and np.isnan(pa) and n == 1


def test_logaddexp_ties_are_exact():
    ln2 = f32(0.69314718)
    inf = float("inf")
    for t in (0.0, 1.25, -7.0, 88.0, -88.0, 3e38, -inf, inf):
        want = f32(t) + ln2
        assert _forward("logaddexp", t, 3.0, t, -5.0) == (want, -1.0), t               # 1/2 * 3 + 1/2 * -5
        assert _forward("logaddexp_tf", t, 3.0, t, -5.0) == (want, 1.5), t
        assert _forward("logaddexp_ft", t, 3.0, t, -5.0) == (want, -2.5), t
        assert _tape("logaddexp", t, t) == (want, 0.5, 0.5, 1), t
        assert _tape("logaddexp_tf", t, t) == (want, 0.5, 0.0, 1), t
        assert _tape("logaddexp_ft", t, t) == (want, 0.0, 0.5, 1), t
    # one operand at -inf: the other one, with the whole tangent
    assert _forward("logaddexp", 2.0, 3.0, -inf, -5.0) == (2.0, 3.0)
    assert _forward("logaddexp", -inf, 3.0, 2.0, -5.0) == (2.0, -5.0)


def test_sigmoid_saturates_exactly():
    assert _forward("sigmoid", 200.0, 3.0) == (1.0, 0.0) and _forward("sigmoid", -200.0, 3.0) == (0.0, 0.0)
    assert _tape("sigmoid", 200.0) == (1.0, 0.0, 0.0, 1) and _tape("sigmoid", -200.0) == (0.0, 0.0, 0.0, 1)
    assert _forward("sigmoid", 0.0, 2.0) == (0.5, 0.5)
    # softplus and log_sigmoid take over the argument there, with tangent 1 and 0
    assert _forward("softplus", 200.0, 3.0) == (200.0, 3.0) and _forward("softplus", -200.0, 3.0) == (0.0, 0.0)
    assert _forward("log_sigmoid", -200.0, 3.0) == (-200.0, 3.0) and _forward("log_sigmoid", 200.0, 3.0) == (0.0, 0.0)


def test_gmmvi_value_is_unchanged():
    assert fwd._probe("value", 1.5, 3.0) == (1.5, 0.0)
    import test_custom_tape_host as tape
    assert tape._probe("value", 1.5) == (1.5, 0.0, 0.0, 0)


# ---- the compiler: every new function in every mode -----------------------------------------------------------------------------------------
CHECKS = [("custom_target_check", "hand"), ("custom_target_check_autodiff", "density"), ("custom_target_check_tape", "density"),
          ("custom_target_check_data", "data"), ("custom_target_check_data_tape", "data")]


@pytest.mark.parametrize("check,mode", CHECKS)
def test_every_new_function_compiles_in_every_mode(check, mode):
    from gmmvi_amd import hip_ops
    rc, log = getattr(hip_ops, check)(cases.every_source(mode), "gfx950")
    assert rc == 0, log


@pytest.mark.parametrize("check,name", [("custom_target_check_data", n) for n in sorted(cases.DATA_SOURCES)]
                         + [("custom_target_check_data_tape", n) for n in sorted(cases.DATA_SOURCES)]
                         + [("custom_target_check_autodiff", "specials"), ("custom_target_check_tape", "specials")])
def test_case_sources_compile_for_gfx950(check, name):
    from gmmvi_amd import hip_ops
    source = cases.SPECIALS_SRC if name == "specials" else cases.DATA_SOURCES[name]
    rc, log = getattr(hip_ops, check)(source, "gfx950")
    assert rc == 0, log


@pytest.mark.parametrize("check,mode", CHECKS[1:])
def test_trigamma_of_a_number_is_a_compile_error_with_the_users_line(check, mode):
    """There are no second derivatives: gmmvi_trigamma takes a float and nothing else."""
    from gmmvi_amd import hip_ops
    lines = cases.every_source(mode).split("\n")
    at = next(i for i, text in enumerate(lines) if "gmmvi_trigamma(" in text)
    lines[at] = lines[at].replace("gmmvi_trigamma(1.f + c * c)", "gmmvi_trigamma(a)")
    rc, log = getattr(hip_ops, check)("\n".join(lines), "gfx950")
    assert rc == ERR_ARG
    assert f"gmmvi_user_target.hip:{at + 1}:" in log and "gmmvi_trigamma" in log, log


def test_a_source_that_begins_with_a_directive_keeps_compiling():
    """The declarations go in front of the first line; a directive there still begins its line, and the line numbers stay."""
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check("#define HALF 0.5f\n" + cases.every_source("hand"), "gfx950")
    assert rc == 0, log
    rc, log = hip_ops.custom_target_check("#define HALF 0.5f\nint broken = ;\n" + cases.every_source("hand"), "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_target.hip:2:" in log, log


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def _finite_differences(tgt, x, name):
    """The rule of test_restatements_agree_with_finite_differences (tests/test_custom_target_host.py)."""
    x = x.astype(np.float64)
    _, g = tgt.log_density_and_grad(x)
    h = 1e-6
    for i in range(x.shape[1]):
        e = np.zeros(x.shape[1]); e[i] = h
        fd = (tgt.log_density(x + e) - tgt.log_density(x - e)) / (2 * h)
        np.testing.assert_allclose(g[:, i], fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} coordinate {i}")


def test_restatements_agree_with_finite_differences():
    _finite_differences(*cases.build_specials(9), "specials")
    for name in ("negbin", "erfmix"):
        tgt, x = cases.build_data_case(cases.Case(name, 4, 9, 12, 0, None, 0))
        _finite_differences(tgt, x, name)

