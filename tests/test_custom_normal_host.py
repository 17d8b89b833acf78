"""gmmvi_erfcx, gmmvi_ndtr, gmmvi_log_ndtr and sinh, cosh, asin, acos of user-defined device targets, the part that needs no GPU:
every operation of _lib.EXTRA_OPS through gmmvi_autodiff_probe_extra and gmmvi_tape_probe_extra against SciPy in fp64 on the grids
of tests/custom_normal_cases.py, the exact edge rules, what the plain form log(erfc / 2) does at the same operand, one source per
mode that calls every new function through that mode's run-time compilation for gfx950, and the restatements of the new test
targets against central differences.

Probe bounds (eps32 = np.finfo(float32).eps; the reference is SciPy's fp64 function at the fp32 operand).
  values of erfcx, log_ndtr, and of ndtr over results above 1e-37: 8 ulp of the reference, twice the 3.0 to 3.9 ulp of the NumPy
  prototype the functions were planned on;
  values of sinh, cosh, asin, acos: 4 ulp, the rule of the existing families (tests/test_custom_special_host.py);
  partials per unit tangent: 16 eps32 |d f/d a|; one whose fp64 value is below 1e-37 in magnitude may be off by that value.
An overflow is no rounding error: where the fp64 value or partial lies further beyond fp32's largest number than its bound
(gmmvi_erfcx below -9.38 and its partial from a little above that, gmmvi_log_ndtr below -2.6e19) the result has to be the infinity
of that sign, and an infinity is accepted nowhere else (error_ratio).

Measured on the host (glibc's expf, logf, log1pf) over these grids: values at most 0.18 (erfcx), 0.44 (ndtr) and 0.46 (log_ndtr)
of the bound, partials at most 0.16 of theirs; sinh, cosh, asin, acos at most 0.20 and 0.06."""
import ctypes as C

import numpy as np
import pytest

import custom_normal_cases as cases
import test_custom_autodiff_host as fwd
import test_custom_special_host as special

ERR_ARG = -2
EPS32 = special.EPS32
NORMAL_CUT = special.NORMAL_CUT
FLT_MAX = cases.FLT_MAX
f32 = np.float32
TANGENTS = (1.0, -0.75, 0.0)
# _lib.SPECIAL_OPS of the commit before EXTRA_OPS came: the existing tests parametrize over it
SPECIAL_OPS_BEFORE = ("lgamma", "erf", "erff", "erfc", "erfcf", "digamma", "sigmoid", "softplus", "log_sigmoid",
                      "logaddexp", "logaddexp_tf", "logaddexp_ft", "trigamma")
EXTRA_OPS = ("erfcx", "ndtr", "log_ndtr", "sinh", "sinhf", "cosh", "coshf", "asin", "asinf", "acos", "acosf")


def _forward(op, a, da=1.0):
    from gmmvi_amd import _lib
    v, t = C.c_float(), C.c_float()
    rc = _lib.load().gmmvi_autodiff_probe_extra(_lib.EXTRA_OPS.index(op), a, da, C.byref(v), C.byref(t))
    assert rc == 0, op
    return f32(v.value), f32(t.value)


def _tape(op, a, a_const=False):
    from gmmvi_amd import _lib
    v, pa, n = C.c_float(), C.c_float(), C.c_int()
    rc = _lib.load().gmmvi_tape_probe_extra(_lib.EXTRA_OPS.index(op), a, int(a_const), C.byref(v), C.byref(pa), C.byref(n))
    assert rc == 0, op
    return f32(v.value), f32(pa.value), n.value


def _operands(op):
    return [f32(a) for a in cases.unary_grid(cases.rule_of(op))]


def _want(op, a32):
    """-> (value, d/da) in fp64 at the fp32 operand."""
    value, partial = cases.RULES[cases.rule_of(op)]
    a = np.float64(a32)
    with np.errstate(all="ignore"):
        return float(value(a)), float(partial(a))


def value_bound(op, want):
    """The absolute bound of the value; None where the value is not checked (an ndtr at or below 1e-37)."""
    rule = cases.rule_of(op)
    if rule == "ndtr" and want <= NORMAL_CUT:
        return None
    # (the ulp of fp32's last binade for a value in it or beyond it: np.spacing(FLT_MAX) itself is inf)
    return (8.0 if rule in cases.NORMAL_FAMILY else 4.0) * float(np.spacing(f32(min(abs(want), 0.75 * FLT_MAX))))


def partial_bound(op, want_p):
    """The absolute bound of the partial derivative per unit tangent."""
    if abs(want_p) < NORMAL_CUT:
        return abs(want_p)
    return 16.0 * EPS32 * min(abs(want_p), FLT_MAX)


def error_ratio(got, want, bound):
    """|got - want| / bound.  An infinity of want's sign counts as a value beyond fp32's largest number: it is right (0) where want
    plus the bound lies beyond that number, and wrong (inf) elsewhere; a finite result is measured as it is, so one next to a want
    just beyond the range passes too."""
    if bound is None:
        return 0.0
    if np.isinf(got):
        return 0.0 if (got > 0) == (want > 0) and abs(want) + bound > FLT_MAX else np.inf
    err = abs(float(got) - want)
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


# ---- the lists and the refusals ------------------------------------------------------------------------------------------------------
def test_the_op_list_and_the_refusals():
    from gmmvi_amd import _lib
    lib = _lib.load()
    assert _lib.EXTRA_OPS == EXTRA_OPS
    for op in EXTRA_OPS:
        assert cases.rule_of(op) in cases.RULES, op
    v, t, pa, n = C.c_float(), C.c_float(), C.c_float(), C.c_int()
    outs = [C.byref(v), C.byref(pa), C.byref(n)]
    for bad in (-1, len(EXTRA_OPS), 10 ** 6):
        assert lib.gmmvi_autodiff_probe_extra(bad, 1.0, 1.0, C.byref(v), C.byref(t)) == ERR_ARG
        assert "unknown operation" in lib.gmmvi_last_error(None).decode()
        assert lib.gmmvi_tape_probe_extra(bad, 1.0, 0, *outs) == ERR_ARG
        assert "unknown operation" in lib.gmmvi_last_error(None).decode()
    assert lib.gmmvi_autodiff_probe_extra(len(EXTRA_OPS) - 1, 0.5, 1.0, C.byref(v), C.byref(t)) == 0
    assert lib.gmmvi_tape_probe_extra(len(EXTRA_OPS) - 1, 0.5, 0, *outs) == 0
    assert lib.gmmvi_autodiff_probe_extra(0, 1.0, 1.0, None, C.byref(t)) == ERR_ARG
    assert "must not be NULL" in lib.gmmvi_last_error(None).decode()
    assert lib.gmmvi_autodiff_probe_extra(0, 1.0, 1.0, C.byref(v), None) == ERR_ARG
    for missing in range(3):
        args = list(outs)
        args[missing] = None
        assert lib.gmmvi_tape_probe_extra(0, 1.0, 0, *args) == ERR_ARG
        assert "must not be NULL" in lib.gmmvi_last_error(None).decode()


def test_the_new_symbols_are_exported_once():
    from gmmvi_amd import _lib
    for symbol in ("gmmvi_autodiff_probe_extra", "gmmvi_tape_probe_extra"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
        assert getattr(_lib.load(), symbol) is not None


def test_the_old_list_is_unchanged():
    from gmmvi_amd import _lib
    assert _lib.SPECIAL_OPS == SPECIAL_OPS_BEFORE
    assert not set(_lib.SPECIAL_OPS) & set(_lib.EXTRA_OPS)


def test_the_grids_cross_a_tile_and_hold_the_branch_points():
    for grid in (cases.NDTR_GRID, cases.ERFCX_GRID, cases.HYPERBOLIC_GRID, cases.ARC_GRID):
        assert grid.dtype == np.float32 and grid.size > 64
    tiny = np.nextafter(f32(0), f32(1))
    for grid, thresholds in ((cases.NDTR_GRID, cases.NDTR_THRESHOLDS), (cases.ERFCX_GRID, cases.ERFCX_THRESHOLDS)):
        assert {-tiny, tiny} <= set(grid.tolist())
        for t in thresholds:
            t = f32(t)
            assert {np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf))} <= set(grid.tolist())
    assert {-14.5, -20.0, -38.0} <= set(cases.NDTR_GRID.tolist()) and {f32(1e-6), f32(1e3), f32(1e18), f32(1e30)} <= set(cases.ERFCX_GRID.tolist())
    _forward("erfcx", 0.0)                                               # the probes exist: this file needs them throughout


# ---- the probes over the grids ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", EXTRA_OPS)
def test_forward_probe_values_and_tangents(op):
    worst_v, worst_t = 0.0, 0.0
    for a in _operands(op):
        want, want_p = _want(op, a)
        vb, pb = value_bound(op, want), partial_bound(op, want_p)
        for da in TANGENTS:
            v, t = _forward(op, a, da)
            r_v = error_ratio(v, want, vb)
            worst_v = max(worst_v, r_v)
            assert r_v <= 1.0, f"{op}({a!r}): value {v!r}, SciPy fp64 {want!r}, bound {vb!r}"
            if da == 0.0:
                assert t == 0.0 or (np.isnan(t) and abs(want_p) + pb > FLT_MAX), (op, a, t)   # 0 times an infinite partial
                continue
            r_t = error_ratio(np.float64(t) / da, want_p, pb)
            worst_t = max(worst_t, r_t if abs(want_p) >= NORMAL_CUT else 0.0)
            assert r_t <= 1.0, f"{op}({a!r}; {da}): tangent {t!r}, closed form {want_p * da!r}, bound {pb * abs(da)!r}"
    print(f"\n[custom_normal] forward {op}: worst value error {worst_v:.3f} of its bound, worst tangent error {worst_t:.3f} of its bound "
          f"(over partials of at least 1e-37)")


@pytest.mark.parametrize("op", EXTRA_OPS)
def test_tape_probe_values_partials_and_records(op):
    worst_v, worst_p = 0.0, 0.0
    for a in _operands(op):
        want, want_p = _want(op, a)
        v, pa, n = _tape(op, a)
        assert n == 1, (op, a, n)
        r_v = error_ratio(v, want, value_bound(op, want))
        worst_v = max(worst_v, r_v)
        assert r_v <= 1.0, f"{op}({a!r}): value {v!r}, SciPy fp64 {want!r}"
        assert v.view(np.uint32) == _forward(op, a)[0].view(np.uint32), (op, a)               # the same float function, bit for bit
        r_p = error_ratio(pa, want_p, partial_bound(op, want_p))
        worst_p = max(worst_p, r_p if abs(want_p) >= NORMAL_CUT else 0.0)
        assert r_p <= 1.0, f"{op}({a!r}): partial {pa!r}, closed form {want_p!r}"
        assert pa == _forward(op, a, 1.0)[1], (op, a)                   # (the probe's report adds the partial to 0: a -0 comes back as 0)
    for a in _operands(op)[::11]:                                       # a constant: the same value, no record, no partial
        v, pa, n = _tape(op, a, a_const=True)
        assert v.view(np.uint32) == _tape(op, a)[0].view(np.uint32) and pa == 0.0 and n == 0, (op, a)
    print(f"\n[custom_normal] tape {op}: worst value error {worst_v:.3f} of its bound, worst partial error {worst_p:.3f} of its bound "
          f"(over partials of at least 1e-37)")


# ---- the exact rules --------------------------------------------------------------------------------------------------------------------
def _within(op, a):
    v, t = _forward(op, a, 1.0)
    want, want_p = _want(op, f32(a))
    assert np.isfinite(v) and np.isfinite(t), (op, a, v, t)
    assert error_ratio(v, want, value_bound(op, want)) <= 1.0, (op, a, v, want)
    assert error_ratio(t, want_p, partial_bound(op, want_p)) <= 1.0, (op, a, t, want_p)
    return v, t


def test_log_ndtr_at_its_ends():
    inf = float("inf")
    assert _forward("log_ndtr", inf, 3.0) == (0.0, 0.0)
    assert _tape("log_ndtr", inf) == (0.0, 0.0, 1)
    assert _forward("log_ndtr", -inf, 1.0)[0] == -inf and _tape("log_ndtr", -inf)[0] == -inf
    for a in (-14.5, -20.0, -38.0, -1e10):
        v, t = _within("log_ndtr", a)
        assert t > 0
    # finite as long as x^2 / 2 is, -inf beyond; the partial phi / Phi ~ -x stays finite and positive for every finite x
    edge = f32(cases.HALF_SQUARE_OVERFLOW)
    assert np.isfinite(_forward("log_ndtr", np.nextafter(edge, f32(0)))[0])
    assert _forward("log_ndtr", -1e30)[0] == -inf
    for a in (-1e30, -FLT_MAX):
        t = _forward("log_ndtr", a, 1.0)[1]
        assert np.isfinite(t) and abs(float(t) / -a - 1.0) <= 16 * EPS32, (a, t)
    assert _forward("ndtr", inf, 1.0) == (1.0, 0.0) and _forward("ndtr", -inf, 1.0) == (0.0, 0.0)
    assert _forward("ndtr", 0.0, 2.0)[0] == 0.5


def test_erfcx_at_its_ends():
    inf = float("inf")
    v, t = _within("erfcx", 1e30)
    assert v > 0
    for a in (1e18, FLT_MAX):
        v, _ = _forward("erfcx", a)
        assert v > 0 and abs(float(v) * float(f32(a)) * np.sqrt(np.pi) - 1.0) <= 1e-4, (a, v)    # 1 / (x sqrt(pi)); FLT_MAX: a subnormal
    assert _forward("erfcx", inf) [0] == 0.0
    assert _forward("erfcx", -10.0, 1.0) == (inf, -inf)
    assert _tape("erfcx", -10.0) == (inf, -inf, 1)
    assert _forward("erfcx", -inf, 1.0) == (inf, -inf)
    assert _forward("erfcx", 0.0, 1.0)[0] == 1.0


def test_nan_in_gives_nan_out():
    for op in EXTRA_OPS:
        v, t = _forward(op, float("nan"), 1.0)
        assert np.isnan(v) and np.isnan(t), op
        v, pa, n = _tape(op, float("nan"))
        assert np.isnan(v) and np.isnan(pa) and n == 1, op


def test_asin_and_acos_at_and_beyond_one():
    inf = float("inf")
    for spelling in ("asin", "asinf"):
        v, t = _forward(spelling, 1.0, 1.0)
        assert abs(float(v) - np.pi / 2) <= 4 * np.spacing(f32(np.pi / 2)) and t == inf
        assert _tape(spelling, -1.0)[1] == inf
        assert np.isnan(_forward(spelling, 1.5, 1.0)[0]) and np.isnan(_forward(spelling, 1.5, 1.0)[1])
    for spelling in ("acos", "acosf"):
        assert _forward(spelling, 1.0, 1.0) == (0.0, -inf)
        assert np.isnan(_forward(spelling, -1.5, 1.0)[0]) and np.isnan(_tape(spelling, -1.5)[1])


# ---- the reason for the change --------------------------------------------------------------------------------------------------------
def test_the_plain_form_is_minus_infinity_where_log_ndtr_meets_its_bound():
    """log(0.5 erfc(-x / sqrt 2)) through the probes that were there before: erfcf has underflowed at 14.5 / sqrt(2) = 10.25."""
    for x in (-14.5, -20.0, -38.0):
        z = f32(-x) * f32(0.70710678)
        tail, d_tail = special._forward("erfc", z, 1.0)
        assert tail == 0.0
        plain, d_plain = fwd._probe("log", f32(0.5) * tail, d_tail)
        assert plain == -np.inf and not np.isfinite(d_plain)
        _within("log_ndtr", x)
    # the fp64 values the issue quotes
    for x, want in ((-14.5, -108.72), (-20.0, -203.92), (-38.0, -726.56)):
        assert abs(float(_forward("log_ndtr", x)[0]) - want) < 0.01


# ---- the compiler: every new function in every mode -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("check,mode", special.CHECKS)
def test_every_new_function_compiles_in_every_mode(check, mode):
    from gmmvi_amd import hip_ops
    rc, log = getattr(hip_ops, check)(cases.every_source(mode), "gfx950")
    assert rc == 0, log


@pytest.mark.parametrize("check,name", [("custom_target_check_data", n) for n in sorted(cases.DATA_SOURCES)]
                         + [("custom_target_check_data_tape", n) for n in sorted(cases.DATA_SOURCES)]
                         + [("custom_target_check_autodiff", "normals"), ("custom_target_check_tape", "normals")])
def test_case_sources_compile_for_gfx950(check, name):
    from gmmvi_amd import hip_ops
    source = cases.NORMALS_SRC if name == "normals" else cases.DATA_SOURCES[name]
    rc, log = getattr(hip_ops, check)(source, "gfx950")
    assert rc == 0, log


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def test_restatements_agree_with_finite_differences():
    from gmmvi_amd import _lib
    assert len(_lib.EXTRA_OPS) == len(EXTRA_OPS)                          # the restatements restate sources that need the functions
    special._finite_differences(*cases.build_normals(9), "normals")
    tgt, x = cases.build_data_case(cases.Case("tobit", 4, 9, 12, 0, None, 0))
    assert (tgt.data[:, -1] == 0).any() and (tgt.data[:, -1] > 0).any()
    special._finite_differences(tgt, x, "tobit")
    # probit away from the planted row: there |d lp / d eta| is 20 and the fixed step of the rule is too coarse for its curvature
    tgt, x = cases.build_data_case(cases.Case("probit", 4, 9, 12, 0, None, 0))
    assert abs(float(tgt.data[0, :-1].astype(np.float64) @ x[0].astype(np.float64)) - cases.PLANTED_ETA) < 1e-4 and tgt.data[0, -1] == 1
    away = cases.Probit(tgt.data[1:], tgt.params(), d=4)
    special._finite_differences(away, x, "probit")
