"""User-defined device targets differentiated on a tape, the part that needs no GPU: the run-time compiler builds source + tape
text for gfx950 without a device (gmmvi_custom_target_check_tape), compile errors come back as argument errors with the user's
own line numbers, every rule of the tape's number type is evaluated on a host tape through gmmvi_tape_probe against NumPy and
against the forward mode's probe, the slab plan keeps its promises, and DeviceTapeLNPDF rejects bad arguments before it touches
the device.

Probe bounds (those of tests/test_custom_autodiff_host.py, whose rules and operand grid are used): values within 4 ulp of
NumPy's fp32 function; each recorded partial within 16 * eps32 * |partial| of the fp64 closed form at the fp32 operands, and
within the same bound of the forward mode's tangent for (da, db) = (1, 0) and (0, 1)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import custom_tape_cases as cases
import test_custom_autodiff_host as fwd
from helpers import use_host_context

ERR_ARG = -2
EPS32 = fwd.EPS32
f32 = np.float32


# ---- the compiler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_case_sources_compile_for_gfx950(name):
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_tape(cases.SOURCES[name], "gfx950")
    assert rc == 0, log


def test_new_case_sources_also_compile_in_the_forward_mode():
    """The contract is one: a density text is valid in both modes."""
    from gmmvi_amd import hip_ops
    for name in ("chain", "branchy"):
        rc, log = hip_ops.custom_target_check_autodiff(cases.SOURCES[name], "gfx950")
        assert rc == 0, log


def test_the_mode_macro_is_defined():
    from gmmvi_amd import hip_ops
    text = "// a density\n#ifndef GMMVI_CUSTOM_TAPE\n#error no tape macro\n#endif\n" + cases.CHAIN_SRC
    assert hip_ops.custom_target_check_tape(text, "gfx950")[0] == 0
    rc, log = hip_ops.custom_target_check_autodiff(text, "gfx950")
    assert rc == ERR_ARG and "no tape macro" in log


def test_syntax_error_is_an_argument_error_with_the_users_line():
    from gmmvi_amd import _lib, hip_ops
    lines = cases.CHAIN_SRC.split("\n")
    bad_line = next(i for i, text in enumerate(lines) if "const T t" in text)
    lines[bad_line] = "        const T t = x[i] * ;"
    rc, log = hip_ops.custom_target_check_tape("\n".join(lines), "gfx950")
    assert rc == ERR_ARG
    assert f":{bad_line + 1}:" in log, log
    assert "error" in log
    assert log.strip() in _lib.load().gmmvi_last_error(None).decode()
    rc, log = hip_ops.custom_target_check_tape("int broken = ;\n" + cases.CHAIN_SRC, "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_target.hip:1:" in log, log


def test_source_without_the_function_names_it():
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_tape("__device__ float something_else(const float* x) { return x[0]; }\n", "gfx950")
    assert rc == ERR_ARG and "does not define gmmvi_user_density" in log
    rc, log = hip_ops.custom_target_check_tape(cases.auto.base.ROSENBROCK_SRC, "gfx950")     # a hand-written-gradient source
    assert rc == ERR_ARG and "does not define gmmvi_user_density" in log


def test_function_outside_the_surface_is_a_compile_error():
    from gmmvi_amd import hip_ops
    src = cases.auto.ROSENBROCK_SRC
    rc, log = hip_ops.custom_target_check_tape(src.replace("return -(", "return lgammaf(u) - ("), "gfx950")
    assert rc == ERR_ARG
    assert log.strip() and "lgammaf" in log
    rc, log = hip_ops.custom_target_check_tape(src.replace("return -(", "return lgammaf(a) - ("), "gfx950")
    assert rc == 0, log


def test_null_arguments_are_argument_errors():
    from gmmvi_amd import _lib
    lib = _lib.load()
    assert lib.gmmvi_custom_target_check_tape(None, b"gfx950", None, 0) == ERR_ARG
    assert lib.gmmvi_custom_target_check_tape(b"", None, None, 0) == ERR_ARG
    buf = C.create_string_buffer(b"\xff" * 16, 16)
    assert lib.gmmvi_custom_target_check_tape(b"nonsense", b"gfx950", buf, 16) == ERR_ARG
    assert len(buf.value) == 15
    v, pa, pb, n = C.c_float(), C.c_float(), C.c_float(), C.c_int()
    outs = [C.byref(v), C.byref(pa), C.byref(pb), C.byref(n)]
    for missing in range(4):
        args = list(outs)
        args[missing] = None
        assert lib.gmmvi_tape_probe(0, 1.0, 1.0, 0, 0, *args) == ERR_ARG
    for bad in (-1, len(_lib.AUTODIFF_OPS), 10 ** 6):
        assert lib.gmmvi_tape_probe(bad, 1.0, 1.0, 0, 0, *outs) == ERR_ARG
        assert "unknown operation" in lib.gmmvi_last_error(None).decode()
    assert lib.gmmvi_tape_probe(len(_lib.AUTODIFF_OPS) - 1, 1.0, 1.0, 0, 0, *outs) == 0
    s, l = C.c_int(), C.c_int()
    assert lib.gmmvi_custom_tape_plan(10, 10, 0, None, C.byref(l)) == ERR_ARG
    assert lib.gmmvi_custom_tape_plan(10, 10, 0, C.byref(s), None) == ERR_ARG


def test_constants_and_symbols():
    from gmmvi_amd import _lib, hip_ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmmvi_hip.h")).read()
    for name in ("RECORD_BYTES", "DEFAULT_CAPACITY", "SCRATCH_BYTES"):
        assert int(re.search(rf"#define GMMVI_CUSTOM_TAPE_{name} (\d+)", header).group(1)) == getattr(_lib, "CUSTOM_TAPE_" + name)
    assert _lib.CUSTOM_TAPE_RECORD_BYTES == 16 + 4 and _lib.CUSTOM_TAPE_SCRATCH_BYTES == 2 << 30
    for symbol in ("gmmvi_custom_target_check_tape", "gmmvi_custom_target_compile_tape", "gmmvi_custom_tape_plan",
                   "gmmvi_custom_tape_length", "gmmvi_target_custom_tape", "gmmvi_tape_probe"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    assert "tape" in hip_ops.CUSTOM_TARGET_MODES and "reverse" not in hip_ops.CUSTOM_TARGET_MODES
    assert [f[0] for f in _lib.TargetSpec._fields_][-2:] == ["custom", "custom_params"]       # no new struct, no new target kind


# ---- the probe -----------------------------------------------------------------------------------------------------------
def _probe(op, a, b=0.0, a_const=False, b_const=False):
    from gmmvi_amd import _lib
    v, pa, pb, n = C.c_float(), C.c_float(), C.c_float(), C.c_int()
    rc = _lib.load().gmmvi_tape_probe(_lib.AUTODIFF_OPS.index(op), a, b, int(a_const), int(b_const), C.byref(v), C.byref(pa),
                                      C.byref(pb), C.byref(n))
    assert rc == 0, op
    return f32(v.value), f32(pa.value), f32(pb.value), n.value


def _operands(op):
    """-> [(a, b)] of the forward test's grid, inside the rule's domain."""
    return sorted({(a, b) for a, b, _, _ in fwd._grid(op)})


@pytest.mark.parametrize("op", fwd._all_ops())
def test_probe_values_and_partials(op):
    rule, form = fwd._split(op)
    worst_ulp, worst_p, worst_f = 0.0, 0.0, 0.0
    for a, b in _operands(op):
        v, pa, pb, n = _probe(op, a, b)
        a32, b32 = f32(a), f32(b)
        if rule in fwd.COMPARISONS:
            assert v == f32(fwd.COMPARISONS[rule](a32, b32)) and (pa, pb, n) == (0.0, 0.0, 0), (op, a, b)
            continue
        value, dfa, dfb, _ = fwd.RULES[rule]
        with np.errstate(all="ignore"):
            want = f32(value(a32, b32))
            ulps = fwd._ulps(v, want)
            a64, b64 = np.float64(a32), np.float64(b32)
            want_a = 0.0 if form == "ft" else float(dfa(a64, b64))
            want_b = 0.0 if form == "tf" or dfb is None else float(dfb(a64, b64))
        worst_ulp = max(worst_ulp, ulps)
        assert ulps <= 4.0, f"{op}({a}, {b}): value {v!r}, NumPy fp32 {want!r}, {ulps:.1f} ulp"
        assert n == (0 if rule == "value" else 1), (op, a, b, n)
        fa, fb = fwd._probe(op, a, 1.0, b, 0.0)[1], fwd._probe(op, a, 0.0, b, 1.0)[1]
        for which, got, want_p, forward in (("a", pa, want_a, fa), ("b", pb, want_b, fb)):
            bound = 16.0 * EPS32 * abs(want_p)
            err, err_f = abs(float(got) - want_p), abs(float(got) - float(forward))
            if bound > 0:
                worst_p, worst_f = max(worst_p, err / bound), max(worst_f, err_f / bound)
            assert err <= bound, f"{op}({a}, {b}): partial by {which} {got!r}, closed form {want_p!r}, error {err:.3e} > {bound:.3e}"
            assert err_f <= bound, f"{op}({a}, {b}): partial by {which} {got!r}, forward mode {forward!r}, {err_f:.3e} > {bound:.3e}"
    print(f"\n[custom_tape] {op}: worst value error {worst_ulp:.2f} ulp (bound 4), worst partial error {worst_p:.3f} of its bound "
          f"against the closed form, {worst_f:.3f} against the forward mode")


@pytest.mark.parametrize("op", fwd._all_ops())
def test_probe_constants_get_no_partial_and_make_no_record(op):
    rule, form = fwd._split(op)
    binary = rule in fwd.COMPARISONS or fwd.RULES[rule][2] is not None
    makes_records = rule not in fwd.COMPARISONS and rule != "value"
    for a, b in _operands(op)[::7]:
        full = _probe(op, a, b)
        for a_const, b_const in ((True, False), (False, True), (True, True)):
            v, pa, pb, n = _probe(op, a, b, a_const, b_const)
            assert v == full[0] or (np.isnan(v) and np.isnan(full[0])), (op, a, b)
            a_moves = not a_const and form != "ft"
            b_moves = not b_const and form != "tf" and binary
            if a_const or form == "ft":
                assert pa == 0.0, (op, a, b, "a is a constant and has a partial")
            if b_const or form == "tf" or not binary:
                assert pb == 0.0, (op, a, b, "b is a constant and has a partial")
            assert n == (1 if makes_records and (a_moves or b_moves) else 0), (op, a, b, a_const, b_const, n)
            if a_moves and makes_records and not (np.isnan(pa) and np.isnan(full[1])):
                assert pa == full[1], (op, a, b)
            if b_moves and makes_records and rule != "pow" and not (np.isnan(pb) and np.isnan(full[2])):
                assert pb == full[2], (op, a, b)


def test_probe_tie_rules_hold_exactly():
    for spelling in ("fabs", "fabsf"):
        for zero in (0.0, -0.0):
            v, pa, _, n = _probe(spelling, zero)
            assert v == 0.0 and not np.signbit(v) and pa == 0.0 and n == 1
        assert _probe(spelling, 2.0)[:2] == (2.0, 1.0) and _probe(spelling, -2.0)[:2] == (2.0, -1.0)
    for name in ("fmax", "fmin", "fmaxf", "fminf"):
        for tie in (1.25, 0.0, -7.0):
            assert _probe(name, tie, tie)[:3] == (f32(tie), 1.0, 0.0)              # the first operand takes the partial
            assert _probe(name + "_tf", tie, tie)[:3] == (f32(tie), 1.0, 0.0)
            assert _probe(name + "_ft", tie, tie)[:3] == (f32(tie), 0.0, 0.0)      # first a float: a constant, it wins the tie
    assert _probe("fmax", 1.0, 2.0)[:3] == (2.0, 0.0, 1.0) and _probe("fmax", 2.0, 1.0)[:3] == (2.0, 1.0, 0.0)
    assert _probe("fmin", 1.0, 2.0)[:3] == (1.0, 1.0, 0.0) and _probe("fmin", 2.0, 1.0)[:3] == (1.0, 0.0, 1.0)
    # pow: exponent 0 has partial 0 by the base even at a = 0; a constant exponent keeps a negative base usable
    assert _probe("pow_tf", 0.0, 0.0)[:2] == (1.0, 0.0)
    assert _probe("pow", -2.0, 2.0, b_const=True) == (4.0, -4.0, 0.0, 1)
    v, pa, pb, n = _probe("pow", -2.0, 2.0)
    assert (v, pa, n) == (4.0, -4.0, 1) and np.isnan(pb)                            # an exponent that moves takes ln(a)
    # the same node twice: both partials belong to it
    assert _probe("value", 1.5) == (1.5, 0.0, 0.0, 0)


# ---- the slab plan ---------------------------------------------------------------------------------------------------------
def test_plan_promises():
    from gmmvi_amd import _lib, hip_ops
    per_wave = 64 * _lib.CUSTOM_TAPE_RECORD_BYTES
    for n in (1, 63, 64, 65, 200, 1000, 10000, 123457):
        for cap in (1, 8, 1020, 20480):
            for budget in (cap * per_wave, cap * per_wave + 1, 3 * cap * per_wave, 7 * cap * per_wave - 1, 1 << 31, 0):
                slabs, lanes = hip_ops.custom_tape_plan(n, cap, budget)
                assert lanes % 64 == 0 and lanes >= 64 and slabs >= 1
                assert slabs * lanes >= n
                assert (slabs - 1) * lanes < n, "the last slab is empty"
                assert lanes * cap * _lib.CUSTOM_TAPE_RECORD_BYTES <= (budget or _lib.CUSTOM_TAPE_SCRATCH_BYTES)
                if lanes * (slabs - 1) > 0:                      # more than one slab only where one would not fit
                    assert ((n + 63) // 64) * cap * per_wave > (budget or _lib.CUSTOM_TAPE_SCRATCH_BYTES)
    assert hip_ops.custom_tape_plan(200, 1020, 64 * 1020 * 20) == (4, 64)
    assert hip_ops.custom_tape_plan(200, 1020, 0) == (1, 256)
    lib = _lib.load()
    s, l = C.c_int(), C.c_int()
    assert lib.gmmvi_custom_tape_plan(200, 1020, 64 * 1020 * 20 - 1, C.byref(s), C.byref(l)) == ERR_ARG
    message = lib.gmmvi_last_error(None).decode()
    assert "1020" in message and str(64 * 1020 * 20) in message
    for n, cap in ((0, 8), (-1, 8), (8, 0), (8, -2)):
        assert lib.gmmvi_custom_tape_plan(n, cap, 0, C.byref(s), C.byref(l)) == ERR_ARG


# ---- the references ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d", [("chain", 2), ("chain", 7), ("branchy", 4)])
def test_restatements_agree_with_finite_differences(name, d):
    """The rule of test_restatements_agree_with_finite_differences (tests/test_custom_target_host.py) on the two new densities."""
    tgt, x = cases.build_case(name, d, 9)
    x = x.astype(np.float64)
    _, g = tgt.log_density_and_grad(x)
    h = 1e-6
    for i in range(d):
        e = np.zeros(d); e[i] = h
        fd = (tgt.log_density(x + e) - tgt.log_density(x - e)) / (2 * h)
        np.testing.assert_allclose(g[:, i], fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} coordinate {i}")


def test_kernel_cases_cover_the_issues_table():
    from gmmvi_amd import _lib
    by_name = {}
    for name, d, n in cases.KERNEL_CASES + [cases.MAX_DIM_CASE]:
        by_name.setdefault(name, set()).add((d, n))
    assert {n for _, n in by_name["rosenbrock"]} == {1, 63, 64, 65, 200}
    assert by_name["quartic"] == {(d, 70) for d in (3, 15, 16, 17, 50, 120)}
    assert by_name["planar"] == {(10, 300)} and by_name["allops"] == {(6, 200)} and by_name["branchy"] == {(4, 130)}
    assert by_name["chain"] == {(2, 70), (513, 70), (4096, 70), (_lib.MAX_DIM_DIAG, 2)}
    # branchy: both tape lengths in every wave of its case
    _, x = cases.build_case("branchy", 4, 130)
    for w in range(0, 130, 64):
        signs = x[w:w + 64, 0] > 0
        assert signs.any() and not signs.all()


# ---- the class -------------------------------------------------------------------------------------------------------------
def test_device_tape_lnpdf_argument_errors(monkeypatch):
    from gmmvi_amd import _lib
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    use_host_context(monkeypatch, device_lnpdf)
    compiled = []
    monkeypatch.setattr(device_lnpdf.hip_ops, "custom_target_compile", lambda ctx, source, **kw: compiled.append(kw) or object())
    for bad in (0, -3, 2.5, _lib.MAX_DIM_DIAG + 1):
        with pytest.raises(ValueError, match="num_dimensions"):
            device_lnpdf.DeviceTapeLNPDF(cases.CHAIN_SRC, bad, params=[2.0, 0.5])
    with pytest.raises(ValueError, match="one-dimensional"):
        device_lnpdf.DeviceTapeLNPDF(cases.CHAIN_SRC, 2, params=np.ones((2, 2)))
    for name in ("tape_capacity", "scratch_bytes"):
        for bad in (0, -1, 2.5):
            with pytest.raises(ValueError, match=name):
                device_lnpdf.DeviceTapeLNPDF(cases.CHAIN_SRC, 2, params=[2.0, 0.5], **{name: bad})
    assert compiled == []
    # D = 513 and the largest diagonal dimension are taken; the forward mode refuses both
    for d in (513, _lib.MAX_DIM_DIAG):
        t = device_lnpdf.DeviceTapeLNPDF(cases.CHAIN_SRC, d, params=[2.0, 0.5], tape_capacity=100, scratch_bytes=1 << 20)
        assert t.get_num_dimensions() == d and (t.tape_capacity, t.scratch_bytes) == (100, 1 << 20)
        with pytest.raises(ValueError, match="512"):
            device_lnpdf.DeviceAutodiffLNPDF(cases.CHAIN_SRC, d)
    assert compiled == [{"mode": "tape"}] * 2


def test_class_facts():
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceAutodiffLNPDF, DeviceLNPDF, DeviceTapeLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi.experiments.target_distributions.device_lnpdf import DeviceTapeLNPDF as Alias
    assert Alias is DeviceTapeLNPDF
    assert issubclass(DeviceTapeLNPDF, DeviceLNPDF) and not issubclass(DeviceTapeLNPDF, DeviceAutodiffLNPDF)
    assert DeviceTapeLNPDF.log_density_and_grad is not LNPDF.log_density_and_grad
    assert DeviceTapeLNPDF.log_density is not DeviceLNPDF.log_density
    assert not hasattr(DeviceTapeLNPDF, "_fast_path_target")
    assert DeviceTapeLNPDF.gradient_on_demand is True
    assert type(DeviceTapeLNPDF.__new__(DeviceTapeLNPDF, "", 2, tape_capacity=4)) is DeviceTapeLNPDF
    # the classes beside it are what they were
    assert hasattr(DeviceAutodiffLNPDF, "_fast_path_target") and not hasattr(DeviceLNPDF, "_fast_path_target")


def test_unknown_mode_names_still_raise():
    from gmmvi_amd import hip_ops
    for mode in ("reverse", "Tape", ""):
        with pytest.raises(ValueError, match="mode"):
            hip_ops.custom_target_compile(None, cases.CHAIN_SRC, mode=mode)
