"""The vector primitives of user-defined device targets, the part that needs no GPU: every operation of _lib.VECTOR_OPS through
gmmvi_autodiff_probe_vector and gmmvi_tape_probe_vector against an fp64 NumPy restatement at the fp32 operands, the record count
and the exact gradients of the tape, one source per mode that calls all three primitives compiled for gfx950 without a device,
and the restated test targets against central differences.

Probe bounds.  Values: VALUE_EPS * eps32 * sum |terms| (tests/custom_vector_cases.py derives the multiple from the order
include/gmmvi_hip.h states; the fp32 NumPy restatement in that order is shown to stay inside it first).  Tangents and gradient
entries: the rule of tests/test_custom_autodiff_host.py, the fp64 closed form within 16 * eps32 * |partial|."""
import ctypes as C

import numpy as np
import pytest

import custom_vector_cases as cases
from gmmvi_amd import _lib, hip_ops

EPS32 = cases.EPS32
ERR_ARG = -2
PRIMITIVE_CASES = cases.primitive_cases()


def test_the_list_and_the_symbols():
    assert _lib.VECTOR_OPS == ("dot", "sqdist", "sumsq")
    for symbol in ("gmmvi_autodiff_probe_vector", "gmmvi_tape_probe_vector"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    lib = _lib.load()
    x = np.ones(4, np.float32)
    v, n, t, g = C.c_float(), C.c_int(), np.zeros(cases.W, np.float32), np.zeros(4, np.float32)
    xp, tp, gp = (a.ctypes.data_as(C.c_void_p) for a in (x, t, g))
    for bad in (-1, len(_lib.VECTOR_OPS)):
        assert lib.gmmvi_autodiff_probe_vector(bad, xp, 4, 0, 4, xp, 0.0, 0, C.byref(v), tp) == ERR_ARG
        assert lib.gmmvi_tape_probe_vector(bad, xp, 4, 0, 4, xp, 0.0, C.byref(v), gp, C.byref(n)) == ERR_ARG
    for first, count in ((-1, 2), (3, 2), (0, 5)):                      # a range that leaves [0, D)
        assert lib.gmmvi_autodiff_probe_vector(0, xp, 4, first, count, xp, 0.0, 0, C.byref(v), tp) == ERR_ARG
        assert lib.gmmvi_tape_probe_vector(0, xp, 4, first, count, xp, 0.0, C.byref(v), gp, C.byref(n)) == ERR_ARG
    assert lib.gmmvi_autodiff_probe_vector(0, None, 4, 0, 4, xp, 0.0, 0, C.byref(v), tp) == ERR_ARG
    assert lib.gmmvi_autodiff_probe_vector(0, xp, 4, 0, 4, None, 0.0, 0, C.byref(v), tp) == ERR_ARG
    assert lib.gmmvi_tape_probe_vector(1, xp, 4, 0, 4, None, 0.0, C.byref(v), gp, C.byref(n)) == ERR_ARG
    assert lib.gmmvi_tape_probe_vector(2, xp, 4, 0, 4, None, 0.0, C.byref(v), gp, C.byref(n)) == 0   # gmmvi_sumsq takes no c
    assert lib.gmmvi_autodiff_probe_vector(len(_lib.VECTOR_OPS) - 1, xp, 4, 0, 4, None, 0.0, 0, C.byref(v), tp) == 0


@pytest.mark.parametrize("op", _lib.VECTOR_OPS)
def test_every_primitive_through_both_probes(op):
    worst_32 = worst_v = worst_g = 0.0
    for d, first, n in PRIMITIVE_CASES:
        x, c, center = cases.primitive_operands(d)
        terms, partials = cases.terms64(op, x, first, n, c, center)
        want, scale = float(terms.sum()), float(np.abs(terms).sum())
        bound = cases.VALUE_EPS * EPS32 * scale
        want_g = np.zeros(d)
        want_g[first:first + n] = partials
        tag = f"{op} D={d} first={first} n={n}"
        # the fp32 restatement in the header's order stays inside the bound
        e_32 = abs(float(cases.value32(op, x, first, n, c, center)) - want)
        assert e_32 <= bound, f"{tag}: the fp32 restatement misses the bound: {e_32:.3e} > {bound:.3e}"
        values, tangents = cases.probe_forward_gradient(op, x, first, n, c, center)
        v_t, g_t, records = cases.probe_tape(op, x, first, n, c, center)
        # one value function: every pass, the tape and the restatement in the header's order give the same bits
        for v in values + [v_t]:
            assert np.float32(v).view(np.uint32) == cases.value32(op, x, first, n, c, center).view(np.uint32), tag
            assert abs(float(v) - want) <= bound, f"{tag}: value {v!r}, fp64 {want!r}"
        assert records == (1 if n >= 1 else 0), tag
        for name, g in (("tangents", tangents), ("tape gradient", g_t)):
            err = np.abs(g.astype(np.float64) - want_g)
            assert np.all(err <= 16.0 * EPS32 * np.abs(want_g)), f"{tag}: {name} {g!r}, closed form {want_g!r}"
            if np.any(want_g != 0):
                worst_g = max(worst_g, float((err[want_g != 0] / (16.0 * EPS32 * np.abs(want_g[want_g != 0]))).max()))
        np.testing.assert_array_equal(tangents.view(np.uint32), g_t.view(np.uint32), err_msg=tag)
        if scale > 0:
            worst_32, worst_v = max(worst_32, e_32 / bound), max(worst_v, abs(float(v_t) - want) / bound)
        if n == 0:
            assert np.float32(v_t).view(np.uint32) == 0 and not np.any(g_t.view(np.uint32)), tag     # the constant +0
    print(f"\n[custom_vector] {op}: worst value error {worst_v:.3f} of its bound ({cases.VALUE_EPS:g} eps32 sum|terms|; the fp32 "
          f"restatement {worst_32:.3f}), worst gradient error {worst_g:.3f} of its bound")


def test_dot_gradient_is_the_coefficients_bit_for_bit():
    for d, first, n in PRIMITIVE_CASES:
        x, c, center = cases.primitive_operands(d)
        assert np.all(c != 0)
        want = np.zeros(d, np.float32)
        want[first:first + n] = c[:n]
        _, g_t, records = cases.probe_tape("dot", x, first, n, c, center)
        _, tangents = cases.probe_forward_gradient("dot", x, first, n, c, center)
        assert records == (1 if n else 0)
        inside = slice(first, first + n)
        np.testing.assert_array_equal(tangents[inside].view(np.uint32), want[inside].view(np.uint32))
        np.testing.assert_array_equal(g_t.view(np.uint32), want.view(np.uint32))      # the sweep adds c[i] * 1 to a zeroed entry
        outside = np.ones(d, bool)
        outside[inside] = False
        assert not np.any(g_t[outside].view(np.uint32)) and not np.any(tangents[outside].view(np.uint32))


def test_sqdist_and_sumsq_gradients_are_exact_where_the_difference_is():
    """2 (x - c) is one rounding of the difference and an exact doubling; with adjoint 1 the sweep adds it to 0."""
    for d, first, n in PRIMITIVE_CASES:
        x, c, center = cases.primitive_operands(d)
        for op, sub in (("sqdist", c[:n]), ("sumsq", center)):
            want = np.zeros(d, np.float32)
            want[first:first + n] = np.float32(2) * (x[first:first + n] - sub).astype(np.float32)
            _, g_t, _ = cases.probe_tape(op, x, first, n, c, center)
            np.testing.assert_array_equal(g_t, want)


@pytest.mark.parametrize("mode", ["hand", "autodiff", "tape", "data", "data_tape"])
def test_a_source_with_all_three_primitives_compiles_in_every_mode(mode):
    check = {"hand": hip_ops.custom_target_check, "autodiff": hip_ops.custom_target_check_autodiff,
             "tape": hip_ops.custom_target_check_tape, "data": hip_ops.custom_target_check_data,
             "data_tape": hip_ops.custom_target_check_data_tape}[mode]
    status, log = check(cases.ALL_THREE[mode])
    assert status == 0, log


def test_every_test_source_compiles():
    for name, src in cases.SOURCES.items():
        for check in (hip_ops.custom_target_check_data, hip_ops.custom_target_check_data_tape):
            status, log = check(src)
            assert status == 0, f"{name}: {log}"
    for name, src in cases.DENSITY_SOURCES.items():
        for check in (hip_ops.custom_target_check_autodiff, hip_ops.custom_target_check_tape):
            status, log = check(src)
            assert status == 0, f"{name}: {log}"
    for name, src in cases.HAND_SOURCES.items():
        status, log = hip_ops.custom_target_check(src)
        assert status == 0, f"{name}: {log}"


def test_a_dual_or_a_node_as_coefficients_does_not_compile():
    """Products of two differentiated vectors are out of scope: c is const float*, so a T there is a compile error."""
    src = ("template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
           "    T h[2] = {x[0], x[1]};\n    return gmmvi_dot(x, 0, h, 2);\n}\n")
    for check in (hip_ops.custom_target_check_autodiff, hip_ops.custom_target_check_tape):
        status, log = check(src)
        assert status == ERR_ARG and "gmmvi_dot" in log


def _central_differences(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[i] = h
        g[:, i] = (f(x + e) - f(x - e)) / (2 * h)
    return g


@pytest.mark.parametrize("name,d", [("logit_vec", 7), ("rbf_vec", 7), ("mixed", 7), ("single", 5), ("ranges", cases.RANGES_D)])
def test_restated_densities_agree_with_central_differences(name, d):
    tgt, x = cases.build_density_case(name, d, 6)
    x = x.astype(np.float64)
    _, g = tgt.log_density_and_grad(x)
    fd = _central_differences(lambda y: tgt.log_density_and_grad(y)[0], x)
    np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=name)


@pytest.mark.parametrize("name", ["logit_vec", "rbf_vec", "mixed"])
def test_restated_data_targets_agree_with_central_differences(name):
    for batch in (None, 5):
        tgt, x = cases.build_data_case(cases.Case(name, 7, 6, 11, 0, batch, 2))
        x = x.astype(np.float64)
        _, g = tgt.evaluate(x)
        fd = _central_differences(lambda y: tgt.evaluate(y)[0], x)
        np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} batch {batch}")


def test_logit_vec_restates_logit():
    """The same rows and x: the two targets are the same function, their fp64 values agree to fp64 rounding."""
    c = cases.Case("logit_vec", 17, 9, 11, 0, None, 0)
    a, x = cases.build_data_case(c)
    b, x_b = cases.build_data_case(c._replace(name="logit"))
    np.testing.assert_array_equal(x, x_b)
    np.testing.assert_array_equal(a.data, b.data)
    for u, v in zip(a.evaluate(x.astype(np.float64)), b.evaluate(x.astype(np.float64))):
        np.testing.assert_allclose(u, v, rtol=1e-12, atol=1e-12)
