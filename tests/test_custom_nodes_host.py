"""The primitives of user-defined device targets on arrays of the mode's number type (gmmvi_wdot, gmmvi_logsumexp), the part that
needs no GPU: both operations of _lib.NODE_OPS through gmmvi_autodiff_probe_nodes and gmmvi_tape_probe_nodes against an fp64
NumPy restatement at the fp32 operands, the slot counts of the node-array record, the edges, the sources of the test targets
compiled for gfx950 without a device, and the restated test targets against central differences.

Probe bounds (tests/custom_nodes_cases.py derives them from the order include/gmmvi_hip.h states).  gmmvi_wdot's value: the
bound of gmmvi_dot, VALUE_EPS * eps32 * sum |terms|.  gmmvi_logsumexp's value: logsumexp_value_bound, absolute.  Gradient
entries: gradient_eps(op, n) * eps32 * the sum over the paths of |contribution|.  The fp32 NumPy restatement in the stated order
is shown to stay inside the value bound first."""
import ctypes as C
import math

import numpy as np
import pytest

import custom_nodes_cases as cases
import custom_vector_cases as vec
from gmmvi_amd import _lib, hip_ops

EPS32 = cases.EPS32
ERR_ARG = -2
PROBE_CASES = cases.probe_cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_list_and_the_symbols():
    assert _lib.NODE_OPS == ("wdot", "logsumexp")
    assert _lib.VECTOR_OPS == ("dot", "sqdist", "sumsq")                # the existing list stays as it is
    for symbol in ("gmmvi_autodiff_probe_nodes", "gmmvi_tape_probe_nodes", "gmmvi_autodiff_probe_nodes_inputs",
                   "gmmvi_tape_probe_nodes_inputs"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    lib = _lib.load()
    x = np.ones(80, np.float32)
    v, r, t, g = C.c_float(), C.c_int(), np.zeros(cases.W, np.float32), np.zeros(80, np.float32)
    xp, tp, gp = (a.ctypes.data_as(C.c_void_p) for a in (x, t, g))

    def forward(op=0, x=xp, d=8, first=0, n=4, src=4, every=0, seed=0, value=C.byref(v), out=tp):
        return lib.gmmvi_autodiff_probe_nodes(op, x, d, first, n, src, every, seed, value, out)

    def tape(op=0, x=xp, d=8, first=0, n=4, src=4, every=0, value=C.byref(v), out=gp, records=C.byref(r)):
        return lib.gmmvi_tape_probe_nodes(op, x, d, first, n, src, every, value, out, records)

    assert forward() == 0 and tape() == 0
    for probe in (forward, tape):
        for bad in (dict(op=-1), dict(op=len(_lib.NODE_OPS)), dict(x=None), dict(value=None), dict(out=None),
                    dict(d=80, n=65, src=0), dict(src=5), dict(first=5), dict(first=-1), dict(n=-1), dict(src=-1), dict(every=-1),
                    dict(d=-8), dict(d=0, n=0, src=0)):
            assert probe(**bad) == ERR_ARG, bad
        assert probe(d=80, n=64, src=16) == 0                           # the largest array
    assert forward(seed=-1) == ERR_ARG and tape(records=None) == ERR_ARG


@pytest.mark.parametrize("op", _lib.NODE_OPS)
def test_both_primitives_through_both_probes(op):
    worst_32 = worst_v = worst_g = 0.0
    for n, first, src, every, overlapping in PROBE_CASES:
        x = cases.probe_operands(n)
        d = x.size
        assert d == n + 16
        h = cases.entries(x, src, n)
        const = cases.constants(n, every)
        want, scale, want_g, g_scale, p = cases.reference64(op, x, first, n, src, every, h)
        bound = cases.WDOT_VALUE_EPS * EPS32 * scale if op == "wdot" else cases.logsumexp_value_bound(n, want)
        tag = f"{op} n={n} first={first} src={src} every={every}"
        v32 = cases.value32(op, x, first, n, h)
        e_32 = abs(float(v32) - want)
        assert e_32 <= bound, f"{tag}: the fp32 restatement misses the bound: {e_32:.3e} > {bound:.3e}"
        values, tangents = cases.probe_forward_gradient(op, x, first, n, src, every)
        v_t, g_t, records = cases.probe_tape(op, x, first, n, src, every)
        for v in values + [v_t]:                                        # one value function: every pass and the tape agree
            assert _bits(v) == _bits(v_t), tag
            assert abs(float(v) - want) <= bound, f"{tag}: value {v!r}, fp64 {want!r}, bound {bound:.3e}"
        if op == "wdot":
            assert _bits(v_t) == _bits(v32), tag
            assert _bits(v_t) == _bits(vec.probe_tape("dot", x, first, n, h, 0.0)[0]), tag
        # the slots: one tanh record per entry that is not a constant, the header and its payload unless the result is a constant
        constant_result = op == "logsumexp" and const.all()
        assert records == int((~const).sum()) + (0 if constant_result else 1 + (n + 1) // 2), tag
        g_bound = cases.gradient_eps(op, n) * EPS32 * g_scale
        for name, g in (("tangents", tangents), ("tape gradient", g_t)):
            err = np.abs(g.astype(np.float64) - want_g)
            assert np.all(err <= g_bound), f"{tag}: {name} {g!r}, fp64 {want_g!r}"
            if np.any(g_bound > 0):
                worst_g = max(worst_g, float((err[g_bound > 0] / g_bound[g_bound > 0]).max()))
        if not (overlapping and op == "wdot"):                          # one path per input: the two modes form the same bits
            np.testing.assert_array_equal(tangents, g_t, err_msg=tag)
        if bound > 0:
            worst_32, worst_v = max(worst_32, e_32 / bound), max(worst_v, abs(float(v_t) - want) / bound)
    print(f"\n[custom_nodes] {op}: worst value error {worst_v:.3f} of its bound (the fp32 restatement {worst_32:.3f}), worst "
          f"gradient error {worst_g:.3f} of its bound")


def test_wdot_gradient_by_the_inputs_is_the_entries_bit_for_bit():
    """Disjoint ranges: the sweep adds h[i].v * 1 to a zeroed entry, the forward pass adds h[k].v to a zero tangent."""
    for n, first, src, every, overlapping in PROBE_CASES:
        if overlapping:
            continue
        x = cases.probe_operands(n)
        h = cases.entries(x, src, n)
        _, g_t, _ = cases.probe_tape("wdot", x, first, n, src, every)
        _, tangents = cases.probe_forward_gradient("wdot", x, first, n, src, every)
        np.testing.assert_array_equal(_bits(g_t[first:first + n]), _bits(h))
        np.testing.assert_array_equal(_bits(tangents[first:first + n]), _bits(h))
        outside = np.ones(x.size, bool)
        outside[first:first + n] = False
        outside[src:src + n] = False
        assert not np.any(g_t[outside]) and not np.any(tangents[outside])
        const = cases.constants(n, every)
        assert not np.any(g_t[src:src + n][const]) and not np.any(tangents[src:src + n][const])


def test_the_partials_of_logsumexp_sum_to_one():
    """On an array whose entries are the inputs themselves the tape gradient and the tangents are the partials p_i of
    logsumexp_partial, with nothing multiplied in: their fp64 sum is 1 within n * eps32, in both gradient modes.  Each is the fp64
    softmax entry within a relative eps32 * (spread + 2 + (ceil(n / 4) + 2) / 2 + 1 / 2), spread = max |a[i] - m|: the rounding
    of a[i] - m is spread * eps32 / 2 at most, in the numerator and in the terms of s; expf is within 1 ulp in both; the partial
    sums of s and the division as in tests/custom_nodes_cases.py."""
    for n in (1, 2, 3, 15, 16, 17, 33):
        for src in (0, 5, 16):
            x = cases.probe_operands(n, seed=23 + src)
            values, tangents, v_t, g_t, records = cases.probe_inputs("logsumexp", x, 0, n, src)
            assert records == 1 + (n + 1) // 2
            a = x[src:src + n].astype(np.float64)
            want = np.exp(a - a.max()) / np.exp(a - a.max()).sum()
            p_eps = (a.max() - a.min()) + 2.0 + (math.ceil(n / 4) + 2) / 2.0 + 0.5
            for name, g in (("tangents", tangents), ("tape gradient", g_t)):
                p = g[src:src + n].astype(np.float64)
                assert abs(p.sum() - 1.0) <= n * EPS32, f"n={n} src={src}: {name} sum to {p.sum()!r}"
                assert np.all(np.abs(p - want) <= p_eps * EPS32 * want), (n, src, name)
                outside = np.ones(x.size, bool)
                outside[src:src + n] = False
                assert not np.any(g[outside])
            np.testing.assert_array_equal(_bits(tangents), _bits(g_t))
            assert all(_bits(v) == _bits(v_t) for v in values)


def test_an_array_of_minus_inf_inputs_is_the_constant_minus_inf():
    """m == -inf with n > 0: the constant -inf, zero partials, no record, in both gradient modes; one finite entry among them
    takes the whole partial."""
    x = np.full(20, -np.inf, np.float32)
    values, tangents, v_t, g_t, records = cases.probe_inputs("logsumexp", x, 0, 5, 3)
    assert records == 0 and _bits(v_t) == _bits(np.float32(-np.inf)) and all(_bits(v) == _bits(v_t) for v in values)
    assert not np.any(_bits(g_t)) and not np.any(_bits(tangents))
    x[5] = 0.75
    values, tangents, v_t, g_t, records = cases.probe_inputs("logsumexp", x, 0, 5, 3)
    want = np.zeros(20, np.float32)
    want[5] = 1
    assert records == 4 and _bits(v_t) == _bits(np.float32(0.75)) and all(_bits(v) == _bits(v_t) for v in values)
    np.testing.assert_array_equal(_bits(g_t), _bits(want))
    np.testing.assert_array_equal(_bits(tangents), _bits(want))


def test_edges():
    x = cases.probe_operands(4)
    for op in _lib.NODE_OPS:                                            # n = 0: a constant, no record, zero gradient
        v, g, records = cases.probe_tape(op, x, 3, 0, 5, 0)
        values, tangents = cases.probe_forward_gradient(op, x, 3, 0, 5, 0)
        want = np.float32(0) if op == "wdot" else np.float32(-np.inf)
        assert records == 0 and _bits(v) == _bits(want) and all(_bits(u) == _bits(want) for u in values)
        assert not np.any(_bits(g)) and not np.any(_bits(tangents))
    # n = 1: the entry itself with partial 1, so the gradient is the tanh partial and nothing else
    v, g, records = cases.probe_tape("logsumexp", x, 0, 1, 2, 0)
    _, tangents = cases.probe_forward_gradient("logsumexp", x, 0, 1, 2, 0)
    assert records == 1 + 2 and abs(float(v) - math.tanh(float(x[2]))) <= 2 * EPS32
    e = np.exp(np.float32(-2) * np.abs(x[2]))
    np.testing.assert_allclose(g[2], 4 * e / ((1 + e) * (1 + e)), rtol=4 * EPS32)
    np.testing.assert_array_equal(_bits(g), _bits(tangents))
    assert np.count_nonzero(g) == 1
    # fmaxf drops NaNs, so an array of NaN entries has m == -inf as well: the constant -inf, no node-array record (outside the
    # contract, stated in include/gmmvi_hip.h)
    y = np.full(20, np.nan, np.float32)
    v, g, records = cases.probe_tape("logsumexp", y, 0, 3, 1, 0)
    values, tangents = cases.probe_forward_gradient("logsumexp", y, 0, 3, 1, 0)
    assert records == 3 and _bits(v) == _bits(np.float32(-np.inf)) and all(_bits(u) == _bits(v) for u in values)
    assert not np.any(_bits(g)) and not np.any(_bits(tangents))


@pytest.mark.parametrize("mode", ["hand", "autodiff", "tape", "data", "data_tape"])
def test_a_source_with_both_primitives_compiles_in_every_mode(mode):
    check = {"hand": hip_ops.custom_target_check, "autodiff": hip_ops.custom_target_check_autodiff,
             "tape": hip_ops.custom_target_check_tape, "data": hip_ops.custom_target_check_data,
             "data_tape": hip_ops.custom_target_check_data_tape}[mode]
    status, log = check(cases.BOTH[mode])
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


def test_floats_where_the_input_view_belongs_do_not_compile():
    for check in (hip_ops.custom_target_check_autodiff, hip_ops.custom_target_check_tape):
        status, log = check(cases.WDOT_ON_FLOATS_SRC)
        assert status == ERR_ARG and "gmmvi_wdot" in log


def test_a_text_that_hides_the_name_does_not_compile_on_the_tape():
    """The node-array overloads and their branch of the sweep exist only in a text that names the primitives: a text that pastes
    the name together finds no overload for the tape's number instead of making a record that its sweep could not read."""
    src = ("#define PRIMITIVE(name) gmmvi_##name\n"
           "template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
           "    T h[2] = {x[0], x[1]};\n    return PRIMITIVE(wdot)(x, 0, h, 2);\n}\n")
    assert "gmmvi_wdot" not in src
    status, log = hip_ops.custom_target_check_tape(src)
    assert status == ERR_ARG and "gmmvi_wdot" in log
    status, log = hip_ops.custom_target_check_tape(src + "// gmmvi_wdot\n")
    assert status == 0, log


def _central_differences(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[i] = h
        g[:, i] = (f(x + e) - f(x - e)) / (2 * h)
    return g


DATA_SHAPES = [("softmax_vec", (4, 3), cases.softmax_dim(4, 3)), ("mlp_vec", (3, 5, 3), cases.mlp_dim(3, 5, 3)), ("mixed_nodes", (), 17)]


@pytest.mark.parametrize("name,shape,d", DATA_SHAPES)
def test_restated_data_targets_agree_with_central_differences(name, shape, d):
    for batch in (None, 5):
        tgt, x = cases.build_data_case(cases.Case(name, d, 6, 11, 0, batch, 2), shape)
        x = x.astype(np.float64)
        _, g = tgt.evaluate(x)
        fd = _central_differences(lambda y: tgt.evaluate(y)[0], x)
        np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} batch {batch}")


@pytest.mark.parametrize("name,shape,d", DATA_SHAPES[:2] + [("single_wdot", None, 5), ("single_lse", None, 5), ("single_lse", None, 20)])
def test_restated_densities_agree_with_central_differences(name, shape, d):
    tgt, x = cases.reference((name, d, 6) if shape is None else (name, shape, d, 6))[:2]
    x = x.astype(np.float64)
    _, g = tgt.log_density_and_grad(x)
    fd = _central_differences(lambda y: tgt.log_density_and_grad(y)[0], x)
    np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=name)
