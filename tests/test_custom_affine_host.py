"""gmmvi_affine of user-defined device targets, the part that needs no GPU: gmmvi_autodiff_probe_affine and gmmvi_tape_probe_affine
against an fp64 NumPy restatement at the fp32 operands, the bits the contract states, the slot counts of the record group, the
edges, the sources of the test targets compiled for gfx950 without a device, and the restated test targets against central
differences.  tests/custom_affine_cases.py derives the two bounds."""
import ctypes as C

import numpy as np
import pytest

import custom_affine_cases as cases
import custom_nodes_cases as nodes
from gmmvi_amd import _lib, hip_ops

EPS32 = cases.EPS32
ERR_ARG = -2
PROBE_CASES = cases.probe_cases()
CHECKS = {"hand": hip_ops.custom_target_check, "autodiff": hip_ops.custom_target_check_autodiff,
          "tape": hip_ops.custom_target_check_tape, "data": hip_ops.custom_target_check_data,
          "data_tape": hip_ops.custom_target_check_data_tape}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_lists_and_the_symbols():
    assert _lib.NODE_OPS == ("wdot", "logsumexp")                       # the existing lists stay as they are
    assert _lib.VECTOR_OPS == ("dot", "sqdist", "sumsq")
    for symbol in ("gmmvi_autodiff_probe_affine", "gmmvi_tape_probe_affine"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    lib = _lib.load()
    x = np.ones(6000, np.float32)
    v, r, t = C.c_float(), C.c_int(), np.zeros(cases.W, np.float32)
    g, out = np.zeros(x.size, np.float32), np.zeros(64, np.float32)
    xp, tp, gp, op = (a.ctypes.data_as(C.c_void_p) for a in (x, t, g, out))

    def forward(x=xp, d=20, w=4, si=1, sj=5, b=8, sb=5, n=4, m=3, src=0, every=0, inputs=0, floats=0, pick=-1, seed=0, values=op,
                value=C.byref(v), res=tp):
        return lib.gmmvi_autodiff_probe_affine(x, d, w, si, sj, b, sb, n, m, src, every, inputs, floats, pick, seed, values, value, res)

    def tape(x=xp, d=20, w=4, si=1, sj=5, b=8, sb=5, n=4, m=3, src=0, every=0, inputs=0, floats=0, pick=-1, values=op,
             value=C.byref(v), res=gp, records=C.byref(r)):
        return lib.gmmvi_tape_probe_affine(x, d, w, si, sj, b, sb, n, m, src, every, inputs, floats, pick, values, value, res, records)

    for probe in (forward, tape):
        assert probe() == 0
        for bad in (dict(x=None), dict(values=None), dict(value=None), dict(res=None), dict(d=0), dict(d=-20),
                    dict(n=65, d=6000, sj=66, b=-1), dict(m=65, d=6000, b=-1), dict(n=-1), dict(m=-1),
                    dict(d=18), dict(d=19, b=9), dict(w=-1), dict(si=0), dict(si=-1), dict(sj=0), dict(sj=-5), dict(sb=0),
                    dict(sb=-5), dict(src=17), dict(src=-1), dict(every=-1), dict(pick=3), dict(pick=-2), dict(w=7)):
            assert probe(**bad) == ERR_ARG, bad
        assert probe(b=-1, sb=-7) == 0                                  # no bias: its stride is not looked at
        assert probe(d=6000, n=64, m=64, w=64, si=1, sj=65, b=128, sb=65, pick=63) == 0     # the largest call
        assert probe(d=6000, n=64, m=64, w=64, si=64, sj=1, b=64 + 64 * 64, sb=1) == 0
    assert forward(seed=-1) == ERR_ARG and tape(records=None) == ERR_ARG


def _case(n, m, name, bias, every, inputs=False, floats=False, src=0):
    """-> (x, layout, h [n] as the probes formed it, const [n])."""
    lay, d = cases.probe_layout(n, m, name, bias)
    x = cases.probe_operands(d)
    if inputs:
        h, const = x[src:src + n].copy(), np.zeros(n, bool)
    else:
        h, const = nodes.entries(x, src, n), nodes.constants(n, every)
    if floats:
        const = np.ones(n, bool)
    return x, lay, h, const


def _check_one(tag, x, lay, src, every, h, const, inputs, floats, worst):
    """Every pick of one call through both probes against fp64, within the two bounds."""
    n, m = lay.n, lay.m
    want32 = cases.out32(x, lay, h)
    for pick in range(-1, m):
        outs_f, values_f, tangents = cases.probe_forward_gradient(x, lay, src, every, pick, inputs, floats)
        out_t, v_t, g_t, records = cases.probe_tape(x, lay, src, every, pick, inputs, floats)
        want, scale, want_g, g_scale, spread = cases.reference64(x, lay, src, h, const, not inputs, out_t, pick)
        bound = cases.WDOT_VALUE_EPS * EPS32 * scale + 0.5 * EPS32 * np.abs(want) * (lay.b >= 0)
        where = f"{tag} pick={pick}"
        # one value function: the fp32 restatement in the stated order, every forward pass and the tape have the same bits
        np.testing.assert_array_equal(_bits(out_t), _bits(want32), err_msg=where)
        for o in outs_f:
            np.testing.assert_array_equal(_bits(o), _bits(out_t), err_msg=where)
        assert np.all(np.abs(out_t.astype(np.float64) - want) <= bound), f"{where}: out {out_t!r}, fp64 {want!r}, bound {bound!r}"
        assert all(_bits(v) == _bits(v_t) for v in values_f), where
        if pick >= 0:
            assert _bits(v_t) == _bits(out_t[pick]), where
        made = 0 if inputs or floats else int((~const).sum())
        assert records == made + cases.slots(n, m) == made + (n + 1) // 2 + 2 + m, where
        g_bound = cases.gradient_eps(n, m, pick, spread) * EPS32 * g_scale
        for name, g in (("tangents", tangents), ("tape gradient", g_t)):
            err = np.abs(g.astype(np.float64) - want_g)
            assert np.all(err <= g_bound), f"{where}: {name} {g!r}, fp64 {want_g!r}, bound {g_bound!r}"
            if np.any(g_bound > 0):
                worst[1] = max(worst[1], float((err[g_bound > 0] / g_bound[g_bound > 0]).max()))
        # forward against tape, concatenated over every seed pass: within the two bounds
        assert np.all(np.abs(tangents.astype(np.float64) - g_t) <= 2 * g_bound), where
        if np.any(bound > 0):
            worst[0] = max(worst[0], float((np.abs(out_t - want)[bound > 0] / bound[bound > 0]).max()))
        if pick >= 0 and not (inputs and src >= lay.w):
            # the weights' gradient is h[i].v exactly on row pick and zero elsewhere, the bias's is 1
            idx, bias = lay.weights(), lay.biases()
            for name, g in (("tangents", tangents), ("tape gradient", g_t)):
                np.testing.assert_array_equal(_bits(g[idx[:, pick]]), _bits(h), err_msg=f"{where} {name}")
                rest = np.delete(idx, pick, axis=1)
                assert not np.any(g[rest]), f"{where} {name}"
                if bias is not None:
                    assert g[bias[pick]] == 1 and not np.any(np.delete(g[bias], pick)), f"{where} {name}"
                assert not np.any(g[src:src + n][const]), f"{where} {name}"


def test_the_tanh_array_through_both_probes():
    worst = [0.0, 0.0]
    seen_d = set()
    for n, m, name, bias, every in PROBE_CASES:
        x, lay, h, const = _case(n, m, name, bias, every)
        seen_d.add(x.size)
        _check_one(f"{lay} every={every}", x, lay, 0, every, h, const, False, False, worst)
    assert min(seen_d) < 16 < 32 < max(seen_d)
    print(f"\n[custom_affine] tanh entries: worst value error {worst[0]:.3f} of its bound, worst gradient error {worst[1]:.3f} of its bound")


def test_the_inputs_as_the_array_and_an_input_on_two_paths():
    """h[i] = x[src + i].  src = 0: entries and weights are disjoint.  src = w: entry i is also the weight (i, 0) of the call (both
    layouts start output 0 at w; for the row-major layout entry i is weight (0, i) or beyond), so an input collects the share of
    a weight and the share of an entry."""
    worst = [0.0, 0.0]
    for n, m, name, bias, every in PROBE_CASES:
        if every:
            continue
        for src in (0, n + 1):
            x, lay, h, const = _case(n, m, name, bias, 0, inputs=True, src=src)
            assert src in (0, lay.w)
            _check_one(f"{lay} inputs src={src}", x, lay, src, 0, h, const, True, False, worst)
    print(f"\n[custom_affine] input entries: worst value error {worst[0]:.3f} of its bound, worst gradient error {worst[1]:.3f} of its bound")


def test_the_overload_that_takes_constants():
    worst = [0.0, 0.0]
    for n, m, name, bias, every in PROBE_CASES:
        if every:
            continue
        x, lay, h, const = _case(n, m, name, bias, 0, floats=True)
        _check_one(f"{lay} floats", x, lay, 0, 0, h, const, False, True, worst)
        # the same values as nodes: the two overloads give the same bits
        out_nodes = cases.probe_tape(x, lay, 0, 0, 0)[0]
        np.testing.assert_array_equal(_bits(cases.probe_tape(x, lay, 0, 0, 0, floats=True)[0]), _bits(out_nodes))
    print(f"\n[custom_affine] float entries: worst value error {worst[0]:.3f} of its bound, worst gradient error {worst[1]:.3f} of its bound")


def test_with_unit_stride_an_output_has_the_bits_of_wdot_and_one_add():
    for n, m, name, bias, every in PROBE_CASES:
        x, lay, h, const = _case(n, m, name, bias, every)
        if lay.si != 1:
            continue
        out = cases.probe_tape(x, lay, 0, every, 0)[0]
        for j in range(m):
            s = nodes.probe_tape("wdot", x, lay.w + j * lay.sj, n, 0, every)[0]
            want = np.float32(s + x[lay.b + j * lay.sb]) if bias else s
            assert _bits(out[j]) == _bits(want), (lay, every, j)


def test_edges():
    x = cases.probe_operands(24)
    for name in ("unit", "keras"):
        # m = 0: nothing written, no record
        lay = (cases.unit_layout if name == "unit" else cases.keras_layout)(5, 4, 0)
        out, v, g, records = cases.probe_tape(x, lay, 0, 0, -1, inputs=True)
        _, values, tangents = cases.probe_forward_gradient(x, lay, 0, 0, -1, inputs=True)
        assert records == 0 and out.size == 0 and not np.any(_bits(g)) and not np.any(_bits(tangents))
        # n = 0: out[j] is the bias, an input: no record, the unit gradient
        for m in (1, 3):
            lay = (cases.unit_layout if name == "unit" else cases.keras_layout)(5, 0, m)
            for pick in range(m):
                out, v, g, records = cases.probe_tape(x, lay, 0, 0, pick)
                outs, values, tangents = cases.probe_forward_gradient(x, lay, 0, 0, pick)
                want = np.zeros(x.size, np.float32)
                want[lay.biases()[pick]] = 1
                assert records == 0
                np.testing.assert_array_equal(_bits(out), _bits(x[lay.biases()]))
                np.testing.assert_array_equal(_bits(outs[0]), _bits(out))
                assert _bits(v) == _bits(x[lay.biases()[pick]]) and all(_bits(u) == _bits(v) for u in values)
                np.testing.assert_array_equal(_bits(g), _bits(want))
                np.testing.assert_array_equal(_bits(tangents), _bits(want))
            # and without a bias the constant 0
            lay = (cases.unit_layout if name == "unit" else cases.keras_layout)(5, 0, m, bias=False)
            out, v, g, records = cases.probe_tape(x, lay, 0, 0, 0)
            assert records == 0 and not np.any(_bits(out)) and not np.any(_bits(g))


@pytest.mark.parametrize("mode", ["autodiff", "tape", "data", "data_tape"])
def test_every_test_source_compiles(mode):
    sources = cases.SOURCES if mode in ("data", "data_tape") else cases.DENSITY_SOURCES
    for name, src in sources.items():
        status, log = CHECKS[mode](src)
        assert status == 0, f"{name}: {log}"


def test_the_hand_written_source_compiles():
    for name, src in cases.HAND_SOURCES.items():
        status, log = CHECKS["hand"](src)
        assert status == 0, f"{name}: {log}"


def test_floats_where_the_input_view_belongs_do_not_compile():
    for mode in ("autodiff", "tape"):
        status, log = CHECKS[mode](cases.AFFINE_ON_FLOATS_SRC)
        assert status == ERR_ARG and "gmmvi_affine" in log


def test_a_text_that_hides_the_name_does_not_compile_on_the_tape():
    """The overloads on tape nodes and their branch of the sweep exist only in a text that names the primitive."""
    src = ("#define PRIMITIVE(name) gmmvi_##name\n"
           "template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params) {\n"
           "    T h[2] = {x[0], x[1]}, out[1];\n    PRIMITIVE(affine)(x, 2, 1, 3, 4, 3, h, 2, out, 1);\n    return out[0];\n}\n")
    assert "gmmvi_affine" not in src
    status, log = hip_ops.custom_target_check_tape(src)
    assert status == ERR_ARG and "gmmvi_affine" in log
    status, log = hip_ops.custom_target_check_tape(src + "// gmmvi_affine\n")
    assert status == 0, log
    status, log = hip_ops.custom_target_check_autodiff(src)            # the forward mode has no record to misread
    assert status == 0, log


def _central_differences(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[i] = h
        g[:, i] = (f(x + e) - f(x - e)) / (2 * h)
    return g


DATA_SHAPES = [("mlp2_affine", (3, 5, 4, 3)), ("mlp2_affine", (2, 1, 1, 2)), ("keras_affine", (3, 5, 3)), ("keras_affine", (2, 1, 2)),
               ("mixed_affine", (17,))]


@pytest.mark.parametrize("name,shape", DATA_SHAPES)
def test_restated_data_targets_agree_with_central_differences(name, shape):
    for batch in (None, 5):
        tgt, x = cases.build_data_case(cases.Case(name, cases.dim(name, shape), 6, 11, 0, batch, 2), shape)
        x = x.astype(np.float64)
        _, g = tgt.evaluate(x)
        fd = _central_differences(lambda y: tgt.evaluate(y)[0], x)
        np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} batch {batch}")


@pytest.mark.parametrize("key", [("mlp2_affine", (3, 5, 4, 3), 59, 6), ("keras_affine", (3, 5, 3), 38, 6), ("pick_affine", 0, 12, 6),
                                 ("pick_affine", 2, 17, 6)])
def test_restated_densities_agree_with_central_differences(key):
    tgt, x = cases.reference(key)[:2]
    x = x.astype(np.float64)
    _, g = tgt.log_density_and_grad(x)
    fd = _central_differences(lambda y: tgt.log_density_and_grad(y)[0], x)
    np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=str(key))


def test_the_tape_lengths_of_the_issue():
    assert cases.mlp2_lengths(3, 5, 4, 3) == (38, 55)
    assert cases.mlp2_lengths(16, 32, 32, 8) == (188, 854)
    assert cases.mlp2_dim(16, 32, 32, 8) == 1864
