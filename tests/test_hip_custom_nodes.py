"""GPU tests of the primitives of user-defined device targets on arrays of the mode's number type (gmmvi_wdot and
gmmvi_logsumexp: csrc/custom_target_vector.inc, their overloads in csrc/custom_target_autodiff.inc and
csrc/custom_target_tape.inc, the node-array record in the sweep of both tape modes): a softmax regression and a one-hidden-layer
network against fp64 in every mode, through the C ABI; the value call against the gradient call bit for bit; the tape lengths,
which follow from the texts; agreement with the scalar-loop twins and between forward and reverse mode; two kinds of record at
one record index in one wave; an output that is a single node-array node; a tape that overflows on a payload slot; an array of
-inf nodes; the predictive density and the diagonal Stein iteration above the forward cap.

Kernel bound: _bound of tests/test_hip_custom_target.py, unchanged: the device's largest error against the fp64 NumPy
restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|, for lp and for the gradient.  Every case prints its ratios before it asserts."""
import functools

import numpy as np
import pytest

import custom_nodes_cases as cases
import custom_predictive_cases as pred_cases
import test_hip_custom_data as data_mode
import test_hip_custom_data_own as own_mode
import test_hip_custom_data_tape as tape_data_mode
import test_hip_custom_predictive as predictive
import test_hip_custom_tape as tape_mode
import test_hip_custom_target as hand
from custom_data_own_cases import OwnBatches
from test_hip_custom_target import _bound

pytestmark = pytest.mark.gpu

N = 65                                                               # one tile and one lane of the next
DENSITY_MODES = ("hand", "autodiff", "tape")
DATA_MODES = ("data", "data_tape", "data_own", "data_tape_own")
TAPE_ENTRIES = ("tape", "data_tape", "data_tape_own")
SOFTMAX_SHAPES = ((2, 1), (4, 3), (3, 4), (5, 3), (10, 6))           # (F, K): D = 3, 15, 16, 18, 66
SOFTMAX_ABOVE_THE_FORWARD_CAP = (99, 6)                              # D = 600
MLP_SHAPES = ((2, 1, 2), (3, 5, 3))                                  # (F, H, K): D = 7, 38
MLP_BIG = (16, 32, 8)                                                # D = 808


def _dim(shape):
    return cases.softmax_dim(*shape) if len(shape) == 2 else cases.mlp_dim(*shape)


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name, mode):
    from gmmvi_amd import hip_ops
    if (name, mode) not in _handles:
        if mode in ("data", "data_tape"):
            src = cases.SOURCES[name]
        else:
            src = cases.HAND_SOURCES[name] if mode == "hand" else cases.DENSITY_SOURCES[name]
        _handles[(name, mode)] = hip_ops.custom_target_compile(ctx, src, mode=mode)
    return _handles[(name, mode)]


def _launch_density(ctx, name, mode, tgt, x, want_grad, capacity=0):
    """-> (lp, grad | None) through gmmvi_target_custom or gmmvi_target_custom_tape, canary rows behind both outputs."""
    handle = _handle(ctx, name, mode)
    if mode == "tape":
        rc, lp, g = tape_mode._launch(ctx, handle, tgt.params(), x, want_grad, capacity)
    else:
        rc, lp, g = hand._launch(ctx, handle, tgt.params(), x, want_grad, 0)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    return lp, g


def _launch_data(ctx, name, mode, tgt, x, want_grad, chunks=0):
    """-> (lp, grad | None) through the entry of ``mode``; the own-batch entries take the batch of ``tgt`` per sample."""
    kind = "data_tape" if "tape" in mode else "data"
    handle = _handle(ctx, name, kind)
    if mode.endswith("_own"):
        rc, lp, g = own_mode._launch(ctx, "tape" if kind == "data_tape" else "data", handle, OwnBatches(tgt), x, want_grad, chunks)
    elif kind == "data_tape":
        rc, lp, g = tape_data_mode._launch(ctx, handle, tgt, x, want_grad, chunks)
    else:
        rc, lp, g = data_mode._launch(ctx, handle, tgt, x, want_grad, chunks)
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    return lp, g


def _check(tag, lp, g, lp64, g64, lp32, g32):
    e_lp, b_lp, r_lp = _bound(lp, lp64, lp32)
    line = f"[custom_nodes] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
    if g is not None:
        e_g, b_g, r_g = _bound(g, g64, g32)
        line += f", gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})"
    print("\n" + line)
    assert np.all(np.isfinite(lp)) and (g is None or np.all(np.isfinite(g)))
    assert e_lp <= b_lp, f"{tag}: lp error {e_lp:.3e} > {b_lp:.3e}"
    if g is not None:
        assert e_g <= b_g, f"{tag}: gradient error {e_g:.3e} > {b_g:.3e}"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _data_case(name, mode, d):
    """67 rows in 3 chunks; the own-batch entries draw B = 5 of them per sample."""
    return cases.Case(name, d, N, 67, 3, 5 if mode.endswith("_own") else None, 3 if mode.endswith("_own") else 0)


def _data_reference(c, shape, mode):
    if not mode.endswith("_own"):
        return cases.reference(c, shape)
    key = (c, shape, "own")
    if key not in cases._refs:
        tgt, x = cases.build_data_case(c, shape)
        own = OwnBatches(tgt)
        lp64, g64 = own.evaluate(x.astype(np.float64))
        lp32, g32 = own.as_dtype(np.float32).evaluate(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        cases._refs[key] = (tgt, x, lp64, g64, lp32, g32)
    return cases._refs[key]


def _run(ctx, name, mode, shape, want_grad=True):
    """-> (tag, lp, g, the references) of ``name`` at ``shape`` through the entry of ``mode``: the density form with one fixed row
    in the modes without a data set, else 67 rows in 3 chunks."""
    d = _dim(shape)
    if mode in DENSITY_MODES:
        ref = cases.reference((name, shape, d, N))
        lp, g = _launch_density(ctx, name, mode, ref[0], ref[1], want_grad)
        return f"{name} {mode} {shape} D={d}", lp, g, ref[2:]
    c = _data_case(name, mode, d)
    ref = _data_reference(c, shape, mode)
    lp, g = _launch_data(ctx, name, mode, ref[0], ref[1], want_grad, c.chunks)
    return f"{cases.case_id(c)} {shape} {mode}", lp, g, ref[2:]


# ---- 1. against fp64 ---------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(mode, shape) for mode in DENSITY_MODES + DATA_MODES for shape in SOFTMAX_SHAPES]
SOFTMAX_CASES += [(mode, SOFTMAX_ABOVE_THE_FORWARD_CAP) for mode in TAPE_ENTRIES]


@pytest.mark.parametrize("mode,shape", SOFTMAX_CASES, ids=lambda v: str(v))
def test_softmax_vec_matches_fp64_reference(ctx, mode, shape):
    tag, lp, g, ref = _run(ctx, "softmax_vec", mode, shape)
    _check(tag, lp, g, *ref)
    tag, lp_v, _, _ = _run(ctx, "softmax_vec", mode, shape, False)
    _check(tag + " values only", lp_v, None, *ref)


MLP_CASES = [(mode, shape) for mode in ("autodiff", "tape") + DATA_MODES for shape in MLP_SHAPES]
MLP_CASES += [(mode, MLP_BIG) for mode in TAPE_ENTRIES]


@pytest.mark.parametrize("mode,shape", MLP_CASES, ids=lambda v: str(v))
def test_mlp_vec_matches_fp64_reference(ctx, mode, shape):
    tag, lp, g, ref = _run(ctx, "mlp_vec", mode, shape)
    _check(tag, lp, g, *ref)
    tag, lp_v, _, _ = _run(ctx, "mlp_vec", mode, shape, False)
    _check(tag + " values only", lp_v, None, *ref)


# ---- 2. bits: outputs that are one primitive and nothing else ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single_wdot", "single_lse"])
@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_output_that_is_a_single_node_array_node(ctx, name, mode):
    """One function gives the value in all three number types: the value call and the gradient call agree bit for bit.
    single_wdot is sum x[j]^2 with every entry an input node: both shares of x[j] go into the gradient, x[j] + x[j] exactly."""
    for d in (1, 5, 17):
        tgt, x, lp64, g64, lp32, g32 = cases.reference((name, d, N))
        lp, g = _launch_density(ctx, name, mode, tgt, x, True)
        _check(f"{name} {mode} D={d}", lp, g, lp64, g64, lp32, g32)
        lp_v, _ = _launch_density(ctx, name, mode, tgt, x, False)
        np.testing.assert_array_equal(_bits(lp_v), _bits(lp))
        lp_b, g_b = _launch_density(ctx, name, mode, tgt, x, True)
        np.testing.assert_array_equal(_bits(lp_b), _bits(lp))
        np.testing.assert_array_equal(_bits(g_b), _bits(g))
        if name == "single_wdot":
            want = np.zeros_like(x)
            want[:, :16] = np.float32(2) * x[:, :16]
            np.testing.assert_array_equal(g, want)
        else:
            assert not np.any(_bits(g[:, 16:]))


# ---- 3. agreement ------------------------------------------------------------------------------------------------------------------
def _agree(tag, a, b, bound_a, bound_b):
    d = float(np.abs(a.astype(np.float64) - b).max())
    print(f"[custom_nodes] {tag}: differ by {d:.3e} ({d / (bound_a + bound_b):.3f} of the two bounds)")
    assert d <= bound_a + bound_b, tag


@pytest.mark.parametrize("pair,shape", [("softmax", (4, 3)), ("softmax", SOFTMAX_ABOVE_THE_FORWARD_CAP), ("mlp", (3, 5, 3))])
def test_vec_source_agrees_with_its_loop_twin(ctx, pair, shape):
    _, lp, g, ref = _run(ctx, pair + "_vec", "data_tape", shape)
    tag, lp_l, g_l, ref_l = _run(ctx, pair + "_loop", "data_tape", shape)
    _check(f"{pair}_vec {shape} data_tape", lp, g, *ref)
    _check(tag, lp_l, g_l, *ref_l)
    lp64, g64, lp32, g32 = ref
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    _agree(f"{pair} {shape} vec against loop, lp", lp, lp_l, b_lp, b_lp)
    _agree(f"{pair} {shape} vec against loop, gradient", g, g_l, b_g, b_g)


@pytest.mark.parametrize("name,shape", [("softmax_vec", (10, 6)), ("mlp_vec", (3, 5, 3))])
def test_forward_mode_and_reverse_mode_agree(ctx, name, shape):
    _, lp_f, g_f, ref = _run(ctx, name, "data", shape)
    _, lp_r, g_r, _ = _run(ctx, name, "data_tape", shape)
    lp64, g64, lp32, g32 = ref
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    _agree(f"{name} {shape} forward against reverse, lp", lp_f, lp_r, b_lp, 0.0)
    _agree(f"{name} {shape} forward against reverse, gradient", g_f, g_r, b_g, 0.0)


# ---- 4. tape lengths ---------------------------------------------------------------------------------------------------------------
def _fresh(ctx, src, tag):
    """A handle of its own (the module cache keys on the text), so that its remembered lengths are this test's."""
    from gmmvi_amd import hip_ops
    return hip_ops.custom_target_compile(ctx, src + f"\n// {tag}\n", mode="data_tape")


def _length_after_one_call(ctx, name, shape):
    from gmmvi_amd import hip_ops
    d = _dim(shape)
    handle = _fresh(ctx, cases.SOURCES[name], f"tape length {shape}")
    tgt, x = cases.build_data_case(cases.Case(name, d, N, 5, 0, None, 0), shape)
    assert hip_ops.custom_tape_length(ctx, handle, d) == 0
    (rc, _, _), launches = tape_data_mode._launches(ctx, lambda: tape_data_mode._launch(ctx, handle, tgt, x, True))
    assert rc == 0
    return hip_ops.custom_tape_length(ctx, handle, d), launches


@pytest.mark.parametrize("pair", ["softmax", "mlp"])
def test_tape_lengths_follow_from_the_texts(ctx, pair):
    """The length is the longer of the row's and the prior's tape; the prior is 4 records (gmmvi_sumsq, *, /, -) everywhere.
    softmax, F = 3, K = 4.  vec: per class gmmvi_dot and the + of the bias, 2 K; gmmvi_logsumexp 1 + ceil(K / 2); the final -:
    2 K + ceil(K / 2) + 2 = 12.  loop: per class F products and F adds (the bias is an input, read without a record), 2 F K; K - 1
    gmmvi_logaddexp; the final -: 2 F K + K = 28.
    mlp, F = 3, H = 5, K = 3.  vec: per hidden unit gmmvi_dot, + and tanh, 3 H; per class gmmvi_wdot 1 + ceil(H / 2) and the +;
    gmmvi_logsumexp 1 + ceil(K / 2); the final -: 3 H + K (2 + ceil(H / 2)) + ceil(K / 2) + 2 = 34.  loop: H (2 F + 1) + 2 H K
    + (K - 1) + 1 = 68."""
    shape = (3, 4) if pair == "softmax" else (3, 5, 3)
    vec, _ = _length_after_one_call(ctx, pair + "_vec", shape)
    loop, _ = _length_after_one_call(ctx, pair + "_loop", shape)
    print(f"\n[custom_nodes] tape lengths, {pair} {shape}: vec {vec}, loop {loop}")
    if pair == "softmax":
        f, k = shape
        assert (vec, loop) == (2 * k + (k + 1) // 2 + 2, 2 * f * k + k) == (12, 28)
        assert vec == loop - (2 * f - 1) * k + (k + 1) // 2 + 2
    else:
        f, h, k = shape
        assert (vec, loop) == (3 * h + k * (2 + (h + 1) // 2) + (k + 1) // 2 + 2, h * (2 * f + 1) + 2 * h * k + k) == (34, 68)
        assert vec == loop - 2 * h * (f - 1) - k * (2 * h - 2 - (h + 1) // 2) - k + (k + 1) // 2 + 2


def test_mlp_vec_fits_the_first_launch_at_d_808_where_the_loop_twin_takes_two(ctx):
    """(F, H, K) = (16, 32, 8): mlp_vec needs 3 * 32 + 8 * (2 + 16) + 4 + 2 = 246 slots, within the 1 024 the first launch
    sizes; mlp_loop needs 32 * 33 + 2 * 32 * 8 + 8 = 1 576 records and is launched a second time."""
    vec, launches = _length_after_one_call(ctx, "mlp_vec", MLP_BIG)
    assert (vec, launches) == (246, 1)
    loop, launches = _length_after_one_call(ctx, "mlp_loop", MLP_BIG)
    assert (loop, launches) == (1576, 2)


# ---- 5. two kinds of record at one record index in one wave ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TAPE_ENTRIES)
def test_mixed_record_kinds_in_one_wave(ctx, mode):
    d = 17
    if mode == "tape":
        tgt, x, lp64, g64, lp32, g32 = cases.reference(("mixed_nodes", (), d, N))
        lp, g = _launch_density(ctx, "mixed_nodes", mode, tgt, x, True)
    else:
        c = _data_case("mixed_nodes", mode, d)
        tgt, x, lp64, g64, lp32, g32 = _data_reference(c, (), mode)
        lp, g = _launch_data(ctx, "mixed_nodes", mode, tgt, x, True, c.chunks)
    first_wave = x[:64, 0] > 0
    assert first_wave.any() and (~first_wave).any()
    _check(f"mixed_nodes {mode} D={d}", lp, g, lp64, g64, lp32, g32)
    for pick, what in ((x[:, 0] > 0, "primitive lanes"), (x[:, 0] <= 0, "loop lanes")):
        _check(f"mixed_nodes {mode} D={d}, {what}", lp[pick], g[pick], lp64[pick], g64[pick], lp32[pick], g32[pick])


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------
def test_a_tape_that_overflows_on_a_payload_slot(ctx):
    """single_lse at D = 17 is 8 payload slots and the header.  A capacity of 4 ends inside the payload: the count still advances
    to 9, the call is launched again at that length, and the result has the bits of a call with ample capacity."""
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = cases.reference(("single_lse", 17, N))
    handle = hip_ops.custom_target_compile(ctx, cases.SINGLE_LSE_SRC + "\n// overflow on a payload slot\n", mode="tape")
    (rc, lp, g), launches = tape_mode._tape_launches(ctx, lambda: tape_mode._launch(ctx, handle, tgt.params(), x, True, 4))
    assert rc == 0 and launches == 2
    assert hip_ops.custom_tape_length(ctx, handle, 17) == 9
    (rc, lp_big, g_big), launches = tape_mode._tape_launches(ctx, lambda: tape_mode._launch(ctx, handle, tgt.params(), x, True, 64))
    assert rc == 0 and launches == 1
    np.testing.assert_array_equal(_bits(lp), _bits(lp_big))
    np.testing.assert_array_equal(_bits(g), _bits(g_big))
    _check("single_lse from a capacity of 4", lp, g, lp64, g64, lp32, g32)


def test_a_row_tape_that_overflows_on_a_payload_slot(ctx):
    """softmax_vec at (F, K) = (10, 6) is 12 records, 3 payload slots, the header and the final -: a capacity of 13 ends inside
    the payload."""
    shape = (10, 6)
    c = cases.Case("softmax_vec", _dim(shape), N, 5, 0, None, 0)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c, shape)
    handle = _fresh(ctx, cases.SOURCES["softmax_vec"], "overflow on a payload slot")
    (rc, lp, g), launches = tape_data_mode._launches(ctx, lambda: tape_data_mode._launch(ctx, handle, tgt, x, True, 0, 13))
    assert rc == 0 and launches == 2
    _check("softmax_vec from a capacity of 13", lp, g, lp64, g64, lp32, g32)


@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_an_array_of_minus_inf_nodes_is_the_constant_minus_inf(ctx, mode):
    """Three nodes whose values are -inf, and n = 0: the constant -inf, no record, zero partials; the density is x[0] + 1.  The
    tape: two records per -inf node, two slots for the gmmvi_logsumexp of one entry, the final +: 9."""
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = cases.reference(("all_minus_inf", 5, N))
    lp, g = _launch_density(ctx, "all_minus_inf", mode, tgt, x, True)
    _check(f"all_minus_inf {mode}", lp, g, lp64, g64, lp32, g32)
    np.testing.assert_array_equal(g, g64.astype(np.float32))
    if mode == "tape":
        assert hip_ops.custom_tape_length(ctx, _handle(ctx, "all_minus_inf", mode), 5) == 9


# ---- 7. downstream -----------------------------------------------------------------------------------------------------------------
def test_log_predictive_over_held_out_rows(ctx):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF
    rng = np.random.default_rng(31)
    f, k, t, held_out = 4, 3, 40, 5
    d = cases.softmax_dim(f, k)
    rows = cases.rows_for(rng, "softmax_vec", t + held_out, f, k).astype(np.float32)
    train, test = rows[:t], rows[t:]
    target = DeviceDataLNPDF(cases.SOURCES["softmax_vec"], d, train, params=cases.PRIOR)
    ref_tgt = cases.Softmax(train, cases.PRIOR, d=d)
    x = (rng.normal(size=(130, d)) * 0.7).astype(np.float32)
    l64 = pred_cases.row_terms(ref_tgt, x.astype(np.float64), test)
    l32 = pred_cases.row_terms(cases.fp32_twin(ref_tgt), x, test)
    out = [o.numpy() for o in target.log_predictive(x, test)]
    assert all(o.shape == (held_out,) for o in out)
    predictive._check("softmax_vec log_predictive over 5 held-out rows", out, pred_cases.reference64(l64), pred_cases.twin32(l32))


def test_diagonal_stein_iteration_above_the_forward_cap(monkeypatch):
    """test_diagonal_stein_iteration_above_the_forward_cap of tests/test_hip_custom_data_tape.py, its set-up, its follow-up and its
    tolerance, with softmax_vec for the source, its restatement for the oracle's target and rows of 99 features and a label in
    [0, 6): D = 600, T = 40, three iterations."""
    f, k = SOFTMAX_ABOVE_THE_FORWARD_CAP
    d = cases.softmax_dim(f, k)
    monkeypatch.setitem(tape_data_mode.cases.SOURCES, "logit", cases.SOURCES["softmax_vec"])
    monkeypatch.setattr(tape_data_mode.cases.base, "Logit", functools.partial(cases.Softmax, d=d))
    monkeypatch.setattr(tape_data_mode, "_logit_rows", lambda rng, t, dim: cases.rows_for(rng, "softmax_vec", t, f, k).astype(np.float32))
    ref, target, o, g, per_iter = tape_data_mode._diagonal_pair(d, None)
    assert isinstance(ref, cases.Softmax) and "gmmvi_logsumexp" in target.source and ref.data.shape == (40, f + 1)
    tape_data_mode._follow(o, g, 3, d)
    assert int(g.sample_db.num_samples_written) == 3 * per_iter and target.call_count == 0
