"""GPU tests of gmmvi_affine of user-defined device targets (csrc/custom_target_vector.inc, its overloads in
csrc/custom_target_autodiff.inc and csrc/custom_target_tape.inc, the record group in the sweep of both tape modes): a network with
two hidden layers and a row-major two-layer network against fp64 in every mode, through the C ABI; the value call against the
gradient call bit for bit; entering a record group at each of its headers; agreement with the twins that call gmmvi_dot and
gmmvi_wdot or scalar loops, and between forward and reverse mode; the tape lengths, which follow from the texts; tapes that
overflow inside a group; two kinds of record in one wave; the predictive density and the diagonal Stein iteration above the
forward cap.

Kernel bound: _bound of tests/test_hip_custom_target.py, unchanged: the device's largest error against the fp64 NumPy
restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|, for lp and for the gradient.  Every case prints its ratios before it asserts."""
import numpy as np
import pytest

import custom_affine_cases as cases
import custom_predictive_cases as pred_cases
import test_hip_custom_data as data_mode
import test_hip_custom_data_own as own_mode
import test_hip_custom_data_tape as tape_data_mode
import test_hip_custom_nodes as nodes_gpu
import test_hip_custom_predictive as predictive
import test_hip_custom_tape as tape_mode
import test_hip_custom_target as hand
from custom_data_own_cases import OwnBatches
from test_hip_custom_target import _bound

pytestmark = pytest.mark.gpu

N = nodes_gpu.N                                                      # 65: one tile and one lane of the next
DENSITY_MODES = ("autodiff", "tape")
DATA_MODES = nodes_gpu.DATA_MODES
ALL_MODES = DENSITY_MODES + DATA_MODES
TAPE_ENTRIES = nodes_gpu.TAPE_ENTRIES
MLP2_SHAPES = ((2, 1, 1, 2), (3, 5, 4, 3))                           # (F, H1, H2, K): D = 9, 59
MLP2_BIG = (16, 32, 32, 8)                                           # D = 1 864
KERAS_SHAPES = ((3, 5, 3), (2, 1, 2))                                # (F, H, K): D = 38, 7
_bits = nodes_gpu._bits
_data_case = nodes_gpu._data_case


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name, mode):
    from gmmvi_amd import hip_ops
    if (name, mode) not in _handles:
        src = cases.SOURCES[name] if mode in ("data", "data_tape") else cases.DENSITY_SOURCES[name]
        _handles[(name, mode)] = hip_ops.custom_target_compile(ctx, src, mode=mode)
    return _handles[(name, mode)]


def _launch_density(ctx, name, mode, tgt, x, want_grad, capacity=0, handle=None):
    """-> (lp, grad | None) through gmmvi_target_custom or gmmvi_target_custom_tape, canary rows behind both outputs."""
    handle = handle or _handle(ctx, name, mode)
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
    line = f"[custom_affine] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
    if g is not None:
        e_g, b_g, r_g = _bound(g, g64, g32)
        line += f", gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})"
    print("\n" + line)
    assert np.all(np.isfinite(lp)) and (g is None or np.all(np.isfinite(g)))
    assert e_lp <= b_lp, f"{tag}: lp error {e_lp:.3e} > {b_lp:.3e}"
    if g is not None:
        assert e_g <= b_g, f"{tag}: gradient error {e_g:.3e} > {b_g:.3e}"


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
    d = cases.dim(name, shape)
    if mode in DENSITY_MODES:
        ref = cases.reference((name, shape, d, N))
        lp, g = _launch_density(ctx, name, mode, ref[0], ref[1], want_grad)
        return f"{name} {mode} {shape} D={d}", lp, g, ref[2:]
    c = _data_case(name, mode, d)
    ref = _data_reference(c, shape, mode)
    lp, g = _launch_data(ctx, name, mode, ref[0], ref[1], want_grad, c.chunks)
    return f"{cases.case_id(c)} {shape} {mode}", lp, g, ref[2:]


# ---- 1. against fp64 ---------------------------------------------------------------------------------------------------------------
FP64_CASES = [("mlp2_affine", mode, shape) for mode in ALL_MODES for shape in MLP2_SHAPES]
FP64_CASES += [("mlp2_affine", mode, MLP2_BIG) for mode in TAPE_ENTRIES]
FP64_CASES += [("keras_affine", mode, shape) for mode in ALL_MODES for shape in KERAS_SHAPES]


@pytest.mark.parametrize("name,mode,shape", FP64_CASES, ids=lambda v: str(v))
def test_affine_sources_match_the_fp64_reference(ctx, name, mode, shape):
    tag, lp, g, ref = _run(ctx, name, mode, shape)
    _check(tag, lp, g, *ref)
    tag, lp_v, _, _ = _run(ctx, name, mode, shape, False)
    _check(tag + " values only", lp_v, None, *ref)


# ---- 2. entering the group at header j ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DENSITY_MODES)
@pytest.mark.parametrize("pick", [0, 1, 2])
def test_an_output_that_is_one_header_of_a_group(ctx, mode, pick):
    """pick_affine returns out[pick] of one call with m = 3 whose entries are input nodes: the sweep enters the group at header
    pick.  One function gives the value in all three number types; the gradient is copies of inputs and ones, so it is exact."""
    for d in (12, 17):
        tgt, x, lp64, g64, lp32, g32 = cases.reference(("pick_affine", pick, d, N))
        lp, g = _launch_density(ctx, "pick_affine", mode, tgt, x, True)
        _check(f"pick_affine {mode} D={d} pick={pick}", lp, g, lp64, g64, lp32, g32)
        lp_v, _ = _launch_density(ctx, "pick_affine", mode, tgt, x, False)
        np.testing.assert_array_equal(_bits(lp_v), _bits(lp))
        lp_b, g_b = _launch_density(ctx, "pick_affine", mode, tgt, x, True)
        np.testing.assert_array_equal(_bits(lp_b), _bits(lp))
        np.testing.assert_array_equal(_bits(g_b), _bits(g))
        n = (d - 3) // 4
        at = n + pick * (n + 1)
        want = np.zeros_like(x)
        want[:, at:at + n] = x[:, :n]                                   # x[0 .. n) on weight row pick
        want[:, at + n] = 1                                             # 1 on bias pick
        want[:, :n] = x[:, at:at + n]                                   # the weights on the entries
        np.testing.assert_array_equal(g, want)
        np.testing.assert_array_equal(g, g32)


# ---- 3. agreement ------------------------------------------------------------------------------------------------------------------
def _agree(tag, a, b, bound_a, bound_b):
    d = float(np.abs(a.astype(np.float64) - b).max())
    print(f"[custom_affine] {tag}: differ by {d:.3e} ({d / (bound_a + bound_b):.3f} of the two bounds)")
    assert d <= bound_a + bound_b, tag


@pytest.mark.parametrize("mode", ["data", "data_tape"])
def test_mlp2_affine_agrees_with_its_vec_twin(ctx, mode):
    """The same sums in the same order and the same bias adds: lp bit for bit.  The gradients take their sums in other orders."""
    shape = (3, 5, 4, 3)
    tag, lp, g, ref = _run(ctx, "mlp2_affine", mode, shape)
    tag_v, lp_v, g_v, ref_v = _run(ctx, "mlp2_vec", mode, shape)
    _check(tag, lp, g, *ref)
    _check(tag_v, lp_v, g_v, *ref_v)
    np.testing.assert_array_equal(_bits(lp), _bits(lp_v))
    lp64, g64, lp32, g32 = ref
    b_g = _bound(g32, g64, g32)[1]
    _agree(f"mlp2 {shape} {mode} affine against vec, gradient", g, g_v, b_g, b_g)


def test_mlp2_affine_agrees_with_its_vec_twin_above_the_forward_cap(ctx):
    tag, lp, g, ref = _run(ctx, "mlp2_affine", "data_tape", MLP2_BIG)
    tag_v, lp_v, g_v, ref_v = _run(ctx, "mlp2_vec", "data_tape", MLP2_BIG)
    _check(tag_v, lp_v, g_v, *ref_v)
    np.testing.assert_array_equal(_bits(lp), _bits(lp_v))
    lp64, g64, lp32, g32 = ref
    b_g = _bound(g32, g64, g32)[1]
    _agree(f"mlp2 {MLP2_BIG} affine against vec, gradient", g, g_v, b_g, b_g)


@pytest.mark.parametrize("mode", ["data", "data_tape"])
def test_keras_affine_agrees_with_its_loop_twin(ctx, mode):
    shape = (3, 5, 3)
    tag, lp, g, ref = _run(ctx, "keras_affine", mode, shape)
    tag_l, lp_l, g_l, ref_l = _run(ctx, "keras_loop", mode, shape)
    _check(tag, lp, g, *ref)
    _check(tag_l, lp_l, g_l, *ref_l)
    lp64, g64, lp32, g32 = ref
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    _agree(f"keras {shape} {mode} affine against loop, lp", lp, lp_l, b_lp, b_lp)
    _agree(f"keras {shape} {mode} affine against loop, gradient", g, g_l, b_g, b_g)


@pytest.mark.parametrize("name,shape", [("mlp2_affine", (3, 5, 4, 3)), ("keras_affine", (3, 5, 3))])
def test_forward_mode_and_reverse_mode_agree(ctx, name, shape):
    _, lp_f, g_f, ref = _run(ctx, name, "data", shape)
    _, lp_r, g_r, _ = _run(ctx, name, "data_tape", shape)
    lp64, g64, lp32, g32 = ref
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    _agree(f"{name} {shape} forward against reverse, lp", lp_f, lp_r, b_lp, b_lp)
    _agree(f"{name} {shape} forward against reverse, gradient", g_f, g_r, b_g, b_g)


# ---- 4. tape lengths ---------------------------------------------------------------------------------------------------------------
def _fresh(ctx, src, tag, mode="data_tape"):
    """A handle of its own (the module cache keys on the text), so that its remembered lengths are this test's."""
    from gmmvi_amd import hip_ops
    return hip_ops.custom_target_compile(ctx, src + f"\n// {tag}\n", mode=mode)


def _length_after_one_call(ctx, name, shape):
    from gmmvi_amd import hip_ops
    d = cases.dim(name, shape)
    handle = _fresh(ctx, cases.SOURCES[name], f"tape length {shape}")
    tgt, x = cases.build_data_case(cases.Case(name, d, N, 5, 0, None, 0), shape)
    assert hip_ops.custom_tape_length(ctx, handle, d) == 0
    (rc, _, _), launches = tape_data_mode._launches(ctx, lambda: tape_data_mode._launch(ctx, handle, tgt, x, True))
    assert rc == 0
    return hip_ops.custom_tape_length(ctx, handle, d), launches


@pytest.mark.parametrize("shape", [(3, 5, 4, 3), MLP2_BIG])
def test_tape_lengths_follow_from_the_texts(ctx, shape):
    """The length of a data tape is the longer of the row's and the prior's.  With L(n, m) = ceil(n / 2) + 2 + m slots per group:
    mlp2_affine is L(F, H1), H1 tanh records, L(H1, H2), H2 tanh records, L(H2, K), gmmvi_logsumexp 1 + ceil(K / 2), the final -.
    mlp2_vec: per unit of layer one gmmvi_dot, + and tanh, 3 H1; per unit of layer two gmmvi_wdot 1 + ceil(H1 / 2), + and tanh;
    per class gmmvi_wdot 1 + ceil(H2 / 2) and +; the same tail.  38 against 55 at (3, 5, 4, 3), 188 against 854 at
    (16, 32, 32, 8): both fit the 1 024 records of the first launch."""
    f, h1, h2, k = shape
    up = lambda n: (n + 1) // 2
    tail = 1 + up(k) + 1
    want_affine = (up(f) + 2 + h1) + h1 + (up(h1) + 2 + h2) + h2 + (up(h2) + 2 + k) + tail
    want_vec = 3 * h1 + h2 * (3 + up(h1)) + k * (2 + up(h2)) + tail
    assert (want_affine, want_vec) == cases.mlp2_lengths(*shape) == ((38, 55) if shape == (3, 5, 4, 3) else (188, 854))
    affine, launches_a = _length_after_one_call(ctx, "mlp2_affine", shape)
    vec, launches_v = _length_after_one_call(ctx, "mlp2_vec", shape)
    print(f"\n[custom_affine] tape lengths, mlp2 {shape}: affine {affine}, vec {vec}")
    assert (affine, vec) == (want_affine, want_vec) and (launches_a, launches_v) == (1, 1)


def test_the_density_tape_is_the_row_the_prior_and_one_add(ctx):
    """The density form is row + prior on one tape: the prior is 4 records (gmmvi_sumsq, *, /, -) and the sum one more."""
    from gmmvi_amd import hip_ops
    shape = (3, 5, 4, 3)
    d = cases.dim("mlp2_affine", shape)
    tgt, x = cases.reference(("mlp2_affine", shape, d, N))[:2]
    handle = _fresh(ctx, cases.DENSITY_SOURCES["mlp2_affine"], "density tape length", mode="tape")
    _launch_density(ctx, "mlp2_affine", "tape", tgt, x, True, handle=handle)
    assert hip_ops.custom_tape_length(ctx, handle, d) == cases.mlp2_lengths(*shape)[0] + 4 + 1


# ---- 5. tapes that overflow inside a group -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,where", [(1, "inside the payload"), (3, "on a descriptor slot"), (5, "on a header")])
def test_a_tape_that_overflows_inside_a_group(ctx, capacity, where):
    """pick_affine at D = 17 (n = 3) is 2 payload slots, 2 descriptor slots and 3 headers: 7.  The count still advances to 7, the
    call is launched again at that length, and the result has the bits of a call with ample capacity."""
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = cases.reference(("pick_affine", 2, 17, N))
    handle = _fresh(ctx, cases.PICK_AFFINE_SRC, f"overflow {where}", mode="tape")
    (rc, lp, g), launches = tape_mode._tape_launches(ctx, lambda: tape_mode._launch(ctx, handle, tgt.params(), x, True, capacity))
    assert rc == 0 and launches == 2
    assert hip_ops.custom_tape_length(ctx, handle, 17) == 7
    (rc, lp_big, g_big), launches = tape_mode._tape_launches(ctx, lambda: tape_mode._launch(ctx, handle, tgt.params(), x, True, 64))
    assert rc == 0 and launches == 1
    np.testing.assert_array_equal(_bits(lp), _bits(lp_big))
    np.testing.assert_array_equal(_bits(g), _bits(g_big))
    _check(f"pick_affine from a capacity of {capacity}", lp, g, lp64, g64, lp32, g32)


def test_a_row_tape_that_overflows_on_a_descriptor_slot(ctx):
    """mlp2_affine at (3, 5, 4, 3): the first group is 2 payload slots, then its descriptors: a capacity of 3 ends between them."""
    shape = (3, 5, 4, 3)
    c = cases.Case("mlp2_affine", cases.dim("mlp2_affine", shape), N, 5, 0, None, 0)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c, shape)
    handle = _fresh(ctx, cases.SOURCES["mlp2_affine"], "overflow on a descriptor slot")
    (rc, lp, g), launches = tape_data_mode._launches(ctx, lambda: tape_data_mode._launch(ctx, handle, tgt, x, True, 0, 3))
    assert rc == 0 and launches == 2
    _check("mlp2_affine from a capacity of 3", lp, g, lp64, g64, lp32, g32)
    (rc, lp_big, g_big), launches = tape_data_mode._launches(ctx, lambda: tape_data_mode._launch(ctx, handle, tgt, x, True, 0, 64))
    assert rc == 0 and launches == 1
    np.testing.assert_array_equal(_bits(lp), _bits(lp_big))
    np.testing.assert_array_equal(_bits(g), _bits(g_big))


# ---- 6. two kinds of record in one wave --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TAPE_ENTRIES)
def test_mixed_record_kinds_in_one_wave(ctx, mode):
    d = 17
    if mode == "tape":
        tgt, x, lp64, g64, lp32, g32 = cases.reference(("mixed_affine", (d,), d, N))
        lp, g = _launch_density(ctx, "mixed_affine", mode, tgt, x, True)
    else:
        c = _data_case("mixed_affine", mode, d)
        tgt, x, lp64, g64, lp32, g32 = _data_reference(c, (d,), mode)
        lp, g = _launch_data(ctx, "mixed_affine", mode, tgt, x, True, c.chunks)
    first_wave = x[:64, 0] > 0
    assert first_wave.any() and (~first_wave).any()
    _check(f"mixed_affine {mode} D={d}", lp, g, lp64, g64, lp32, g32)
    for pick, what in ((x[:, 0] > 0, "primitive lanes"), (x[:, 0] <= 0, "loop lanes")):
        _check(f"mixed_affine {mode} D={d}, {what}", lp[pick], g[pick], lp64[pick], g64[pick], lp32[pick], g32[pick])


# ---- 7. downstream -----------------------------------------------------------------------------------------------------------------
def test_log_predictive_over_held_out_rows(ctx):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF
    rng = np.random.default_rng(37)
    f, h, k, t, held_out = 4, 5, 3, 40, 5
    d = cases.keras_dim(f, h, k)
    rows = cases.rows_for(rng, "keras_affine", t + held_out, f, k).astype(np.float32)
    train, test = rows[:t], rows[t:]
    params = cases.PRIOR + [h, 0]
    target = DeviceDataLNPDF(cases.SOURCES["keras_affine"], d, train, params=params)
    ref_tgt = cases.Keras(train, params, d=d)
    x = (rng.normal(size=(130, d)) * 0.7).astype(np.float32)
    l64 = pred_cases.row_terms(ref_tgt, x.astype(np.float64), test)
    l32 = pred_cases.row_terms(cases.fp32_twin(ref_tgt), x, test)
    out = [o.numpy() for o in target.log_predictive(x, test)]
    assert all(o.shape == (held_out,) for o in out)
    predictive._check("keras_affine log_predictive over 5 held-out rows", out, pred_cases.reference64(l64), pred_cases.twin32(l32))


def test_diagonal_stein_iteration_above_the_forward_cap(monkeypatch):
    """test_diagonal_stein_iteration_above_the_forward_cap of tests/test_hip_custom_data_tape.py, its set-up, its follow-up and its
    tolerance, with mlp2_affine for the source, its restatement for the oracle's target and rows of 9 features and a label in
    [0, 6): (F, H1, H2, K) = (9, 16, 16, 6), D = 534, T = 40, three iterations."""
    f, h1, h2, k = 9, 16, 16, 6
    d = cases.mlp2_dim(f, h1, h2, k)
    assert d == 534
    monkeypatch.setitem(tape_data_mode.cases.SOURCES, "logit", cases.SOURCES["mlp2_affine"])
    monkeypatch.setattr(tape_data_mode.cases.base, "Logit",
                        lambda data, params, **kw: cases.Mlp2(data, list(params) + [h1, h2], d=d, **kw))
    monkeypatch.setattr(tape_data_mode, "_logit_rows", lambda rng, t, dim: cases.rows_for(rng, "mlp2_affine", t, f, k).astype(np.float32))
    ref, target, o, g, per_iter = tape_data_mode._diagonal_pair(d, None)
    assert isinstance(ref, cases.Mlp2) and "gmmvi_affine" in target.source and ref.data.shape == (40, f + 1)
    tape_data_mode._follow(o, g, 3, d)
    assert int(g.sample_db.num_samples_written) == 3 * per_iter and target.call_count == 0
