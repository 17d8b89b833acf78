"""GPU tests of the vector primitives of user-defined device targets (csrc/custom_target_vector.inc, their overloads in
csrc/custom_target_autodiff.inc and csrc/custom_target_tape.inc, the vector record in the sweep of both tape modes): targets
written with gmmvi_dot, gmmvi_sqdist and gmmvi_sumsq against fp64 in every mode, through the C ABI; the value call against the
gradient call bit for bit; the tape lengths, which follow from the texts; agreement with the scalar-loop source and between
forward and reverse mode; two kinds of record at one record index in one wave; overlapping sub-ranges and an output that is a
single vector node; the predictive density and the diagonal Stein iteration above the forward cap.

Kernel bound: _bound of tests/test_hip_custom_target.py, unchanged: the device's largest error against the fp64 NumPy
restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|, for lp and for the gradient.  Every case prints its ratios before it asserts.

Tape lengths.  The issue that asked for these tests derives  length(logit_vec) == length(logit) - 2 * 17 + 1  at D = 17 from the
row term alone; gmmvi_custom_tape_length is the longest tape of the row term AND the prior, and the loop prior of ``logit``
makes 4 D + 2 = 70 records there, more than its row's 2 D + 9 = 43 (gmmvi_data_tape_probe reports 70 on the host).  The
relation is therefore asserted where the row decides, against ``logit_loop_row`` (the loop row with the gmmvi_sumsq prior), and
all three absolute lengths are asserted as well: 70, 43 and 10."""
import numpy as np
import pytest

import custom_predictive_cases as pred_cases
import custom_vector_cases as cases
import test_hip_custom_data as data_mode
import test_hip_custom_data_own as own_mode
import test_hip_custom_data_tape as tape_data_mode
import test_hip_custom_predictive as predictive
import test_hip_custom_tape as tape_mode
import test_hip_custom_target as hand
from custom_data_own_cases import OwnBatches
from custom_data_tape_cases import SOURCES as LOOP_SOURCES
from test_hip_custom_target import _bound

pytestmark = pytest.mark.gpu

N = 65                                                               # one tile and one lane of the next
DIMS = (1, 17, 67)
ABOVE_THE_FORWARD_CAP = 600
DENSITY_MODES = ("hand", "autodiff", "tape")
DATA_MODES = ("data", "data_tape", "data_own", "data_tape_own")


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name, mode):
    from gmmvi_amd import hip_ops
    if (name, mode) not in _handles:
        if mode in ("data", "data_tape"):
            src = LOOP_SOURCES[name] if name == "logit" else cases.SOURCES[name]
        else:
            src = cases.HAND_SOURCES[name] if mode == "hand" else cases.DENSITY_SOURCES[name]
        _handles[(name, mode)] = hip_ops.custom_target_compile(ctx, src, mode=mode)
    return _handles[(name, mode)]


def _launch_density(ctx, name, mode, tgt, x, want_grad):
    """-> (lp, grad | None) through gmmvi_target_custom or gmmvi_target_custom_tape, canary rows behind both outputs."""
    handle = _handle(ctx, name, mode)
    if mode == "tape":
        rc, lp, g = tape_mode._launch(ctx, handle, tgt.params(), x, want_grad)
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
    line = f"[custom_vector] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
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


# ---- 1. against fp64 ---------------------------------------------------------------------------------------------------------------
DENSITY_CASES = [(name, mode, d) for name in ("logit_vec", "rbf_vec") for mode in DENSITY_MODES for d in DIMS]
DENSITY_CASES += [(name, "tape", ABOVE_THE_FORWARD_CAP) for name in ("logit_vec", "rbf_vec")]


@pytest.mark.parametrize("name,mode,d", DENSITY_CASES, ids=lambda v: str(v))
def test_density_matches_fp64_reference(ctx, name, mode, d):
    tgt, x, lp64, g64, lp32, g32 = cases.reference((name, d, N))
    lp, g = _launch_density(ctx, name, mode, tgt, x, True)
    _check(f"{name} {mode} D={d}", lp, g, lp64, g64, lp32, g32)
    lp_v, _ = _launch_density(ctx, name, mode, tgt, x, False)
    _check(f"{name} {mode} D={d} values only", lp_v, None, lp64, g64, lp32, g32)


def _data_case(name, mode, d):
    """67 rows in 3 chunks; the own-batch entries draw B = 5 of them per sample."""
    return cases.Case(name, d, N, 67, 3, 5 if mode.endswith("_own") else None, 3 if mode.endswith("_own") else 0)


def _data_reference(c, mode):
    if not mode.endswith("_own"):
        return cases.reference(c)
    key = (c, "own")
    if key not in cases._refs:
        tgt, x = cases.build_data_case(c)
        own = OwnBatches(tgt)
        lp64, g64 = own.evaluate(x.astype(np.float64))
        lp32, g32 = own.as_dtype(np.float32).evaluate(x)
        for a in (lp64, g64, lp32, g32, x):
            a.setflags(write=False)
        cases._refs[key] = (tgt, x, lp64, g64, lp32, g32)
    return cases._refs[key]


DATA_CASES = [(name, mode, d) for name in ("logit_vec", "rbf_vec") for mode in DATA_MODES for d in DIMS]
DATA_CASES += [(name, mode, ABOVE_THE_FORWARD_CAP) for name in ("logit_vec", "rbf_vec") for mode in ("data_tape", "data_tape_own")]


@pytest.mark.parametrize("name,mode,d", DATA_CASES, ids=lambda v: str(v))
def test_data_target_matches_fp64_reference(ctx, name, mode, d):
    c = _data_case(name, mode, d)
    tgt, x, lp64, g64, lp32, g32 = _data_reference(c, mode)
    lp, g = _launch_data(ctx, name, mode, tgt, x, True, c.chunks)
    _check(f"{cases.case_id(c)} {mode}", lp, g, lp64, g64, lp32, g32)
    lp_v, _ = _launch_data(ctx, name, mode, tgt, x, False, c.chunks)
    _check(f"{cases.case_id(c)} {mode} values only", lp_v, None, lp64, g64, lp32, g32)


@pytest.mark.parametrize("mode", ["data", "data_tape"])
def test_shared_minibatch_matches_fp64_reference(ctx, mode):
    c = cases.Case("logit_vec", 17, N, 67, 0, 5, 3)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    lp, g = _launch_data(ctx, c.name, mode, tgt, x, True)
    _check(f"{cases.case_id(c)} {mode}", lp, g, lp64, g64, lp32, g32)


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["logit_vec", "rbf_vec"])
@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_density_value_call_and_gradient_call_give_the_same_lp_bits(ctx, name, mode):
    for d in (17, 67):
        tgt, x = cases.reference((name, d, N))[:2]
        lp_g, g = _launch_density(ctx, name, mode, tgt, x, True)
        lp_v, _ = _launch_density(ctx, name, mode, tgt, x, False)
        np.testing.assert_array_equal(_bits(lp_v), _bits(lp_g))
        lp_b, g_b = _launch_density(ctx, name, mode, tgt, x, True)
        np.testing.assert_array_equal(_bits(lp_b), _bits(lp_g))
        np.testing.assert_array_equal(_bits(g_b), _bits(g))


@pytest.mark.parametrize("name", ["logit_vec", "rbf_vec"])
@pytest.mark.parametrize("mode", DATA_MODES)
def test_data_value_call_and_gradient_call_give_the_same_lp_bits(ctx, name, mode):
    """The forward entries add the rows in one order on both calls: 67 rows in 3 chunks.  The value call of the tape entries is
    the data mode's, whose order over the rows differs from the tape kernel's, so there the two calls can only agree in every bit
    where no order exists: one row in one chunk (B = 1 for the own batches), which still shows that the float and the recorded
    instantiation of each primitive give the same bits."""
    rows = 67 if "tape" not in mode else 1
    own = mode.endswith("_own")
    c = cases.Case(name, 67, N, rows if not own else 9, 3 if rows > 1 else 1, (5 if rows > 1 else 1) if own else None, 3 if own else 0)
    tgt, x = cases.build_data_case(c)
    lp_g, g = _launch_data(ctx, name, mode, tgt, x, True, c.chunks)
    lp_v, _ = _launch_data(ctx, name, mode, tgt, x, False, c.chunks)
    np.testing.assert_array_equal(_bits(lp_v), _bits(lp_g))
    lp_b, g_b = _launch_data(ctx, name, mode, tgt, x, True, c.chunks)
    np.testing.assert_array_equal(_bits(lp_b), _bits(lp_g))
    np.testing.assert_array_equal(_bits(g_b), _bits(g))


# ---- 3. tape length ----------------------------------------------------------------------------------------------------------------
def _fresh(ctx, src, tag):
    """A handle of its own (the module cache keys on the text), so that its remembered lengths are this test's."""
    from gmmvi_amd import hip_ops
    return hip_ops.custom_target_compile(ctx, src + f"\n// {tag}\n", mode="data_tape")


def test_tape_lengths_follow_from_the_texts(ctx):
    from gmmvi_amd import hip_ops
    loop = _fresh(ctx, LOOP_SOURCES["logit"], "tape length")
    loop_row = _fresh(ctx, cases.SOURCES["logit_loop_row"], "tape length")
    vec = _fresh(ctx, cases.SOURCES["logit_vec"], "tape length")
    d = 17
    tgt, x = cases.build_data_case(cases.Case("logit_vec", d, N, 5, 0, None, 0))
    for handle in (loop, loop_row, vec):
        assert hip_ops.custom_tape_length(ctx, handle, d) == 0
        rc, _, _ = tape_data_mode._launch(ctx, handle, tgt, x, True)
        assert rc == 0
    lengths = [hip_ops.custom_tape_length(ctx, h, d) for h in (loop, loop_row, vec)]
    print(f"\n[custom_vector] tape lengths at D = {d}: logit {lengths[0]}, loop row with the gmmvi_sumsq prior {lengths[1]}, "
          f"logit_vec {lengths[2]}")
    # the row: 2 records per coordinate, or one for gmmvi_dot, and 9 behind them; the prior: 4 per coordinate and 2, or 3
    assert lengths == [4 * d + 2, 2 * d + 9, 1 + 9]
    assert lengths[2] == lengths[1] - 2 * d + 1
    big = ABOVE_THE_FORWARD_CAP
    tgt_big, x_big = cases.build_data_case(cases.Case("logit_vec", big, N, 5, 0, None, 0))
    rc, _, _ = tape_data_mode._launch(ctx, vec, tgt_big, x_big, True)
    assert rc == 0
    assert hip_ops.custom_tape_length(ctx, vec, big) == hip_ops.custom_tape_length(ctx, vec, d) == 10


def test_one_launch_at_d_4096_where_the_loop_source_takes_two(ctx):
    from gmmvi_amd import hip_ops
    c = cases.Case("logit_vec", 4096, 5, 5, 0, None, 0)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    vec = _fresh(ctx, cases.SOURCES["logit_vec"], "one launch")
    assert hip_ops.custom_tape_length(ctx, vec, c.d) == 0
    (rc, lp, g), launches = tape_data_mode._launches(ctx, lambda: tape_data_mode._launch(ctx, vec, tgt, x, True))
    assert rc == 0 and launches == 1
    assert hip_ops.custom_tape_length(ctx, vec, c.d) == 10
    _check(cases.case_id(c), lp, g, lp64, g64, lp32, g32)


# ---- 4. agreement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [17, ABOVE_THE_FORWARD_CAP])
def test_logit_vec_agrees_with_the_loop_source(ctx, d):
    c = cases.Case("logit_vec", d, N, 67, 3, None, 0)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    loop_tgt, x_l, l64, lg64, l32, lg32 = cases.reference(c._replace(name="logit"))
    np.testing.assert_array_equal(x, x_l)
    lp, g = _launch_data(ctx, "logit_vec", "data_tape", tgt, x, True, c.chunks)
    lp_l, g_l = _launch_data(ctx, "logit", "data_tape", loop_tgt, x, True, c.chunks)
    _check(f"{cases.case_id(c)} data_tape", lp, g, lp64, g64, lp32, g32)
    _check(f"logit (loops) D={d} data_tape", lp_l, g_l, l64, lg64, l32, lg32)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1] + _bound(l32, l64, l32)[1], _bound(g32, g64, g32)[1] + _bound(lg32, lg64, lg32)[1]
    d_lp, d_g = float(np.abs(lp.astype(np.float64) - lp_l).max()), float(np.abs(g.astype(np.float64) - g_l).max())
    print(f"[custom_vector] logit_vec against the loop source at D={d}: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the two "
          f"bounds), the gradient by {d_g:.3e} ({d_g / b_g:.3f})")
    assert d_lp <= b_lp and d_g <= b_g


def test_forward_mode_and_reverse_mode_agree(ctx):
    c = cases.Case("logit_vec", 67, N, 67, 3, None, 0)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    lp_f, g_f = _launch_data(ctx, c.name, "data", tgt, x, True, c.chunks)
    lp_r, g_r = _launch_data(ctx, c.name, "data_tape", tgt, x, True, c.chunks)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    d_lp, d_g = float(np.abs(lp_f.astype(np.float64) - lp_r).max()), float(np.abs(g_f.astype(np.float64) - g_r).max())
    print(f"\n[custom_vector] {cases.case_id(c)} forward against reverse: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), "
          f"the gradient by {d_g:.3e} ({d_g / b_g:.3f})")
    assert d_lp <= b_lp and d_g <= b_g
    _check(f"{cases.case_id(c)} data", lp_f, g_f, lp64, g64, lp32, g32)


# ---- 5. two kinds of record at one record index in one wave ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tape", "data_tape", "data_tape_own"])
def test_mixed_record_kinds_in_one_wave(ctx, mode):
    d = 17
    if mode == "tape":
        tgt, x, lp64, g64, lp32, g32 = cases.reference(("mixed", d, N))
        lp, g = _launch_density(ctx, "mixed", mode, tgt, x, True)
    else:
        c = _data_case("mixed", mode, d)
        tgt, x, lp64, g64, lp32, g32 = _data_reference(c, mode)
        lp, g = _launch_data(ctx, "mixed", mode, tgt, x, True, c.chunks)
    first_wave = x[:64, 0] > 0
    assert first_wave.any() and (~first_wave).any()
    _check(f"mixed {mode} D={d}", lp, g, lp64, g64, lp32, g32)
    for pick, what in ((x[:, 0] > 0, "gmmvi_dot lanes"), (x[:, 0] <= 0, "loop lanes")):
        _check(f"mixed {mode} D={d}, {what}", lp[pick], g[pick], lp64[pick], g64[pick], lp32[pick], g32[pick])


# ---- 6. sub-ranges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_overlapping_sub_ranges(ctx, mode):
    tgt, x, lp64, g64, lp32, g32 = cases.reference(("ranges", cases.RANGES_D, N))
    lp, g = _launch_density(ctx, "ranges", mode, tgt, x, True)
    _check(f"ranges {mode}", lp, g, lp64, g64, lp32, g32)
    assert not np.any(_bits(g[:, :3]))                                # no primitive reads x[0 .. 3)
    lp_v, _ = _launch_density(ctx, "ranges", mode, tgt, x, False)
    _check(f"ranges {mode} values only", lp_v, None, lp64, g64, lp32, g32)


@pytest.mark.parametrize("mode", ["autodiff", "tape"])
def test_output_that_is_a_single_vector_node(ctx, mode):
    for d in (1, 17):
        tgt, x, lp64, g64, lp32, g32 = cases.reference(("single", d, N))
        lp, g = _launch_density(ctx, "single", mode, tgt, x, True)
        _check(f"single {mode} D={d}", lp, g, lp64, g64, lp32, g32)
        np.testing.assert_array_equal(_bits(g), _bits(np.broadcast_to(tgt.params()[:d], g.shape)))   # the coefficients themselves
        lp_v, _ = _launch_density(ctx, "single", mode, tgt, x, False)
        np.testing.assert_array_equal(_bits(lp_v), _bits(lp))


# ---- 7. downstream -----------------------------------------------------------------------------------------------------------------
def test_log_predictive_over_held_out_rows(ctx):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF
    rng = np.random.default_rng(31)
    d, t, held_out = 17, 40, 5
    rows = np.concatenate([rng.normal(size=(t + held_out, d)) / np.sqrt(d),
                           rng.choice([-1.0, 1.0], size=(t + held_out, 1))], axis=1).astype(np.float32)
    train, test = rows[:t], rows[t:]
    params = [0.25, 2.0]
    target = DeviceDataLNPDF(cases.SOURCES["logit_vec"], d, train, params=params)
    ref_tgt = cases.LogitVec(train, params)
    x = (rng.normal(size=(130, d)) * 0.7).astype(np.float32)
    l64 = pred_cases.row_terms(ref_tgt, x.astype(np.float64), test)
    l32 = pred_cases.row_terms(cases.fp32_twin(ref_tgt), x, test)
    out = [o.numpy() for o in target.log_predictive(x, test)]
    assert all(o.shape == (held_out,) for o in out)
    predictive._check("logit_vec log_predictive over 5 held-out rows", out, pred_cases.reference64(l64), pred_cases.twin32(l32))


def test_diagonal_stein_iteration_above_the_forward_cap(monkeypatch):
    """test_diagonal_stein_iteration_above_the_forward_cap of tests/test_hip_custom_data_tape.py, its set-up, its follow-up and its
    tolerance, with logit_vec for the source and its restatement for the oracle's target: D = 600, T = 40, three iterations."""
    monkeypatch.setitem(tape_data_mode.cases.SOURCES, "logit", cases.SOURCES["logit_vec"])
    monkeypatch.setattr(tape_data_mode.cases.base, "Logit", cases.LogitVec)
    ref, target, o, g, per_iter = tape_data_mode._diagonal_pair(ABOVE_THE_FORWARD_CAP, None)
    assert isinstance(ref, cases.LogitVec) and "gmmvi_dot" in target.source and "gmmvi_sumsq" in target.source
    tape_data_mode._follow(o, g, 3, ABOVE_THE_FORWARD_CAP)
    assert int(g.sample_db.num_samples_written) == 3 * per_iter and target.call_count == 0
