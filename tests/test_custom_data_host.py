"""User-defined device targets summed over a data set, the part that needs no GPU: the run-time compiler builds source +
dual-number text + tile mover + Feistel stream + kernels for gfx950 without a device (gmmvi_custom_target_check_data), compile
errors come back as argument errors with the user's own line numbers and name a missing function, the NumPy restatements agree
with central differences, the minibatch stream and the launch plan do what include/gmmvi_hip.h says, DeviceDataLNPDF rejects
bad arguments before it touches the device, and every planted fault of tests/custom_data_cases.py exceeds ten times the bound
of the GPU test (tests/test_hip_custom_data.py) on the references alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import custom_data_cases as cases
from helpers import use_host_context
from test_hip_custom_target import _bound

ERR_ARG = -2


def _w():
    from gmmvi_amd import _lib
    return _lib.CUSTOM_AUTODIFF_TANGENTS


def _all_cases():
    from gmmvi_amd import _lib
    return cases.kernel_cases(_lib.CUSTOM_AUTODIFF_TANGENTS, _lib.CUSTOM_STAGED_MAX_DIM)


def _plan(c):
    from gmmvi_amd import hip_ops
    return hip_ops.custom_data_plan(c.n, c.rows if c.batch is None else c.batch, c.chunks)


# ---- the compiler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_case_sources_compile_for_gfx950(name):
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_data(cases.SOURCES[name], "gfx950")
    assert rc == 0, log


def test_syntax_error_is_an_argument_error_with_the_users_line():
    from gmmvi_amd import _lib, hip_ops
    lines = cases.STUDENT_SRC.split("\n")
    bad_line = next(i for i, text in enumerate(lines) if "T r = row[D];" in text)
    lines[bad_line] = "    T r = row[D] - ;"
    rc, log = hip_ops.custom_target_check_data("\n".join(lines), "gfx950")
    assert rc == ERR_ARG
    assert f":{bad_line + 1}:" in log, log                     # clang's file:line:column of the user's own text
    assert "error" in log
    assert log.strip() in _lib.load().gmmvi_last_error(None).decode()
    rc, log = hip_ops.custom_target_check_data("int broken = ;\n" + cases.STUDENT_SRC, "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_target.hip:1:" in log, log


def _split_source(src):
    head, tail = src.split("template <class T, class X>\n__device__ T gmmvi_user_prior")
    return head, "template <class T, class X>\n__device__ T gmmvi_user_prior" + tail


def test_source_without_a_function_names_the_missing_one():
    from gmmvi_amd import hip_ops
    row_only, prior_only = _split_source(cases.LOGIT_SRC)
    rc, log = hip_ops.custom_target_check_data(prior_only, "gfx950")
    assert rc == ERR_ARG and "does not define gmmvi_user_row" in log and "does not define gmmvi_user_prior" not in log, log
    rc, log = hip_ops.custom_target_check_data(row_only, "gfx950")
    assert rc == ERR_ARG and "does not define gmmvi_user_prior" in log and "does not define gmmvi_user_row" not in log, log
    # a density of the differentiated mode is not a data-mode source, and the other way round
    import custom_autodiff_cases as autodiff
    rc, log = hip_ops.custom_target_check_data(autodiff.ROSENBROCK_SRC, "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_row" in log and "gmmvi_user_prior" in log
    rc, log = hip_ops.custom_target_check_autodiff(cases.LOGIT_SRC, "gfx950")
    assert rc == ERR_ARG and "gmmvi_user_density" in log


def test_function_outside_the_surface_is_a_compile_error():
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_data(cases.STUDENT_SRC.replace("return -0.5f * (nu", "return lgammaf(r) - 0.5f * (nu"), "gfx950")
    assert rc == ERR_ARG and log.strip() and "lgammaf" in log
    rc, log = hip_ops.custom_target_check_data(cases.STUDENT_SRC.replace("return -0.5f * (nu", "return lgammaf(nu) - 0.5f * (nu"), "gfx950")
    assert rc == 0, log


def test_null_arguments_are_argument_errors():
    from gmmvi_amd import _lib
    lib = _lib.load()
    assert lib.gmmvi_custom_target_check_data(None, b"gfx950", None, 0) == ERR_ARG
    assert lib.gmmvi_custom_target_check_data(b"", None, None, 0) == ERR_ARG
    buf = C.create_string_buffer(b"\xff" * 16, 16)
    assert lib.gmmvi_custom_target_check_data(b"nonsense", b"gfx950", buf, 16) == ERR_ARG
    assert len(buf.value) == 15


def test_constants_and_symbols():
    from gmmvi_amd import _lib
    from gmmvi_amd.experiments.target_distributions import minibatch_stream
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    feistel = open(os.path.join(root, "gmmvi_amd", "csrc", "feistel.h")).read()
    assert int(re.search(r"GMMVI_STREAM_DATA_MINIBATCH = (\d+);", feistel).group(1)) == minibatch_stream.STREAM_DATA_MINIBATCH == 5
    for symbol in ("gmmvi_custom_target_check_data", "gmmvi_custom_target_compile_data", "gmmvi_target_custom_data",
                   "gmmvi_custom_data_plan"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
    # no new struct and no new member of the target descriptor came with the feature
    assert [f[0] for f in _lib.TargetSpec._fields_][-2:] == ["custom", "custom_params"]
    assert _lib.load().gmmvi_struct_bytes(4) == 0


# ---- the references --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["logit", "student", "nodata"])
@pytest.mark.parametrize("batch", [None, 4])
def test_restatements_agree_with_central_differences(name, batch):
    c = cases.Case(name, 6, 5, 11, 0, batch, 2)
    tgt, x = cases.build_case(c)
    x = x.astype(np.float64)
    lp, g = tgt.evaluate(x)
    h = 1e-6
    for i in range(c.d):
        e = np.zeros(c.d); e[i] = h
        fd = (tgt.evaluate(x + e)[0] - tgt.evaluate(x - e)[0]) / (2 * h)
        np.testing.assert_allclose(g[:, i], fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} coordinate {i}")


def test_restatement_follows_the_call_counter():
    c = cases.Case("logit", 5, 3, 9, 0, 4, 0)
    tgt, x = cases.build_case(c)
    assert tgt.call_count == 0
    first = tgt.log_density(x)
    assert tgt.call_count == 1
    second, _ = tgt.log_density_and_grad(x)
    assert tgt.call_count == 2 and not np.array_equal(first, second)
    tgt.log_density(x[:0])
    assert tgt.call_count == 2
    full = tgt.full()
    a = full.log_density(x)
    assert full.call_count == 0 and np.array_equal(a, full.log_density(x))


def test_kernel_cases_sit_on_the_seams():
    from gmmvi_amd import _lib
    w, cap = _w(), _lib.CUSTOM_STAGED_MAX_DIM
    all_cases = _all_cases()
    full = [c for c in all_cases if c.batch is None]
    mini = [c for c in all_cases if c.batch is not None]
    assert {1, 63, 64, 65, 130} <= {c.n for c in full}
    assert {w - 1, w, w + 1, 2 * w + 1, cap, cap + 1} <= {c.d for c in full}
    assert {1, 3, 4, 5, 257} <= {c.rows for c in full if c.chunks == 0}
    assert {2, 3} <= {c.chunks for c in full if c.rows == 67}
    assert any(c.chunks > c.rows for c in full)
    assert {"logit", "student", "nodata"} <= {c.name for c in full}
    for t in (9, 257, 1025):
        assert {(1, 0), (1, 3), (5, 0), (5, 3), (t, 0), (t, 3)} <= {(c.batch, c.call) for c in mini if c.rows == t}
    assert len(set(all_cases)) == len(all_cases)
    # the automatic plan of the 257-row cases has a chunk seam, and the largest minibatch is merged from many chunks
    assert all(_plan(c)[0] > 1 for c in full if c.rows == 257)
    assert max(_plan(c)[0] for c in mini) >= 16


# ---- the stream ------------------------------------------------------------------------------------------------------------
def test_data_minibatch_rows():
    from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms
    for t in (9, 257, 1025):
        for b in (1, 5, t):
            rows = ms.data_minibatch_rows(9, 3, b, t)
            assert rows.shape == (b,) and rows.dtype == np.int64
            assert len(set(rows.tolist())) == b and rows.min() >= 0 and rows.max() < t
            j = np.arange(b)
            np.testing.assert_array_equal(rows, ms.permute_rows(9, 3, np.zeros_like(j), j, t, stream=5))
        whole = ms.data_minibatch_rows(9, 3, t, t)
        np.testing.assert_array_equal(np.sort(whole), np.arange(t))
        # a smaller batch is the head of the larger one: row j does not depend on B
        np.testing.assert_array_equal(ms.data_minibatch_rows(9, 3, 5, t), whole[:5])
        assert not np.array_equal(whole, ms.data_minibatch_rows(9, 4, t, t))
        assert not np.array_equal(whole, ms.data_minibatch_rows(10, 3, t, t))
        assert not np.array_equal(whole, ms.permute_rows(9, 3, np.zeros(t, np.int64), np.arange(t), t, stream=4))
    for bad in (0, 10):
        with pytest.raises(ValueError):
            ms.data_minibatch_rows(9, 3, bad, 9)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_launch_plan():
    from gmmvi_amd import _lib, hip_ops
    for n in (1, 64, 65, 300, 10 ** 4, 10 ** 6):
        for rows in (1, 3, 4, 31, 32, 33, 67, 257, 569, 20000, 2 ** 31 - 1):
            for request in (0, 1, 2, 3, 7, 10 ** 5):
                chunks, per = hip_ops.custom_data_plan(n, rows, request)
                assert chunks >= 1 and per >= 1
                assert chunks * per >= rows, (n, rows, request)
                assert (chunks - 1) * per < rows, (n, rows, request)          # the last chunk is not empty
                if request > 0:
                    assert chunks <= min(request, rows, 65535)
                    if rows % min(request, rows) == 0 and request <= 65535:
                        assert chunks == min(request, rows)                    # an exact split is honoured as asked
    assert hip_ops.custom_data_plan(5, 3, 9) == (3, 1)                         # clamped to one row per chunk
    assert hip_ops.custom_data_plan(5, 67, 3) == (3, 23) and hip_ops.custom_data_plan(5, 67, 2) == (2, 34)
    assert hip_ops.custom_data_plan(64, 20000)[0] > 1
    assert hip_ops.custom_data_plan(10 ** 4, 4) == (1, 4)
    # auto never leaves a chunk with fewer than 32 rows (8 per wave) unless there is one chunk
    for n, rows in ((64, 20000), (300, 569), (10 ** 4, 569), (1, 33), (1, 63), (1, 64)):
        chunks, per = hip_ops.custom_data_plan(n, rows)
        assert chunks == 1 or per >= 32, (n, rows, chunks, per)
    lib = _lib.load()
    a, b = C.c_int(), C.c_int()
    for n, rows, request in ((0, 5, 0), (5, 0, 0), (5, 2 ** 31, 0), (5, 5, -1)):
        assert lib.gmmvi_custom_data_plan(n, rows, request, C.byref(a), C.byref(b)) == ERR_ARG
    assert lib.gmmvi_custom_data_plan(5, 5, 0, None, C.byref(b)) == ERR_ARG


# ---- the class -------------------------------------------------------------------------------------------------------------
def test_device_data_lnpdf_argument_errors(monkeypatch):
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    use_host_context(monkeypatch, device_lnpdf)
    data = np.zeros((9, 6), np.float32)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="num_dimensions"):
            device_lnpdf.DeviceDataLNPDF(cases.LOGIT_SRC, bad, data, params=[0.0, 1.0])
    for d in (513, 1024):
        with pytest.raises(ValueError, match="512"):
            device_lnpdf.DeviceDataLNPDF(cases.LOGIT_SRC, d, data)
    for bad_data in (np.zeros(9), np.zeros((3, 3, 3)), np.zeros((0, 6)), np.zeros((9, 0))):
        with pytest.raises(ValueError, match="two-dimensional"):
            device_lnpdf.DeviceDataLNPDF(cases.LOGIT_SRC, 5, bad_data)
    for bad_batch in (0, 10, -1, 2.5):
        with pytest.raises(ValueError, match="batch_size"):
            device_lnpdf.DeviceDataLNPDF(cases.LOGIT_SRC, 5, data, batch_size=bad_batch)
    with pytest.raises(ValueError, match="one-dimensional"):
        device_lnpdf.DeviceDataLNPDF(cases.LOGIT_SRC, 5, data, params=np.ones((2, 2)))


def test_class_facts():
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF, DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi_amd.experiments.target_distributions.minibatch_stream import MinibatchLNPDF
    from gmmvi.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF as Alias
    assert Alias is DeviceDataLNPDF
    assert issubclass(DeviceDataLNPDF, MinibatchLNPDF) and not issubclass(DeviceDataLNPDF, DeviceLNPDF)
    assert DeviceDataLNPDF.gradient_on_demand is True
    assert DeviceDataLNPDF.log_density_and_grad is not LNPDF.log_density_and_grad
    assert not hasattr(DeviceDataLNPDF, "_fast_path_target")
    assert hasattr(DeviceDataLNPDF, "log_density_full")


# ---- the bound of the GPU test can see the mistakes a kernel of this kind makes ------------------------------------------------
def _exemptions(c, plan):
    """fault -> why case ``c`` cannot show it (on lp and on the gradient alike, unless the reason says otherwise)."""
    length = c.rows if c.batch is None else c.batch
    out = {}
    if length < 2:
        out["drop_last_row"] = "the only row: dropping it leaves an empty sum, which is the no-row fault of another shape"
        out["drop_first_row_of_wave_1"] = "one row: wave 1 has none"
    if plan[0] < 2:
        out["drop_first_row_of_last_chunk"] = "one chunk: no chunk seam"
    if c.batch is None:
        out["unit_scale"] = "full data: s is 1"
        out["next_call"] = "full data: no stream"
    elif c.batch == c.rows:
        out["unit_scale"] = "B = T: s is 1"
        out["next_call"] = "B = T: every call is a permutation of all rows, the same sum in another order"
    return out


# nodata's row term has zero tangents: a fault in the row list or in s cannot show in its gradient
GRADIENT_BLIND = {"nodata": ("drop_last_row", "drop_first_row_of_wave_1", "drop_first_row_of_last_chunk", "unit_scale", "next_call")}


def test_exemptions_are_the_expected_ones():
    """The exempt (case, fault) pairs by name: nothing is skipped silently, and every fault is shown by many cases."""
    shown = {f: 0 for f in cases.FAULTS}
    for c in _all_cases():
        ex = _exemptions(c, _plan(c))
        for f in cases.FAULTS:
            shown[f] += f not in ex
        if c.batch is None:
            assert {"unit_scale", "next_call"} <= set(ex)
        assert "no_prior" not in ex and ("drop_last_row" in ex) == ((c.rows if c.batch is None else c.batch) == 1)
    assert all(v >= 6 for v in shown.values()), shown


@pytest.mark.parametrize("c", _all_cases(), ids=cases.case_id)
def test_planted_faults_exceed_ten_times_the_gpu_bound(c):
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    plan = _plan(c)
    _, b_lp, _ = _bound(lp32, lp64, lp32)
    _, b_g, _ = _bound(g32, g64, g32)
    # the device's own summation order stays far inside the bound: what the factor 10 is measured against
    dlp, dg = cases.fp32_twin(tgt).evaluate_in_device_order(x, plan)
    e_lp, e_g = _bound(dlp, lp64, lp32)[0], _bound(dg, g64, g32)[0]
    print(f"\n[custom_data] {cases.case_id(c)} plan {plan}: device-order fp32 NumPy error {e_lp / b_lp:.3f} (lp), {e_g / b_g:.3f} (gradient) "
          f"of the bound")
    assert e_lp <= 0.5 * b_lp and e_g <= 0.5 * b_g
    exempt = _exemptions(c, plan)
    x64 = x.astype(np.float64)
    for fault in cases.FAULTS:
        if fault in exempt:
            print(f"[custom_data] {cases.case_id(c)}: {fault} exempt ({exempt[fault]})")
            continue
        flp, fg = tgt.evaluate(x64, fault=fault, plan=plan)
        r_lp = float(np.abs(flp - lp64).max()) / b_lp
        r_g = float(np.abs(fg - g64).max()) / b_g
        print(f"[custom_data] {cases.case_id(c)}: {fault} moves lp by {r_lp:.3g} and the gradient by {r_g:.3g} times the bound")
        assert r_lp > 10.0, f"{fault}: lp moves by {r_lp:.3g} times the bound"
        if fault in GRADIENT_BLIND.get(c.name, ()):
            assert r_g == 0.0, "a row term without tangents moved the gradient"
        else:
            assert r_g > 10.0, f"{fault}: the gradient moves by {r_g:.3g} times the bound"
