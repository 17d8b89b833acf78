"""Reverse-mode gradients of user-defined device targets summed over a data set, the part that needs no GPU: the run-time
compiler builds source + data-mode text + tape number type + kernels for gfx950 without a device
(gmmvi_custom_target_check_data_tape) and names a missing function; the plan (gmmvi_custom_data_tape_plan) keeps its promises
over a grid and refuses bad arguments; the lane bodies of the kernels, run on the host by gmmvi_data_tape_probe, meet the bound of
the GPU test against fp64 and agree with an fp32 NumPy restatement in the device's order; every planted fault, those of
tests/custom_data_cases.py and the three of tests/custom_data_tape_cases.py, exceeds that bound a hundred times on every case it
applies to; and DeviceDataTapeLNPDF checks its arguments before it touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import custom_data_cases as old
import custom_data_tape_cases as cases
from helpers import use_host_context
from test_hip_custom_target import _bound

ERR_ARG = -2
ALL_CASES = cases.kernel_cases()


def _plan(c, capacity=1 << 14, scratch=0):
    from gmmvi_amd import hip_ops
    return hip_ops.custom_data_tape_plan(c.n, c.rows if c.batch is None else c.batch, c.d, capacity, c.chunks, scratch)


# ---- the compiler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_case_sources_compile_for_gfx950(name):
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check_data_tape(cases.SOURCES[name], "gfx950")
    assert rc == 0, log


def test_compile_errors_name_the_users_line_and_the_missing_function():
    from gmmvi_amd import _lib, hip_ops
    lines = old.STUDENT_SRC.split("\n")
    bad_line = next(i for i, text in enumerate(lines) if "T r = row[D];" in text)
    lines[bad_line] = "    T r = row[D] - ;"
    rc, log = hip_ops.custom_target_check_data_tape("\n".join(lines), "gfx950")
    assert rc == ERR_ARG and f":{bad_line + 1}:" in log and "error" in log, log
    assert log.strip() in _lib.load().gmmvi_last_error(None).decode()
    head, tail = old.LOGIT_SRC.split("template <class T, class X>\n__device__ T gmmvi_user_prior")
    prior_only = "template <class T, class X>\n__device__ T gmmvi_user_prior" + tail
    rc, log = hip_ops.custom_target_check_data_tape(prior_only, "gfx950")
    assert rc == ERR_ARG and "does not define gmmvi_user_row" in log and "does not define gmmvi_user_prior" not in log, log
    rc, log = hip_ops.custom_target_check_data_tape(head, "gfx950")
    assert rc == ERR_ARG and "does not define gmmvi_user_prior" in log and "does not define gmmvi_user_row" not in log, log
    import custom_tape_cases as tape
    rc, log = hip_ops.custom_target_check_data_tape(tape.CHAIN_SRC, "gfx950")          # gmmvi_user_density only
    assert rc == ERR_ARG and "does not define gmmvi_user_row" in log and "does not define gmmvi_user_prior" in log, log
    lib = _lib.load()
    assert lib.gmmvi_custom_target_check_data_tape(None, b"gfx950", None, 0) == ERR_ARG
    assert lib.gmmvi_custom_target_check_data_tape(b"", None, None, 0) == ERR_ARG


def test_constants_and_symbols():
    from gmmvi_amd import _lib, hip_ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmmvi_hip.h")).read()
    for name in ("RECORD_BYTES", "DEFAULT_CAPACITY", "SCRATCH_BYTES"):
        assert int(re.search(rf"#define GMMVI_CUSTOM_TAPE_{name} (\d+)", header).group(1)) == getattr(_lib, "CUSTOM_TAPE_" + name)
    assert _lib.CUSTOM_TAPE_DEFAULT_CAPACITY == cases.DEFAULT_CAPACITY and _lib.CUSTOM_AUTODIFF_MAX_DIM == cases.OLD_CAP
    for symbol in ("gmmvi_custom_target_check_data_tape", "gmmvi_custom_target_compile_data_tape", "gmmvi_custom_data_tape_plan",
                   "gmmvi_target_custom_data_tape", "gmmvi_data_tape_probe"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
        assert re.search(rf"\bint {symbol}\(", header)
    assert "data_tape" in hip_ops.CUSTOM_TARGET_MODES and "reverse" not in hip_ops.CUSTOM_TARGET_MODES
    assert [f[0] for f in _lib.TargetSpec._fields_][-2:] == ["custom", "custom_params"]       # no new struct, no new target kind
    assert _lib.load().gmmvi_struct_bytes(4) == 0


# ---- the plan --------------------------------------------------------------------------------------------------------------
def _wave_bytes(d, capacity):
    from gmmvi_amd import _lib
    return 64 * (capacity * _lib.CUSTOM_TAPE_RECORD_BYTES + 4 * d)


def test_plan_properties():
    from gmmvi_amd import _lib, hip_ops
    default = _lib.CUSTOM_TAPE_SCRATCH_BYTES
    for n in (1, 64, 65, 130, 10 ** 4, 10 ** 6):
        tiles = (n + 63) // 64
        for rows in (1, 3, 7, 8, 9, 67, 257, 1000, 2 ** 31 - 1):
            for d, capacity in ((1, 1), (5, 16), (512, 1100), (4096, 9000), (_lib.MAX_DIM_DIAG, 1024)):
                wave = _wave_bytes(d, capacity)
                for request in (0, 1, 2, 3, 9, 10 ** 5):
                    for budget in (0, wave, 3 * wave, 7 * wave + 5, 1 << 28):
                        if (budget or default) < wave:
                            continue
                        what = (n, rows, d, capacity, request, budget)
                        chunks, per, slabs, each = hip_ops.custom_data_tape_plan(*what)
                        fit = (budget or default) // wave
                        assert chunks >= 1 and per >= 1 and slabs >= 1 and each >= 1, what
                        assert chunks * per >= rows and (chunks - 1) * per < rows, what        # the last chunk is not empty
                        assert slabs * each >= tiles and (slabs - 1) * each < tiles, what      # nor is the last slab
                        assert chunks * each * wave <= (budget or default), what               # one slab fits the budget
                        if request > 0:
                            most = min(request, rows, 65535, fit)
                            assert chunks <= most, what
                            if rows % most == 0:
                                assert chunks == most, what                                    # an exact split is honoured
                        else:
                            assert chunks == 1 or per >= 8, what                               # auto: 8 rows per wave or one chunk
                            assert tiles * chunks <= max(4 * 256 + tiles, tiles), what
    # the automatic plan fills the device when the rows allow it
    assert hip_ops.custom_data_tape_plan(64, 20000, 5, 16)[:2] == (1000, 20)     # 1024 asked for, then evened out
    assert hip_ops.custom_data_tape_plan(10 ** 4, 1000, 32, 128)[0] == 7


def test_plan_exact_values_and_refusals():
    from gmmvi_amd import _lib, hip_ops
    c = cases.SLAB_CASE
    one_tile = _wave_bytes(c.d, 16)
    assert hip_ops.custom_data_tape_plan(c.n, c.rows, c.d, 16, 0, one_tile) == (1, 5, 3, 1)     # slabs = 3
    assert hip_ops.custom_data_tape_plan(c.n, c.rows, c.d, 16, 0, 0) == (1, 5, 1, 3)
    assert hip_ops.custom_data_tape_plan(65, 67, 17, 64, 2) == (2, 34, 1, 2)
    assert hip_ops.custom_data_tape_plan(65, 67, 17, 64, 3) == (3, 23, 1, 2)
    assert hip_ops.custom_data_tape_plan(65, 3, 3, 64, 9) == (3, 1, 1, 2)                       # clamped to one row per chunk
    assert hip_ops.custom_data_tape_plan(65, 67, 17, 64, 3, 2 * _wave_bytes(17, 64)) == (2, 34, 2, 1)   # and to what fits
    assert hip_ops.custom_data_tape_plan(65, 257, 5, 64)[0] > 1                                 # the automatic 257-row case
    assert all(_plan(k)[0] > 1 for k in ALL_CASES if k.rows == 257 and k.batch is None and k.chunks == 0)
    lib = _lib.load()
    o = [C.c_int() for _ in range(4)]
    refs = [C.byref(v) for v in o]
    for n, rows, d, cap, request in ((0, 5, 5, 16, 0), (5, 0, 5, 16, 0), (5, 2 ** 31, 5, 16, 0), (5, 5, 0, 16, 0),
                                     (5, 5, _lib.MAX_DIM_DIAG + 1, 16, 0), (5, 5, 5, 0, 0), (5, 5, 5, 16, -1)):
        assert lib.gmmvi_custom_data_tape_plan(n, rows, d, cap, request, 0, *refs) == ERR_ARG, (n, rows, d, cap, request)
    for missing in range(4):
        args = [None if i == missing else refs[i] for i in range(4)]
        assert lib.gmmvi_custom_data_tape_plan(5, 5, 5, 16, 0, 0, *args) == ERR_ARG
    # a budget below one tile with one chunk: both byte counts
    assert lib.gmmvi_custom_data_tape_plan(5, 5, 5, 16, 0, one_tile - 1, *refs) == ERR_ARG
    message = lib.gmmvi_last_error(None).decode()
    assert str(one_tile) in message and str(one_tile - 1) in message, message
    assert lib.gmmvi_custom_data_tape_plan(5, 5, 5, 16, 0, one_tile, *refs) == 0


# ---- the lane bodies on the host ----------------------------------------------------------------------------------------------
def _probe(tgt, x, plan, capacity):
    from gmmvi_amd import _lib
    lib = _lib.load()
    n, d = x.shape
    x = np.ascontiguousarray(x, np.float32)
    data, params = np.ascontiguousarray(tgt.data), tgt.params()
    lp, grad = np.full(n, np.nan, np.float32), np.full((n, d), np.nan, np.float32)
    needed = C.c_int(-1)
    mini = tgt.batch_size is not None
    rc = lib.gmmvi_data_tape_probe(d, params.ctypes.data, data.ctypes.data, data.shape[0], data.shape[1], int(mini),
                                   tgt.batch_size if mini else data.shape[0], tgt.seed, tgt.call_count, x.ctypes.data, n, plan[0],
                                   plan[1], capacity, lp.ctypes.data, grad.ctypes.data, C.byref(needed))
    return rc, lp, grad, needed.value


# the probe's row term and prior are the logit text: tile seam (N = 65 needs none on the host, kept for the lane loop), chunk
# seams with a ragged last chunk, a minibatch in two chunks, the old cap from above
PROBE_CASES = [(cases.Case("logit", 5, 65, 5, 0, None, 0), (1, 5)), (cases.Case("logit", 17, 65, 67, 2, None, 0), (2, 34)),
               (cases.Case("logit", 17, 65, 67, 3, None, 0), (3, 23)), (cases.Case("logit", 5, 65, 257, 0, 5, 3), (2, 3)),
               (cases.Case("logit", 5, 65, 9, 0, 9, 0), (9, 1)), (cases.Case("logit", 513, 65, 5, 0, None, 0), (1, 5))]


@pytest.mark.parametrize("c,plan", PROBE_CASES, ids=[cases.case_id(c) for c, _ in PROBE_CASES])
def test_probe_against_fp64_and_in_device_order(c, plan):
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    row_records, prior_records = 2 * c.d + 8, 4 * c.d + 2            # logit: a product and a sum per coordinate and the tail;
                                                                     # the prior: -, /, *, + per coordinate, then * and -
    rc, lp, g, needed = _probe(tgt, x, plan, 4 * c.d + 64)
    assert rc == 0
    e_lp, b_lp, r_lp = _bound(lp, lp64, lp32)
    e_g, b_g, r_g = _bound(g, g64, g32)
    order_lp, order_g = cases.evaluate_in_tape_order(cases.fp32_twin(tgt), x, plan)
    d_lp, d_g = float(np.abs(lp.astype(np.float64) - order_lp).max()), float(np.abs(g.astype(np.float64) - order_g).max())
    print(f"\n[custom_data_tape] probe {cases.case_id(c)} plan {plan}: needed {needed}; lp error {e_lp:.3e} ({e_lp / b_lp:.3f} of the "
          f"bound, ratio {r_lp:.2f}), gradient error {e_g:.3e} ({e_g / b_g:.3f}, ratio {r_g:.2f}); against fp32 NumPy in the same "
          f"order: lp {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), gradient {d_g:.3e} ({d_g / b_g:.3f})")
    assert e_lp <= b_lp and e_g <= b_g
    # the same operations in the same order, rounded by two math libraries: a small part of what the bound allows
    assert d_lp <= 0.25 * b_lp and d_g <= 0.25 * b_g
    assert 2 * c.d <= needed == max(row_records, prior_records)
    # exactly the needed capacity gives the same bits; one record less reports the length and claims no gradient
    rc, lp_e, g_e, needed_e = _probe(tgt, x, plan, needed)
    assert rc == 0 and needed_e == needed
    np.testing.assert_array_equal(lp_e.view(np.uint32), lp.view(np.uint32))
    np.testing.assert_array_equal(g_e.view(np.uint32), g.view(np.uint32))
    rc, lp_s, g_s, needed_s = _probe(tgt, x, plan, needed - 1)
    assert rc == 0 and needed_s == needed
    np.testing.assert_array_equal(lp_s.view(np.uint32), lp.view(np.uint32))
    assert np.all(np.isnan(g_s))


def test_probe_refuses_bad_arguments():
    c = cases.Case("logit", 5, 3, 9, 0, None, 0)
    tgt, x = cases.build_case(c)
    assert _probe(tgt, x, (1, 9), 64)[0] == 0
    for plan in ((1, 8), (2, 9), (0, 9), (3, 0)):                    # rows uncovered, an empty last chunk, nothing
        assert _probe(tgt, x, plan, 64)[0] == ERR_ARG, plan
    assert _probe(tgt, x, (1, 9), 0)[0] == ERR_ARG
    mini = cases.build_case(cases.Case("logit", 5, 3, 9, 0, 4, 0))[0]
    assert _probe(mini, x, (2, 4), 64)[0] == ERR_ARG and _probe(mini, x, (1, 4), 64)[0] == 0 and _probe(mini, x, (2, 2), 64)[0] == 0


# ---- the restatements and the faults ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 4])
def test_ragged_restatement_agrees_with_central_differences(batch):
    c = cases.Case("ragged", 6, 5, 13, 0, batch, 2)
    tgt, x = cases.build_case(c)
    x = x.astype(np.float64)
    lp, g = tgt.evaluate(x)
    h = 1e-6
    for i in range(c.d):
        e = np.zeros(c.d); e[i] = h
        fd = (tgt.evaluate(x + e)[0] - tgt.evaluate(x - e)[0]) / (2 * h)
        np.testing.assert_allclose(g[:, i], fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"coordinate {i}")
    # every repeat count and both signs of the residual occur, in every tile of the kernel case
    tgt, x = cases.build_case(cases.Case("ragged", 6, 65, 13, 1, None, 0))
    assert set(tgt.data[:, -1].astype(int)) == {0, 1, 2, 3}
    r = tgt.data[:, -2][None, :] - x.astype(np.float64) @ tgt.data[:, :-2].T.astype(np.float64)
    assert (r[:64] > 0).any() and (r[:64] < 0).any() and (r[64:] > 0).any() and (r[64:] < 0).any()


def test_kernel_cases_sit_on_the_seams():
    from gmmvi_amd import _lib
    full = [c for c in ALL_CASES if c.batch is None]
    mini = [c for c in ALL_CASES if c.batch is not None]
    assert {1, 63, 64, 65, 130} <= {c.n for c in full}
    assert {1, 2, 512, 513, 1100, 4096} <= {c.d for c in full if c.name == "logit"}
    assert 2 * 4096 > _lib.CUSTOM_TAPE_DEFAULT_CAPACITY >= 2 * 1100 // 3
    assert {1, 2, 3} <= {c.rows for c in full if c.name == "student"}
    assert {("logit", 2), ("logit", 3), ("student", 2), ("student", 3)} <= {(c.name, c.chunks) for c in full if c.rows == 67}
    assert any(c.chunks > c.rows for c in full)
    assert {"logit", "student", "nodata", "ragged"} <= {c.name for c in full}
    for t in (9, 257, 1025):
        assert {(1, 0), (1, 3), (5, 0), (5, 3), (t, 0), (t, 3)} <= {(c.batch, c.call) for c in mini if c.rows == t}
    assert any(c.d == 513 and c.batch == 257 and c.chunks == 2 and c.call == 3 for c in mini)
    assert len(set(ALL_CASES)) == len(ALL_CASES)


def _exemptions(c, plan):
    """fault -> why case ``c`` cannot show it."""
    length = c.rows if c.batch is None else c.batch
    out = {}
    if length < 2:
        out["drop_last_row"] = "the only row: dropping it leaves an empty sum"
        out["drop_first_row_of_wave_1"] = "one row: there is no second one"
        out["row_gradient_kept"] = "one row: no previous row"
    if plan[0] < 2:
        out["drop_first_row_of_last_chunk"] = "one chunk: no chunk seam"
    if c.batch is None or c.batch == c.rows:
        out["unit_scale"] = "s is 1"
        out["scaled_prior"] = "s is 1"
        out["next_call"] = "full data has no stream; at B = T every call permutes the same rows"
    if c.name == "nodata":
        out["row_gradient_kept"] = "the row term has no gradient"
    return out


@pytest.mark.parametrize("c", ALL_CASES, ids=cases.case_id)
def test_planted_faults_exceed_a_hundred_times_the_gpu_bound(c):
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    chunks, per = _plan(c)[:2]
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    # the device's own summation order in fp32 stays far inside the bound: what the factor is measured against
    dlp, dg = cases.evaluate_in_tape_order(cases.fp32_twin(tgt), x, (chunks, per))
    e_lp, e_g = _bound(dlp, lp64, lp32)[0], _bound(dg, g64, g32)[0]
    print(f"\n[custom_data_tape] {cases.case_id(c)} plan {(chunks, per)}: device-order fp32 NumPy error {e_lp / b_lp:.3f} (lp), "
          f"{e_g / b_g:.3f} (gradient) of the bound")
    assert e_lp <= 0.5 * b_lp and e_g <= 0.5 * b_g
    exempt = _exemptions(c, (chunks, per))
    x64 = x.astype(np.float64)
    for fault in old.FAULTS + cases.TAPE_FAULTS:
        if fault in exempt:
            print(f"[custom_data_tape] {cases.case_id(c)}: {fault} exempt ({exempt[fault]})")
            continue
        if fault in old.FAULTS:
            flp, fg = tgt.evaluate(x64, fault=fault, plan=(chunks, per))
        else:
            flp, fg = cases.evaluate_with_tape_fault(tgt, x64, fault)
        r_lp, r_g = float(np.abs(flp - lp64).max()) / b_lp, float(np.abs(fg - g64).max()) / b_g
        print(f"[custom_data_tape] {cases.case_id(c)}: {fault} moves lp by {r_lp:.3g} and the gradient by {r_g:.3g} times the bound")
        assert max(r_lp, r_g) >= 100.0, f"{fault}: lp moves by {r_lp:.3g}, the gradient by {r_g:.3g} times the bound"


def test_every_fault_is_shown_by_many_cases():
    shown = {f: 0 for f in old.FAULTS + cases.TAPE_FAULTS}
    for c in ALL_CASES:
        ex = _exemptions(c, _plan(c)[:2])
        for f in shown:
            shown[f] += f not in ex
    assert all(v >= 6 for v in shown.values()), shown


# ---- the class -------------------------------------------------------------------------------------------------------------
def test_device_data_tape_lnpdf_arguments(monkeypatch):
    from gmmvi_amd import _lib
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    use_host_context(monkeypatch, device_lnpdf)
    compiled = []
    monkeypatch.setattr(device_lnpdf.hip_ops, "custom_target_compile", lambda ctx, source, **kw: compiled.append(kw) or object())
    data = np.zeros((9, 6), np.float32)
    make = device_lnpdf.DeviceDataTapeLNPDF
    for bad in (0, -3, 2.5, _lib.MAX_DIM_DIAG + 1):
        with pytest.raises(ValueError, match="num_dimensions"):
            make(old.LOGIT_SRC, bad, data, params=[0.0, 1.0])
    for bad_data in (np.zeros(9), np.zeros((3, 3, 3)), np.zeros((0, 6)), np.zeros((9, 0))):
        with pytest.raises(ValueError, match="two-dimensional"):
            make(old.LOGIT_SRC, 5, bad_data)
    for bad_batch in (0, 10, -1, 2.5):
        with pytest.raises(ValueError, match="batch_size"):
            make(old.LOGIT_SRC, 5, data, batch_size=bad_batch)
    with pytest.raises(ValueError, match="one-dimensional"):
        make(old.LOGIT_SRC, 5, data, params=np.ones((2, 2)))
    for name in ("tape_capacity", "scratch_bytes"):
        for bad in (0, -1, 2.5):
            with pytest.raises(ValueError, match=name):
                make(old.LOGIT_SRC, 5, data, **{name: bad})
    assert compiled == []
    for d in (513, _lib.MAX_DIM_DIAG):
        t = make(old.LOGIT_SRC, d, data, params=[0.0, 1.0], batch_size=4, seed=3, tape_capacity=100, scratch_bytes=1 << 20)
        assert t.get_num_dimensions() == d and (t.tape_capacity, t.scratch_bytes, t.batch_size, t.seed) == (100, 1 << 20, 4, 3)
        with pytest.raises(ValueError, match="512"):
            device_lnpdf.DeviceDataLNPDF(old.LOGIT_SRC, d, data)
    assert compiled == [{"mode": "data_tape"}] * 2


def test_class_facts():
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF, DeviceDataTapeLNPDF, DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi_amd.experiments.target_distributions.minibatch_stream import MinibatchLNPDF
    from gmmvi.experiments.target_distributions.device_lnpdf import DeviceDataTapeLNPDF as Alias
    assert Alias is DeviceDataTapeLNPDF
    assert issubclass(DeviceDataTapeLNPDF, MinibatchLNPDF) and not issubclass(DeviceDataTapeLNPDF, (DeviceLNPDF, DeviceDataLNPDF))
    assert DeviceDataTapeLNPDF.gradient_on_demand is True
    assert DeviceDataTapeLNPDF.log_density_and_grad is not LNPDF.log_density_and_grad
    assert not hasattr(DeviceDataTapeLNPDF, "_fast_path_target") and hasattr(DeviceDataTapeLNPDF, "log_density_full")
