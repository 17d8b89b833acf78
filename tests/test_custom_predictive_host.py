"""Predictive density of data-set device targets, the part that needs no GPU: the four sources compile for gfx950 in both data
modes (which now carry the predictive kernels), the fp64 reference is the textbook one-liner, every planted fault of
tests/custom_predictive_cases.py exceeds ten times the bound of the GPU test (tests/test_hip_custom_predictive.py) on the
references alone while the fp32 twin stays inside it, the host probe (the device's own tile reduction and tile merge, compiled
for the host) meets the bound and the edge-value rules of include/gmmvi_hip.h, the plan function does what the header says, the
classes refuse bad arguments before they touch the device, and the ABI has grown by three plain functions and nothing else.

Bound: _bound of tests/test_hip_custom_target.py, unchanged: 16 times the fp32 twin's error plus 4 eps32 max|reference|, per
output over the entries whose reference is finite; entries with a non-finite reference are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import custom_predictive_cases as cases
from helpers import use_host_context
from test_hip_custom_target import _bound

ERR_ARG = -2
OUTPUTS = ("lpd", "mean", "var")


# ---- the compiler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["data", "data_tape"])
@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_case_sources_compile_with_the_predictive_kernels(name, mode):
    from gmmvi_amd import hip_ops
    check = hip_ops.custom_target_check_data if mode == "data" else hip_ops.custom_target_check_data_tape
    rc, log = check(cases.SOURCES[name], "gfx950")
    assert rc == 0, log


def test_abi_pins():
    from gmmvi_amd import _lib, hip_ops
    for symbol in ("gmmvi_custom_data_predictive_plan", "gmmvi_custom_data_predictive", "gmmvi_custom_data_predictive_probe"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
        assert hasattr(_lib.load(), symbol)
    assert [f[0] for f in _lib.TargetSpec._fields_][-2:] == ["custom", "custom_params"]
    assert _lib.load().gmmvi_struct_bytes(4) == 0
    for name in ("custom_data_predictive_plan", "custom_data_predictive", "custom_data_predictive_probe"):
        assert callable(getattr(hip_ops, name))


# ---- the references --------------------------------------------------------------------------------------------------------
def test_reference_is_the_textbook_one_liner():
    from scipy.special import logsumexp
    tag, tgt, x = cases.fault_cases()[1]
    l64 = cases.reference(tag, tgt, x)[0]
    lpd, mean, var = cases.reference64(l64)
    np.testing.assert_allclose(lpd, logsumexp(l64, axis=0) - np.log(l64.shape[0]), rtol=1e-13, atol=0)
    np.testing.assert_allclose(mean, l64.mean(axis=0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(var, np.var(l64, axis=0, ddof=1), rtol=1e-12, atol=0)
    one = cases.reference64(l64[:1])
    np.testing.assert_array_equal(one[0], l64[0])
    np.testing.assert_array_equal(one[2], np.zeros(l64.shape[1]))


def test_twin_stays_inside_the_bound_and_every_fault_leaves_ten_times_the_bound():
    """On the four cases of the table: the twin itself is inside the bound on every output; each fault of FAULTS exceeds ten
    times the bound on at least one output of at least one case.  A fault added to FAULTS that no case catches fails here."""
    caught = {fault: [] for fault in cases.FAULTS}
    for tag, tgt, x in cases.fault_cases():
        l64, l32, ref, twin = cases.reference(tag, tgt, x)
        for k, name in enumerate(OUTPUTS):
            e, b, _, exact = cases.compare(_bound, twin[k], ref[k], twin[k])
            assert exact and cases.within(e, b), (tag, name, e, b)
        for fault in cases.FAULTS:
            bad = cases.twin32(l32, fault)
            for k, name in enumerate(OUTPUTS):
                e, b, _, _ = cases.compare(_bound, bad[k], ref[k], twin[k])
                if not cases.within(e, 10.0 * b):
                    caught[fault].append((tag, name, e / b if np.isfinite(e) else float("inf")))
    for fault, hits in caught.items():
        print(f"[custom_predictive] {fault}: " + ", ".join(f"{t} {n} {r:.3g}x the bound" for t, n, r in hits))
    assert all(caught.values()), {f: h for f, h in caught.items() if not h}
    # what each case is there to show
    seen = {fault: {(t, n) for t, n, _ in hits} for fault, hits in caught.items()}
    for fault in ("drop_last_tile", "duplicate_tail", "no_log_n"):
        assert {("logit-N65", "lpd"), ("logit-N130", "lpd")} <= seen[fault], fault
    assert any(n == "var" and t.startswith("logit") for t, n in seen["biased_variance"])
    assert ("affine-30x-300", "lpd") in seen["no_shift"]
    assert ("affine-0.1x-1000", "var") in seen["naive_variance"]


# ---- the host probe: the device's own combine code ---------------------------------------------------------------------------
def _probe_check(tag, l32, ref, twin, chunks=0):
    from gmmvi_amd import hip_ops
    out = hip_ops.custom_data_predictive_probe(l32, chunks)
    for k, name in enumerate(OUTPUTS):
        e, b, r, exact = cases.compare(_bound, out[k], ref[k], twin[k])
        print(f"[custom_predictive] probe {tag}: {name} error {e:.3e} (bound {b:.3e}, ratio to the twin {r:.2f})")
        assert exact, (tag, name)
        assert cases.within(e, b), f"{tag}: {name} error {e:.3e} > {b:.3e}"
    return out


def test_probe_meets_the_bound_on_the_fault_cases():
    for tag, tgt, x in cases.fault_cases():
        l64, l32, ref, twin = cases.reference(tag, tgt, x)
        _probe_check(tag, l32, ref, twin)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_probe_meets_the_bound_at_the_tile_seams(n):
    tgt, x = cases.build_case(cases.Case("logit", 5, n, 5, 0))
    l64, l32, ref, twin = cases.reference(f"seam-N{n}", tgt, x)
    out = _probe_check(f"logit N = {n}", l32, ref, twin)
    if n == 1:
        np.testing.assert_array_equal(out[2], np.zeros(5, np.float32))
        np.testing.assert_array_equal(out[0], l32[0])
    for chunks in (1, 2, 5):                               # chunks split the rows, never a reduction
        again = _probe_check(f"logit N = {n}, {chunks} chunk(s)", l32, ref, twin, chunks)
        for a, b in zip(out, again):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("e", cases.edge_cases(65), ids=lambda e: e.name)
def test_probe_edge_values(e):
    from gmmvi_amd import hip_ops
    l64, l32 = cases.edge_matrix(e, np.float64), cases.edge_matrix(e, np.float32)
    ref, twin = cases.reference64(l64), cases.twin32(l32)
    out = hip_ops.custom_data_predictive_probe(l32)
    for m, want in enumerate(e.lpd):
        if want is None:
            assert np.isfinite(ref[0][m]) and np.isfinite(out[0][m])
        elif np.isnan(want):
            assert np.isnan(out[0][m]) and np.isnan(twin[0][m])
        else:
            assert out[0][m] == want and twin[0][m] == want and ref[0][m] == want
    err, b, r, exact = cases.compare(_bound, out[0], ref[0], twin[0])
    print(f"[custom_predictive] probe edge '{e.name}': lpd error {err:.3e} (bound {b:.3e})")
    assert exact and cases.within(err, b)
    ordinary = np.all(np.isfinite(l64), axis=0)            # mean and var are promised only for columns of finite values
    for k in (1, 2):
        err, b, _, _ = cases.compare(_bound, out[k][ordinary], ref[k][ordinary], twin[k][ordinary])
        assert cases.within(err, b) or not ordinary.any()


def test_probe_refusals():
    from gmmvi_amd import _lib
    lib = _lib.load()
    l = np.zeros((3, 2), np.float32)
    out = [np.zeros(2, np.float32) for _ in range(3)]
    ptr = [o.ctypes.data for o in out]
    assert lib.gmmvi_custom_data_predictive_probe(None, 3, 2, 0, *ptr) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_probe(l.ctypes.data, 3, 2, 0, None, ptr[1], ptr[2]) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_probe(l.ctypes.data, 0, 2, 0, *ptr) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_probe(l.ctypes.data, 3, 0, 0, *ptr) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_probe(l.ctypes.data, 3, 2, -1, *ptr) == ERR_ARG


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan():
    from gmmvi_amd import _lib, hip_ops
    for n in (1, 63, 64, 65, 130, 2000, 10 ** 6):
        for rows in (1, 3, 4, 5, 31, 32, 33, 67, 257, 1000, 2 ** 31 - 1):
            for request in (0, 1, 2, 3, 7, 10 ** 5):
                tiles, chunks, per = hip_ops.custom_data_predictive_plan(n, rows, request)
                assert tiles == -(-n // 64)
                assert (chunks, per) == hip_ops.custom_data_plan(n, rows, request)       # the chunk rules of the value call
                assert chunks >= 1 and per >= 1 and chunks * per >= rows and (chunks - 1) * per < rows
                if request > 0:
                    assert chunks <= min(request, rows, 65535)
    assert hip_ops.custom_data_predictive_plan(130, 67, 2) == (3, 2, 34)
    assert hip_ops.custom_data_predictive_plan(130, 67, 3) == (3, 3, 23)
    assert hip_ops.custom_data_predictive_plan(65, 5, 9) == (2, 5, 1)                   # forced up to one row per chunk
    assert hip_ops.custom_data_predictive_plan(65, 257)[1] > 1                           # the automatic plan has a chunk seam
    assert hip_ops.custom_data_predictive_plan(10 ** 4, 4) == (157, 1, 4)
    lib = _lib.load()
    a, b, c = C.c_int(), C.c_int(), C.c_int64()
    for n, rows, request in ((0, 5, 0), (5, 0, 0), (5, 2 ** 31, 0), (5, 5, -1)):
        assert lib.gmmvi_custom_data_predictive_plan(n, rows, request, C.byref(a), C.byref(b), C.byref(c)) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_plan(5, 5, 0, None, C.byref(b), C.byref(c)) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_plan(5, 5, 0, C.byref(a), None, C.byref(c)) == ERR_ARG
    assert lib.gmmvi_custom_data_predictive_plan(5, 5, 0, C.byref(a), C.byref(b), None) == ERR_ARG
    with pytest.raises(_lib.GmmviError):
        hip_ops.custom_data_predictive_plan(0, 5)


# ---- the classes -----------------------------------------------------------------------------------------------------------
class _NoDevice:
    """Stands where the context would: any use is a failure of 'before the device is touched'."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched: ctx.{name}")


@pytest.mark.parametrize("cls_name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_argument_errors_come_before_the_device(monkeypatch, cls_name):
    from gmmvi_amd import hip_ops
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    cls = getattr(device_lnpdf, cls_name)
    monkeypatch.setattr(device_lnpdf, "get_context", lambda: _NoDevice())
    data = np.zeros((9, 6), np.float32)
    src = cases.SOURCES["logit"]
    for bad in ([np.zeros((3, 6))], "test", np.zeros((3, 6))):
        with pytest.raises(ValueError, match="eval_sets"):
            cls(src, 5, data, eval_sets=bad)
    for bad in (np.zeros(6), np.zeros((2, 3, 6)), np.zeros((3, 5)), np.zeros((0, 6))):
        with pytest.raises(ValueError, match="eval_sets\\['test'\\]"):
            cls(src, 5, data, eval_sets={"test": bad})
    # an object that has everything log_predictive reads, and no device
    use_host_context(monkeypatch, device_lnpdf)
    monkeypatch.setattr(hip_ops, "custom_target_compile", lambda *a, **k: None)
    target = cls(src, 5, data, params=[0.0, 1.0], batch_size=4, eval_sets={"test": np.zeros((3, 6))}, report_waic=True)
    assert target.report_waic is True and set(target._eval_sets_dev) == {"test"}
    target.ctx = _NoDevice()
    x = np.zeros((4, 5), np.float32)
    for bad in (np.zeros(6), np.zeros((3, 5)), np.zeros((3, 7)), np.zeros((0, 6)), np.zeros((2, 3, 6))):
        with pytest.raises(ValueError, match="rows must be two-dimensional"):
            target.log_predictive(x, bad)
    assert target.call_count == 0
    plain = cls(src, 5, data)
    plain.ctx = _NoDevice()
    assert plain.expensive_metrics(None, x) == {}          # both keywords at their defaults: the base class's answer, no device


def test_class_facts():
    import inspect
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF, DeviceDataTapeLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    for cls in (DeviceDataLNPDF, DeviceDataTapeLNPDF):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-2:] == ["eval_sets", "report_waic"]
        assert cls.expensive_metrics is not LNPDF.expensive_metrics
        assert callable(cls.log_predictive) and callable(cls.waic)
    assert list(inspect.signature(DeviceDataLNPDF.__init__).parameters)[1:7] == ["source", "num_dimensions", "data", "params",
                                                                                 "batch_size", "seed"]
