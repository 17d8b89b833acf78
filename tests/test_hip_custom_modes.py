"""GPU test of the five compile modes of user-defined device targets against the eight entries that take a handle: every entry
launches the handles of the modes listed for it below and refuses every other one before any launch, with GMMVI_ERR_ARG, a
message that names the compile entry the handle came from and an entry that does launch it, the outputs bit-unchanged and nothing
in the profile report.  The pattern is written out here, not read from the library.  Shapes: D = 2, N = 2 samples, T = 3 rows,
minibatches of B = 2."""
import ctypes as C
import re

import numpy as np
import pytest

import custom_autodiff_cases
import custom_data_cases
import custom_data_tape_cases
import custom_tape_cases
import custom_target_cases
from test_hip_custom_target import SENTINEL

pytestmark = pytest.mark.gpu

ERR_ARG = -2
D, N, T, B = 2, 2, 3, 2
COLS = D + 1                                                         # a logit row: D features and the label

# mode -> (the compile entry of the mode, a source for it)
MODES = {"hand": ("gmmvi_custom_target_compile", custom_target_cases.SOURCES["rosenbrock"]),
         "autodiff": ("gmmvi_custom_target_compile_autodiff", custom_autodiff_cases.SOURCES["rosenbrock"]),
         "data": ("gmmvi_custom_target_compile_data", custom_data_cases.SOURCES["logit"]),
         "tape": ("gmmvi_custom_target_compile_tape", custom_tape_cases.SOURCES["rosenbrock"]),
         "data_tape": ("gmmvi_custom_target_compile_data_tape", custom_data_tape_cases.SOURCES["logit"])}
# entry -> the modes whose handles it takes
ACCEPTS = {"gmmvi_target_custom": ("hand", "autodiff"),
           "gmmvi_target_custom_data": ("data",),
           "gmmvi_target_custom_data_own_batches": ("data",),
           "gmmvi_target_custom_tape": ("tape",),
           "gmmvi_target_custom_data_tape": ("data_tape",),
           "gmmvi_target_custom_data_tape_own_batches": ("data_tape",),
           "gmmvi_custom_data_predictive": ("data", "data_tape"),
           "gmmvi_custom_tape_length": ("hand", "autodiff", "data", "tape", "data_tape")}
# mode -> the entries that launch its handles (gmmvi_custom_tape_length launches nothing)
LAUNCHERS = {mode: [entry for entry, modes in ACCEPTS.items() if mode in modes and entry != "gmmvi_custom_tape_length"] for mode in MODES}


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


@pytest.fixture(scope="module")
def handles(ctx):
    """One handle per mode, released (with the CustomTarget objects) when the module is done."""
    from gmmvi_amd import hip_ops
    compiled = {mode: hip_ops.custom_target_compile(ctx, source, mode=mode) for mode, (_, source) in MODES.items()}
    yield compiled
    compiled.clear()


@pytest.fixture(scope="module")
def inputs(ctx):
    """x [N, D], params (a, b of rosenbrock; mean, scale of the logit prior) and rows [T, COLS] on the device."""
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.normal(size=(T, D)), rng.choice([-1.0, 1.0], size=(T, 1))], axis=1).astype(np.float32)
    return ctx.asarray(rng.normal(size=(N, D)).astype(np.float32)), ctx.asarray(np.array([1.0, 2.0], np.float32)), ctx.asarray(rows)


def _call(ctx, entry, handle, inputs, lp, grad, pred, length):
    x, params, rows = inputs
    lib, h = ctx.lib, handle.handle
    if entry == "gmmvi_target_custom":
        return lib.gmmvi_target_custom(ctx.handle, h, D, params.ptr, x.ptr, N, lp.ptr, grad.ptr, 0)
    if entry == "gmmvi_target_custom_data":
        return lib.gmmvi_target_custom_data(ctx.handle, h, D, params.ptr, rows.ptr, T, COLS, 1, B, 7, 0, x.ptr, N, lp.ptr, grad.ptr, 0)
    if entry == "gmmvi_target_custom_data_own_batches":
        return lib.gmmvi_target_custom_data_own_batches(ctx.handle, h, D, params.ptr, rows.ptr, T, COLS, B, 7, 0, x.ptr, N, lp.ptr,
                                                        grad.ptr, 0)
    if entry == "gmmvi_target_custom_tape":
        return lib.gmmvi_target_custom_tape(ctx.handle, h, D, params.ptr, x.ptr, N, lp.ptr, grad.ptr, 0, 0)
    if entry == "gmmvi_target_custom_data_tape":
        return lib.gmmvi_target_custom_data_tape(ctx.handle, h, D, params.ptr, rows.ptr, T, COLS, 1, B, 7, 0, x.ptr, N, lp.ptr,
                                                 grad.ptr, 0, 0, 0)
    if entry == "gmmvi_target_custom_data_tape_own_batches":
        return lib.gmmvi_target_custom_data_tape_own_batches(ctx.handle, h, D, params.ptr, rows.ptr, T, COLS, B, 7, 0, x.ptr, N,
                                                             lp.ptr, grad.ptr, 0, 0, 0)
    if entry == "gmmvi_custom_data_predictive":
        return lib.gmmvi_custom_data_predictive(ctx.handle, h, D, params.ptr, rows.ptr, T, COLS, x.ptr, N, pred[0].ptr, pred[1].ptr,
                                                pred[2].ptr, 0)
    assert entry == "gmmvi_custom_tape_length"
    return lib.gmmvi_custom_tape_length(ctx.handle, h, D, C.byref(length))


@pytest.mark.parametrize("entry", list(ACCEPTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_entry_takes_or_refuses_the_handle(ctx, handles, inputs, mode, entry):
    lib = ctx.lib
    handle = handles[mode]
    lp, grad = ctx.full((N,), SENTINEL), ctx.full((N, D), SENTINEL)
    pred = [ctx.full((T,), SENTINEL) for _ in range(3)]
    length = C.c_int(-1)
    ctx.check(lib.gmmvi_profile_enable(ctx.handle, 1))
    try:
        rc = _call(ctx, entry, handle, inputs, lp, grad, pred, length)
        message = lib.gmmvi_last_error(ctx.handle).decode()
    finally:
        report = C.create_string_buffer(1 << 16)
        ctx.check(lib.gmmvi_profile_report(ctx.handle, report, len(report)))
        ctx.check(lib.gmmvi_profile_enable(ctx.handle, 0))
    ctx.check(lib.gmmvi_sync(ctx.handle))
    out = [a.numpy() for a in (lp, grad, *pred)]
    if mode in ACCEPTS[entry]:
        assert rc == 0, message
        if entry == "gmmvi_custom_tape_length":
            assert length.value >= 0 and report.value == b""
            written = []
        else:
            assert report.value != b""
            written = out[2:] if entry == "gmmvi_custom_data_predictive" else out[:2]
        for a in written:
            assert np.all(np.isfinite(a)) and not np.any(a == SENTINEL)
    else:
        assert rc == ERR_ARG
        assert re.search(rf"\b{MODES[mode][0]}\b", message), message
        assert any(re.search(rf"\b{name}\b", message) for name in LAUNCHERS[mode]), message
        assert report.value == b"", report.value
        written = []
    bits = np.array(SENTINEL).view(np.uint32)
    for a in out:
        if not any(a is w for w in written):
            assert np.all(a.view(np.uint32) == bits)
