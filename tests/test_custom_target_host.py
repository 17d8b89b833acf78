"""User-defined device targets, the part that needs no GPU: the run-time compiler builds source + wrapper kernels for gfx950
without a device (gmmvi_custom_target_check), compile errors come back as argument errors with the compiler log, and the
Python class rejects bad arguments before it touches the device."""
import numpy as np
import pytest

import custom_target_cases as cases
from helpers import use_host_context

ERR_ARG = -2


@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_case_sources_compile_for_gfx950(name):
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check(cases.SOURCES[name], "gfx950")
    assert rc == 0, log


def test_syntax_error_is_an_argument_error_with_the_offending_line():
    from gmmvi_amd import _lib, hip_ops
    lines = cases.ROSENBROCK_SRC.split("\n")
    bad_line = next(i for i, text in enumerate(lines) if "const float u" in text)
    lines[bad_line] = "    const float u = a - ;"
    rc, log = hip_ops.custom_target_check("\n".join(lines), "gfx950")
    assert rc == ERR_ARG
    assert log.strip()
    assert f":{bad_line + 1}:" in log, log                     # clang's file:line:column of the user's own text
    assert "error" in log
    assert log.strip() in _lib.load().gmmvi_last_error(None).decode()


def test_source_without_the_function_names_it():
    from gmmvi_amd import hip_ops
    rc, log = hip_ops.custom_target_check("__device__ float something_else(const float* x) { return x[0]; }\n", "gfx950")
    assert rc == ERR_ARG
    assert "gmmvi_user_target" in log


def test_null_arguments_are_argument_errors():
    from gmmvi_amd import _lib
    lib = _lib.load()
    assert lib.gmmvi_custom_target_check(None, b"gfx950", None, 0) == ERR_ARG
    assert lib.gmmvi_custom_target_check(b"", None, None, 0) == ERR_ARG
    # the log is cut to the caller's buffer and stays a C string
    import ctypes as C
    buf = C.create_string_buffer(b"\xff" * 16, 16)
    assert lib.gmmvi_custom_target_check(b"nonsense", b"gfx950", buf, 16) == ERR_ARG
    assert len(buf.value) == 15


def test_more_estimator_reads_no_target_gradients():
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import DiagonalMoreNgEstimator, MoreNgEstimator, SteinNgEstimator
    assert MoreNgEstimator.uses_target_gradients is False
    assert DiagonalMoreNgEstimator.uses_target_gradients is False
    assert SteinNgEstimator.uses_target_gradients is True


def test_struct_mirror_has_the_custom_members():
    from gmmvi_amd import _lib
    names = [f[0] for f in _lib.TargetSpec._fields_]
    assert names[-2:] == ["custom", "custom_params"]
    assert _lib.CUSTOM_STAGED_MAX_DIM == 120
    for symbol in ("gmmvi_custom_target_check", "gmmvi_custom_target_compile", "gmmvi_custom_target_release",
                   "gmmvi_target_custom"):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1


def test_device_lnpdf_argument_errors(monkeypatch):
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    use_host_context(monkeypatch, device_lnpdf)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="num_dimensions"):
            device_lnpdf.DeviceLNPDF(cases.ROSENBROCK_SRC, bad, params=[1.0, 100.0])
    with pytest.raises(ValueError, match="one-dimensional"):
        device_lnpdf.DeviceLNPDF(cases.ROSENBROCK_SRC, 2, params=np.ones((2, 2)))
    with pytest.raises(ValueError, match="one-dimensional"):
        device_lnpdf.DeviceLNPDF(cases.ROSENBROCK_SRC, 2, params=np.ones((2, 2)), has_gradient=False)


def test_values_only_object_leaves_the_gradient_call_alone():
    """has_gradient decides the CLASS: SampleSelector.get_target_grads looks at type(target).log_density_and_grad."""
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.lnpdf import LNPDF
    from gmmvi.experiments.target_distributions.device_lnpdf import DeviceLNPDF as Alias
    assert Alias is DeviceLNPDF
    assert DeviceLNPDF.log_density_and_grad is LNPDF.log_density_and_grad
    assert not hasattr(DeviceLNPDF, "_fast_path_target")
    with_grad = DeviceLNPDF.__new__(DeviceLNPDF, "", 2)
    values_only = DeviceLNPDF.__new__(DeviceLNPDF, "", 2, has_gradient=False)
    assert isinstance(with_grad, DeviceLNPDF) and type(values_only) is DeviceLNPDF
    assert type(with_grad).log_density_and_grad is not LNPDF.log_density_and_grad
    assert hasattr(with_grad, "_fast_path_target")


def test_restatements_agree_with_finite_differences():
    """The fp64 restatements are the references of the GPU tests: their gradients against central differences."""
    for name, d in (("rosenbrock", 2), ("quartic", 5), ("planar", 10)):
        tgt, x = cases.build_case(name, d, 7)
        x = x.astype(np.float64)
        _, g = tgt.log_density_and_grad(x)
        h = 1e-6
        for i in range(d):
            e = np.zeros(d); e[i] = h
            fd = (tgt.log_density(x + e) - tgt.log_density(x - e)) / (2 * h)
            np.testing.assert_allclose(g[:, i], fd, rtol=2e-5, atol=2e-5 * np.abs(g).max(), err_msg=f"{name} coordinate {i}")
