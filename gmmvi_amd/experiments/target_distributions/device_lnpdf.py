"""User-defined target evaluated on the device (no upstream counterpart; upstream's custom targets are Python subclasses of
LNPDF, examples/4_gmmvi_runner_with_custom_environments.py).

The target is HIP source text that defines

    __device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad);

(contract: include/gmmvi_hip.h).  It is compiled at run time for the device of the context and evaluated by the
library's wrapper kernels (csrc/custom_target.hip): the samples never leave the device, and the single-call and the sharded
iteration take it as target kind 5.

``DeviceAutodiffLNPDF`` takes the log density alone,

    template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params);

and the library differentiates it in forward mode (csrc/custom_target_autodiff.inc): upstream's "write log_density, the framework
differentiates it" (SampleSelector.get_target_grads) on the device.

``DeviceTapeLNPDF`` takes the same density text and differentiates it in reverse mode on a tape (csrc/custom_target_tape.inc):
the cost of the gradient does not grow with the dimension, so it runs up to the largest diagonal-covariance dimension, on the
modular path.

``DeviceDataLNPDF`` takes one data row's log-likelihood and the prior,

    template <class T, class X> __device__ T gmmvi_user_row  (X x, int D, const float* row, int C, const float* params);
    template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params);

and the library spreads the rows over waves and workgroups, differentiates, sums in a fixed order and can draw a minibatch per
call (csrc/custom_target_data.inc): log p(x) = log prior(x) + sum_r log p(data_r | x) without a hand-written kernel file.

``DeviceDataTapeLNPDF`` takes the same two templates and differentiates them in reverse mode, one row at a time on a short tape
(csrc/custom_target_data_tape.inc): such posteriors up to the largest diagonal-covariance dimension.

In every one of these texts ``x`` also takes three vector primitives, which each mode differentiates in closed form
(csrc/custom_target_vector.inc; on the tape one record per call whatever ``n`` is, in forward mode no loop with tangents):

    gmmvi_dot(x, first, c, n)          sum over i < n of c[i] * x[first + i]
    gmmvi_sqdist(x, first, c, n)       sum over i < n of (x[first + i] - c[i])^2
    gmmvi_sumsq(x, first, n, center)   sum over i < n of (x[first + i] - center)^2

``c`` is a ``const float*`` that stays readable and unchanged until the kernel ends (``row``, ``params``, a static table; never an
array local to the function), ``0 <= first`` and ``first + n <= D`` are the caller's duty, ``n <= 0`` gives the constant 0.  A
logistic row is then ``T z = gmmvi_dot(x, 0, row, D) * row[D];`` and a normal prior ``-0.5f / (s * s) * gmmvi_sumsq(x, 0, D, m)``.
"""
import numpy as np

from ... import _lib, hip_ops
from ...device import get_context
from .lnpdf import LNPDF
from .minibatch_stream import MinibatchLNPDF


def _checked_dimension(num_dimensions):
    if int(num_dimensions) != num_dimensions or int(num_dimensions) < 1:
        raise ValueError(f"num_dimensions must be a positive integer, got {num_dimensions!r}")
    return int(num_dimensions)


def _host_params(params):
    """``params`` as a contiguous one-dimensional fp32 host array (None stays None), or ValueError; touches no device."""
    if params is not None:
        params = np.ascontiguousarray(np.asarray(params.numpy() if hasattr(params, "numpy") else params), np.float32)
        if params.ndim != 1:
            raise ValueError(f"params must be one-dimensional, got shape {params.shape}")
    return params


class _DeviceTarget:
    """What the classes of this module share; the tape options and the rule of the first gradient call: the two tape classes."""

    def get_num_dimensions(self):
        return self._num_dimensions

    def _x(self, x):
        x = self.ctx.asarray(x)
        if len(x.shape) != 2 or x.shape[1] != self._num_dimensions:
            raise ValueError(f"samples: expected [n, {self._num_dimensions}], got {x.shape}")
        return x

    def _set_tape_options(self, tape_capacity, scratch_bytes):
        for name, value in (("tape_capacity", tape_capacity), ("scratch_bytes", scratch_bytes)):
            if value is not None and (int(value) != value or int(value) < 1):
                raise ValueError(f"{name} must be a positive integer or None, got {value!r}")
        self.tape_capacity = 0 if tape_capacity is None else int(tape_capacity)
        self.scratch_bytes = 0 if scratch_bytes is None else int(scratch_bytes)

    def _tape_keywords(self, want_grad=True):
        # the asked-for capacity sizes the first gradient launch; afterwards the handle knows what the target needs
        first = want_grad and self.tape_capacity and hip_ops.custom_tape_length(self.ctx, self._handle, self._num_dimensions) == 0
        return {"tape_capacity": self.tape_capacity if first else 0, "scratch_bytes": self.scratch_bytes}


class DeviceLNPDF(_DeviceTarget, LNPDF):
    """``DeviceLNPDF(source, num_dimensions, params=None, has_gradient=True)``; pass it as ``config['target_fn']``.

    params: the target's own numbers (1-D, fp32 on the device; ``None``: the function gets a null pointer).
    has_gradient=False: the source ignores ``grad``.  The object then implements ``log_density`` only, exactly like a Python
    black-box target: it runs under the gradient-free estimators (MORE), and a first-order estimator raises the
    ``NotImplementedError`` of ``LNPDF.log_density_and_grad``."""

    def __new__(cls, source=None, num_dimensions=None, params=None, has_gradient=True):
        if cls is DeviceLNPDF and has_gradient:
            cls = _DeviceLNPDFWithGradient
        return object.__new__(cls)

    def __init__(self, source, num_dimensions, params=None, has_gradient=True):
        super().__init__(use_log_density_and_grad=True)
        if _checked_dimension(num_dimensions) > _lib.MAX_DIM_DIAG:
            raise ValueError(f"num_dimensions must be <= {_lib.MAX_DIM_DIAG}, got {num_dimensions}")
        params = _host_params(params)
        self.ctx = get_context()
        self.source = str(source)
        self.has_gradient = bool(has_gradient)
        self._num_dimensions = int(num_dimensions)
        self._params_dev = None if params is None or params.size == 0 else self.ctx.asarray(params)
        self._handle = self._compile()

    def _compile(self):
        return hip_ops.custom_target_compile(self.ctx, self.source)

    def log_density(self, x):
        return hip_ops.target_custom(self.ctx, self._handle, self._params_dev, self._x(x), want_grad=False)[0]


class _DeviceLNPDFWithGradient(DeviceLNPDF):
    """What ``DeviceLNPDF(..., has_gradient=True)`` constructs: the gradient call and the descriptor of the plans."""

    def log_density_and_grad(self, x):
        return hip_ops.target_custom(self.ctx, self._handle, self._params_dev, self._x(x), want_grad=True)

    def _fast_path_target(self):
        """Descriptor for the single-call and the sharded iteration (optimization/fused.py, sharded.py)."""
        return _lib.TargetSpec(kind=5, custom=self._handle.ptr,
                               custom_params=None if self._params_dev is None else self._params_dev.ptr)


class DeviceAutodiffLNPDF(_DeviceLNPDFWithGradient):
    """``DeviceAutodiffLNPDF(source, num_dimensions, params=None)``: ``source`` defines ``gmmvi_user_density``, the log density
    as a template over the number type (contract and the functions it may call: include/gmmvi_hip.h), and the gradient comes
    from the library's dual numbers, ``ceil(D / _lib.CUSTOM_AUTODIFF_TANGENTS)`` passes per sample.  Everything a
    ``DeviceLNPDF`` with a hand-written gradient does, this does: Stein and MORE estimators, target kind 5 in both plans."""

    # the gradient costs passes the value call does not: an estimator that reads no target gradients (MORE) gets values only
    # (SampleSelector.get_target_grads)
    gradient_on_demand = True

    def __init__(self, source, num_dimensions, params=None):
        try:
            too_large = int(num_dimensions) == num_dimensions and int(num_dimensions) > _lib.CUSTOM_AUTODIFF_MAX_DIM
        except (TypeError, ValueError):
            too_large = False
        if too_large:
            raise ValueError(f"num_dimensions must be <= {_lib.CUSTOM_AUTODIFF_MAX_DIM} for a differentiated target, got "
                             f"{num_dimensions}: the gradient costs ceil(D / {_lib.CUSTOM_AUTODIFF_TANGENTS}) passes per sample; "
                             "above that, write the gradient by hand and use DeviceLNPDF")
        super().__init__(source, num_dimensions, params, has_gradient=True)

    def _compile(self):
        return hip_ops.custom_target_compile(self.ctx, self.source, autodiff=True)


class DeviceTapeLNPDF(DeviceLNPDF):
    """``DeviceTapeLNPDF(source, num_dimensions, params=None, tape_capacity=None, scratch_bytes=None)``: ``source`` defines
    ``gmmvi_user_density``, the text a ``DeviceAutodiffLNPDF`` takes, and the gradient comes from reverse mode: every sample
    records its evaluation on a tape in device scratch and walks it back (csrc/custom_target_tape.inc), one recorded evaluation
    and one sweep whatever the dimension, up to ``_lib.MAX_DIM_DIAG``.

    tape_capacity: records per sample of the first gradient call (None: the library's default, then what the target has needed);
    scratch_bytes: the budget of the tape scratch (None: ``_lib.CUSTOM_TAPE_SCRATCH_BYTES``); more samples than fit are
    processed in slabs.  A gradient call reads the needed tape length back from the device and so waits for the stream: there is
    no ``_fast_path_target``, the iteration runs module by module."""

    # the gradient costs a tape the value call does not write: an estimator that reads no target gradients gets values only
    gradient_on_demand = True

    def __new__(cls, *args, **kwargs):
        return object.__new__(cls)

    def __init__(self, source, num_dimensions, params=None, tape_capacity=None, scratch_bytes=None):
        self._set_tape_options(tape_capacity, scratch_bytes)
        super().__init__(source, num_dimensions, params, has_gradient=True)

    def _compile(self):
        return hip_ops.custom_target_compile(self.ctx, self.source, mode="tape")

    def log_density(self, x):
        return hip_ops.target_custom_tape(self.ctx, self._handle, self._params_dev, self._x(x), want_grad=False)[0]

    def log_density_and_grad(self, x):
        return hip_ops.target_custom_tape(self.ctx, self._handle, self._params_dev, self._x(x), want_grad=True, **self._tape_keywords())


class _DeviceDataTarget(_DeviceTarget, MinibatchLNPDF):
    """What ``DeviceDataLNPDF`` and ``DeviceDataTapeLNPDF`` share: the argument checks, the upload, the call counter of
    ``MinibatchLNPDF`` and ``log_density_full``.  A subclass names its compile mode, checks the dimension and launches."""

    gradient_on_demand = True
    _mode = None

    def _check_dimension(self, num_dimensions):
        raise NotImplementedError

    def _target_call(self, x, want_grad, batch_size, call):
        raise NotImplementedError

    @staticmethod
    def _host_rows(rows, columns, name):
        """``rows`` as a contiguous fp32 host array [M >= 1, columns], or ValueError; touches no device."""
        rows = np.ascontiguousarray(np.asarray(rows.numpy() if hasattr(rows, "numpy") else rows), np.float32)
        if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] != columns:
            raise ValueError(f"{name} must be two-dimensional [rows >= 1, {columns}] (the columns of the training data), got shape "
                             f"{rows.shape}")
        return rows

    def __init__(self, source, num_dimensions, data, params=None, batch_size=None, seed=0, use_own_batch_per_sample=False,
                 eval_sets=None, report_waic=False):
        super().__init__(seed)
        if use_own_batch_per_sample and batch_size is None:
            raise ValueError("use_own_batch_per_sample needs a batch_size: without one every sample sees all rows")
        self._check_dimension(_checked_dimension(num_dimensions))
        data = np.ascontiguousarray(np.asarray(data.numpy() if hasattr(data, "numpy") else data), np.float32)
        if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError(f"data must be two-dimensional [rows >= 1, floats per row >= 1], got shape {data.shape}")
        if batch_size is not None and (int(batch_size) != batch_size or not 1 <= int(batch_size) <= data.shape[0]):
            raise ValueError(f"batch_size must be an integer in 1..{data.shape[0]} (the rows of data) or None, got {batch_size!r}")
        params = _host_params(params)
        if eval_sets is not None:
            if not isinstance(eval_sets, dict):
                raise ValueError(f"eval_sets must be a dict name -> [rows, {data.shape[1]}] array or None, got {type(eval_sets)}")
            eval_sets = {str(name): self._host_rows(rows, data.shape[1], f"eval_sets[{name!r}]") for name, rows in eval_sets.items()}
        self.ctx = get_context()
        self.source = str(source)
        self.report_waic = bool(report_waic)
        self._data_columns = int(data.shape[1])
        self._eval_sets_dev = {} if eval_sets is None else {name: self.ctx.asarray(rows) for name, rows in eval_sets.items()}
        self.batch_size = None if batch_size is None else int(batch_size)
        self.use_own_batch_per_sample = bool(use_own_batch_per_sample)
        self.num_data = int(data.shape[0])
        self._num_dimensions = int(num_dimensions)
        self._data_dev = self.ctx.asarray(data)
        self._params_dev = None if params is None or params.size == 0 else self.ctx.asarray(params)
        self._handle = hip_ops.custom_target_compile(self.ctx, self.source, mode=self._mode)

    def _batch_keywords(self, batch_size):
        """What a subclass adds to its ``hip_ops`` call for the row list: nothing for a shared batch or the full data."""
        return {"own_batches": True} if self.use_own_batch_per_sample and batch_size is not None else {}

    def _launch(self, x, call, want_grad):
        return self._target_call(self._x(x), want_grad, self.batch_size, call)

    def _evaluate(self, x, want_grad):
        if self.batch_size is None:                       # no stream, no counter
            return self._launch(self.ctx.asarray(x), 0, want_grad)
        return super()._evaluate(x, want_grad)

    def log_density_full(self, x):
        """The full-data log density (all rows in index order, s = 1) of a minibatch target; the call counter stays."""
        return self._target_call(self._x(x), False, None, 0)[0]

    def log_predictive(self, samples, rows=None):
        """Per row of ``rows`` [M, C] (None: the training data on the device) over the samples [N, D]: ``lpd`` = log (1/N) sum_n
        p(row | x_n), ``mean`` = the mean and ``var`` = the unbiased variance over the samples of log p(row | x_n); the prior
        takes no part (csrc/custom_target_data.inc, one reduction over the samples on the device).  -> (lpd, mean, var), device
        arrays of length M.  The call counter of a minibatch target stays."""
        if rows is not None:
            rows = self._host_rows(rows, self._data_columns, "rows")
        x = self._x(samples)
        if x.shape[0] < 1:
            raise ValueError("log_predictive needs at least one sample")
        rows_dev = self._data_dev if rows is None else self.ctx.asarray(rows)
        return hip_ops.custom_data_predictive(self.ctx, self._handle, self._params_dev, rows_dev, x)

    def waic(self, samples):
        """WAIC over the training rows: ``lppd`` = sum_m lpd[m], ``p_waic`` = sum_m var[m] and ``elpd_waic`` = lppd - p_waic of
        ``log_predictive(samples)``; the sums over the rows are taken in fp64 on the host."""
        lpd, _, var = self.log_predictive(samples)
        lppd = float(np.sum(lpd.numpy(), dtype=np.float64))
        p_waic = float(np.sum(var.numpy(), dtype=np.float64))
        return {"lppd": lppd, "p_waic": p_waic, "elpd_waic": lppd - p_waic}

    def expensive_metrics(self, model, samples) -> dict:
        """Per evaluation set of ``eval_sets``: ``{name}_lpd``, the mean over its rows of the log posterior-predictive density,
        and ``{name}_mean_ll``, the mean over rows and samples of the row's log-likelihood; with ``report_waic`` also ``lppd``,
        ``p_waic`` and ``elpd_waic`` of the training rows.  Neither keyword given: the empty dict of ``LNPDF``."""
        metrics = dict()
        for name, rows_dev in self._eval_sets_dev.items():
            lpd, mean, _ = hip_ops.custom_data_predictive(self.ctx, self._handle, self._params_dev, rows_dev, self._x(samples))
            metrics[f"{name}_lpd"] = float(np.mean(lpd.numpy(), dtype=np.float64))
            metrics[f"{name}_mean_ll"] = float(np.mean(mean.numpy(), dtype=np.float64))
        if self.report_waic:
            metrics.update(self.waic(samples))
        return metrics


class DeviceDataLNPDF(_DeviceDataTarget):
    """``DeviceDataLNPDF(source, num_dimensions, data, params=None, batch_size=None, seed=0, use_own_batch_per_sample=False,
    eval_sets=None, report_waic=False)``: ``source`` defines
    ``gmmvi_user_row`` and ``gmmvi_user_prior`` (contract: include/gmmvi_hip.h), ``data`` is the 2-D data set, uploaded once as
    fp32, and the target is ``prior(x) + s * sum_r row(x, data[r])``.

    batch_size=None: all rows in index order, s = 1.  A batch size B: every evaluation draws the B rows of
    ``minibatch_stream.data_minibatch_rows(seed, call_count, B, T)``, one batch shared by all samples, with s = T / B, and
    ``call_count`` advances after each evaluation that receives at least one sample (the protocol of ``MinibatchLNPDF``);
    ``log_density_full(x)`` is then the full-data value in index order, counter untouched.
    use_own_batch_per_sample=True (upstream's option of that name; it needs a batch size): sample n of an evaluation draws its
    own B rows, row n of ``minibatch_stream.data_minibatch_rows_per_sample(seed, call_count, N, B, T)``, so the minibatch error
    differs from sample to sample instead of shifting a whole iteration; sample 0 sees the shared batch of the same call.  The
    counter, ``log_density_full``, ``log_predictive`` and ``waic`` are as without it.
    The gradient comes from the library's dual numbers (num_dimensions <= _lib.CUSTOM_AUTODIFF_MAX_DIM) and is computed only
    for an estimator that reads it.  There is no ``_fast_path_target``: the iteration runs module by module, as for the other
    minibatch targets.
    eval_sets: a dict name -> [M, C] array of held-out rows with the columns of ``data``, uploaded once; ``expensive_metrics``
    then reports ``{name}_lpd`` and ``{name}_mean_ll`` for each, and with report_waic=True the WAIC of the training rows
    (``log_predictive``, ``waic``)."""

    _mode = "data"

    def _check_dimension(self, num_dimensions):
        if num_dimensions > _lib.CUSTOM_AUTODIFF_MAX_DIM:
            raise ValueError(f"num_dimensions must be <= {_lib.CUSTOM_AUTODIFF_MAX_DIM} for a differentiated target, got "
                             f"{num_dimensions}: the gradient costs ceil(D / {_lib.CUSTOM_AUTODIFF_TANGENTS}) passes per sample "
                             "and row")

    def _target_call(self, x, want_grad, batch_size, call):
        return hip_ops.target_custom_data(self.ctx, self._handle, self._params_dev, self._data_dev, x, want_grad=want_grad,
                                          batch_size=batch_size, seed=self.seed, call=call, **self._batch_keywords(batch_size))


class DeviceDataTapeLNPDF(_DeviceDataTarget):
    """``DeviceDataTapeLNPDF(source, num_dimensions, data, params=None, batch_size=None, seed=0, use_own_batch_per_sample=False,
    tape_capacity=None, scratch_bytes=None, eval_sets=None, report_waic=False)``: the source, the data, the minibatches (shared or
    one per sample), the call counter and the values of a ``DeviceDataLNPDF``, with
    the gradient from reverse mode (csrc/custom_target_data_tape.inc): every sample records one row's term at a time on a short
    tape in device scratch, reused for every row, and walks it back into a gradient accumulator.  The cost per row does not grow
    with ``ceil(D / 16)``, and ``num_dimensions`` goes up to ``_lib.MAX_DIM_DIAG``.

    tape_capacity: records per sample of the first gradient call (None: the library's default, then what the target has needed:
    the longest single row term or the prior); scratch_bytes: the budget of tapes and accumulators (None:
    ``_lib.CUSTOM_TAPE_SCRATCH_BYTES``); more tiles of 64 samples than fit are processed in slabs.  A gradient call reads the
    needed tape length back and so waits for the stream; there is no ``_fast_path_target``.
    Where forward mode stays the faster route (MI355X, logit, 10^4 samples, 1000 rows or minibatches of 64): at
    every dimension it reaches.  A gradient call of ``DeviceDataLNPDF`` takes a sixth of the time at D = 32, under a half at
    D = 128 and the same time at D = 512, because its dual numbers stay in registers while a tape goes through memory; this
    class is for num_dimensions above ``_lib.CUSTOM_AUTODIFF_MAX_DIM``.
    use_own_batch_per_sample: as for ``DeviceDataLNPDF``.  Own batches cost this class 5 - 8 % of a gradient call and the forward
    route 11 % at D = 32, 89 % at D = 128 and 2.1 x at D = 512 (per-lane row loads in every pass), so toward the forward cap this
    class is the faster own-batch route as well.
    Neither class chooses for the other.  eval_sets, report_waic: as for ``DeviceDataLNPDF``."""

    _mode = "data_tape"

    def __init__(self, source, num_dimensions, data, params=None, batch_size=None, seed=0, use_own_batch_per_sample=False,
                 tape_capacity=None, scratch_bytes=None, eval_sets=None, report_waic=False):
        self._set_tape_options(tape_capacity, scratch_bytes)
        super().__init__(source, num_dimensions, data, params, batch_size, seed, use_own_batch_per_sample, eval_sets, report_waic)

    def _check_dimension(self, num_dimensions):
        if num_dimensions > _lib.MAX_DIM_DIAG:
            raise ValueError(f"num_dimensions must be <= {_lib.MAX_DIM_DIAG}, got {num_dimensions}")

    def _target_call(self, x, want_grad, batch_size, call):
        return hip_ops.target_custom_data_tape(self.ctx, self._handle, self._params_dev, self._data_dev, x, want_grad=want_grad,
                                               batch_size=batch_size, seed=self.seed, call=call, **self._tape_keywords(want_grad),
                                               **self._batch_keywords(batch_size))
