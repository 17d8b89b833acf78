"""Shape-checked Python wrappers over the C ABI (include/gmmvi_hip.h).  Every wrapper validates operand shapes on
the host before the launch, so a kernel never sees a grid/operand mismatch."""
import math

import numpy as np

from . import _lib
from .device import DeviceArray

F32, I32 = np.dtype(np.float32), np.dtype(np.int32)


def _req(a, shape, dtype=F32, name="array"):
    if not isinstance(a, DeviceArray):
        raise TypeError(f"{name}: expected DeviceArray, got {type(a)}")
    if a.dtype != dtype or tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {dtype}{tuple(shape)}, got {a.dtype}{a.shape}")
    return a.ptr


def _opt(a, shape, dtype=F32, name="array"):
    return None if a is None else _req(a, shape, dtype, name)


def packed_stride(d):
    s = int(_lib.load().gmmvi_packed_stride(int(d)))
    if s == 0:
        raise _lib.GmmviError(f"dimension {d} is not supported by the register-resident kernels (D <= {_lib.MAX_DIM})")
    return s


def pack_components(ctx, means, chols, family=_lib.GAUSS, nu=0.0, want_inverse=False):
    """-> (packed [K, stride], inv_chols [K,D,D] or None)."""
    k, d = means.shape
    _req(means, (k, d), name="means"); _req(chols, (k, d, d), name="chols")
    packed = ctx.empty((k, packed_stride(d)))
    inv = ctx.empty((k, d, d)) if want_inverse else None
    ctx.check(ctx.lib.gmmvi_pack_components(ctx.handle, family, float(nu), k, d, means.ptr, chols.ptr, packed.ptr,
                                            None if inv is None else inv.ptr))
    return packed, inv


def cholesky(ctx, covs):
    k, d, _ = covs.shape
    _req(covs, (k, d, d), name="covs")
    chols = ctx.empty((k, d, d))
    ok = ctx.empty((k,), np.int32)
    ctx.check(ctx.lib.gmmvi_cholesky(ctx.handle, k, d, covs.ptr, chols.ptr, ok.ptr))
    return chols, ok


def mixture_eval(ctx, packed, logw, x, d, family=_lib.GAUSS, nu=0.0, want_ld=False, want_lp=True, want_grad=False):
    """-> (ld [K,N] | None, lp [N] | None, grad [N,D] | None)."""
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, packed_stride(d)), name="packed"); _req(logw, (k,), name="logw"); _req(x, (n, d), name="x")
    ld = ctx.empty((k, n)) if want_ld else None
    lp = ctx.empty((n,)) if want_lp else None
    grad = ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_mixture_eval(ctx.handle, family, float(nu), k, d, packed.ptr, logw.ptr, x.ptr, n,
                                             None if ld is None else ld.ptr, None if lp is None else lp.ptr,
                                             None if grad is None else grad.ptr))
    return ld, lp, grad


def mixture_eval_dual(ctx, packed, logw, logw2, x, d, want_ld=True, want_grad=True):
    """One sweep, two mixtures over the same components -> (ld | None, lp, grad | None, lp2)."""
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, packed_stride(d)), name="packed"); _req(logw, (k,), name="logw"); _req(logw2, (k,), name="logw2")
    _req(x, (n, d), name="x")
    ld = ctx.empty((k, n)) if want_ld else None
    lp, lp2 = ctx.empty((n,)), ctx.empty((n,))
    grad = ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_mixture_eval_dual(ctx.handle, _lib.GAUSS, 0.0, k, d, packed.ptr, logw.ptr, logw2.ptr,
                                                  x.ptr, n, None if ld is None else ld.ptr, lp.ptr,
                                                  None if grad is None else grad.ptr, lp2.ptr))
    return ld, lp, grad, lp2


def target_planar(ctx, prior_std, goals, likelihood_std, x, want_grad=True):
    n, d = x.shape
    g = goals.shape[0]
    _req(prior_std, (d,), name="prior_std"); _req(goals, (g, 2), name="goals"); _req(x, (n, d), name="x")
    lp = ctx.empty((n,))
    grad = ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_target_planar(ctx.handle, d, prior_std.ptr, g, goals.ptr, float(likelihood_std), x.ptr,
                                              n, lp.ptr, None if grad is None else grad.ptr))
    return lp, grad


def _ptr(a):
    return None if a is None else a.ptr


def _custom_entry(lib, stem, mode):
    """The entry of compile mode ``mode`` among ``stem``, ``stem``_autodiff, ..., one per member of CUSTOM_TARGET_MODES."""
    return getattr(lib, stem if mode == "hand" else f"{stem}_{mode}")


def _custom_target_check(mode, source, arch):
    import ctypes as C
    log = C.create_string_buffer(1 << 16)
    rc = _custom_entry(_lib.load(), "gmmvi_custom_target_check", mode)(str(source).encode(), str(arch).encode(), log, len(log))
    return int(rc), log.value.decode(errors="replace")


def custom_target_check(source, arch="gfx950"):
    """Compiles a user target's source behind the wrapper kernels for ``arch`` (csrc/custom_compile.hip) without a device.
    -> (status, compiler log): 0 when it compiles, GMMVI_ERR_ARG (-2) with the log otherwise."""
    return _custom_target_check("hand", source, arch)


def custom_target_check_autodiff(source, arch="gfx950"):
    """custom_target_check for a source that defines ``gmmvi_user_density`` (the log density only; the library's dual-number
    text differentiates it).  -> (status, compiler log)."""
    return _custom_target_check("autodiff", source, arch)


def custom_target_check_data(source, arch="gfx950"):
    """custom_target_check for a source that defines ``gmmvi_user_row`` and ``gmmvi_user_prior`` (a target summed over a data set,
    csrc/custom_target_data.inc).  -> (status, compiler log)."""
    return _custom_target_check("data", source, arch)


def custom_target_check_tape(source, arch="gfx950"):
    """custom_target_check for a source that defines ``gmmvi_user_density``, compiled for the tape mode (reverse-mode
    differentiation, csrc/custom_target_tape.inc).  -> (status, compiler log)."""
    return _custom_target_check("tape", source, arch)


def custom_target_check_data_tape(source, arch="gfx950"):
    """custom_target_check for a source that defines ``gmmvi_user_row`` and ``gmmvi_user_prior``, compiled for the data mode with
    reverse-mode gradients (csrc/custom_target_data_tape.inc).  -> (status, compiler log)."""
    return _custom_target_check("data_tape", source, arch)


def custom_data_tape_plan(n, rows, d, capacity, chunks_requested=0, scratch_bytes=0):
    """The plan of a gradient call of ``target_custom_data_tape`` for n samples and a row list of ``rows`` at dimension d and
    ``capacity`` records per lane within ``scratch_bytes`` (0: the default budget) (gmmvi_custom_data_tape_plan; needs no device)
    -> (chunks, rows_per_chunk, slabs, tiles_per_slab)."""
    import ctypes as C
    out = [C.c_int() for _ in range(4)]
    lib = _lib.load()
    _lib.check(None, lib.gmmvi_custom_data_tape_plan(int(n), int(rows), int(d), int(capacity), int(chunks_requested),
                                                     int(scratch_bytes), *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def custom_tape_plan(n, capacity, scratch_bytes=0):
    """The slab plan of a tape-mode gradient call on n samples at ``capacity`` records per lane within ``scratch_bytes`` (0: the
    default budget) (gmmvi_custom_tape_plan; needs no device) -> (slabs, lanes_per_slab)."""
    import ctypes as C
    slabs, lanes = C.c_int(), C.c_int()
    lib = _lib.load()
    _lib.check(None, lib.gmmvi_custom_tape_plan(int(n), int(capacity), int(scratch_bytes), C.byref(slabs), C.byref(lanes)))
    return slabs.value, lanes.value


def custom_data_plan(n, rows, chunks_requested=0):
    """The launch plan of ``target_custom_data`` for n samples and a row list of ``rows`` (gmmvi_custom_data_plan; needs no
    device) -> (chunks, rows_per_chunk)."""
    import ctypes as C
    chunks, per = C.c_int(), C.c_int()
    lib = _lib.load()
    _lib.check(None, lib.gmmvi_custom_data_plan(int(n), int(rows), int(chunks_requested), C.byref(chunks), C.byref(per)))
    return chunks.value, per.value


def custom_data_predictive_plan(n, rows, chunks_requested=0):
    """The launch plan of ``custom_data_predictive`` for n samples and an evaluation set of ``rows``
    (gmmvi_custom_data_predictive_plan; needs no device) -> (tiles, chunks, rows_per_chunk)."""
    import ctypes as C
    tiles, chunks, per = C.c_int(), C.c_int(), C.c_int64()
    lib = _lib.load()
    _lib.check(None, lib.gmmvi_custom_data_predictive_plan(int(n), int(rows), int(chunks_requested), C.byref(tiles),
                                                           C.byref(chunks), C.byref(per)))
    return tiles.value, chunks.value, per.value


def custom_data_predictive_probe(l, chunks_requested=0):
    """The tile reduction and the tile merge of the predictive kernels on the host (gmmvi_custom_data_predictive_probe; needs no
    device) for a host matrix l [n, rows] of row terms -> (lpd [rows], mean [rows], var [rows]) as NumPy arrays."""
    l = np.ascontiguousarray(l, np.float32)
    if l.ndim != 2:
        raise ValueError(f"l: expected a two-dimensional array, got {l.shape}")
    n, m = l.shape
    out = [np.empty(m, np.float32) for _ in range(3)]
    lib = _lib.load()
    _lib.check(None, lib.gmmvi_custom_data_predictive_probe(l.ctypes.data, n, m, int(chunks_requested),
                                                            *[o.ctypes.data for o in out]))
    return tuple(out)


class CustomTarget:
    """A compiled user target of a context (gmmvi_custom_target); released with the object."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    @property
    def ptr(self):
        return self.handle.value

    def __del__(self):
        try:
            if self.handle:
                self.ctx.lib.gmmvi_custom_target_release(self.ctx.handle, self.handle)
                self.handle = None
        except Exception:
            pass


CUSTOM_TARGET_MODES = ("hand", "autodiff", "data", "tape", "data_tape")


def custom_target_compile(ctx, source, autodiff=False, mode=None):
    """Compiles ``source`` (the contract: include/gmmvi_hip.h) for the context's device -> CustomTarget.  mode: "hand" (the
    source defines ``gmmvi_user_target``), "autodiff" (``gmmvi_user_density``, the library differentiates it) or "data"
    (``gmmvi_user_row`` and ``gmmvi_user_prior``, launched by ``target_custom_data``) or "tape" (``gmmvi_user_density``,
    differentiated in reverse mode, launched by ``target_custom_tape``) or "data_tape" (the source of "data", its gradient in
    reverse mode, launched by ``target_custom_data_tape``); None: ``autodiff`` chooses between the first two.  A source that does not compile raises GmmviError with the compiler log."""
    import ctypes as C
    if mode is None:
        mode = "autodiff" if autodiff else "hand"
    if mode not in CUSTOM_TARGET_MODES:
        raise ValueError(f"mode: expected one of {CUSTOM_TARGET_MODES}, got {mode!r}")
    h = C.c_void_p()
    ctx.check(_custom_entry(ctx.lib, "gmmvi_custom_target_compile", mode)(ctx.handle, str(source).encode(), C.byref(h)))
    return CustomTarget(ctx, h)


def _custom_arguments(handle, x, params, rows=None, predictive=False):
    """The host checks of every launcher of a user target, in the order they have always had: the handle, x [n, D], for a
    launcher that takes one its row array [rows, C] ("rows" and not empty for the predictive density, else "data"), then params
    (1-D or None) -> (n, D) or (n, D, rows, C)."""
    if not isinstance(handle, CustomTarget):
        raise TypeError(f"handle: expected CustomTarget, got {type(handle)}")
    if predictive and len(x.shape) != 2:
        raise ValueError(f"x: expected a two-dimensional array, got {x.shape}")
    n, d = shapes = x.shape
    _req(x, (n, d), name="x")
    if rows is not None:
        name = "rows" if predictive else "data"
        if len(rows.shape) != 2:
            raise ValueError(f"{name}: expected a two-dimensional array, got {rows.shape}")
        _req(rows, tuple(rows.shape), name=name)
        shapes = (n, d) + tuple(rows.shape)
        if predictive and (n < 1 or rows.shape[0] < 1):
            raise ValueError(f"the predictive density needs at least one sample and one row, got {n} and {rows.shape[0]}")
    if params is not None:
        if len(params.shape) != 1:
            raise ValueError(f"params: expected a one-dimensional array, got {params.shape}")
        _req(params, params.shape, name="params")
    return shapes


def target_custom(ctx, handle, params, x, want_grad=True, route=0):
    """User target ``handle`` on x [n, D] (csrc/custom_target.hip).  params: the target's 1-D device array or None; route: 0
    auto, 1 staged (LDS), 2 direct.  -> (lp [n], grad [n, D] or None)."""
    n, d = _custom_arguments(handle, x, params)
    lp, grad = ctx.empty((n,)), ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_target_custom(ctx.handle, handle.handle, d, _ptr(params), x.ptr, n, lp.ptr, _ptr(grad), int(route)))
    return lp, grad


def _target_custom_data(ctx, stem, handle, params, data, x, want_grad, batch_size, seed, call, chunks, own_batches, *tail):
    """What ``target_custom_data`` and ``target_custom_data_tape`` share: the checks, one argument list, and the choice between the
    entry ``stem``, which takes the minibatch flag and B, and its ``_own_batches`` twin, which takes B alone.  tail: what the
    entry takes behind chunks."""
    if own_batches and batch_size is None:
        raise ValueError("own_batches needs a batch_size: the full-data row list is the same for every sample")
    n, d, t, c = _custom_arguments(handle, x, params, data)
    lp, grad = ctx.empty((n,)), ctx.empty((n, d)) if want_grad else None
    if n > 0:
        entry = getattr(ctx.lib, stem + "_own_batches" if own_batches else stem)
        batch = (int(batch_size),) if own_batches else (0, t) if batch_size is None else (1, int(batch_size))
        ctx.check(entry(ctx.handle, handle.handle, d, _ptr(params), data.ptr, t, c, *batch, int(seed) & 0xFFFFFFFFFFFFFFFF,
                        int(call) & 0xFFFFFFFF, x.ptr, n, lp.ptr, _ptr(grad), int(chunks), *tail))
    return lp, grad


def target_custom_data(ctx, handle, params, data, x, want_grad=True, batch_size=None, seed=0, call=0, chunks=0, own_batches=False):
    """Data-mode user target ``handle`` on x [n, D]: prior(x) + s * sum of the row terms over data [T, C]
    (csrc/custom_target_data.inc).  batch_size None: all rows in index order, s = 1; a number: the minibatch of (seed, call)
    with s = T / batch_size, one batch shared by all samples or, with own_batches, a batch of its own for every sample
    (``minibatch_stream.data_minibatch_rows_per_sample``; gmmvi_target_custom_data_own_batches).  chunks: 0 lets the library plan
    the launch, a positive number forces that many row chunks.  -> (lp [n], grad [n, D] or None)."""
    return _target_custom_data(ctx, "gmmvi_target_custom_data", handle, params, data, x, want_grad, batch_size, seed, call, chunks,
                               own_batches)


def target_custom_tape(ctx, handle, params, x, want_grad=True, tape_capacity=0, scratch_bytes=0):
    """Tape-mode user target ``handle`` on x [n, D] (csrc/custom_target_tape.inc): the gradient from one recorded evaluation
    and one backward sweep per sample.  tape_capacity: records per lane, 0 what the handle has needed at this D so far;
    scratch_bytes: the budget of the tape scratch, 0 the default.  A gradient call synchronises the stream.
    -> (lp [n], grad [n, D] or None)."""
    n, d = _custom_arguments(handle, x, params)
    lp, grad = ctx.empty((n,)), ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_target_custom_tape(ctx.handle, handle.handle, d, _ptr(params), x.ptr, n, lp.ptr, _ptr(grad),
                                                   int(tape_capacity), int(scratch_bytes)))
    return lp, grad


def target_custom_data_tape(ctx, handle, params, data, x, want_grad=True, batch_size=None, seed=0, call=0, chunks=0,
                            tape_capacity=0, scratch_bytes=0, own_batches=False):
    """``target_custom_data`` for a handle of mode "data_tape": the same target, the same value call, and the gradient from
    reverse mode on a tape that is reused for every row (csrc/custom_target_data_tape.inc), at any D up to ``_lib.MAX_DIM_DIAG``.
    tape_capacity: records per lane, 0 what the handle has needed at this D so far; scratch_bytes: the budget of the tapes and
    accumulators, 0 the default.  own_batches: as for ``target_custom_data`` (gmmvi_target_custom_data_tape_own_batches).  A
    gradient call synchronises the stream.  -> (lp [n], grad [n, D] or None)."""
    return _target_custom_data(ctx, "gmmvi_target_custom_data_tape", handle, params, data, x, want_grad, batch_size, seed, call,
                               chunks, own_batches, int(tape_capacity), int(scratch_bytes))


def custom_data_predictive(ctx, handle, params, rows, x, chunks=0):
    """Predictive density of a handle of mode "data" or "data_tape" (csrc/custom_target_data.inc): with l[n, m] the row term of
    sample x[n] on rows[m], per row  lpd = log mean_n exp(l),  mean = mean_n l  and  var = the unbiased variance of l over the
    samples.  rows [M, C]: the evaluation set; chunks: 0 lets the library plan the launch, a positive number forces that many
    row chunks (no output bit depends on it).  -> (lpd [M], mean [M], var [M])."""
    n, d, m, c = _custom_arguments(handle, x, params, rows, predictive=True)
    lpd, mean, var = ctx.empty((m,)), ctx.empty((m,)), ctx.empty((m,))
    ctx.check(ctx.lib.gmmvi_custom_data_predictive(ctx.handle, handle.handle, d, _ptr(params), rows.ptr, m, c, x.ptr, n, lpd.ptr,
                                                   mean.ptr, var.ptr, int(chunks)))
    return lpd, mean, var


def custom_tape_length(ctx, handle, d):
    """The longest tape (records per lane) a gradient launch of ``handle`` has needed at dimension d; 0: none yet."""
    import ctypes as C
    length = C.c_int()
    ctx.check(ctx.lib.gmmvi_custom_tape_length(ctx.handle, handle.handle, int(d), C.byref(length)))
    return length.value


def target_logreg(ctx, A, prior_mean, prior_std, x, want_grad=True):
    """Logistic-regression posterior (csrc/logreg.hip).  A: [M, D] signed data matrix diag(s) X~.  -> (lp [n], grad [n, D])."""
    m, d = A.shape
    n = x.shape[0]
    _req(A, (m, d), name="A"); _req(x, (n, d), name="x")
    lp = ctx.empty((n,))
    grad = ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_target_logreg(ctx.handle, d, m, A.ptr, float(prior_mean), float(prior_std), x.ptr, n, lp.ptr,
                                              None if grad is None else grad.ptr))
    return lp, grad


def _minibatch_target(ctx, entry, head, seed, call, tail, x, d, want_grad):
    """lp [n] and grad [n, d] of a minibatch target: entry(handle, *head, seed, call, *tail, x, n, lp, grad) with the seed
    and the call counter cut to the 64 and 32 bits the stream takes."""
    n = x.shape[0]
    _req(x, (n, d), name="x")
    lp = ctx.empty((n,))
    grad = ctx.empty((n, d)) if want_grad else None
    if n > 0:
        ctx.check(entry(ctx.handle, *head, int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFF, *tail, x.ptr, n, lp.ptr,
                        None if grad is None else grad.ptr))
    return lp, grad


def _predict_slabs(ctx, entry, head, W, d, X, out_shape):
    """Forward pass of every weight vector W [S, d] on every row X [M, F] -> out [S, M, ...]: entry(handle, *head, W, S, X, M,
    out) over slabs of W, since the kernels' grid takes at most 65535 weight vectors per launch."""
    s, (m, f) = W.shape[0], X.shape
    _req(W, (s, d), name="W"); _req(X, (m, f), name="X")
    out = ctx.empty((s, m) + tuple(out_shape))
    if m > 0:
        for s0 in range(0, s, 65535):
            s1 = min(s, s0 + 65535)
            ctx.check(entry(ctx.handle, *head, W.rows(s0, s1).ptr, s1 - s0, X.ptr, m, out.rows(s0, s1).ptr))
    return out


def target_logreg_mb(ctx, A, batch_size, num_batches, seed, call, prior_mean, prior_std, x, want_grad=True):
    """Minibatch logistic-regression posterior (csrc/logreg_mb.hip).  A: [T, D] signed training rows; sample n takes batch
    n mod num_batches of the permutation of (seed, call).  -> (lp [n], grad [n, D])."""
    t, d = A.shape
    _req(A, (t, d), name="A")
    return _minibatch_target(ctx, ctx.lib.gmmvi_target_logreg_mb, (d, t, A.ptr, int(batch_size), int(num_batches)), seed, call,
                             (float(prior_mean), float(prior_std)), x, d, want_grad)


def mlp_num_parameters(num_features, hidden_units, num_outputs=1):
    """Per layer W [in, out], then b [out], over num_features -> hidden_units ... -> num_outputs (1 for a regressor, the
    number of classes for a classifier)."""
    d, last = 0, int(num_features)
    for width in [int(h) for h in hidden_units] + [int(num_outputs)]:
        d += last * width + width
        last = width
    return d


def bnn_classifier_num_parameters(num_features, hidden, num_classes):
    return mlp_num_parameters(num_features, (hidden,), num_classes)


def target_bnn(ctx, X, y, hidden_units, seed, call, batch_size, likelihood_scaling, prior_std, x, want_grad=True):
    """Bayesian-neural-network regression posterior (csrc/bnn.hip).  X: [T, F] training features, y: [T] labels,
    hidden_units (H1, H2); the minibatch rows come from the stream of (seed, call).  -> (lp [n], grad [n, D])."""
    t, f = X.shape
    h1, h2 = (int(h) for h in hidden_units)
    _req(X, (t, f), name="X"); _req(y, (t,), name="y")
    return _minibatch_target(ctx, ctx.lib.gmmvi_target_bnn, (f, h1, h2, t, X.ptr, y.ptr), seed, call,
                             (int(batch_size), float(likelihood_scaling), float(prior_std)), x,
                             mlp_num_parameters(f, (h1, h2)), want_grad)


def bnn_predict(ctx, hidden_units, W, X):
    """Network outputs of every weight vector on every row (csrc/bnn.hip), forward only.  W: [S, D], X: [M, F] -> [S, M]."""
    _, f = X.shape
    h1, h2 = (int(h) for h in hidden_units)
    return _predict_slabs(ctx, ctx.lib.gmmvi_bnn_predict, (f, h1, h2), W, mlp_num_parameters(f, (h1, h2)), X, ())


def target_bnn_classifier(ctx, X, labels, hidden, num_classes, seed, call, batch_size, likelihood_scaling, prior_std, x,
                          want_grad=True):
    """Bayesian-neural-network classification posterior (csrc/bnn_classifier.hip).  X: [T, F] training features, labels:
    [T] int32 in [0, num_classes), one ReLU layer of ``hidden`` units; the minibatch rows come from the stream of
    (seed, call).  -> (lp [n], grad [n, D])."""
    t, f = X.shape
    h, c = int(hidden), int(num_classes)
    _req(X, (t, f), name="X"); _req(labels, (t,), I32, name="labels")
    return _minibatch_target(ctx, ctx.lib.gmmvi_target_bnn_classifier, (f, h, c, t, X.ptr, labels.ptr), seed, call,
                             (int(batch_size), float(likelihood_scaling), float(prior_std)), x,
                             mlp_num_parameters(f, (h,), c), want_grad)


def bnn_classifier_predict(ctx, hidden, num_classes, W, X):
    """Logits of every weight vector on every row (csrc/bnn_classifier.hip), forward only.  W: [S, D], X: [M, F]
    -> [S, M, C]."""
    (_, f), h, c = X.shape, int(hidden), int(num_classes)
    return _predict_slabs(ctx, ctx.lib.gmmvi_bnn_classifier_predict, (f, h, c), W, mlp_num_parameters(f, (h,), c), X, (c,))


MLP_MAX_FEATURES, MLP_MAX_HIDDEN, MLP_MAX_HIDDEN_LAYERS = 1024, 128, _lib.MLP_MAX_LAYERS - 1     # csrc/bnn_mlp.hip
MLP_MIN_CLASSES, MLP_MAX_CLASSES, MLP_MAX_BATCH = 2, 16, 1024


def mlp_desc(num_features, hidden_units, activations, loss, num_outputs=1):
    """The gmmvi_mlp_desc of a network, checked against what csrc/bnn_mlp.hip takes (ValueError names the limit).
    activations: one name per layer, the output layer included ("linear" there); loss: "mse" (one output) or
    "sparse_categorical_crossentropy" (num_outputs classes)."""
    hidden = [int(h) for h in hidden_units]
    acts = list(activations)
    f, c = int(num_features), int(num_outputs)
    if not 1 <= len(hidden) <= MLP_MAX_HIDDEN_LAYERS:
        raise ValueError(f"hidden_units must name 1 to {MLP_MAX_HIDDEN_LAYERS} hidden layers, got {tuple(hidden)}")
    if not 1 <= f <= MLP_MAX_FEATURES:
        raise ValueError(f"the network takes 1 to {MLP_MAX_FEATURES} features, got {f}")
    if not all(1 <= h <= MLP_MAX_HIDDEN for h in hidden):
        raise ValueError(f"hidden layers must have 1 to {MLP_MAX_HIDDEN} units, got {tuple(hidden)}")
    if len(acts) != len(hidden) + 1:
        raise ValueError(f"activations must name one activation per layer, the output layer included "
                         f"({len(hidden) + 1}), got {len(acts)}")
    unknown = [a for a in acts if a not in _lib.MLP_ACTIVATIONS]
    if unknown:
        raise ValueError(f"activations must be among {sorted(_lib.MLP_ACTIVATIONS)}, got {unknown}")
    if acts[-1] != "linear":
        raise ValueError(f"the output layer's activation must be 'linear', got {acts[-1]!r}")
    if loss not in _lib.MLP_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_lib.MLP_LOSSES)}, got {loss!r}")
    if loss == "mse" and c != 1:
        raise ValueError(f"the mse loss takes one output, got {c}")
    if loss != "mse" and not MLP_MIN_CLASSES <= c <= MLP_MAX_CLASSES:
        raise ValueError(f"num_classes must lie in [{MLP_MIN_CLASSES}, {MLP_MAX_CLASSES}], got {c}")
    d = mlp_num_parameters(f, hidden, c)
    if d > _lib.MAX_DIM_DIAG:
        raise ValueError(f"the network has {d} parameters, more than the {_lib.MAX_DIM_DIAG} a diagonal mixture takes")
    desc = _lib.MlpDesc()
    desc.n_layers = len(hidden) + 1
    for i, w in enumerate([f] + hidden + [c]):
        desc.widths[i] = w
    for i, a in enumerate(acts):
        desc.activations[i] = _lib.MLP_ACTIVATIONS[a]
    desc.loss = _lib.MLP_LOSSES[loss]
    return desc


def target_mlp(ctx, X, y, hidden_units, activations, loss, num_outputs, seed, call, batch_size, likelihood_scaling, prior_std,
               x, want_grad=True):
    """Generic Bayesian-neural-network posterior (csrc/bnn_mlp.hip).  X: [T, F] training features; y: [T] f32 labels (loss
    "mse", num_outputs 1) or int32 labels in [0, num_outputs) ("sparse_categorical_crossentropy"); the minibatch rows come
    from the stream of (seed, call).  -> (lp [n], grad [n, D])."""
    t, f = X.shape
    desc = mlp_desc(f, hidden_units, activations, loss, num_outputs)
    _req(X, (t, f), name="X"); _req(y, (t,), F32 if loss == "mse" else I32, name="y")
    if not 1 <= int(batch_size) <= min(t, MLP_MAX_BATCH):
        raise ValueError(f"batch_size must lie in [1, {min(t, MLP_MAX_BATCH)}] (the training-set size, at most "
                         f"{MLP_MAX_BATCH}), got {batch_size}")
    if not prior_std > 0:
        raise ValueError("prior_std must be positive")
    return _minibatch_target(ctx, ctx.lib.gmmvi_target_mlp, (desc, t, X.ptr, y.ptr), seed, call,
                             (int(batch_size), float(likelihood_scaling), float(prior_std)), x,
                             mlp_num_parameters(f, hidden_units, num_outputs), want_grad)


def mlp_predict(ctx, hidden_units, activations, loss, num_outputs, W, X):
    """Network outputs of every weight vector on every row (csrc/bnn_mlp.hip), forward only.  W: [S, D], X: [M, F]
    -> [S, M] ("mse") or logits [S, M, C]."""
    _, f = X.shape
    desc = mlp_desc(f, hidden_units, activations, loss, num_outputs)
    return _predict_slabs(ctx, ctx.lib.gmmvi_mlp_predict, (desc,), W, mlp_num_parameters(f, hidden_units, num_outputs), X,
                          () if loss == "mse" else (int(num_outputs),))


TALOS_DIM = 34                                         # csrc/talos.hip: 28 joints, base position, roll / pitch / yaw
TALOS_TABLE_SIZE = 8 + 28 * 28 + 4 * 16                 # header, joint records, tip records (talos_ik.py)


def target_talos(ctx, model, context, x, want_grad=True):
    """Talos inverse-kinematics target (csrc/talos.hip).  model: the packed table of talos_ik.TalosModel, context: [3] the
    left gripper's goal, x: [n, 34].  -> (lp [n], grad [n, 34])."""
    n = x.shape[0]
    _req(model, (TALOS_TABLE_SIZE,), name="model"); _req(context, (3,), name="context"); _req(x, (n, TALOS_DIM), name="x")
    lp = ctx.empty((n,))
    grad = ctx.empty((n, TALOS_DIM)) if want_grad else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_target_talos(ctx.handle, model.ptr, context.ptr, x.ptr, n, lp.ptr,
                                             None if grad is None else grad.ptr))
    return lp, grad


def talos_fk(ctx, model, x):
    """Forward kinematics of the Talos model (csrc/talos.hip).  -> (poses [n, 4, 12]: per tip world position and row-major
    rotation, com [n, 3]: world centre of mass)."""
    n = x.shape[0]
    _req(model, (TALOS_TABLE_SIZE,), name="model"); _req(x, (n, TALOS_DIM), name="x")
    poses = ctx.empty((n, 4, 12))
    com = ctx.empty((n, 3))
    if n > 0:
        ctx.check(ctx.lib.gmmvi_talos_fk(ctx.handle, model.ptr, x.ptr, n, poses.ptr, com.ptr))
    return poses, com


def sample_components(ctx, means, chols, offsets, n, seed=0, first_index=0, stream_id=0, eps=None):
    """offsets: DeviceArray int32 [K+1] prefix sums with offsets[K] == n.  -> (x [n,D], mapping [n] int32)."""
    k, d = means.shape
    _req(means, (k, d), name="means"); _req(chols, (k, d, d), name="chols"); _req(offsets, (k + 1,), I32, "offsets")
    if eps is not None:
        _req(eps, (n, d), name="eps")
    x = ctx.empty((n, d))
    mapping = ctx.empty((n,), np.int32)
    if n > 0:
        ctx.check(ctx.lib.gmmvi_sample_components(ctx.handle, k, d, means.ptr, chols.ptr, offsets.ptr, n,
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), int(stream_id),
                                                  None if eps is None else eps.ptr, x.ptr, mapping.ptr))
    return x, mapping


def philox_normals(ctx, seed, first_index, n, d, stream_id=0):
    out = ctx.empty((n, d))
    if n > 0:
        ctx.check(ctx.lib.gmmvi_philox_normals(ctx.handle, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index),
                                               int(stream_id), n, d, out.ptr))
    return out


def philox_uniforms(ctx, seed, first_index, n, stream_id=1):
    out = ctx.empty((n,))
    if n > 0:
        ctx.check(ctx.lib.gmmvi_philox_uniforms(ctx.handle, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index),
                                                int(stream_id), n, out.ptr))
    return out


def stein(ctx, packed, x, ld, qgrad, bg, tgrad, d, mapping=None, map_offset=0, self_normalized=True,
          own_samples_only=False):
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, packed_stride(d)), name="packed"); _req(x, (n, d), name="x")
    _req(qgrad, (n, d), name="qgrad"); _req(tgrad, (n, d), name="tgrad")
    if own_samples_only:
        _req(mapping, (n,), I32, "mapping")
    else:
        _req(ld, (k, n), name="ld"); _req(bg, (n,), name="bg")
    flags = (_lib.SELF_NORMALIZED if self_normalized else 0) | (_lib.OWN_SAMPLES_ONLY if own_samples_only else 0)
    h_neg = ctx.empty((k, d, d))
    g_neg = ctx.empty((k, d))
    ctx.check(ctx.lib.gmmvi_stein(ctx.handle, k, d, packed.ptr, x.ptr, n, None if ld is None else ld.ptr, qgrad.ptr,
                                  None if bg is None else bg.ptr, tgrad.ptr,
                                  None if mapping is None else mapping.ptr, int(map_offset), flags, h_neg.ptr,
                                  g_neg.ptr))
    return h_neg, g_neg


def more(ctx, packed, chols, x, ld, logq, bg, tlp, l2, d, mapping=None, map_offset=0, self_normalized=True,
         own_samples_only=False):
    """MORE estimate (gmmvi_more) -> (h_neg [K,D,D], g_neg [K,D])."""
    k = packed.shape[0]
    n = x.shape[0]
    if d >= _lib.MAX_DIM:
        raise ValueError(f"MORE estimator: D = {d} is not supported by the HIP kernels (D <= {_lib.MAX_DIM - 1})")
    _req(packed, (k, packed_stride(d)), name="packed"); _req(chols, (k, d, d), name="chols"); _req(x, (n, d), name="x")
    _req(logq, (n,), name="logq"); _req(tlp, (n,), name="tlp"); _req(l2, (k,), name="l2")
    if own_samples_only:
        _req(mapping, (n,), I32, "mapping")
    else:
        _req(ld, (k, n), name="ld"); _req(bg, (n,), name="bg")
    flags = (_lib.SELF_NORMALIZED if self_normalized else 0) | (_lib.OWN_SAMPLES_ONLY if own_samples_only else 0)
    h_neg = ctx.empty((k, d, d))
    g_neg = ctx.empty((k, d))
    ctx.check(ctx.lib.gmmvi_more(ctx.handle, k, d, packed.ptr, chols.ptr, x.ptr, n, None if ld is None else ld.ptr,
                                 logq.ptr, None if bg is None else bg.ptr, tlp.ptr,
                                 None if mapping is None else mapping.ptr, int(map_offset), flags, l2.ptr, h_neg.ptr,
                                 g_neg.ptr))
    return h_neg, g_neg


def more_blocked(ctx, packed, chols, x, ld, logq, bg, tlp, l2, d, mapping=None, map_offset=0, self_normalized=True,
                 own_samples_only=False):
    """MORE estimate for 64 <= D <= 128 from the blocked component blocks (gmmvi_more_blocked) -> (h_neg [K,D,D],
    g_neg [K,D])."""
    if not _lib.MORE_BLOCKED_MIN_DIM <= d <= _lib.MORE_BLOCKED_MAX_DIM:
        raise ValueError(f"MORE estimator (blocked route): D = {d} is outside the supported range "
                         f"{_lib.MORE_BLOCKED_MIN_DIM} <= D <= {_lib.MORE_BLOCKED_MAX_DIM}")
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, packed_stride(d)), name="packed"); _req(chols, (k, d, d), name="chols"); _req(x, (n, d), name="x")
    _req(logq, (n,), name="logq"); _req(tlp, (n,), name="tlp"); _req(l2, (k,), name="l2")
    if own_samples_only:
        _req(mapping, (n,), I32, "mapping")
    else:
        _req(ld, (k, n), name="ld"); _req(bg, (n,), name="bg")
    flags = (_lib.SELF_NORMALIZED if self_normalized else 0) | (_lib.OWN_SAMPLES_ONLY if own_samples_only else 0)
    h_neg = ctx.empty((k, d, d))
    g_neg = ctx.empty((k, d))
    ctx.check(ctx.lib.gmmvi_more_blocked(ctx.handle, k, d, packed.ptr, chols.ptr, x.ptr, n, None if ld is None else ld.ptr,
                                         logq.ptr, None if bg is None else bg.ptr, tlp.ptr,
                                         None if mapping is None else mapping.ptr, int(map_offset), flags, l2.ptr,
                                         h_neg.ptr, g_neg.ptr))
    return h_neg, g_neg


def update_components_kl(ctx, means, chols, h_neg, g_neg, stepsizes, temperature, l2_init, last_eta, l2, num_updates,
                         want_info=False, reference=False, want_packed=False):
    """-> (success, kl | None, probes | None[, packed])."""
    k, d = means.shape
    _req(means, (k, d), name="means"); _req(chols, (k, d, d), name="chols")
    _req(h_neg, (k, d, d), name="h_neg"); _req(g_neg, (k, d), name="g_neg"); _req(stepsizes, (k,), name="stepsizes")
    _req(last_eta, (k,), name="last_eta"); _req(l2, (k,), name="l2"); _req(num_updates, (k,), name="num_updates")
    success = ctx.empty((k,), np.int32)
    kl = ctx.empty((k,)) if want_info else None
    probes = ctx.empty((k,), np.int32) if want_info else None
    args = [ctx.handle, k, d, means.ptr, chols.ptr, h_neg.ptr, g_neg.ptr, stepsizes.ptr, float(temperature),
            float(l2_init), last_eta.ptr, l2.ptr, num_updates.ptr, success.ptr, None if kl is None else kl.ptr,
            None if probes is None else probes.ptr]
    if reference:
        ctx.check(ctx.lib.gmmvi_update_components_kl_reference(*args))
        return success, kl, probes
    packed = ctx.empty((k, packed_stride(d))) if want_packed else None
    ctx.check(ctx.lib.gmmvi_update_components_kl(*args, None if packed is None else packed.ptr))
    return (success, kl, probes, packed) if want_packed else (success, kl, probes)


def stein_update_kl(ctx, packed_old, x, ld, qgrad, bg, tgrad, means, chols, stepsizes, temperature, l2_init, last_eta, l2,
                    num_updates, self_normalized=True, explicit_estimate=False):
    """Test-only (gmmvi_stein_update_kl): the Stein partials and the update that finishes the estimate itself, as the single-call
    iteration runs them -> (success, packed_new, h_neg scratch, g_neg scratch, partials per component)."""
    import ctypes
    k, d = means.shape
    n = x.shape[0]
    _req(packed_old, (k, packed_stride(d)), name="packed_old"); _req(x, (n, d), name="x"); _req(ld, (k, n), name="ld")
    _req(qgrad, (n, d), name="qgrad"); _req(bg, (n,), name="bg"); _req(tgrad, (n, d), name="tgrad")
    _req(means, (k, d), name="means"); _req(chols, (k, d, d), name="chols"); _req(stepsizes, (k,), name="stepsizes")
    _req(last_eta, (k,), name="last_eta"); _req(l2, (k,), name="l2"); _req(num_updates, (k,), name="num_updates")
    flags = (_lib.SELF_NORMALIZED if self_normalized else 0) | (_lib.EXPLICIT_ESTIMATE if explicit_estimate else 0)
    h_neg, g_neg = ctx.full((k, d, d), float("nan")), ctx.full((k, d), float("nan"))     # (stay NaN where a route never writes them)
    success = ctx.empty((k,), np.int32)
    packed = ctx.empty((k, packed_stride(d)))
    r = ctypes.c_int32(0)
    ctx.check(ctx.lib.gmmvi_stein_update_kl(ctx.handle, k, d, packed_old.ptr, x.ptr, n, ld.ptr, qgrad.ptr, bg.ptr, tgrad.ptr, flags,
                                            h_neg.ptr, g_neg.ptr, means.ptr, chols.ptr, stepsizes.ptr, float(temperature),
                                            float(l2_init), last_eta.ptr, l2.ptr, num_updates.ptr, success.ptr, packed.ptr,
                                            ctypes.byref(r)))
    return success, packed, h_neg, g_neg, int(r.value)


def update_components_plain(ctx, mode, means, chols, h_neg, g_neg, stepsizes, l2_init, l2, num_updates):
    k, d = means.shape
    _req(means, (k, d), name="means"); _req(chols, (k, d, d), name="chols")
    _req(h_neg, (k, d, d), name="h_neg"); _req(g_neg, (k, d), name="g_neg"); _req(stepsizes, (k,), name="stepsizes")
    _req(l2, (k,), name="l2"); _req(num_updates, (k,), name="num_updates")
    success = ctx.empty((k,), np.int32)
    fn = ctx.lib.gmmvi_update_components_direct if mode == "direct" else ctx.lib.gmmvi_update_components_iblr
    ctx.check(fn(ctx.handle, k, d, means.ptr, chols.ptr, h_neg.ptr, g_neg.ptr, stepsizes.ptr, float(l2_init), l2.ptr,
                 num_updates.ptr, success.ptr))
    return success


# ---- dedicated kernels for diagonal mixtures (csrc/diag_sweep.hip): O(D) per (sample, component) pair ----------------------
def _diag_dim(d, what):
    if not 1 <= d <= _lib.MAX_DIM_DIAG:
        raise ValueError(f"{what}: D = {d} is outside the diagonal kernels' range 1 <= D <= {_lib.MAX_DIM_DIAG}")


def _dense_dim(d, what):
    if not 1 <= d <= _lib.MAX_DIM_BLOCKED:
        raise ValueError(f"{what}: dense [K, D, D] factors exist for 1 <= D <= {_lib.MAX_DIM_BLOCKED} only, got D = {d}")


def diag_packed_stride(d):
    _diag_dim(d, "diag_packed_stride")
    return int(_lib.load().gmmvi_diag_packed_stride(int(d)))


def diag_pack(ctx, means, sigma):
    """(means [K,D], standard deviations [K,D]) -> component blocks [K, diag_packed_stride(D)]."""
    k, d = means.shape
    _diag_dim(d, "diag_pack")
    _req(means, (k, d), name="means"); _req(sigma, (k, d), name="sigma")
    packed = ctx.empty((k, diag_packed_stride(d)))
    ctx.check(ctx.lib.gmmvi_diag_pack(ctx.handle, k, d, means.ptr, sigma.ptr, packed.ptr))
    return packed


def diag_mixture_eval(ctx, packed, logw, x, d, want_ld=False, want_lp=True, want_grad=False, logw2=None):
    """-> (ld [K,N] | None, lp [N] | None, grad [N,D] | None[, lp2 [N] when logw2 is given])."""
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, diag_packed_stride(d)), name="packed"); _req(logw, (k,), name="logw"); _req(x, (n, d), name="x")
    if logw2 is not None:
        _req(logw2, (k,), name="logw2")
        want_lp = True
    ld = ctx.empty((k, n)) if want_ld else None
    lp = ctx.empty((n,)) if want_lp else None
    grad = ctx.empty((n, d)) if want_grad else None
    lp2 = ctx.empty((n,)) if logw2 is not None else None
    if n > 0:
        ctx.check(ctx.lib.gmmvi_diag_mixture_eval(ctx.handle, k, d, packed.ptr, logw.ptr, None if logw2 is None else logw2.ptr,
                                                  x.ptr, n, None if ld is None else ld.ptr, None if lp is None else lp.ptr,
                                                  None if grad is None else grad.ptr, None if lp2 is None else lp2.ptr))
    return (ld, lp, grad) if logw2 is None else (ld, lp, grad, lp2)


def diag_sample(ctx, means, sigma, offsets, n, seed=0, first_index=0, stream_id=0, eps=None):
    """x = mu_k + sigma_k * eps in component order -> (x [n,D], mapping [n] int32); arguments as sample_components."""
    k, d = means.shape
    _diag_dim(d, "diag_sample")
    _req(means, (k, d), name="means"); _req(sigma, (k, d), name="sigma"); _req(offsets, (k + 1,), I32, "offsets")
    if eps is not None:
        _req(eps, (n, d), name="eps")
    x = ctx.empty((n, d))
    mapping = ctx.empty((n,), np.int32)
    if n > 0:
        ctx.check(ctx.lib.gmmvi_diag_sample(ctx.handle, k, d, means.ptr, sigma.ptr, offsets.ptr, n,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), int(stream_id),
                                            None if eps is None else eps.ptr, x.ptr, mapping.ptr))
    return x, mapping


def diag_stein(ctx, packed, x, ld, qgrad, bg, tgrad, d, mapping=None, map_offset=0, self_normalized=True,
               own_samples_only=False):
    """Stein estimate of a diagonal mixture -> (h_neg_diag [K,D], g_neg [K,D])."""
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, diag_packed_stride(d)), name="packed"); _req(x, (n, d), name="x")
    _req(qgrad, (n, d), name="qgrad"); _req(tgrad, (n, d), name="tgrad")
    if own_samples_only:
        _req(mapping, (n,), I32, "mapping")
    else:
        _req(ld, (k, n), name="ld"); _req(bg, (n,), name="bg")
    flags = (_lib.SELF_NORMALIZED if self_normalized else 0) | (_lib.OWN_SAMPLES_ONLY if own_samples_only else 0)
    h_neg = ctx.empty((k, d))
    g_neg = ctx.empty((k, d))
    ctx.check(ctx.lib.gmmvi_diag_stein(ctx.handle, k, d, packed.ptr, x.ptr, n, None if ld is None else ld.ptr, qgrad.ptr,
                                       None if bg is None else bg.ptr, tgrad.ptr, None if mapping is None else mapping.ptr,
                                       int(map_offset), flags, h_neg.ptr, g_neg.ptr))
    return h_neg, g_neg


def more_diag(ctx, packed, x, ld, logq, bg, tlp, l2, d, mapping=None, map_offset=0, self_normalized=True,
              own_samples_only=False):
    """Gradient-free MORE estimate of a diagonal mixture (gmmvi_more_diag: regression on [z^2, z, 1]) -> (h_neg_diag [K,D],
    g_neg [K,D]); NaN rows for a component whose ridge system is not positive definite."""
    if not 1 <= d <= _lib.MORE_DIAG_MAX_DIM:
        raise ValueError(f"MORE estimator (diagonal route): D = {d} is outside the supported range "
                         f"1 <= D <= {_lib.MORE_DIAG_MAX_DIM}")
    k = packed.shape[0]
    n = x.shape[0]
    _req(packed, (k, diag_packed_stride(d)), name="packed"); _req(x, (n, d), name="x")
    _req(logq, (n,), name="logq"); _req(tlp, (n,), name="tlp"); _req(l2, (k,), name="l2")
    if own_samples_only:
        _req(mapping, (n,), I32, "mapping")
    else:
        _req(ld, (k, n), name="ld"); _req(bg, (n,), name="bg")
    flags = (_lib.SELF_NORMALIZED if self_normalized else 0) | (_lib.OWN_SAMPLES_ONLY if own_samples_only else 0)
    h_neg = ctx.empty((k, d))
    g_neg = ctx.empty((k, d))
    ctx.check(ctx.lib.gmmvi_more_diag(ctx.handle, k, d, packed.ptr, x.ptr, n, None if ld is None else ld.ptr, logq.ptr,
                                      None if bg is None else bg.ptr, tlp.ptr, None if mapping is None else mapping.ptr,
                                      int(map_offset), flags, l2.ptr, h_neg.ptr, g_neg.ptr))
    return h_neg, g_neg


def diag_embed(ctx, chols_diag):
    """[K,D] sigma -> dense lower-triangular factors [K,D,D] = diag(sigma) for the dense density / sampling kernels."""
    k, d = chols_diag.shape
    _dense_dim(d, "diag_embed")
    _req(chols_diag, (k, d), name="chols_diag")
    dense = ctx.empty((k, d, d))
    ctx.check(ctx.lib.gmmvi_diag_embed(ctx.handle, k, d, chols_diag.ptr, dense.ptr))
    return dense


def diag_extract(ctx, dense):
    """[K,D,D] -> its diagonals [K,D]."""
    k, d, _ = dense.shape
    _dense_dim(d, "diag_extract")
    _req(dense, (k, d, d), name="dense")
    diag = ctx.empty((k, d))
    ctx.check(ctx.lib.gmmvi_diag_extract(ctx.handle, k, d, dense.ptr, diag.ptr))
    return diag


def reciprocal(ctx, a):
    if a.dtype != F32:
        raise ValueError("reciprocal: fp32 only")
    out = ctx.empty(a.shape)
    ctx.check(ctx.lib.gmmvi_reciprocal_f32(ctx.handle, a.ptr, a.size, out.ptr))
    return out


def update_components_diag(ctx, mode, means, chols_diag, h_neg_diag, g_neg, stepsizes, temperature, l2_init, last_eta, l2,
                           num_updates, want_info=False):
    """Diagonal-covariance component update, mode "kl" or "iblr" -> (success, kl | None, probes | None)."""
    k, d = means.shape
    _diag_dim(d, "update_components_diag")
    _req(means, (k, d), name="means"); _req(chols_diag, (k, d), name="chols_diag")
    _req(h_neg_diag, (k, d), name="h_neg_diag"); _req(g_neg, (k, d), name="g_neg")
    _req(stepsizes, (k,), name="stepsizes"); _req(l2, (k,), name="l2"); _req(num_updates, (k,), name="num_updates")
    success = ctx.empty((k,), np.int32)
    if mode == "iblr":
        ctx.check(ctx.lib.gmmvi_update_components_diag_iblr(ctx.handle, k, d, means.ptr, chols_diag.ptr, h_neg_diag.ptr,
                                                            g_neg.ptr, stepsizes.ptr, float(l2_init), l2.ptr,
                                                            num_updates.ptr, success.ptr))
        return success, None, None
    if mode != "kl":
        raise ValueError(f"update_components_diag: unknown mode {mode!r}")
    _req(last_eta, (k,), name="last_eta")
    kl = ctx.empty((k,)) if want_info else None
    probes = ctx.empty((k,), np.int32) if want_info else None
    ctx.check(ctx.lib.gmmvi_update_components_diag_kl(ctx.handle, k, d, means.ptr, chols_diag.ptr, h_neg_diag.ptr,
                                                      g_neg.ptr, stepsizes.ptr, float(temperature), float(l2_init),
                                                      last_eta.ptr, l2.ptr, num_updates.ptr, success.ptr,
                                                      None if kl is None else kl.ptr,
                                                      None if probes is None else probes.ptr))
    return success, kl, probes


def mmd_pair_sum(ctx, a, b, inv_bandwidth):
    """sum_i sum_j exp(-sum_d inv_bandwidth[d] (a[i,d] - b[j,d])^2) -> Python float (fp64 sum)."""
    na, d = a.shape
    nb = b.shape[0]
    _req(a, (na, d), name="a"); _req(b, (nb, d), name="b"); _req(inv_bandwidth, (d,), name="inv_bandwidth")
    if na == 0 or nb == 0:
        return 0.0
    # fp64 scratch / result held in fp32-typed device buffers of twice the length (DeviceArray is 4-byte typed)
    scratch = ctx.empty((2 * int(ctx.lib.gmmvi_mmd_scratch_doubles(na, nb)),))
    out = ctx.empty((2,))
    ctx.check(ctx.lib.gmmvi_mmd_pair_sum(ctx.handle, a.ptr, na, b.ptr, nb, d, inv_bandwidth.ptr, scratch.ptr, out.ptr))
    return float(out.numpy().view(np.float64)[0])


def expected_log_ratios(ctx, ld, bg, tlp, logq, beta, logw, self_normalized=True, reward_out=None, want_ess=False,
                        logq_parts=None):
    """logq_parts ([R, N], R >= 2) replaces logq (pass None): the chunk partials of a component-split sweep, merged by the kernel
    while it reads them."""
    k, n = ld.shape
    _req(ld, (k, n), name="ld"); _req(bg, (n,), name="bg"); _req(tlp, (n,), name="tlp")
    _req(logw, (k,), name="logw")
    if reward_out is not None:
        _req(reward_out, (k,), name="reward_out")
    e = ctx.empty((k,))
    ess = ctx.empty((k,)) if want_ess else None
    tail = (float(beta), logw.ptr, 1 if self_normalized else 0, e.ptr, None if reward_out is None else reward_out.ptr,
            None if ess is None else ess.ptr)
    if logq_parts is not None:
        if logq is not None:
            raise ValueError("expected_log_ratios: give logq or logq_parts, not both")
        r = logq_parts.shape[0]
        if r < 2:
            raise ValueError("expected_log_ratios: logq_parts needs at least two partial rows")
        _req(logq_parts, (r, n), name="logq_parts")
        ctx.check(ctx.lib.gmmvi_expected_log_ratios_parts(ctx.handle, k, n, ld.ptr, bg.ptr, tlp.ptr, logq_parts.ptr, r, *tail))
    else:
        _req(logq, (n,), name="logq")
        ctx.check(ctx.lib.gmmvi_expected_log_ratios(ctx.handle, k, n, ld.ptr, bg.ptr, tlp.ptr, logq.ptr, *tail))
    return e, ess


def update_weights(ctx, mode, logw, e, stepsize, beta, want_info=False):
    k = logw.shape[0]
    _req(logw, (k,), name="logw"); _req(e, (k,), name="E"); _req(stepsize, (1,), name="stepsize")
    info = ctx.empty((2,)) if (want_info and mode == "trust-region") else None
    if mode == "trust-region":
        ctx.check(ctx.lib.gmmvi_update_weights_kl(ctx.handle, k, logw.ptr, e.ptr, stepsize.ptr, float(beta),
                                                  None if info is None else info.ptr))
    else:
        ctx.check(ctx.lib.gmmvi_update_weights_direct(ctx.handle, k, logw.ptr, e.ptr, stepsize.ptr, float(beta)))
    return info


def component_stepsize_improvement(ctx, stepsizes, prev, last, mn, mx, inc, dec):
    k = stepsizes.shape[0]
    _req(stepsizes, (k,), name="stepsizes"); _req(prev, (k,), name="prev"); _req(last, (k,), name="last")
    ctx.check(ctx.lib.gmmvi_component_stepsize_improvement(ctx.handle, k, stepsizes.ptr, prev.ptr, last.ptr, float(mn),
                                                           float(mx), float(inc), float(dec)))


def weight_stepsize_improvement(ctx, logw, rewards_last, state, mn, mx, inc, dec):
    k = logw.shape[0]
    _req(logw, (k,), name="logw"); _req(rewards_last, (k,), name="rewards_last"); _req(state, (2,), name="state")
    ctx.check(ctx.lib.gmmvi_weight_stepsize_improvement(ctx.handle, k, logw.ptr, rewards_last.ptr, state.ptr, float(mn),
                                                        float(mx), float(inc), float(dec)))


def combine_partials(ctx, lp_parts, grad_parts, d):
    r, n = lp_parts.shape
    _req(lp_parts, (r, n), name="lp_parts")
    if grad_parts is not None:
        _req(grad_parts, (r, n, d), name="grad_parts")
    lp = ctx.empty((n,))
    grad = ctx.empty((n, d)) if grad_parts is not None else None
    ctx.check(ctx.lib.gmmvi_combine_partials(ctx.handle, r, n, d, lp_parts.ptr,
                                             None if grad_parts is None else grad_parts.ptr, lp.ptr,
                                             None if grad is None else grad.ptr))
    return lp, grad


def gather_rows(ctx, src, idx):
    """dst[i] = src[idx[i]] along axis 0 (idx: DeviceArray int32 or host array)."""
    if not isinstance(idx, DeviceArray):
        idx = ctx.asarray(np.asarray(idx, np.int32), np.int32)
    n = idx.shape[0]
    _req(idx, (n,), I32, "idx")
    inner = src.shape[1:]
    words = math.prod(inner) if inner else 1
    dst = ctx.empty((n,) + tuple(inner), src.dtype)
    if n > 0:
        ctx.check(ctx.lib.gmmvi_gather_rows(ctx.handle, src.ptr, idx.ptr, n, words, dst.ptr))
    return dst


def logaddexp(ctx, a, ca, b, cb):
    """-> log(exp(a + ca) + exp(b + cb)), element-wise (a, b: [n] float32 DeviceArrays; ca, cb: floats)."""
    if a.shape != b.shape or a.dtype != F32 or b.dtype != F32:
        raise ValueError("logaddexp: shape/dtype mismatch")
    out = ctx.empty(a.shape)
    ctx.check(ctx.lib.gmmvi_logaddexp_f32(ctx.handle, out.ptr, a.ptr, float(ca), b.ptr, float(cb), a.size))
    return out


def segment_lse_into(ctx, out, col0, offsets, logw, ld):
    """out[g, col0 + n] = log sum_{j in [offsets[g], offsets[g+1])} exp(logw[j] + ld[j, n]); out: [rows >= G, width] DeviceArray,
    offsets: int32 DeviceArray [G + 1], ld: [Kw, N]."""
    kw, n = ld.shape
    g = offsets.shape[0] - 1
    if out.ndim != 2 or out.shape[0] < g or out.shape[1] < col0 + n or logw.shape != (kw,):
        raise ValueError("segment_lse_into: shape mismatch")
    ctx.check(ctx.lib.gmmvi_segment_lse_f32(ctx.handle, g, offsets.ptr, logw.ptr, ld.ptr, n, out.ptr, out.shape[1], int(col0)))
    return out


def copy_2d(ctx, dst, dst_row, dst_col, src, src_row, src_col, rows, cols):
    """dst[dst_row + r, dst_col + c] = src[src_row + r, src_col + c] (2-D float32 DeviceArrays)."""
    if rows <= 0 or cols <= 0:
        return dst
    if (dst_row + rows > dst.shape[0] or dst_col + cols > dst.shape[1] or src_row + rows > src.shape[0]
            or src_col + cols > src.shape[1]):
        raise ValueError("copy_2d: block out of range")
    ctx.check(ctx.lib.gmmvi_copy_2d_f32(ctx.handle, dst.ptr + (dst_row * dst.shape[1] + dst_col) * 4, dst.shape[1],
                                        src.ptr + (src_row * src.shape[1] + src_col) * 4, src.shape[1], int(rows), int(cols)))
    return dst


def exp_into(ctx, dst, src):
    if dst.shape != src.shape or dst.dtype != F32 or src.dtype != F32:
        raise ValueError("exp_into: shape/dtype mismatch")
    ctx.check(ctx.lib.gmmvi_exp_f32(ctx.handle, dst.ptr, src.ptr, src.size))
    return dst


def copy_batch(ctx, pairs):
    """pairs: list of (dst DeviceArray view, src DeviceArray) of equal size; one launch per group of 8."""
    import ctypes as C
    pairs = [(d, s) for d, s in pairs if s.size > 0]
    for i in range(0, len(pairs), 8):
        grp = pairs[i:i + 8]
        for d, s in grp:
            if d.size != s.size or d.dtype != s.dtype:
                raise ValueError("copy_batch: size/dtype mismatch")
        n = len(grp)
        dst = (C.c_void_p * n)(*[d.ptr for d, _ in grp])
        src = (C.c_void_p * n)(*[s.ptr for _, s in grp])
        nb = (C.c_size_t * n)(*[s.nbytes for _, s in grp])
        ctx.check(ctx.lib.gmmvi_copy_batch(ctx.handle, n, dst, src, nb))


def concat(ctx, parts):
    """One flat fp32 buffer holding the (flattened) parts back to back; a single copy launch (<= 8 parts)."""
    total = sum(int(p.size) for p in parts)
    out = ctx.empty((total,))
    pairs, off = [], 0
    for p in parts:
        n = int(p.size)
        pairs.append((out.rows(off, off + n), p.reshape(-1)))
        off += n
    copy_batch(ctx, pairs)
    return out


def unpack_gathered(ctx, gathered, n_ranks, sizes):
    """Inverse of concat after an all-gather: gathered = [n_ranks][sum(sizes)] -> one [n_ranks * size_j] array per part."""
    import ctypes as C
    chunk = int(sum(sizes))
    if gathered.size != n_ranks * chunk:
        raise ValueError("unpack_gathered: gathered buffer has the wrong size")
    outs = [ctx.empty((n_ranks * int(sz),)) for sz in sizes]
    n = len(sizes)
    words = (C.c_size_t * n)(*[int(sz) for sz in sizes])
    dst = (C.c_void_p * n)(*[o.ptr for o in outs])
    ctx.check(ctx.lib.gmmvi_unpack_gathered(ctx.handle, gathered.ptr, int(n_ranks), chunk, n, words, dst))
    return outs
