"""GPU tests of own minibatches per sample for user-defined device targets summed over a data set
(gmmvi_target_custom_data_own_batches, gmmvi_target_custom_data_tape_own_batches; gmmvi_data_rows_own_* of
csrc/custom_target_data.inc, gmmvi_data_tape_rows_own of csrc/custom_target_data_tape.inc; ``use_own_batch_per_sample=True``):
both entries through the C ABI against the fp64 per-sample restatement of tests/custom_data_own_cases.py at the seams of the
64-sample tile, of an epoch of the stream, of B = T, of fewer positions than waves, of the pass width, the staged route's cap and
the forward mode's cap, of the row chunks and of the tape's slabs; determinism; agreement across chunk counts, between forward and
reverse mode and with the shared-batch and the full-data call; the refusals; and both classes in the modular iteration and under
a gradient-free estimator.

Kernel bound: the rule of tests/test_hip_custom_target.py, unchanged (its _bound): the device's largest error against the fp64
NumPy restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|, for lp and the gradient.  Every case prints its ratios before it asserts.
tests/test_custom_data_own_host.py shows what that bound can see."""
import numpy as np
import pytest

import custom_data_own_cases as cases
import test_hip_custom_data as data_mode
import test_hip_custom_data_tape as tape_mode
import test_hip_custom_target as hand
from gmmvi_amd import _lib
from helpers import samtron_config
from oracle import train as otrain
from test_hip_custom_target import SENTINEL, _bound

pytestmark = pytest.mark.gpu

ERR_ARG = -2
KERNEL_CASES = cases.kernel_cases()
KINDS = ("data", "tape")
TAGS = {"data": "target_custom_data_own", "tape": "target_custom_data_tape_own"}


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def _handle(ctx, kind, name):
    """The handles of the shared-batch test files: ragged is compiled for the forward mode here."""
    if kind == "tape":
        return tape_mode._handle(ctx, name)
    if name not in data_mode._handles:
        from gmmvi_amd import hip_ops
        data_mode._handles[name] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode="data")
    return data_mode._handles[name]


def _launch(ctx, kind, handle, own, x, want_grad, chunks=0, capacity=0, scratch=0):
    """The own-batch entry of ``kind`` for the restatement ``own`` (its data, params, batch, seed and current call) on outputs with
    CANARY_ROWS extra rows of SENTINEL behind them -> (rc, lp, grad | None); the extra rows are checked here: bit-unchanged."""
    tgt = own.tgt
    n, d = x.shape
    t, c = tgt.data.shape
    xd, pd, dd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    lp = ctx.full((n + hand.CANARY_ROWS,), SENTINEL)
    grad = ctx.full((n + hand.CANARY_ROWS, d), SENTINEL) if want_grad else None
    head = (ctx.handle, handle.handle, d, pd.ptr, dd.ptr, t, c, tgt.batch_size, tgt.seed, tgt.call_count, xd.ptr, n, lp.ptr,
            None if grad is None else grad.ptr, chunks)
    if kind == "tape":
        rc = ctx.lib.gmmvi_target_custom_data_tape_own_batches(*head, capacity, scratch)
    else:
        rc = ctx.lib.gmmvi_target_custom_data_own_batches(*head)
    if rc != 0:
        return rc, None, None
    sentinel_bits = np.array(SENTINEL).view(np.uint32)
    lp_h = lp.numpy()
    assert np.all(lp_h[n:].view(np.uint32) == sentinel_bits), "lp written past N"
    g_h = None
    if want_grad:
        g_h = grad.numpy()
        assert np.all(g_h[n:].view(np.uint32) == sentinel_bits), "gradient written past N"
        g_h = g_h[:n]
    return rc, lp_h[:n], g_h


def _check(tag, lp, g, lp64, g64, lp32, g32):
    e_lp, b_lp, r_lp = _bound(lp, lp64, lp32)
    line = f"[custom_data_own] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
    if g is not None:
        e_g, b_g, r_g = _bound(g, g64, g32)
        line += f", gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})"
    print("\n" + line)
    assert np.all(np.isfinite(lp)) and (g is None or np.all(np.isfinite(g)))
    assert e_lp <= b_lp, f"{tag}: lp error {e_lp:.3e} > {b_lp:.3e}"
    if g is not None:
        assert e_g <= b_g, f"{tag}: gradient error {e_g:.3e} > {b_g:.3e}"


def _has_gradient(kind, c):
    return kind == "tape" or c.d <= cases.FORWARD_CAP


# the forward class runs D = 513 as a value call; 1100 is the tape class's alone
PAIRS = [(kind, c) for kind in KINDS for c in KERNEL_CASES if kind == "tape" or c.d <= cases.FORWARD_CAP + 1]


@pytest.mark.parametrize("kind,c", PAIRS, ids=lambda v: v if isinstance(v, str) else cases.case_id(v))
def test_kernel_matches_fp64_reference(ctx, kind, c):
    own, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, kind, c.name)
    if _has_gradient(kind, c):
        (rc, lp, g), launches = tape_mode._launches(ctx, lambda: _launch(ctx, kind, handle, own, x, True, c.chunks), TAGS[kind])
        assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
        assert launches >= 1                                         # the own-batch kernels ran, under their own tag
        _check(f"{kind} {cases.case_id(c)}", lp, g, lp64, g64, lp32, g32)
    (rc, lp_v, g_v), launches = tape_mode._launches(ctx, lambda: _launch(ctx, kind, handle, own, x, False, c.chunks), TAGS["data"])
    assert rc == 0 and g_v is None and launches == 1
    _check(f"{kind} {cases.case_id(c)} values only", lp_v, None, lp64, g64, lp32, g32)


SEAM_CASES = [cases.Case("logit", 17, 65, 257, 3, 64, 3), cases.Case("ragged", 6, 65, 9, 0, 5, 3)]


@pytest.mark.parametrize("c", SEAM_CASES, ids=cases.case_id)
def test_same_call_twice_gives_the_same_bits(ctx, c):
    own, x = cases.reference(c)[:2]
    for kind in KINDS:
        handle = _handle(ctx, kind, c.name)
        for chunks in (1, 3):
            _, lp_a, g_a = _launch(ctx, kind, handle, own, x, True, chunks)
            _, lp_b, g_b = _launch(ctx, kind, handle, own, x, True, chunks)
            np.testing.assert_array_equal(lp_a.view(np.uint32), lp_b.view(np.uint32))
            np.testing.assert_array_equal(g_a.view(np.uint32), g_b.view(np.uint32))


@pytest.mark.parametrize("c", SEAM_CASES, ids=cases.case_id)
def test_tape_value_call_gives_the_bits_of_the_forward_class(ctx, c):
    own, x = cases.reference(c)[:2]
    for chunks in (c.chunks, 1):
        rc_t, lp_t, _ = _launch(ctx, "tape", _handle(ctx, "tape", c.name), own, x, False, chunks)
        rc_d, lp_d, _ = _launch(ctx, "data", _handle(ctx, "data", c.name), own, x, False, chunks)
        assert rc_t == 0 and rc_d == 0
        np.testing.assert_array_equal(lp_t.view(np.uint32), lp_d.view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_chunk_counts_agree_within_the_bound(ctx, kind):
    c = SEAM_CASES[0]
    own, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, kind, c.name)
    out = {}
    for chunks in (0, 1, 2, 3):
        rc, lp, g = _launch(ctx, kind, handle, own, x, True, chunks)
        assert rc == 0
        _check(f"{kind} {cases.case_id(c)} chunk request {chunks}", lp, g, lp64, g64, lp32, g32)
        out[chunks] = (lp, g)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    for a, b in ((0, 1), (1, 2), (1, 3), (2, 3)):
        d_lp = float(np.abs(out[a][0].astype(np.float64) - out[b][0]).max())
        d_g = float(np.abs(out[a][1].astype(np.float64) - out[b][1]).max())
        print(f"[custom_data_own] {kind} chunks {a} against {b}: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), the "
              f"gradient by {d_g:.3e} ({d_g / b_g:.3f})")
        assert d_lp <= b_lp and d_g <= b_g


@pytest.mark.parametrize("c", SEAM_CASES + [cases.Case("logit", 512, 65, 9, 0, 5, 3)], ids=cases.case_id)
def test_forward_mode_and_reverse_mode_agree(ctx, c):
    own, x, lp64, g64, lp32, g32 = cases.reference(c)
    rc_f, lp_f, g_f = _launch(ctx, "data", _handle(ctx, "data", c.name), own, x, True, c.chunks)
    rc_r, lp_r, g_r = _launch(ctx, "tape", _handle(ctx, "tape", c.name), own, x, True, c.chunks)
    assert rc_f == 0 and rc_r == 0
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    d_lp, d_g = float(np.abs(lp_f.astype(np.float64) - lp_r).max()), float(np.abs(g_f.astype(np.float64) - g_r).max())
    print(f"\n[custom_data_own] {cases.case_id(c)} forward against reverse: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the "
          f"bound), the gradient by {d_g:.3e} ({d_g / b_g:.3f})")
    assert d_lp <= b_lp and d_g <= b_g


@pytest.mark.parametrize("kind", KINDS)
def test_sample_0_sees_the_shared_batch_and_the_others_do_not(ctx, kind):
    c = cases.Case("logit", 5, 65, 257, 0, 64, 0)                    # 64 of 257 rows: no other sample draws sample 0's set of rows
    own, x, lp64, g64, lp32, g32 = cases.reference(c)
    lists = own.row_lists(c.n)
    assert all(sorted(lists[n]) != sorted(lists[0]) for n in range(1, c.n))
    handle = _handle(ctx, kind, c.name)
    rc, lp, g = _launch(ctx, kind, handle, own, x, True)
    shared = (tape_mode if kind == "tape" else data_mode)._launch(ctx, handle, own.tgt, x, True)
    assert rc == 0 and shared[0] == 0
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    d_lp = np.abs(lp.astype(np.float64) - shared[1])
    d_g = np.abs(g.astype(np.float64) - shared[2]).max(axis=1)
    print(f"\n[custom_data_own] {kind} against the shared batch: sample 0 differs by {d_lp[0] / b_lp:.3f} / {d_g[0] / b_g:.3f} of the "
          f"bound, the others by at least {d_lp[1:].min() / b_lp:.3g} / {d_g[1:].min() / b_g:.3g} bounds")
    assert d_lp[0] <= b_lp and d_g[0] <= b_g
    assert np.all(np.maximum(d_lp[1:] / b_lp, d_g[1:] / b_g) > 100.0)


@pytest.mark.parametrize("name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_full_batches_agree_with_the_full_data_call(ctx, name):
    """B = T: every sample sums all rows, in its own order, with s = 1: log_density_full within the bound of that sum."""
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    c = cases.Case("student", 5, 65, 257, 0, 257, 3)
    own, x = cases.reference(c)[:2]
    full = own.tgt.full()
    lp64, g64 = full.evaluate(x.astype(np.float64))
    lp32, g32 = cases.fp32_twin(full).evaluate(x)
    target = getattr(device_lnpdf, name)(cases.SOURCES[c.name], c.d, own.tgt.data, params=own.tgt.params(), batch_size=257,
                                         seed=own.tgt.seed, use_own_batch_per_sample=True)
    lp, g = (a.numpy() for a in target.log_density_and_grad(x))
    _check(f"{name} B = T against the full-data restatement", lp, g, lp64, g64, lp32, g32)
    lp_full = target.log_density_full(x).numpy()
    b_lp = _bound(lp32, lp64, lp32)[1]
    d_lp = float(np.abs(lp.astype(np.float64) - lp_full).max())
    print(f"[custom_data_own] {name} B = T against log_density_full: {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound)")
    assert d_lp <= b_lp and target.call_count == 1


def test_slabs_form_the_position_from_the_index_in_the_call(ctx):
    from gmmvi_amd import hip_ops
    c = cases.SLAB_CASE
    own, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, "tape", c.name)
    rc, lp_one, g_one = _launch(ctx, "tape", handle, own, x, True)
    assert rc == 0
    _check(cases.case_id(c), lp_one, g_one, lp64, g64, lp32, g32)
    needed = hip_ops.custom_tape_length(ctx, handle, c.d)
    budget = 64 * (needed * _lib.CUSTOM_TAPE_RECORD_BYTES + 4 * c.d)             # one tile with one chunk
    assert hip_ops.custom_data_tape_plan(c.n, c.batch, c.d, needed, 0, budget) == (1, 5, 3, 1)
    (rc, lp, g), launches = tape_mode._launches(ctx, lambda: _launch(ctx, "tape", handle, own, x, True, 0, 0, budget), TAGS["tape"])
    assert rc == 0 and launches == 3
    _check(cases.case_id(c) + " in three slabs", lp, g, lp64, g64, lp32, g32)
    np.testing.assert_array_equal(lp.view(np.uint32), lp_one.view(np.uint32))
    np.testing.assert_array_equal(g.view(np.uint32), g_one.view(np.uint32))


def test_capacity_growth_uses_the_same_rows(ctx):
    from gmmvi_amd import hip_ops
    c = cases.Case("ragged", 6, 65, 9, 0, 5, 3)
    own, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = hip_ops.custom_target_compile(ctx, cases.SOURCES["ragged"] + "\n// own batches, capacity growth\n", mode="data_tape")
    assert hip_ops.custom_tape_length(ctx, handle, c.d) == 0
    (rc, lp, g), launches = tape_mode._launches(ctx, lambda: _launch(ctx, "tape", handle, own, x, True, 0, 4), TAGS["tape"])
    assert rc == 0 and launches == 2 and hip_ops.custom_tape_length(ctx, handle, c.d) > 4
    _check("capacity 4, second attempt", lp, g, lp64, g64, lp32, g32)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(ctx, kind):
    from gmmvi_amd import hip_ops
    lib = ctx.lib
    c = cases.Case("logit", 5, 8, 9, 0, 5, 0)
    own, x = cases.build_case(c)
    tgt = own.tgt
    mine = _handle(ctx, kind, "logit")
    n, d, t, cols = 8, 5, 9, 6
    wide = 513
    xd, pd, dd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    xw, dw = ctx.asarray(np.zeros((n, wide), np.float32)), ctx.asarray(np.zeros((t, wide + 1), np.float32))
    lp, grad, grad_w = ctx.full((n,), SENTINEL), ctx.full((n, d), SENTINEL), ctx.full((n, wide), SENTINEL)

    def call(D=d, data=dd.ptr, T=t, Cc=cols, B=5, X=xd.ptr, N=n, out=lp.ptr, g=grad.ptr, h=mine.handle, chunks=0, cap=0):
        head = (ctx.handle, h, D, pd.ptr, data, T, Cc, B, 9, 0, X, N, out, g, chunks)
        if kind == "tape":
            return lib.gmmvi_target_custom_data_tape_own_batches(*head, cap, 0)
        return lib.gmmvi_target_custom_data_own_batches(*head)

    def last():
        return lib.gmmvi_last_error(ctx.handle).decode()

    assert call(B=0) == ERR_ARG and "B = 0" in last()
    assert call(B=10) == ERR_ARG and "B = 10" in last() and "T = 9" in last()
    assert call(Cc=0) == ERR_ARG and "C = 0" in last()
    assert call(T=0) == ERR_ARG and "T = 0" in last()
    assert call(T=2 ** 31) == ERR_ARG and "2^31" in last()
    for kw, names in ((dict(data=None), "data_dev"), (dict(N=0), "N >= 1"), (dict(X=None), "X_dev"), (dict(out=None), "lp_out_dev"),
                      (dict(D=0), "D >= 1"), (dict(D=_lib.MAX_DIM_DIAG + 1), "GMMVI_MAX_DIM_DIAG"), (dict(chunks=-1), "chunks_requested"),
                      (dict(h=None), "t != nullptr")):
        assert call(**kw) == ERR_ARG and names in last(), (kw, last())
    if kind == "tape":
        assert call(cap=-1) == ERR_ARG and "tape_capacity" in last()
    else:                                                            # the gradient cap of forward mode; a value call runs above it
        assert call(D=wide, data=dw.ptr, Cc=wide + 1, X=xw.ptr, g=grad_w.ptr) == ERR_ARG and "512" in last() and "513" in last()
    # a handle of the other data mode, and of a mode without rows
    other = _handle(ctx, "tape" if kind == "data" else "data", "logit")
    for h in (other, hand._handle(ctx, "rosenbrock")):
        for g in (grad.ptr, None):
            assert call(h=h.handle, g=g) == ERR_ARG
            assert ("gmmvi_custom_target_compile_data" in last()) or ("gmmvi_target_custom_data_tape" in last())
    # the shared-batch entries still know two row lists only
    assert lib.gmmvi_target_custom_data(ctx.handle, _handle(ctx, "data", "logit").handle, d, pd.ptr, dd.ptr, t, cols, 2, 5, 9, 0, xd.ptr,
                                        n, lp.ptr, grad.ptr, 0) == ERR_ARG
    assert lib.gmmvi_target_custom_data_tape(ctx.handle, _handle(ctx, "tape", "logit").handle, d, pd.ptr, dd.ptr, t, cols, 2, 5, 9, 0,
                                             xd.ptr, n, lp.ptr, grad.ptr, 0, 0, 0) == ERR_ARG
    op = hip_ops.target_custom_data_tape if kind == "tape" else hip_ops.target_custom_data
    with pytest.raises(ValueError, match="batch_size"):
        op(ctx, mine, pd, dd, xd, True, own_batches=True)
    # every refusal came before any launch
    ctx.check(lib.gmmvi_sync(ctx.handle))
    bits = np.array(SENTINEL).view(np.uint32)
    assert np.all(lp.numpy().view(np.uint32) == bits) and np.all(grad.numpy().view(np.uint32) == bits)
    assert np.all(grad_w.numpy().view(np.uint32) == bits)
    # and the context works afterwards
    assert call() == 0
    ctx.check(lib.gmmvi_sync(ctx.handle))
    lp64, g64 = own.evaluate(x.astype(np.float64))
    lp32, g32 = own.as_dtype(np.float32).evaluate(x)
    _check(f"{kind} after the refusals", lp.numpy(), grad.numpy(), lp64, g64, lp32, g32)
    lp_o, g_o = op(ctx, mine, pd, dd, xd, True, batch_size=5, seed=9, call=0, own_batches=True)
    np.testing.assert_array_equal(lp_o.numpy().view(np.uint32), lp.numpy().view(np.uint32))
    np.testing.assert_array_equal(g_o.numpy().view(np.uint32), grad.numpy().view(np.uint32))


# ---- the iteration -----------------------------------------------------------------------------------------------------
def _diagonal_pair(name, d, batch_size):
    """The set-up of _diagonal_pair of tests/test_hip_custom_data_tape.py (logit over 40 rows, a diagonal-covariance model, the
    Stein estimator, the KL trust region, K = 3, 40 samples per component) with own batches on both sides: the oracle's target
    is the per-sample restatement, the device's the class ``name`` with use_own_batch_per_sample=True."""
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    k, s, seed = 3, 40, 11
    cfg = samtron_config(s, diag=True)
    data = tape_mode._logit_rows(np.random.default_rng(17), 40, d)
    ref = cases.OwnBatches(cases.tape_cases.base.Logit(data, [0.25, 2.0], batch_size=batch_size, seed=9))
    prior_scale, initial_cov = 0.5, 0.25
    model = otrain.construct_initial_mixture(d, k, 0.0, prior_scale, initial_cov, np.random.default_rng(seed + 1),
                                             use_diagonal_covs=True)
    o = otrain.OracleGMMVI(
        ref, model, temperature=cfg["temperature"], seed=seed, desired_samples_per_component=s, ratio_reused_samples_to_desired=0.0,
        ng_estimator="Stein", only_use_own_samples=cfg["ng_estimator_config"]["only_use_own_samples"],
        use_self_normalized_importance_weights=cfg["ng_estimator_config"]["use_self_normalized_importance_weights"],
        updater=cfg["ng_based_updater_type"], component_stepsize_config=cfg["component_stepsize_adapter_config"],
        weight_updater=cfg["weight_updater_type"], weight_stepsize_config=cfg["weight_stepsize_adapter_config"], adaptive=None,
        max_reward_history_length=400, sample_selector=cfg["sample_selector_type"], max_database_size=cfg["max_database_size"],
        host_rng=np.random.default_rng(seed))
    om = o.model.model
    m = DiagonalGMM(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
    m.seed = seed
    wrapper = GmmWrapper(m, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
    c = dict(cfg)
    c["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=initial_cov)
    target = getattr(device_lnpdf, name)(cases.SOURCES["logit"], d, data, params=ref.tgt.params(), batch_size=batch_size, seed=9,
                                         use_own_batch_per_sample=True)
    g = GMMVI.build_from_config(c, target, wrapper)
    assert g.model.diagonal_covs and g.sample_db.diagonal_covariances and not g._fast_path.eligible()
    assert not hasattr(target, "_fast_path_target")
    return ref, target, o, g, k * s


CLASSES = [("DeviceDataLNPDF", "target_custom_data"), ("DeviceDataTapeLNPDF", "target_custom_data_tape")]


@pytest.mark.parametrize("name,op", CLASSES)
def test_diagonal_stein_iteration_with_own_batches(ctx, monkeypatch, name, op):
    """logit at D = 20, T = 40, B = 8, three iterations against the fp64 oracle whose target is the per-sample restatement
    following the same call counter: sample n of iteration i sees row n of data_minibatch_rows_per_sample(seed, i, N, 8, 40)."""
    from gmmvi_amd import hip_ops
    ref, target, o, g, per_iter = _diagonal_pair(name, 20, 8)
    seen = []
    real = getattr(hip_ops, op)

    def recording(c, handle, params, data, x, want_grad=True, **kw):
        seen.append((kw["call"], kw["batch_size"], kw["seed"], kw.get("own_batches"), bool(want_grad), x.shape[0]))
        return real(c, handle, params, data, x, want_grad, **kw)

    monkeypatch.setattr(hip_ops, op, recording)

    def each(it):
        assert target.call_count == it + 1 == ref.call_count

    tape_mode._follow(o, g, 3, 20, each)
    assert seen == [(i, 8, 9, True, True, per_iter) for i in range(3)], seen
    # at a call, the device gives what the restatement gives at that call
    x = np.random.default_rng(4).normal(size=(65, 20)).astype(np.float32) * 0.5
    assert ref.call_count == 3
    lp64, g64 = ref.evaluate(x.astype(np.float64))
    lp32, g32 = ref.as_dtype(np.float32).evaluate(x)
    lp, grad = target.log_density_and_grad(x)
    _check(f"{name}, own batches of call 3", lp.numpy(), grad.numpy(), lp64, g64, lp32, g32)
    assert target.call_count == 4 and seen[-1] == (3, 8, 9, True, True, 65)


@pytest.mark.parametrize("name,op", CLASSES)
def test_gradient_free_estimator_evaluates_values_only(ctx, monkeypatch, name, op):
    """Under DiagonalMoreNgEstimator the classes are asked for values alone, own batches included."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import DiagonalMoreNgEstimator
    d = 6
    data = tape_mode._logit_rows(np.random.default_rng(17), 40, d)
    target = getattr(device_lnpdf, name)(cases.SOURCES["logit"], d, data, params=[0.25, 2.0], batch_size=8, seed=9,
                                         use_own_batch_per_sample=True)
    wanted = []
    real = getattr(hip_ops, op)

    def recording(c, handle, params, dd, x, want_grad=True, **kw):
        wanted.append((bool(want_grad), kw.get("own_batches")))
        return real(c, handle, params, dd, x, want_grad, **kw)

    monkeypatch.setattr(hip_ops, op, recording)
    g = hand._build_one_component(target, d, "MORE", True)
    assert type(g.ng_estimator) is DiagonalMoreNgEstimator and g.ng_estimator.uses_target_gradients is False
    (_, launches) = tape_mode._launches(ctx, lambda: [g.train_iter() for _ in range(3)], TAGS["data"])
    assert wanted == [(False, True)] * 3, wanted
    assert launches == 3 and target.call_count == 3
    assert int(g.sample_db.num_samples_written) == 3 * hand.E2E_SAMPLES
