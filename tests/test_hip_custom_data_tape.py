"""GPU tests of reverse-mode gradients of user-defined device targets summed over a data set
(csrc/custom_target_data_tape.inc, DeviceDataTapeLNPDF): the two kernels against fp64 at the seams of the 64-sample tile, of the
old cap of the forward mode, of the default tape capacity, of the row chunks and of the slabs, in full-data and in minibatch mode,
with tapes of different lengths in one wave; the value call bit for bit against the data mode; determinism; agreement across
chunk counts, slabs and with forward mode; the exact edge outputs of the sweep; capacity growth and the scratch budget; the
refusals in both directions; and the class in the modular iteration (diagonal Stein above the old cap, minibatches) and under a
gradient-free estimator.

Kernel bound: the rule of tests/test_hip_custom_target.py, unchanged (its _bound): the device's largest error against the fp64
NumPy restatement is at most 16 times the largest error of the fp32 NumPy restatement on the same inputs plus
4 * eps32 * max|reference|; for lp and the gradient of the gradient call and for lp of the value call.  Every case prints its
ratios before it asserts.  tests/test_custom_data_tape_host.py shows what that bound can see."""
import ctypes as C

import numpy as np
import pytest

import custom_data_tape_cases as cases
import test_hip_custom_data as data_mode
import test_hip_custom_target as hand
from gmmvi_amd import _lib
from helpers import samtron_config
from oracle import train as otrain
from test_hip_custom_target import SENTINEL, _bound

pytestmark = pytest.mark.gpu

ERR_ARG = -2
KERNEL_CASES = cases.kernel_cases()


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


_handles = {}


def _handle(ctx, name):
    from gmmvi_amd import hip_ops
    if name not in _handles:
        _handles[name] = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode="data_tape")
    return _handles[name]


def _launch(ctx, handle, tgt, x, want_grad, chunks=0, capacity=0, scratch=0):
    """gmmvi_target_custom_data_tape for the restatement ``tgt`` on outputs with CANARY_ROWS extra rows of SENTINEL behind them
    -> (rc, lp, grad | None); the extra rows are checked here: bit-unchanged."""
    n, d = x.shape
    t, c = tgt.data.shape
    xd, pd, dd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    lp = ctx.full((n + hand.CANARY_ROWS,), SENTINEL)
    grad = ctx.full((n + hand.CANARY_ROWS, d), SENTINEL) if want_grad else None
    mini = tgt.batch_size is not None
    rc = ctx.lib.gmmvi_target_custom_data_tape(ctx.handle, handle.handle, d, pd.ptr, dd.ptr, t, c, int(mini),
                                               tgt.batch_size if mini else t, tgt.seed, tgt.call_count, xd.ptr, n, lp.ptr,
                                               None if grad is None else grad.ptr, chunks, capacity, scratch)
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
    line = f"[custom_data_tape] {tag}: lp error {e_lp:.3e} (bound {b_lp:.3e}, {e_lp / b_lp:.3f} of it, ratio to fp32 NumPy {r_lp:.2f})"
    if g is not None:
        e_g, b_g, r_g = _bound(g, g64, g32)
        line += f", gradient error {e_g:.3e} (bound {b_g:.3e}, {e_g / b_g:.3f} of it, ratio {r_g:.2f})"
    print("\n" + line)
    assert np.all(np.isfinite(lp)) and (g is None or np.all(np.isfinite(g)))
    assert e_lp <= b_lp, f"{tag}: lp error {e_lp:.3e} > {b_lp:.3e}"
    if g is not None:
        assert e_g <= b_g, f"{tag}: gradient error {e_g:.3e} > {b_g:.3e}"


def _launches(ctx, call, tag="target_custom_data_tape"):
    """-> (result of call(), launches with the profiling tag ``tag`` it made)."""
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 1))
    try:
        out = call()
    finally:
        buf = C.create_string_buffer(1 << 16)
        ctx.check(ctx.lib.gmmvi_profile_report(ctx.handle, buf, len(buf)))
        ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 0))
    count = 0
    for line in buf.value.decode().splitlines():
        fields = line.split()
        if fields and fields[0] == tag:
            count += int(fields[1])
    return out, count


@pytest.mark.parametrize("c", KERNEL_CASES, ids=cases.case_id)
def test_kernel_matches_fp64_reference(ctx, c):
    from gmmvi_amd import hip_ops
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, c.name)
    second_attempt = c.d == 4096                                     # a tape beyond the default capacity
    if second_attempt:
        assert hip_ops.custom_tape_length(ctx, handle, c.d) == 0
    (rc, lp, g), launches = _launches(ctx, lambda: _launch(ctx, handle, tgt, x, True, c.chunks))
    assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
    _check(cases.case_id(c), lp, g, lp64, g64, lp32, g32)
    if second_attempt:
        assert launches == 2 and hip_ops.custom_tape_length(ctx, handle, c.d) >= 2 * c.d
    rc, lp_v, g_v = _launch(ctx, handle, tgt, x, False, c.chunks)
    assert rc == 0 and g_v is None
    _check(cases.case_id(c) + " values only", lp_v, None, lp64, g64, lp32, g32)


SEAM_CASE = cases.Case("logit", 17, 65, 67, 3, None, 0)
SEAM_MINIBATCH = cases.Case("student", 5, 65, 257, 0, 257, 3)


@pytest.mark.parametrize("c", [SEAM_CASE, SEAM_MINIBATCH], ids=cases.case_id)
def test_value_call_gives_the_bits_of_the_data_mode(ctx, c):
    tgt, x = cases.reference(c)[:2]
    for chunks in (c.chunks, 1):
        rc, lp, _ = _launch(ctx, _handle(ctx, c.name), tgt, x, False, chunks)
        rc_d, lp_d, _ = data_mode._launch(ctx, data_mode._handle(ctx, c.name), tgt, x, False, chunks)
        assert rc == 0 and rc_d == 0
        np.testing.assert_array_equal(lp.view(np.uint32), lp_d.view(np.uint32))


@pytest.mark.parametrize("c", [SEAM_CASE, SEAM_MINIBATCH], ids=cases.case_id)
def test_same_call_twice_gives_the_same_bits(ctx, c):
    tgt, x = cases.reference(c)[:2]
    handle = _handle(ctx, c.name)
    for chunks in (1, 3):
        _, lp_a, g_a = _launch(ctx, handle, tgt, x, True, chunks)
        _, lp_b, g_b = _launch(ctx, handle, tgt, x, True, chunks)
        np.testing.assert_array_equal(lp_a.view(np.uint32), lp_b.view(np.uint32))
        np.testing.assert_array_equal(g_a.view(np.uint32), g_b.view(np.uint32))


@pytest.mark.parametrize("c", [SEAM_CASE, SEAM_MINIBATCH], ids=cases.case_id)
def test_chunk_counts_agree_within_the_bound(ctx, c):
    """chunks = 1, 2, 3 each meet the kernel bound and differ from each other by no more than it (another chunk count adds the
    same terms in another order)."""
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, c.name)
    out = {}
    for chunks in (1, 2, 3):
        rc, lp, g = _launch(ctx, handle, tgt, x, True, chunks)
        assert rc == 0
        _check(f"{cases.case_id(c)} forced to {chunks} chunk(s)", lp, g, lp64, g64, lp32, g32)
        out[chunks] = (lp, g)
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    for a, b in ((1, 2), (1, 3), (2, 3)):
        d_lp = float(np.abs(out[a][0].astype(np.float64) - out[b][0]).max())
        d_g = float(np.abs(out[a][1].astype(np.float64) - out[b][1]).max())
        print(f"[custom_data_tape] chunks {a} against {b}: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the bound), the gradient "
              f"by {d_g:.3e} ({d_g / b_g:.3f})")
        assert d_lp <= b_lp and d_g <= b_g


def test_slabs_give_the_bits_of_one_launch(ctx):
    from gmmvi_amd import hip_ops
    c = cases.SLAB_CASE
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = _handle(ctx, c.name)
    rc, lp_one, g_one = _launch(ctx, handle, tgt, x, True)
    assert rc == 0
    _check(cases.case_id(c), lp_one, g_one, lp64, g64, lp32, g32)
    needed = hip_ops.custom_tape_length(ctx, handle, c.d)
    budget = 64 * (needed * _lib.CUSTOM_TAPE_RECORD_BYTES + 4 * c.d)             # one tile with one chunk
    assert hip_ops.custom_data_tape_plan(c.n, c.rows, c.d, needed, 0, budget) == (1, 5, 3, 1)
    (rc, lp, g), launches = _launches(ctx, lambda: _launch(ctx, handle, tgt, x, True, 0, 0, budget))
    assert rc == 0 and launches == 3
    np.testing.assert_array_equal(lp.view(np.uint32), lp_one.view(np.uint32))
    np.testing.assert_array_equal(g.view(np.uint32), g_one.view(np.uint32))


@pytest.mark.parametrize("c", [cases.Case("logit", 512, 65, 5, 0, None, 0), cases.Case("student", 17, 65, 67, 0, None, 0)],
                         ids=cases.case_id)
def test_forward_mode_and_reverse_mode_agree(ctx, c):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF, DeviceDataTapeLNPDF
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    fwd = DeviceDataLNPDF(cases.SOURCES[c.name], c.d, tgt.data, params=tgt.params())
    rev = DeviceDataTapeLNPDF(cases.SOURCES[c.name], c.d, tgt.data, params=tgt.params())
    lp_f, g_f = (a.numpy() for a in fwd.log_density_and_grad(x))
    lp_r, g_r = (a.numpy() for a in rev.log_density_and_grad(x))
    b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
    d_lp, d_g = float(np.abs(lp_f.astype(np.float64) - lp_r).max()), float(np.abs(g_f.astype(np.float64) - g_r).max())
    print(f"\n[custom_data_tape] {cases.case_id(c)} forward against reverse: lp differs by {d_lp:.3e} ({d_lp / b_lp:.3f} of the "
          f"bound), the gradient by {d_g:.3e} ({d_g / b_g:.3f})")
    assert d_lp <= b_lp and d_g <= b_g
    np.testing.assert_array_equal(fwd.log_density(x).numpy().view(np.uint32), rev.log_density(x).numpy().view(np.uint32))


EDGE_SRC = ("template <class T, class X> __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {\n"
            "    if (x[0] > 1.f) return x[1];\n"                      # an input
            "    if (x[0] < -1.f) return 3.f;\n"                      # a constant
            "    const T unused = x[0] * x[1];\n"                     # a record behind which the output does not stand
            "    const T out = x[2] * row[0];\n"
            "    const T late = out * x[1];\n"                        # and a record made after the output node
            "    if (gmmvi_value(late) + gmmvi_value(unused) == 12345.f) return late;\n"
            "    return out;\n}\n"
            "template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params) { return 0.f; }\n")


def test_output_that_is_an_input_or_a_constant(ctx):
    """The pattern of test_output_that_is_an_input_or_a_constant (tests/test_hip_custom_tape.py), summed over 3 rows with the
    factors 2, 2, 4: every product and every partial sum is exact (x + x + x is the correctly rounded 3 x, as 3.f * x is)."""
    from gmmvi_amd import hip_ops
    handle = hip_ops.custom_target_compile(ctx, EDGE_SRC, mode="data_tape")
    x = np.random.default_rng(3).normal(size=(130, 3)).astype(np.float32) * 2
    rows = np.array([[2.0], [2.0], [4.0]], np.float32)
    for chunks in (1, 3):
        lp, g = hip_ops.target_custom_data_tape(ctx, handle, None, ctx.asarray(rows), ctx.asarray(x), True, chunks=chunks)
        big, small = x[:, 0] > 1, x[:, 0] < -1
        want_lp = np.where(big, np.float32(3) * x[:, 1], np.where(small, np.float32(9), x[:, 2] * np.float32(8)))
        want_g = np.zeros_like(x)
        want_g[big, 1] = 3
        want_g[~big & ~small, 2] = 8
        assert big.any() and small.any() and (~big & ~small).any()
        np.testing.assert_array_equal(lp.numpy(), want_lp.astype(np.float32))
        np.testing.assert_array_equal(g.numpy(), want_g)


def test_capacity_growth_and_the_scratch_budget(ctx):
    from gmmvi_amd import hip_ops
    c = cases.Case("logit", 5, 65, 5, 0, None, 0)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    handle = hip_ops.custom_target_compile(ctx, cases.SOURCES["logit"] + "\n// capacity growth\n", mode="data_tape")
    assert hip_ops.custom_tape_length(ctx, handle, c.d) == 0
    (rc, lp, g), launches = _launches(ctx, lambda: _launch(ctx, handle, tgt, x, True, 0, 4))
    assert rc == 0 and launches == 2
    _check("capacity 4, second attempt", lp, g, lp64, g64, lp32, g32)
    needed = hip_ops.custom_tape_length(ctx, handle, c.d)
    assert needed > 4
    (rc, lp_b, g_b), launches = _launches(ctx, lambda: _launch(ctx, handle, tgt, x, True))
    assert rc == 0 and launches == 1
    np.testing.assert_array_equal(g_b.view(np.uint32), g.view(np.uint32))
    np.testing.assert_array_equal(lp_b.view(np.uint32), lp.view(np.uint32))
    # a budget that holds a tape of 4 records but not the needed one: refused with both byte counts, the context stays usable
    small = 64 * (4 * _lib.CUSTOM_TAPE_RECORD_BYTES + 4 * c.d)
    rc, _, _ = _launch(ctx, handle, tgt, x, True, 0, 4, small)
    assert rc == ERR_ARG
    message = ctx.lib.gmmvi_last_error(ctx.handle).decode()
    assert str(needed) in message and str(small) in message and str(64 * (needed * _lib.CUSTOM_TAPE_RECORD_BYTES + 4 * c.d)) in message
    rc, _, _ = _launch(ctx, handle, tgt, x, True, 0, 0, 64)
    assert rc == ERR_ARG and "64 bytes" in ctx.lib.gmmvi_last_error(ctx.handle).decode()
    rc, lp_v, _ = _launch(ctx, handle, tgt, x, False, 0, 0, 1)        # the value call needs no scratch budget
    assert rc == 0
    rc, lp_ok, g_ok = _launch(ctx, handle, tgt, x, True)
    assert rc == 0
    np.testing.assert_array_equal(g_ok.view(np.uint32), g.view(np.uint32))


def test_refusals_in_both_directions(ctx):
    from gmmvi_amd import hip_ops
    import custom_tape_cases as tape_cases
    lib = ctx.lib
    c = cases.Case("logit", 5, 8, 9, 0, 5, 0)
    tgt, x = cases.build_case(c)
    mine = _handle(ctx, "logit")
    n, d, t, cols = 8, 5, 9, 6
    xd, pd, dd = ctx.asarray(x), ctx.asarray(tgt.params()), ctx.asarray(tgt.data)
    lp, grad = ctx.full((n,), SENTINEL), ctx.full((n, d), SENTINEL)

    def call(D=d, data=dd.ptr, T=t, Cc=cols, mini=1, B=5, X=xd.ptr, N=n, out=lp.ptr, g=grad.ptr, h=mine.handle, chunks=0, cap=0):
        return lib.gmmvi_target_custom_data_tape(ctx.handle, h, D, pd.ptr, data, T, Cc, mini, B, 9, 0, X, N, out, g, chunks, cap, 0)

    def last():
        return lib.gmmvi_last_error(ctx.handle).decode()

    assert call(B=0) == ERR_ARG and "B = 0" in last()
    assert call(B=10) == ERR_ARG and "B = 10" in last() and "T = 9" in last()
    assert call(mini=0, B=10) == ERR_ARG
    assert call(Cc=0) == ERR_ARG and "C = 0" in last()
    assert call(T=0) == ERR_ARG and "T = 0" in last()
    assert call(T=2 ** 31) == ERR_ARG and "2^31" in last()
    for kw in (dict(data=None), dict(N=0), dict(X=None), dict(out=None), dict(D=0), dict(D=_lib.MAX_DIM_DIAG + 1), dict(mini=2),
               dict(chunks=-1), dict(cap=-1), dict(h=None)):
        assert call(**kw) == ERR_ARG, kw
    # the other four kinds of handle
    others = (hand._handle(ctx, "rosenbrock"), hip_ops.custom_target_compile(ctx, tape_cases.CHAIN_SRC, mode="autodiff"),
              data_mode._handle(ctx, "logit"), hip_ops.custom_target_compile(ctx, tape_cases.CHAIN_SRC, mode="tape"))
    assert len({h.ptr for h in others} | {mine.ptr}) == 5
    for h in others:
        for g in (grad.ptr, None):
            assert call(h=h.handle, g=g) == ERR_ARG and "gmmvi_custom_target_compile_data_tape" in last()
    # the other three entries refuse a handle of this mode and name the entry that takes it
    for g in (grad.ptr, None):
        assert lib.gmmvi_target_custom(ctx.handle, mine.handle, d, pd.ptr, xd.ptr, n, lp.ptr, g, 0) == ERR_ARG
        assert "gmmvi_target_custom_data_tape" in last()
        assert lib.gmmvi_target_custom_data(ctx.handle, mine.handle, d, pd.ptr, dd.ptr, t, cols, 1, 5, 9, 0, xd.ptr, n, lp.ptr, g, 0) == ERR_ARG
        assert "gmmvi_target_custom_data_tape" in last()
        assert lib.gmmvi_target_custom_tape(ctx.handle, mine.handle, d, pd.ptr, xd.ptr, n, lp.ptr, g, 0, 0) == ERR_ARG
        assert "gmmvi_target_custom_data_tape" in last()
    with pytest.raises(_lib.GmmviError, match="gmmvi_target_custom_data_tape"):
        hip_ops.target_custom_data(ctx, mine, pd, dd, xd, True)
    with pytest.raises(ValueError, match="mode"):
        hip_ops.custom_target_compile(ctx, cases.SOURCES["logit"], mode="reverse")
    ctx.check(lib.gmmvi_sync(ctx.handle))
    bits = np.array(SENTINEL).view(np.uint32)
    assert np.all(lp.numpy().view(np.uint32) == bits) and np.all(grad.numpy().view(np.uint32) == bits)
    # the module cache keys on the mode, and the context works afterwards
    assert hip_ops.custom_target_compile(ctx, cases.SOURCES["logit"], mode="data_tape").ptr == mine.ptr
    assert call() == 0
    ctx.check(lib.gmmvi_sync(ctx.handle))
    lp64, g64 = tgt.evaluate(x.astype(np.float64))
    lp32, g32 = cases.fp32_twin(tgt).evaluate(x)
    _check("after the refusals", lp.numpy(), grad.numpy(), lp64, g64, lp32, g32)


# ---- the iteration -----------------------------------------------------------------------------------------------------
def _logit_rows(rng, t, d):
    return np.concatenate([rng.normal(size=(t, d)) / np.sqrt(d), rng.choice([-1.0, 1.0], size=(t, 1))], axis=1).astype(np.float32)


def _diagonal_pair(d, batch_size):
    """The set-up of test_diagonal_stein_iteration_on_the_chain_above_the_forward_cap (tests/test_hip_custom_tape.py) on logit
    over 40 rows: a diagonal-covariance model, the Stein estimator, the KL trust region, K = 3, 40 samples per component."""
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataTapeLNPDF
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    k, s, seed = 3, 40, 11
    cfg = samtron_config(s, diag=True)
    data = _logit_rows(np.random.default_rng(17), 40, d)
    ref = cases.base.Logit(data, [0.25, 2.0], batch_size=batch_size, seed=9)
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
    target = DeviceDataTapeLNPDF(cases.SOURCES["logit"], d, data, params=ref.params(), batch_size=batch_size, seed=9)
    g = GMMVI.build_from_config(c, target, wrapper)
    assert g.model.diagonal_covs and g.sample_db.diagonal_covariances and not g._fast_path.eligible()
    assert not hasattr(target, "_fast_path_target")
    return ref, target, o, g, k * s


def _follow(o, g, iters, d, each=lambda it: None):
    for it in range(iters):
        info = o.train_iter()
        g.train_iter()
        each(it)
        gm = g.model
        assert gm.num_components == o.model.num_components
        tol = 2e-3 * (1 + it)
        dm = np.abs(gm.means.numpy() - o.model.means).max() / max(1.0, np.abs(o.model.means).max())
        dc = np.abs(gm.chol_cov.numpy() - o.model.chol_cov).max() / np.abs(o.model.chol_cov).max()
        dw = np.abs(np.exp(gm.log_weights.numpy()) - o.model.weights).max()
        print(f"\n[custom_data_tape] logit D={d} iteration {it}: means {dm:.2e} sigma {dc:.2e} weights {dw:.2e} (tolerance {tol:.1e})")
        assert dm <= tol, it
        assert dc <= tol, it
        assert dw <= tol, it
        if "success" in info and g.ng_based_updater.last_success is not None:
            np.testing.assert_array_equal(g.ng_based_updater.last_success.numpy().astype(bool), info["success"])
        np.testing.assert_allclose(gm.num_received_updates.numpy(), o.model.num_received_updates)


def test_diagonal_stein_iteration_above_the_forward_cap():
    """logit at D = 600, T = 40 (the forward mode stops at 512), three iterations against the fp64 oracle on the restatement,
    identical draws."""
    ref, target, o, g, per_iter = _diagonal_pair(600, None)
    _follow(o, g, 3, 600)
    assert int(g.sample_db.num_samples_written) == 3 * per_iter and target.call_count == 0


def test_diagonal_stein_iteration_with_minibatches(ctx, monkeypatch):
    """The same at D = 20 with batch_size = 8: the call counter advances once per evaluation, and iteration i evaluates the
    rows of data_minibatch_rows(seed, i, ...): the oracle's target is the restatement at the same call."""
    from gmmvi_amd import hip_ops
    ref, target, o, g, per_iter = _diagonal_pair(20, 8)
    seen = []
    real = hip_ops.target_custom_data_tape

    def recording(c, handle, params, data, x, want_grad=True, **kw):
        seen.append((kw["call"], kw["batch_size"], kw["seed"], bool(want_grad)))
        return real(c, handle, params, data, x, want_grad, **kw)

    monkeypatch.setattr(hip_ops, "target_custom_data_tape", recording)

    def each(it):
        assert target.call_count == it + 1 == ref.call_count

    _follow(o, g, 3, 20, each)
    assert seen == [(i, 8, 9, True) for i in range(3)], seen
    # at a call, the device gives what the restatement gives at that call
    x = np.random.default_rng(4).normal(size=(65, 20)).astype(np.float32) * 0.5
    at3 = ref.as_dtype(np.float64)
    assert at3.call_count == 3
    lp64, g64 = at3.evaluate(x.astype(np.float64))
    lp32, g32 = cases.fp32_twin(at3).evaluate(x)
    lp, grad = target.log_density_and_grad(x)
    _check("minibatch of call 3", lp.numpy(), grad.numpy(), lp64, g64, lp32, g32)
    assert target.call_count == 4 and seen[-1] == (3, 8, 9, True)
    lp_full = target.log_density_full(x).numpy()
    full = ref.full()
    _check("log_density_full", lp_full, None, full.evaluate(x.astype(np.float64))[0], None, cases.fp32_twin(full).evaluate(x)[0], None)
    assert target.call_count == 4


def test_gradient_free_estimator_evaluates_values_only(ctx, monkeypatch):
    """Under DiagonalMoreNgEstimator the class is asked for values alone: no call records a tape."""
    from gmmvi_amd import hip_ops
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataTapeLNPDF
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import DiagonalMoreNgEstimator
    d = 6
    data = _logit_rows(np.random.default_rng(17), 40, d)
    target = DeviceDataTapeLNPDF(cases.SOURCES["logit"], d, data, params=[0.25, 2.0], batch_size=8, seed=9)
    wanted = []
    real = hip_ops.target_custom_data_tape

    def recording(c, handle, params, dd, x, want_grad=True, **kw):
        wanted.append(bool(want_grad))
        return real(c, handle, params, dd, x, want_grad, **kw)

    monkeypatch.setattr(hip_ops, "target_custom_data_tape", recording)
    g = hand._build_one_component(target, d, "MORE", True)
    assert type(g.ng_estimator) is DiagonalMoreNgEstimator and g.ng_estimator.uses_target_gradients is False
    (_, launches) = _launches(ctx, lambda: [g.train_iter() for _ in range(3)])
    assert len(wanted) == 3 and not any(wanted), wanted
    assert launches == 0 and target.call_count == 3
    assert int(g.sample_db.num_samples_written) == 3 * hand.E2E_SAMPLES
