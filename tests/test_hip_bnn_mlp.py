"""GPU tests of the generic Bayesian-neural-network target (csrc/bnn_mlp.hip): the kernel against the fp64 reference on the
same minibatches with the bound of test_hip_bnn_classifier.py (16 times the error of the fp32 NumPy evaluation of the same
formula, here on the same case), reproducibility, labels out of range, the arguments, the forward-only prediction, the
call counter, the agreement with the two specialised kernels on their network shapes and two short trajectories against
the fp64 oracle.

Every case prints the kernel's and the fp32 NumPy mode's errors and their ratio before it asserts; DESIGN.md 4, "Generic
BNN", records the worst ratios once a GPU run exists."""
import numpy as np
import pytest

import bnn_mlp_cases as cases
from bnn_classifier_ref import separable_data
from bnn_mlp_ref import BNNMlpRef, num_parameters
from helpers import samtron_config
from oracle import train as otrain

pytestmark = pytest.mark.gpu

E32_FACTOR = 16.0                                             # another summation order over up to 1024 x 1024 terms
WINE_LP_BOUND, WINE_GRAD_BOUND = 8e-6, 1.3e-5                 # test_hip_bnn.py's bounds of csrc/bnn.hip
MNIST_LP_BOUND, MNIST_GRAD_BOUND = 1.2e-5, 2.2e-5             # test_hip_bnn_classifier.py's bounds of csrc/bnn_classifier.hip
MSE, CE = cases.MSE, cases.CE
_kernel = {}                                                  # case name -> (lp, grad) of the kernel


def _ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def _run(case, X, y, W, seed=cases.SEED, call=cases.CALL, B=None, want_grad=True, s=cases.SCALING, sd=cases.PRIOR_STD):
    from gmmvi_amd import hip_ops
    ctx = _ctx()
    yd = ctx.asarray(y, np.float32 if case["loss"] == MSE else np.int32)
    lp, g = hip_ops.target_mlp(ctx, ctx.asarray(X), yd, case["hidden"], case["acts"], case["loss"], case["C"], seed, call,
                               case["B"] if B is None else B, s, sd, ctx.asarray(np.asarray(W, np.float32)),
                               want_grad=want_grad)
    return lp.numpy(), (g.numpy() if g is not None else None)


def _kernel_result(case):
    if case["name"] not in _kernel:
        b = cases.build(case)
        _kernel[case["name"]] = _run(case, b["X"], b["y"], b["W"])
    return _kernel[case["name"]]


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=lambda c: c["name"])
def test_kernel_matches_fp64_reference(case):
    """Per case: the kernel's error against fp64 stays below 16 times that of the fp32 NumPy mode of the same reference on
    the same weights and rows, for lp and for the gradient; lp alone is bitwise the lp of the call with the gradient."""
    b = cases.build(case)
    lp, g = _kernel_result(case)
    assert lp.shape == (case["N"],) and g.shape == (case["N"], b["ref"].D)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    e_lp, e_g = cases.errors(lp, g, b["lp64"], b["g64"])
    e_lp32, e_g32 = cases.errors(b["lp32"].astype(np.float64), b["g32"].astype(np.float64), b["lp64"], b["g64"])
    print(f"{case['name']}: kernel lp {e_lp:.2e} grad {e_g:.2e}, fp32 NumPy lp {e_lp32:.2e} grad {e_g32:.2e}, ratios "
          f"{e_lp / max(e_lp32, 1e-300):.2f} {e_g / max(e_g32, 1e-300):.2f}")
    assert e_lp <= E32_FACTOR * e_lp32, f"lp relative error {e_lp:.2e} > 16 x {e_lp32:.2e}"
    assert e_g <= E32_FACTOR * e_g32, f"gradient relative error {e_g:.2e} > 16 x {e_g32:.2e}"
    lp2, g2 = _run(case, b["X"], b["y"], b["W"], want_grad=False)
    assert g2 is None
    np.testing.assert_array_equal(lp2, lp)                   # the log density alone: the same sums in the same order


def test_kernel_is_bitwise_reproducible_and_keyed_by_seed_and_call():
    case = cases.CASES[5]                                    # three hidden layers, two chunks
    b = cases.build(case)
    a = _kernel_result(case)
    again = _run(case, b["X"], b["y"], b["W"])
    np.testing.assert_array_equal(a[0], again[0])
    np.testing.assert_array_equal(a[1], again[1])
    c = _run(case, b["X"], b["y"], b["W"], call=cases.CALL + 1)
    d = _run(case, b["X"], b["y"], b["W"], seed=cases.SEED + 1)
    assert np.all(a[0] != c[0]) and np.all(a[0] != d[0])


def test_label_out_of_range_selects_no_logit():
    """Rows whose label lies outside [0, C) keep logsumexp(l) as their loss (no logit is subtracted, none is indexed)."""
    case = cases.CASES[3]                                    # C = 16, B = 64
    b = cases.build(case)
    y_bad = b["y"].copy()
    bad = np.arange(case["T"]) % 3 == 0
    y_bad[bad] = np.where(np.arange(case["T"])[bad] % 2 == 0, 16, -5)
    lp, g = _run(case, b["X"], y_bad, b["W"])
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    y_zero = np.where(bad, 0, b["y"])
    ref = cases.make_ref(case, b["X"], y_zero)
    lp_zero, _ = ref.evaluate_rows(b["W"].astype(np.float64), b["rows"], want_grad=False)
    expect = np.empty_like(lp_zero)
    for i in range(case["N"]):
        r = b["rows"][i]
        logits = ref.forward(b["W"][i].astype(np.float64), ref.X[r])[1][-1]
        expect[i] = lp_zero[i] - cases.SCALING * (case["T"] / case["B"]) * np.sum(logits[bad[r], 0])
    np.testing.assert_allclose(lp, expect, rtol=1e-5)


def _desc(n_layers, widths, acts, loss):
    from gmmvi_amd import _lib
    d = _lib.MlpDesc()
    d.n_layers = n_layers
    for i, w in enumerate(widths):
        d.widths[i] = w
    for i, a in enumerate(acts):
        d.activations[i] = a
    d.loss = loss
    return d


def test_kernel_arguments():
    """Every limit of the C ABI answers GMMVI_ERR_ARG (-2) with a message that names it, and raises ValueError in Python."""
    from gmmvi_amd import hip_ops
    ctx = _ctx()
    X = ctx.asarray(np.zeros((1100, 1024), np.float32))
    y = ctx.asarray(np.zeros(1100, np.int32), np.int32)
    W = ctx.asarray(np.zeros((2, 131072), np.float32))
    lp = ctx.empty((2,))
    f, p = ctx.lib.gmmvi_target_mlp, ctx.lib.gmmvi_mlp_predict
    good = _desc(2, (11, 8, 3), (2, 0), 1)
    assert f(ctx.handle, good, 40, X.ptr, y.ptr, 0, 0, 8, 1.0, 1.0, W.ptr, 0, None, None) == 0                # N == 0: OK
    top = _desc(4, (600, 128, 128, 128, 16), (3, 1, 2, 0), 1)                                                   # D = 112 016
    assert f(ctx.handle, top, 1100, X.ptr, y.ptr, 0, 0, 1024, 1.0, 1.0, W.ptr, 2, lp.ptr, None) == 0
    bad_nets = [(_desc(1, (11, 3), (0,), 1), "n_layers"), (_desc(5, (11, 8, 8, 8, 8), (2, 2, 2, 2), 1), "n_layers"),
                (_desc(2, (0, 8, 3), (2, 0), 1), "1024"), (_desc(2, (1025, 8, 3), (2, 0), 1), "1024"),
                (_desc(2, (11, 0, 3), (2, 0), 1), "128"), (_desc(2, (11, 129, 3), (2, 0), 1), "128"),
                (_desc(3, (11, 8, 129, 3), (2, 2, 0), 1), "128"), (_desc(2, (11, 8, 1), (2, 0), 1), "16"),
                (_desc(2, (11, 8, 17), (2, 0), 1), "16"), (_desc(2, (11, 8, 2), (2, 0), 0), "one output"),
                (_desc(2, (11, 8, 3), (4, 0), 1), "activation"), (_desc(2, (11, 8, 3), (-1, 0), 1), "activation"),
                (_desc(2, (11, 8, 3), (2, 2), 1), "linear"), (_desc(2, (11, 8, 3), (2, 0), 2), "loss"),
                (_desc(3, (1024, 128, 128, 3), (2, 2, 0), 1), "GMMVI_MAX_DIM_DIAG")]
    out = ctx.empty((2, 40, 16))
    for net, word in bad_nets:
        assert f(ctx.handle, net, 40, X.ptr, y.ptr, 0, 0, 8, 1.0, 1.0, W.ptr, 2, lp.ptr, None) == -2, word
        assert word in ctx.lib.gmmvi_last_error(ctx.handle).decode(), word
        assert p(ctx.handle, net, W.ptr, 2, X.ptr, 40, out.ptr) == -2, word
        assert word in ctx.lib.gmmvi_last_error(ctx.handle).decode(), word
    for T, B, sd, word in ((40, 0, 1.0, "B"), (40, 41, 1.0, "B"), (1100, 1025, 1.0, "1024"), (0, 1, 1.0, "T"),
                           (40, 8, 0.0, "prior_std")):
        assert f(ctx.handle, good, T, X.ptr, y.ptr, 0, 0, B, 1.0, sd, W.ptr, 2, lp.ptr, None) == -2, (T, B, sd)
        assert word in ctx.lib.gmmvi_last_error(ctx.handle).decode(), word
    assert f(ctx.handle, None, 40, X.ptr, y.ptr, 0, 0, 8, 1.0, 1.0, W.ptr, 2, lp.ptr, None) == -2
    assert p(ctx.handle, good, W.ptr, 0, X.ptr, 40, out.ptr) == 0                                             # S == 0: OK
    ctx.sync()
    # the Python wrapper refuses the same limits before any launch
    Xs, ys = ctx.asarray(np.zeros((40, 11), np.float32)), ctx.asarray(np.zeros(40, np.int32), np.int32)
    w = ctx.asarray(np.zeros((2, num_parameters(11, (8,), 3)), np.float32))
    for hidden, acts, loss, c, B, sd in (((129,), ("relu", "linear"), CE, 3, 8, 1.), ((), ("linear",), CE, 3, 8, 1.),
                                         ((8,), ("relu", "relu"), CE, 3, 8, 1.), ((8,), ("relu", "linear"), CE, 17, 8, 1.),
                                         ((8,), ("relu", "linear"), CE, 3, 41, 1.), ((8,), ("relu", "linear"), CE, 3, 8, 0.),
                                         ((8,), ("gelu", "linear"), CE, 3, 8, 1.), ((8,), ("relu", "linear"), "hinge", 3, 8, 1.)):
        with pytest.raises(ValueError):
            hip_ops.target_mlp(ctx, Xs, ys, hidden, acts, loss, c, 0, 0, B, 1., sd, w)
    with pytest.raises(ValueError):
        hip_ops.mlp_predict(ctx, (129,), ("relu", "linear"), CE, 3, w, Xs)


def test_predict_matches_reference_forward_pass():
    from gmmvi_amd import hip_ops
    ctx = _ctx()
    rng = np.random.default_rng(3)
    for F, hidden, acts, loss, C, shapes in (
            (33, (17, 16), ("tanh", "sigmoid", "linear"), MSE, 1, ((1, 1), (9, 65), (5, 300))),
            (65, (128, 15, 64), ("relu", "linear", "tanh", "linear"), CE, 16, ((3, 64), (2, 130))),
            (784, (128,), ("relu", "linear"), CE, 10, ((3, 200),))):
        ref = BNNMlpRef(np.zeros((1, F)), np.zeros(1), hidden, acts, loss, num_classes=C)
        for s, m in shapes:
            W = (rng.normal(size=(s, ref.D)) * (2.0 / np.sqrt(F))).astype(np.float32)
            X = rng.normal(size=(m, F)).astype(np.float32)
            out = hip_ops.mlp_predict(ctx, hidden, acts, loss, C, ctx.asarray(W), ctx.asarray(X)).numpy()
            exp = ref.predict(W.astype(np.float64), X.astype(np.float64))
            assert out.shape == ((s, m) if loss == MSE else (s, m, C))
            np.testing.assert_allclose(out, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())


# ---- the LNPDF ---------------------------------------------------------------------------------------------------------
def test_call_counter_advances_as_specified():
    from gmmvi_amd.experiments.target_distributions.bnn import BNN_LNPDF
    case = cases.CASES[4]                                    # (tanh, relu) classifier, C = 2
    b = cases.build(case)
    make = lambda: BNN_LNPDF(features=b["X"], labels=b["y"], hidden_units=case["hidden"], activations=case["acts"], loss=CE,
                             num_classes=2, likelihood_scaling=1., prior_std=1., batch_size=37, seed=10)
    t = make()
    assert t.seed == 10 and t.call_count == 0 and t.get_num_dimensions() == b["ref"].D
    W = (np.random.default_rng(1).normal(size=(50, b["ref"].D)) * 0.3).astype(np.float32)
    lp0 = t.log_density(W).numpy()
    assert t.call_count == 1
    lp1, g1 = t.log_density_and_grad(W)
    assert t.call_count == 2 and g1.shape == (50, b["ref"].D)
    assert np.all(lp0 != lp1.numpy())                        # the same weights on other minibatches
    t.log_density(np.zeros((0, t.get_num_dimensions()), np.float32))
    assert t.call_count == 2                                 # a call without samples draws no batches
    # call c of the target is the stream's call c
    ref = cases.make_ref(case, b["X"], b["y"], batch_size=37, seed=10, likelihood_scaling=1., prior_std=1.)
    from gmmvi_amd.experiments.target_distributions.bnn import minibatch_rows
    lp_ref, _ = ref.evaluate_rows(W.astype(np.float64), minibatch_rows(10, 1, 50, 37, case["T"]), want_grad=False)
    np.testing.assert_allclose(lp1.numpy(), lp_ref, rtol=2e-5)
    # a fresh target with the same seed reproduces the first call bit for bit
    np.testing.assert_array_equal(make().log_density(W).numpy(), lp0)
    # predict goes through the forward-only kernel
    out = t.predict(W[:3], b["X"][:70]).numpy()
    exp = ref.predict(W[:3], b["X"][:70])
    np.testing.assert_allclose(out, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())


# ---- the specialised kernels -------------------------------------------------------------------------------------------
def test_agrees_with_the_regression_kernel_on_the_wine_shape():
    """csrc/bnn.hip on the same rows: the two kernels differ by at most the sum of their bounds against fp64."""
    from gmmvi_amd import hip_ops
    case = cases.WINE_CASE
    b = cases.build(case)
    ctx = _ctx()
    lp, g = _kernel_result(case)
    lpo, go = hip_ops.target_bnn(ctx, ctx.asarray(b["X"]), ctx.asarray(b["y"]), (8, 8), cases.SEED, cases.CALL, case["B"],
                                 cases.SCALING, cases.PRIOR_STD, ctx.asarray(b["W"]))
    e_lp32, e_g32 = cases.errors(b["lp32"].astype(np.float64), b["g32"].astype(np.float64), b["lp64"], b["g64"])
    d_lp, d_g = cases.errors(lp, g, lpo.numpy().astype(np.float64), go.numpy().astype(np.float64))
    print(f"wine shape: generic against specialised lp {d_lp:.2e} grad {d_g:.2e}")
    assert d_lp <= E32_FACTOR * e_lp32 + WINE_LP_BOUND
    assert d_g <= E32_FACTOR * e_g32 + WINE_GRAD_BOUND


def test_agrees_with_the_classifier_kernel_on_the_mnist_shape():
    from gmmvi_amd import hip_ops
    case = cases.MNIST_CASE
    b = cases.build(case)
    ctx = _ctx()
    lp, g = _kernel_result(case)
    lpo, go = hip_ops.target_bnn_classifier(ctx, ctx.asarray(b["X"]), ctx.asarray(b["y"], np.int32), 128, 10, cases.SEED,
                                            cases.CALL, case["B"], cases.SCALING, cases.PRIOR_STD, ctx.asarray(b["W"]))
    e_lp32, e_g32 = cases.errors(b["lp32"].astype(np.float64), b["g32"].astype(np.float64), b["lp64"], b["g64"])
    d_lp, d_g = cases.errors(lp, g, lpo.numpy().astype(np.float64), go.numpy().astype(np.float64))
    print(f"mnist shape: generic against specialised lp {d_lp:.2e} grad {d_g:.2e}")
    assert d_lp <= E32_FACTOR * e_lp32 + MNIST_LP_BOUND
    assert d_g <= E32_FACTOR * e_g32 + MNIST_GRAD_BOUND


# ---- the iteration -----------------------------------------------------------------------------------------------------
def _trajectory(X, y, hidden, acts, loss, C, diag, batch_size=64):
    """test_hip_bnn_classifier.py's trajectory test: SAMTRON-style iterations on the modular path, the fp64 oracle on
    BNNMlpRef and the device on BNN_LNPDF draw the same samples and the same minibatches."""
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    from gmmvi_amd.experiments.target_distributions.bnn import BNN_LNPDF
    k, s, seed, iters = 3, 100, 10000, 6
    cfg = samtron_config(s, diag=True) if diag else samtron_config(s, initial_stepsize=1.0)
    ref = BNNMlpRef(X, y, hidden, acts, loss, num_classes=C, batch_size=batch_size, seed=seed)
    d = ref.D
    model = otrain.construct_initial_mixture(d, k, 0.0, 1.0, 1.0, np.random.default_rng(seed + 1), use_diagonal_covs=diag)
    o = otrain.OracleGMMVI(
        ref, model, temperature=cfg["temperature"], seed=seed,
        desired_samples_per_component=s, ratio_reused_samples_to_desired=0.0, ng_estimator="Stein",
        only_use_own_samples=False, use_self_normalized_importance_weights=True, updater="trust-region",
        component_stepsize_config=cfg["component_stepsize_adapter_config"], weight_updater="trust-region",
        weight_stepsize_config=cfg["weight_stepsize_adapter_config"], adaptive=None, max_reward_history_length=400,
        sample_selector="component-based", max_database_size=cfg["max_database_size"],
        host_rng=np.random.default_rng(seed))
    om = o.model.model
    m = (DiagonalGMM if diag else FullCovGMM)(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
    m.seed = seed
    target = BNN_LNPDF(features=X, labels=y, hidden_units=hidden, activations=acts, loss=loss, num_classes=C,
                       likelihood_scaling=1., prior_std=1., batch_size=batch_size, seed=seed)
    g = GMMVI.build_from_config(cfg, target, GmmWrapper(m, cfg["component_stepsize_adapter_config"]["initial_stepsize"],
                                                        1e-12, 400))
    assert g.model.diagonal_covs == diag and target.get_num_dimensions() == d
    worst = {}
    for it in range(iters):
        o.train_iter()
        g.train_iter()
        gm, omod = g.model, o.model
        tol = 2.0 * (5e-4 if it < 2 else 2e-3 * (1 + it))
        dev = {"means": np.abs(gm.means.numpy() - omod.means).max() / max(1.0, np.abs(omod.means).max()),
               "chols": np.abs(gm.chol_cov.numpy() - omod.chol_cov).max() / np.abs(omod.chol_cov).max()}
        for key, v in dev.items():
            worst[key] = max(worst.get(key, 0.0), v)
            assert v <= tol, f"iteration {it}: {key} deviates by {v:.3e} (> {tol:.1e})"
    print(f"trajectory {hidden} {acts} {loss} (diag={diag}): worst deviations {worst}")
    assert target.call_count == ref.call_count == iters                 # both sides consumed the same minibatches


def test_trajectory_tanh_regressor_full_covariance():
    rng = np.random.default_rng(42)
    X = rng.normal(size=(300, 5)).astype(np.float32)
    y = (np.tanh(X @ rng.normal(size=5)) + 0.1 * rng.normal(size=300)).astype(np.float32)
    assert num_parameters(5, (4,), 1) == 29
    _trajectory(X, y, (4,), ("tanh", "linear"), MSE, None, diag=False)


def test_trajectory_relu_classifier_diagonal():
    X, y = separable_data(300, 12, 3, np.random.default_rng(42))
    assert num_parameters(12, (8, 6), 3) == 179
    _trajectory(X, y, (8, 6), ("relu", "relu", "linear"), CE, 3, diag=True)
