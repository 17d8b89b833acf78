"""GPU tests of the WINE Bayesian-neural-network target (csrc/bnn.hip): the kernel against the fp64 reference on the
same minibatches, the call counter, the forward-only prediction, the trajectory against the fp64 oracle, and the
experiment end to end through the public surface."""
import numpy as np
import pytest

from bnn_ref import BNNRef, load_wine, stream_rows, write_dataset_dir
from helpers import samtron_config
from oracle import train as otrain

pytestmark = pytest.mark.gpu

# about twice the worst relative errors of the first GPU run (lp 4.0e-6 at B = 1, grad 6.4e-6 at F = 20, H = (16, 3))
LP_BOUND, GRAD_BOUND = 8e-6, 1.3e-5


@pytest.fixture(scope="module")
def wine():
    return load_wine()


def _run_kernel(X, y, hidden, seed, call, B, s, sd, W, want_grad=True):
    from gmmvi_amd import hip_ops
    from gmmvi_amd.device import get_context
    ctx = get_context()
    lp, g = hip_ops.target_bnn(ctx, ctx.asarray(np.asarray(X, np.float32)), ctx.asarray(np.asarray(y, np.float32)), hidden,
                               seed, call, B, s, sd, ctx.asarray(np.asarray(W, np.float32)), want_grad=want_grad)
    return lp.numpy(), (g.numpy() if g is not None else None)


def _check_kernel(X, y, hidden, seed, call, B, W, worst, s=1.0, sd=1.0):
    X32, y32, W32 = np.asarray(X, np.float32), np.asarray(y, np.float32), np.asarray(W, np.float32)
    ref = BNNRef(X32, y32, hidden_units=hidden, likelihood_scaling=s, prior_std=sd, batch_size=B, seed=seed)
    rows = stream_rows(seed, call, W.shape[0], B, X.shape[0])
    lp_ref, g_ref = ref.evaluate_rows(W32.astype(np.float64), rows)
    lp, g = _run_kernel(X32, y32, hidden, seed, call, B, s, sd, W32)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    err = np.abs(lp - lp_ref) / np.maximum(np.abs(lp_ref), 1.0)
    gerr = np.abs(g - g_ref).max(1) / np.maximum(np.abs(g_ref).max(1), 1e-30)
    worst["lp"] = max(worst.get("lp", 0.0), float(err.max()))
    worst["grad"] = max(worst.get("grad", 0.0), float(gerr.max()))
    assert err.max() <= LP_BOUND, f"lp relative error {err.max():.2e}"
    assert gerr.max() <= GRAD_BOUND, f"gradient relative error {gerr.max():.2e}"
    lp2, g2 = _run_kernel(X32, y32, hidden, seed, call, B, s, sd, W32, want_grad=False)
    assert g2 is None
    np.testing.assert_array_equal(lp2, lp)                   # the log density alone: the same sums in the same order


@pytest.mark.parametrize("B", [1, 128, 2938])
def test_kernel_matches_fp64_reference_on_wine(wine, B):
    X, y = wine["features_train"], wine["labels_train"]
    rng = np.random.default_rng(B)
    worst = {}
    for n in (1, 63, 400, 2048):
        for scale in (1.0, 0.3):                             # the yml initialisation (prior_scale 1) and a narrower one
            W = rng.normal(size=(n, 177)) * scale
            _check_kernel(X, y, (8, 8), seed=10000, call=n, B=B, W=W, worst=worst, s=1.0, sd=1.0)
    print(f"WINE B = {B}: worst relative errors {worst}")


@pytest.mark.parametrize("F,H1,H2,T", [(1, 1, 1, 5), (3, 5, 2, 37), (11, 8, 8, 300), (20, 16, 3, 130), (32, 16, 16, 257)])
def test_kernel_matches_fp64_reference_synthetic(F, H1, H2, T):
    rng = np.random.default_rng(F * 100 + H1 * 10 + H2)
    X = rng.normal(size=(T, F))
    y = rng.normal(size=T) * 2.0 + 3.0
    d = F * H1 + H1 + H1 * H2 + H2 + H2 + 1
    worst = {}
    for B in sorted({1, min(T, 37), min(T, 128), T}):
        for n in (1, 130):
            W = rng.normal(size=(n, d)) * 0.7
            _check_kernel(X, y, (H1, H2), seed=7, call=3, B=B, W=W, worst=worst, s=0.5, sd=2.0)
    print(f"F={F} H=({H1},{H2}) T={T}: worst relative errors {worst}")


def test_kernel_is_bitwise_reproducible_and_keyed_by_seed_and_call(wine):
    X, y = wine["features_train"], wine["labels_train"]
    W = np.random.default_rng(0).normal(size=(400, 177))
    a = _run_kernel(X, y, (8, 8), 5, 9, 128, 1.0, 1.0, W)
    b = _run_kernel(X, y, (8, 8), 5, 9, 128, 1.0, 1.0, W)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    c = _run_kernel(X, y, (8, 8), 5, 10, 128, 1.0, 1.0, W)
    d = _run_kernel(X, y, (8, 8), 6, 9, 128, 1.0, 1.0, W)
    assert np.all(a[0] != c[0]) and np.all(a[0] != d[0])


def test_kernel_arguments():
    from gmmvi_amd import _lib
    from gmmvi_amd.device import get_context
    ctx = get_context()
    X = ctx.asarray(np.zeros((40, 32), np.float32))
    y = ctx.asarray(np.zeros(40, np.float32))
    W = ctx.asarray(np.zeros((5, 1000), np.float32))
    lp = ctx.empty((5,))
    f = ctx.lib.gmmvi_target_bnn
    assert f(ctx.handle, 11, 8, 8, 40, X.ptr, y.ptr, 0, 0, 8, 1.0, 1.0, W.ptr, 0, None, None) == 0          # N == 0: OK
    for F, H1, H2, T, B, sd in ((0, 8, 8, 40, 8, 1.0), (33, 8, 8, 40, 8, 1.0), (11, 0, 8, 40, 8, 1.0),
                                (11, 17, 8, 40, 8, 1.0), (11, 8, 0, 40, 8, 1.0), (11, 8, 17, 40, 8, 1.0),
                                (11, 8, 8, 40, 0, 1.0), (11, 8, 8, 40, 41, 1.0), (11, 8, 8, 0, 1, 1.0),
                                (11, 8, 8, 40, 8, 0.0)):
        assert f(ctx.handle, F, H1, H2, T, X.ptr, y.ptr, 0, 0, B, 1.0, sd, W.ptr, 5, lp.ptr, None) == -2
    out = ctx.empty((5, 40))
    p = ctx.lib.gmmvi_bnn_predict
    assert p(ctx.handle, 11, 8, 8, W.ptr, 0, X.ptr, 40, out.ptr) == 0
    for F, H1, H2 in ((0, 8, 8), (33, 8, 8), (11, 17, 8), (11, 8, 0)):
        assert p(ctx.handle, F, H1, H2, W.ptr, 5, X.ptr, 40, out.ptr) == -2
    ctx.sync()
    assert _lib.EXPORTED_SYMBOLS.count("gmmvi_target_bnn") == 1 and _lib.EXPORTED_SYMBOLS.count("gmmvi_bnn_predict") == 1


# ---- the LNPDF ---------------------------------------------------------------------------------------------------------
def test_call_counter_advances_as_specified(wine, tmp_path):
    from gmmvi_amd.experiments.target_distributions.bnn import BNN_WINE
    d = write_dataset_dir(tmp_path)
    t = BNN_WINE(dataset_seed=10, likelihood_scaling=1., prior_std=1., batch_size=128, dataset_dir=d)
    assert t.seed == 10 and t.call_count == 0
    W = np.random.default_rng(1).normal(size=(50, 177)).astype(np.float32)
    lp0 = t.log_density(W).numpy()
    assert t.call_count == 1
    lp1, g1 = t.log_density_and_grad(W)
    assert t.call_count == 2
    assert np.all(lp0 != lp1.numpy())                        # the same weights on other minibatches
    t.log_density(np.zeros((0, 177), np.float32))
    assert t.call_count == 2                                 # a call without samples draws no batches
    # call c of the target is the stream's call c
    ref = BNNRef(wine["features_train"], wine["labels_train"], seed=10)
    lp_ref, g_ref = ref.evaluate_rows(W.astype(np.float64), stream_rows(10, 1, 50, 128, 2938))
    np.testing.assert_allclose(lp1.numpy(), lp_ref, rtol=LP_BOUND)
    # a fresh target with the same seed reproduces the first call bit for bit
    t2 = BNN_WINE(dataset_seed=10, likelihood_scaling=1., prior_std=1., batch_size=128, dataset_dir=d)
    np.testing.assert_array_equal(t2.log_density(W).numpy(), lp0)


def test_predict_matches_reference_forward_pass(wine):
    from gmmvi_amd.device import get_context
    from gmmvi_amd import hip_ops
    ctx = get_context()
    rng = np.random.default_rng(3)
    ref = BNNRef(wine["features_train"], wine["labels_train"])
    for s, m in ((1, 1), (37, 979), (300, 981)):
        W = rng.normal(size=(s, 177)).astype(np.float32)
        X = wine["features_test"][:m] if m <= 979 else wine["features_vali"][:m]
        out = hip_ops.bnn_predict(ctx, (8, 8), ctx.asarray(W), ctx.asarray(X)).numpy()
        exp = ref.predict(W.astype(np.float64), X.astype(np.float64))
        assert out.shape == (s, m)
        np.testing.assert_allclose(out, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())
    # a generic shape
    X = rng.normal(size=(70, 20)).astype(np.float32)
    W = rng.normal(size=(9, 20 * 16 + 16 + 16 * 3 + 3 + 3 + 1)).astype(np.float32)
    out = hip_ops.bnn_predict(ctx, (16, 3), ctx.asarray(W), ctx.asarray(X)).numpy()
    exp = BNNRef(X, np.zeros(70), hidden_units=(16, 3)).predict(W.astype(np.float64), X.astype(np.float64))
    np.testing.assert_allclose(out, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())


# ---- the iteration -----------------------------------------------------------------------------------------------------
def test_trajectory_matches_oracle(wine, tmp_path):
    """SAMTRON-style iterations, K = 4, 100 samples per component, on the modular path (D = 177 takes the blocked
    kernels): the fp64 oracle on BNNRef and the device on BNN_WINE draw the same samples and the same minibatches."""
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    from gmmvi_amd.experiments.target_distributions.bnn import BNN_WINE
    k, s, seed, iters = 4, 100, 10000, 10
    cfg = samtron_config(s, initial_stepsize=1.0)
    d = 177
    ref = BNNRef(wine["features_train"], wine["labels_train"], seed=seed)
    model = otrain.construct_initial_mixture(d, k, 0.0, 1.0, 1.0, np.random.default_rng(seed + 1))
    o = otrain.OracleGMMVI(
        ref, model, temperature=cfg["temperature"], seed=seed,
        desired_samples_per_component=s, ratio_reused_samples_to_desired=0.0, ng_estimator="Stein",
        only_use_own_samples=False, use_self_normalized_importance_weights=True, updater="trust-region",
        component_stepsize_config=cfg["component_stepsize_adapter_config"], weight_updater="trust-region",
        weight_stepsize_config=cfg["weight_stepsize_adapter_config"], adaptive=None, max_reward_history_length=400,
        sample_selector="component-based", max_database_size=cfg["max_database_size"],
        host_rng=np.random.default_rng(seed))
    om = o.model.model
    m = FullCovGMM(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
    m.seed = seed
    target = BNN_WINE(dataset_seed=seed, likelihood_scaling=1., prior_std=1., batch_size=128,
                      dataset_dir=write_dataset_dir(tmp_path))
    g = GMMVI.build_from_config(cfg, target, GmmWrapper(m, 1.0, 1e-12, 400))
    assert not g._fast_path.eligible()
    g.ng_based_updater.want_info = True
    worst = {}
    for it in range(iters):
        o.train_iter()
        g.train_iter()
        gm, omod = g.model, o.model
        tol = 2.0 * (5e-4 if it < 2 else 2e-3 * (1 + it))               # test_hip_blocked.py's bounds at D >= 64
        dev = {"means": np.abs(gm.means.numpy() - omod.means).max() / max(1.0, np.abs(omod.means).max()),
               "chols": np.abs(gm.chol_cov.numpy() - omod.chol_cov).max() / np.abs(omod.chol_cov).max()}
        for key, v in dev.items():
            worst[key] = max(worst.get(key, 0.0), v)
            assert v <= tol, f"iteration {it}: {key} deviates by {v:.3e} (> {tol:.1e})"
    print(f"WINE trajectory: worst deviations {worst}")
    assert target.call_count == ref.call_count == iters                 # both sides consumed the same minibatches


def test_wine_end_to_end(tmp_path):
    """get_default_config("SAMTRON", "wine") through GmmviRunner on the fixture directory.  First GPU run (seed 10000):
    bi_test_loss 51.25 at iteration 0 and 10.07 after 30 iterations (bi_test_accuracy, an RMSE, 7.16 -> 3.17; -ELBO
    163 895 -> 82 693)."""
    from gmmvi_amd.configs import get_default_config, update_config
    from gmmvi_amd.gmmvi_runner import GmmviRunner
    cfg = update_config(get_default_config("SAMTRON", "wine"),
                        {"environment_config": {"dataset_dir": write_dataset_dir(tmp_path)}, "seed": 10000})
    runner = GmmviRunner.build_from_config(cfg)
    target = runner.gmmvi.sample_selector.target_distribution
    assert target.dataset_seed == 10000 and target.get_num_dimensions() == 177
    m0 = runner.get_expensive_metrics()
    for _ in range(30):
        runner.gmmvi.train_iter()
    m1 = runner.get_expensive_metrics()
    keys = ("bi_test_loss", "bi_test_accuracy", "bi_vali_loss", "bi_vali_rmse")
    for m in (m0, m1):
        assert all(k in m and np.isfinite(m[k]) for k in keys), m
    print("WINE end to end: iteration 0 " + ", ".join(f"{k} {m0[k]:.4f}" for k in keys) +
          "; after 30 iterations " + ", ".join(f"{k} {m1[k]:.4f}" for k in keys) + f"; -elbo {m0['-elbo']:.1f} -> "
          f"{m1['-elbo']:.1f}")
    assert m1["bi_test_loss"] < m0["bi_test_loss"]
    assert m1["-elbo"] < m0["-elbo"]
