"""GPU tests of the minibatch logistic-regression targets (csrc/logreg_mb.hip): the kernel against the fp64 reference on
the same batches, against the full-data kernel at B = T, reproducibility, argument errors, the call counter, the
trajectory against the fp64 oracle, and the two experiments end to end through the public surface."""
import numpy as np
import pytest

from helpers import samtron_config
from logreg_mb_ref import LogRegMbRef
from logreg_ref import LogRegRef, load_tables, write_dataset_dir
from oracle import train as otrain

pytestmark = pytest.mark.gpu

# errors relative to the scale of the f32 rounding (LogRegMbRef.abs_terms, which counts the cancellation in t = a . w:
# with B = 1 the scaled sum has a single term and nothing averages it out); the full-data kernel's worst figures are
# 9.4e-7 (lp) and 3.1e-6 (gradient) of |lp| and |grad|
LP_BOUND, GRAD_BOUND = 1e-5, 1e-5
INIT = (10.0, 100.0)                   # breast_cancer_mb.yml / german_credit_mb.yml: prior_scale, initial_cov


@pytest.fixture(scope="module")
def data():
    from gmmvi_amd.experiments.target_distributions import logistic_regression as lr
    return {k: lr.preprocess(t, k)[0] for k, t in load_tables().items()}


def _map(ref, iters=60):
    """Newton on the (concave) fp64 full-data posterior from 0 -> (MAP, negative Hessian there)."""
    w = np.zeros(ref.get_num_dimensions())
    for _ in range(iters):
        _, g = ref.log_density_and_grad(w[None])
        step = np.linalg.solve(ref.hessian(w), g[0])
        w = w - step
        if np.abs(step).max() < 1e-12:
            break
    return w, -ref.hessian(w)


def _run_kernel(A, B, nb, seed, call, W, want_grad=True):
    from gmmvi_amd import hip_ops
    from gmmvi_amd.device import get_context
    ctx = get_context()
    lp, g = hip_ops.target_logreg_mb(ctx, ctx.asarray(np.asarray(A, np.float32)), B, nb, seed, call, 0.0, 10.0,
                                     ctx.asarray(np.asarray(W, np.float32)), want_grad=want_grad)
    return lp.numpy(), (g.numpy() if g is not None else None)


def _check_kernel(A, B, own, seed, call, W, worst):
    A32, W32 = np.asarray(A, np.float32), np.asarray(W, np.float32)
    ref = LogRegMbRef(A32, B, use_own_batch_per_sample=own, seed=seed)
    rows = ref.rows(call, W32.shape[0])
    lp_ref, g_ref = ref.evaluate_rows(W32.astype(np.float64), rows)
    lp_scale, g_scale = ref.abs_terms(W32.astype(np.float64), rows)
    lp, g = _run_kernel(A32, B, ref.nb, seed, call, W32)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    err = np.abs(lp - lp_ref) / (lp_scale + 1.0)
    gerr = np.abs(g - g_ref).max(1) / (g_scale + 1.0)
    worst["lp"] = max(worst.get("lp", 0.0), float(err.max()))
    worst["grad"] = max(worst.get("grad", 0.0), float(gerr.max()))
    lp2, g2 = _run_kernel(A32, B, ref.nb, seed, call, W32, want_grad=False)
    assert g2 is None
    np.testing.assert_array_equal(lp2, lp)                   # the log density alone: the same sums in the same order
    return float(err.max()), float(gerr.max())


@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_kernel_matches_fp64_reference(data, dataset_id, own):
    A = data[dataset_id]
    T, D = A.shape
    w_map, prec = _map(LogRegRef(A))
    chol_cov = np.linalg.cholesky(np.linalg.inv(prec))
    rng = np.random.default_rng(T + own)
    worst, bad = {}, []
    for B in (1, 64, T):
        for n in (1, 15, 16, 17, 400, 10000):
            near = w_map + rng.normal(size=(n, D)) @ chol_cov.T                    # the posterior's scale
            init = rng.normal(size=(n, D)) * 10.0                                   # the yml initialisation
            for name, W in (("near", near), ("init", init)):
                e, ge = _check_kernel(A, B, own, seed=10000 + n, call=B + n, W=W, worst=worst)
                if e > LP_BOUND or ge > GRAD_BOUND:
                    bad.append(f"B = {B} N = {n} {name}: lp {e:.2e}, grad {ge:.2e}")
    print(f"{dataset_id} own batches {own}: worst relative errors {worst}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_full_batch_equals_the_full_data_kernel(data, dataset_id):
    from gmmvi_amd import hip_ops
    from gmmvi_amd.device import get_context
    ctx = get_context()
    A = data[dataset_id]
    T, D = A.shape
    W = (np.random.default_rng(5).normal(size=(1000, D)) * 3.0).astype(np.float32)
    lp, g = _run_kernel(A, T, 1, 3, 11, W)
    lp_fd, g_fd = hip_ops.target_logreg(ctx, ctx.asarray(A), 0.0, 10.0, ctx.asarray(W), want_grad=True)
    lp_scale, g_scale = LogRegMbRef(A, T, use_own_batch_per_sample=False).abs_terms(W.astype(np.float64),
                                                                                    np.tile(np.arange(T), (1000, 1)))
    # the same sum in another order: both within f32 summation rounding of each other
    assert (np.abs(lp - lp_fd.numpy()) / (lp_scale + 1.0)).max() <= 2 * LP_BOUND
    assert (np.abs(g - g_fd.numpy()).max(1) / (g_scale + 1.0)).max() <= 2 * GRAD_BOUND


def test_kernel_is_bitwise_reproducible_and_keyed_by_seed_and_call(data):
    A = data["breast_cancer"]
    W = np.random.default_rng(0).normal(size=(400, A.shape[1]))
    nb = A.shape[0] // 64
    a = _run_kernel(A, 64, nb, 5, 9, W)
    b = _run_kernel(A, 64, nb, 5, 9, W)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    c = _run_kernel(A, 64, nb, 5, 10, W)
    d = _run_kernel(A, 64, nb, 6, 9, W)
    assert np.all(a[0] != c[0]) and np.all(a[0] != d[0])


def test_kernel_arguments():
    from gmmvi_amd import _lib
    from gmmvi_amd.device import get_context
    ctx = get_context()
    A = ctx.asarray(np.ones((40, 129), np.float32))
    W = ctx.asarray(np.zeros((5, 129), np.float32))
    lp = ctx.empty((5,))
    f = ctx.lib.gmmvi_target_logreg_mb
    assert f(ctx.handle, 3, 40, A.ptr, 8, 5, 0, 0, 0.0, 10.0, W.ptr, 0, None, None) == 0       # N == 0: nothing launched
    assert f(ctx.handle, 3, 40, A.ptr, 8, 5, 0, 0, 0.0, 10.0, W.ptr, 5, lp.ptr, None) == 0
    bad = ((0, 40, A.ptr, 8, 5, 10.0, W.ptr, lp.ptr),       # D < 1
           (129, 40, A.ptr, 8, 5, 10.0, W.ptr, lp.ptr),     # D > 128
           (3, 40, A.ptr, 0, 1, 10.0, W.ptr, lp.ptr),       # B < 1
           (3, 40, A.ptr, 41, 1, 10.0, W.ptr, lp.ptr),      # B > T
           (3, 40, A.ptr, 8, 0, 10.0, W.ptr, lp.ptr),       # nb < 1
           (3, 40, A.ptr, 8, 6, 10.0, W.ptr, lp.ptr),       # nb B > T
           (3, 40, A.ptr, 8, 5, 0.0, W.ptr, lp.ptr),        # prior_std <= 0
           (3, 40, None, 8, 5, 10.0, W.ptr, lp.ptr),        # A null
           (3, 40, A.ptr, 8, 5, 10.0, None, lp.ptr),        # x null
           (3, 40, A.ptr, 8, 5, 10.0, W.ptr, None))         # lp null
    for d, t, a, b, nb, sd, w, out in bad:
        assert f(ctx.handle, d, t, a, b, nb, 0, 0, 0.0, sd, w, 5, out, None) == -2
        assert "invalid argument" in ctx.lib.gmmvi_last_error(ctx.handle).decode()
    ctx.sync()
    assert _lib.EXPORTED_SYMBOLS.count("gmmvi_target_logreg_mb") == 1


# ---- the LNPDF -------------------------------------------------------------------------------------------------------
def test_call_counter_advances_once_per_evaluation(data, tmp_path):
    from gmmvi_amd.experiments.target_distributions.logistic_regression import make_breast_cancer_mb
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    t = make_breast_cancer_mb(64, 0, True, dataset_dir=write_dataset_dir(tmp_path), seed=10)
    A = data["breast_cancer"]
    assert t.seed == 10 and t.call_count == 0 and t.num_data == 569 and t.num_batches == 8
    W = np.random.default_rng(1).normal(size=(50, 31)).astype(np.float32)
    lp0 = t.log_density(W).numpy()
    assert t.call_count == 1
    lp1, g1 = t.log_density_and_grad(W)
    assert t.call_count == 2
    assert np.all(lp0 != lp1.numpy())                        # the same weights on other batches
    t.log_density(np.zeros((0, 31), np.float32))
    assert t.call_count == 2                                 # a call without samples draws no batches
    fb = t.log_density_fb(W).numpy()
    model = FullCovGMM(np.ones(1), np.zeros((1, 31), np.float32), (100.0 * np.eye(31, dtype=np.float32))[None])
    m = t.expensive_metrics(model, t.ctx.asarray(W))
    assert t.call_count == 2                                 # the full-batch posterior and the metrics leave it alone
    assert list(m) == ["elbo_fb:"] and np.isfinite(m["elbo_fb:"])
    np.testing.assert_allclose(fb, LogRegRef(A).log_density(W.astype(np.float64)), rtol=1e-5)
    np.testing.assert_allclose(m["elbo_fb:"], fb.astype(np.float64).mean() - model.log_density(W).numpy().mean(),
                               rtol=1e-6)
    # call c of the target is the stream's call c
    ref = LogRegMbRef(A, 64, seed=10)
    lp_ref, g_ref = ref.evaluate_rows(W.astype(np.float64), ref.rows(1, 50))
    scale = ref.abs_terms(W.astype(np.float64), ref.rows(1, 50))[0] + 1.0
    assert (np.abs(lp1.numpy() - lp_ref) / scale).max() <= LP_BOUND
    t2 = make_breast_cancer_mb(64, 0, True, dataset_dir=str(tmp_path), seed=10)
    np.testing.assert_array_equal(t2.log_density(W).numpy(), lp0)          # a fresh target replays call 0 bit for bit


# ---- the iteration ---------------------------------------------------------------------------------------------------
def _trajectory(o, g, iters, tol_scale=1.0):
    """test_hip_logreg._trajectory's bounds."""
    for it in range(iters):
        o.train_iter()
        g.train_iter()
        om, gm = o.model, g.model
        assert gm.num_components == om.num_components, f"iteration {it}"
        tol = tol_scale * (5e-4 if it < 2 else 2e-3 * (1 + it))
        dm = np.abs(gm.means.numpy() - om.means).max() / max(1.0, np.abs(om.means).max())
        dc = np.abs(gm.chol_cov.numpy() - om.chol_cov).max() / np.abs(om.chol_cov).max()
        dw = np.abs(np.exp(gm.log_weights.numpy()) - om.weights).max()
        ds = np.abs(gm.stepsizes.numpy() - om.stepsizes).max()
        for name, v in (("means", dm), ("chols", dc), ("logw", dw), ("stepsizes", ds)):
            assert v <= tol, f"iteration {it}: {name} deviates by {v:.3e} (> {tol:.1e})"


@pytest.mark.parametrize("k", [1, 4])
def test_trajectory_matches_oracle(data, k):
    """SAMTRON-style iterations on German Credit with B = 64 and own batches: the fp64 oracle on LogRegMbRef and the
    device on LogisticRegressionMinibatch draw the same samples and the same batches."""
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    from gmmvi_amd.experiments.target_distributions.logistic_regression import LogisticRegressionMinibatch
    A = data["german_credit"]
    d, s, seed, iters = A.shape[1], 100, 31, 20
    cfg = samtron_config(s, initial_stepsize=1.0)
    ps, ic = INIT
    ref = LogRegMbRef(A, 64, seed=seed)
    model = otrain.construct_initial_mixture(d, k, 0.0, ps, ic, np.random.default_rng(seed + 1))
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
    target = LogisticRegressionMinibatch(X=A, labels=np.zeros(A.shape[0]), batch_size=64, size_test_set=0,
                                         use_own_batch_per_sample=True, seed=seed)
    c = dict(cfg)
    c["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=ic)
    g = GMMVI.build_from_config(c, target, GmmWrapper(m, 1.0, 1e-12, 400))
    assert not g._fast_path.eligible()
    g.ng_based_updater.want_info = True
    _trajectory(o, g, iters)
    assert target.call_count == ref.call_count == iters                 # both sides consumed the same batches


# ---- end to end --------------------------------------------------------------------------------------------------------
# largest |mean_d - MAP_d| / sqrt(Sigma_dd) after 100 iterations (Sigma: the inverse negative Hessian at the full-data
# MAP); set at about twice the first GPU run's figures (breast_cancer_mb 1.42, german_credit_mb 0.54: the posterior
# mean is not the MAP, and the iterate carries minibatch noise)
MAP_BOUND = {"breast_cancer_mb": 3.0, "german_credit_mb": 1.2}


@pytest.mark.parametrize("exp_id,dataset_id", [("breast_cancer_mb", "breast_cancer"),
                                               ("german_credit_mb", "german_credit")])
def test_end_to_end(tmp_path, data, exp_id, dataset_id):
    """get_default_config("SAMTRON", exp_id) through GmmviRunner on the fixture directory, 100 iterations."""
    from gmmvi_amd.configs import get_default_config, update_config
    from gmmvi_amd.gmmvi_runner import GmmviRunner
    cfg = update_config(get_default_config("SAMTRON", exp_id),
                        {"environment_config": {"dataset_dir": write_dataset_dir(tmp_path)}, "seed": 10000})
    runner = GmmviRunner.build_from_config(cfg)
    target = runner.gmmvi.sample_selector.target_distribution
    assert target.seed == 10000 and target.batch_size == 64 and target.num_batches == target.num_data // 64
    assert not runner.gmmvi._fast_path.eligible()
    m0 = runner.get_expensive_metrics()
    for _ in range(100):
        runner.gmmvi.train_iter()
    m1 = runner.get_expensive_metrics()
    assert np.isfinite(m0["elbo_fb:"]) and np.isfinite(m1["elbo_fb:"])
    assert m1["elbo_fb:"] > m0["elbo_fb:"]
    w_map, prec = _map(LogRegRef(data[dataset_id]))
    sd = np.sqrt(np.diag(np.linalg.inv(prec)))
    mean = runner.gmmvi.model.means.numpy()[0].astype(np.float64)
    z = np.abs(mean - w_map) / sd
    print(f"{exp_id}: elbo_fb: {m0['elbo_fb:']:.3f} -> {m1['elbo_fb:']:.3f}; max |mean - MAP| / sd = {z.max():.3f}, "
          f"calls {target.call_count}")
    assert z.max() <= MAP_BOUND[exp_id]
