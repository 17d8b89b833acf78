"""GPU tests of the logistic-regression targets (csrc/logreg.hip): the kernel against the fp64 reference, the trajectory
against the fp64 oracle, the single-call iteration and the sharded phases, and the two experiments end to end through
the public surface, judged by the Laplace approximation and importance sampling."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import logsumexp

from helpers import samtron_config
from logreg_ref import LogRegRef, load_tables, write_dataset_dir
from oracle import train as otrain

pytestmark = pytest.mark.gpu

INIT = (10.0, 100.0)                   # breast_cancer.yml / german_credit.yml: prior_scale, initial_cov


@pytest.fixture(scope="module")
def data():
    from gmmvi_amd.experiments.target_distributions import logistic_regression as lr
    return {k: lr.preprocess(t, k)[0] for k, t in load_tables().items()}


def _map(ref, iters=60):
    """Newton on the (concave) fp64 posterior from 0 -> (MAP, negative Hessian there)."""
    w = np.zeros(ref.get_num_dimensions())
    for _ in range(iters):
        _, g = ref.log_density_and_grad(w[None])
        H = ref.hessian(w)
        step = np.linalg.solve(H, g[0])
        w = w - step
        if np.abs(step).max() < 1e-12:
            break
    return w, -ref.hessian(w)


# ---- kernel parity ---------------------------------------------------------------------------------------------------
def _check_kernel(A, W, want_grad, worst):
    from gmmvi_amd import hip_ops
    from gmmvi_amd.device import get_context
    ctx = get_context()
    A = np.asarray(A, np.float32)
    W = np.asarray(W, np.float32)
    ref = LogRegRef(A)
    lp_ref, g_ref = ref.log_density_and_grad(W.astype(np.float64))
    lp, g = hip_ops.target_logreg(ctx, ctx.asarray(A), 0.0, 10.0, ctx.asarray(W), want_grad=want_grad)
    lp = lp.numpy()
    assert np.all(np.isfinite(lp))
    # scale of the f32 rounding: sum_m |log sigma(t_m)| plus the prior's terms
    prior = np.abs(ref._prior(W.astype(np.float64)))
    scale = ref.abs_terms(W) + prior + 1.0
    err = np.abs(lp - lp_ref) / scale
    worst["lp"] = max(worst.get("lp", 0.0), float(err.max()))
    assert err.max() <= 1e-5, f"lp relative error {err.max():.2e}"
    if want_grad:
        g = g.numpy()
        assert np.all(np.isfinite(g))
        t = W.astype(np.float64) @ A.T.astype(np.float64)
        from logreg_ref import sigmoid
        gscale = (sigmoid(-t) @ np.abs(A.astype(np.float64))).max(1) + np.abs(W).max(1) / 100.0 + 1.0
        gerr = np.abs(g - g_ref).max(1) / gscale
        worst["grad"] = max(worst.get("grad", 0.0), float(gerr.max()))
        assert gerr.max() <= 1e-5, f"gradient relative error {gerr.max():.2e}"
    else:
        assert g is None


@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_kernel_matches_fp64_reference_on_the_datasets(data, dataset_id):
    A = data[dataset_id]
    ref = LogRegRef(A)
    w_map, prec = _map(ref)
    chol_cov = np.linalg.cholesky(np.linalg.inv(prec))
    rng = np.random.default_rng(7)
    worst = {}
    for n in (1, 7, 64, 1000, 10007):
        near = w_map + rng.normal(size=(n, A.shape[1])) @ chol_cov.T          # the posterior's scale
        init = rng.normal(size=(n, A.shape[1])) * 10.0                         # the yml initialisation: |a.w| ~ 1e3
        assert n < 64 or np.abs(init @ A.T).max() > 300
        for W in (near, init):
            for want_grad in (True, False):
                _check_kernel(A, W, want_grad, worst)
    print(f"{dataset_id}: worst relative errors {worst}")


@pytest.mark.parametrize("m,d", [(1, 1), (37, 3), (569, 64), (200, 100), (300, 300)])
def test_kernel_matches_fp64_reference_synthetic(m, d):
    rng = np.random.default_rng(m * 1000 + d)
    A = rng.normal(size=(m, d)) * np.where(rng.random(m) < 0.5, -1.0, 1.0)[:, None]
    worst = {}
    for n in (1, 7, 64, 1000, 10007):
        for sd in (0.1, 10.0):
            W = rng.normal(size=(n, d)) * sd
            for want_grad in (True, False):
                _check_kernel(A, W, want_grad, worst)
    print(f"M={m} D={d}: worst relative errors {worst}")


def test_kernel_arguments():
    from gmmvi_amd import _lib
    from gmmvi_amd.device import get_context
    ctx = get_context()
    A = ctx.asarray(np.ones((4, 3), np.float32))
    W = ctx.asarray(np.zeros((5, 3), np.float32))
    lp = ctx.empty((5,))
    assert ctx.lib.gmmvi_target_logreg(ctx.handle, 3, 4, A.ptr, 0.0, 10.0, W.ptr, 0, None, None) == 0      # N == 0: OK
    for d, m, sd in ((0, 4, 10.0), (513, 4, 10.0), (3, 0, 10.0), (3, 4, 0.0)):
        assert ctx.lib.gmmvi_target_logreg(ctx.handle, d, m, A.ptr, 0.0, sd, W.ptr, 5, lp.ptr, None) == -2
    ctx.sync()
    assert _lib.EXPORTED_SYMBOLS.count("gmmvi_target_logreg") == 1


# ---- the iteration ---------------------------------------------------------------------------------------------------
def make_pair(A, k, s, seed, cfg, fused=None):
    """fp64 oracle on LogRegRef and the device GMMVI on LogisticRegression, same initial mixture and seed."""
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    from gmmvi_amd.experiments.target_distributions.logistic_regression import LogisticRegression
    d = A.shape[1]
    ps, ic = INIT
    model = otrain.construct_initial_mixture(d, k, 0.0, ps, ic, np.random.default_rng(seed + 1))
    o = otrain.OracleGMMVI(
        LogRegRef(A), model, temperature=cfg["temperature"], seed=seed,
        desired_samples_per_component=cfg["sample_selector_config"]["desired_samples_per_component"],
        ratio_reused_samples_to_desired=cfg["sample_selector_config"]["ratio_reused_samples_to_desired"],
        ng_estimator=cfg["ng_estimator_type"], only_use_own_samples=False,
        use_self_normalized_importance_weights=cfg["ng_estimator_config"]["use_self_normalized_importance_weights"],
        updater=cfg["ng_based_updater_type"], component_stepsize_config=cfg["component_stepsize_adapter_config"],
        weight_updater=cfg["weight_updater_type"], weight_stepsize_config=cfg["weight_stepsize_adapter_config"],
        adaptive=(dict(cfg["num_component_adapter_config"], prior_mean=0.0, initial_cov=ic)
                  if cfg["num_component_adapter_type"] == "adaptive" else None),
        max_reward_history_length=400, sample_selector=cfg["sample_selector_type"],
        max_database_size=cfg["max_database_size"], host_rng=np.random.default_rng(seed))

    def device():
        om = o.model.model
        m = FullCovGMM(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
        m.seed = seed
        wrapper = GmmWrapper(m, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
        c = dict(cfg)
        c["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=ic)
        g = GMMVI.build_from_config(c, LogisticRegression(X=A, labels=np.zeros(A.shape[0])), wrapper)
        if cfg["num_component_adapter_type"] == "adaptive":
            g.num_component_adapter.rng = np.random.default_rng(seed)
        return g
    return o, device


def test_general_constructor_reproduces_the_signed_matrix(data):
    from gmmvi_amd.experiments.target_distributions.logistic_regression import LogisticRegression
    A = data["german_credit"]
    t = LogisticRegression(X=A, labels=np.zeros(A.shape[0]))            # label 0: s = +1, the rows as given
    np.testing.assert_array_equal(t.A, A)
    t1 = LogisticRegression(X=-A, labels=np.ones(A.shape[0]))           # label 1: s = -1
    np.testing.assert_array_equal(t1.A, A)
    tables = load_tables()
    t2 = LogisticRegression("german_credit", data=tables["german_credit"])
    np.testing.assert_array_equal(t2.A, A)
    w = np.random.default_rng(0).normal(size=(33, A.shape[1])).astype(np.float32)
    np.testing.assert_array_equal(t2.log_density(w).numpy(), t.log_density(w).numpy())


def _trajectory(o, g, iters, tol_scale=1.0, ids=False):
    for it in range(iters):
        o.train_iter()
        g.train_iter()
        om, gm = o.model, g.model
        assert gm.num_components == om.num_components, f"iteration {it}"
        np.testing.assert_array_equal(gm.unique_component_ids, om.unique_component_ids, err_msg=f"iteration {it}")
        if ids:
            continue
        tol = tol_scale * (5e-4 if it < 2 else 2e-3 * (1 + it))
        dm = np.abs(gm.means.numpy() - om.means).max() / max(1.0, np.abs(om.means).max())
        dc = np.abs(gm.chol_cov.numpy() - om.chol_cov).max() / np.abs(om.chol_cov).max()
        dw = np.abs(np.exp(gm.log_weights.numpy()) - om.weights).max()
        ds = np.abs(gm.stepsizes.numpy() - om.stepsizes).max()
        for name, v in (("means", dm), ("chols", dc), ("logw", dw), ("stepsizes", ds)):
            assert v <= tol, f"iteration {it}: {name} deviates by {v:.3e} (> {tol:.1e})"


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("fused", [True, False])
def test_trajectory_matches_oracle(data, k, fused):
    A = data["german_credit"]
    cfg = samtron_config(100, initial_stepsize=1.0)
    o, device = make_pair(A, k, 100, 31, cfg)
    g = device()
    if fused:
        assert g._fast_path.eligible()
    else:
        g.ng_based_updater.want_info = True
    _trajectory(o, g, 20)


def test_adaptive_component_ids_in_lock_step_on_breast_cancer(data):
    from helpers import EXAMPLE6_ADAPTIVE
    A = data["breast_cancer"]
    adaptive = dict(EXAMPLE6_ADAPTIVE, add_iters=30, del_iters=30, num_database_samples=10000)
    cfg = samtron_config(100, initial_stepsize=1.0, adaptive=adaptive)
    o, device = make_pair(A, 1, 100, 5, cfg)
    g = device()
    _trajectory(o, g, 100, ids=True)
    assert o.model.num_components >= 4                                  # three add events


@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_fast_path_equals_modular_path(data, dataset_id):
    A = data[dataset_id]
    cfg = samtron_config(100, initial_stepsize=1.0)
    _, device = make_pair(A, 2, 100, 23, cfg)
    fast, slow = device(), device()
    slow._fast_path.enabled = False
    assert fast._fast_path.eligible() and not slow._fast_path.eligible()
    fast._fast_path.explicit_estimate = True
    for it in range(8):
        fast.train_iter()
        slow.train_iter()
        for name in ("means", "chol_cov", "log_weights", "stepsizes", "last_log_etas", "l2_regularizers",
                     "num_received_updates"):
            np.testing.assert_array_equal(getattr(fast.model, name).numpy(), getattr(slow.model, name).numpy(),
                                          err_msg=f"iteration {it}: {name}")
        np.testing.assert_array_equal(fast.model.reward_slot(0).numpy(), slow.model.reward_slot(0).numpy())
        np.testing.assert_array_equal(fast.weight_stepsize_adapter._state.numpy(),
                                      slow.weight_stepsize_adapter._state.numpy())
    np.testing.assert_array_equal(fast.sample_db.samples.numpy(), slow.sample_db.samples.numpy())
    np.testing.assert_array_equal(fast.sample_db.target_grads.numpy(), slow.sample_db.target_grads.numpy())
    assert int(fast.num_updates) == int(slow.num_updates) == 8


@pytest.mark.parametrize("phased", [True, False])
def test_single_rank_sharded_equals_modular_gmmvi(data, phased, monkeypatch):
    from gmmvi_amd.device import get_context
    from gmmvi_amd.sharded import ShardedGMMVI, HipOps, LocalExchange
    A = data["german_credit"]
    k, s, seed = 3, 60, 17
    cfg = samtron_config(s)
    _, device = make_pair(A, k, s, seed, cfg)
    g = device()
    ctx = get_context()
    if not phased:
        monkeypatch.setenv("GMMVI_FAST_PATH", "0")                      # the module-by-module sharded route
    sh = ShardedGMMVI(HipOps(ctx, g.sample_selector.target_distribution), LocalExchange(), A.shape[1], k,
                      g.model.means.numpy(), g.model.chol_cov.numpy(), s, seed, cfg)
    assert (sh._fast is not None) == phased
    for _ in range(6):
        g.train_iter()
        sh.train_iter()
    sh.flush()
    np.testing.assert_allclose(sh.means.numpy(), g.model.means.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(sh.chols.numpy(), g.model.chol_cov.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(sh.log_weights.numpy(), g.model.log_weights.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(sh.stepsizes.numpy(), g.model.stepsizes.numpy(), rtol=1e-6)


def test_unknown_target_kind_is_an_argument_error():
    from gmmvi_amd import _lib
    from gmmvi_amd.device import get_context
    from gmmvi_amd.optimization.fused import SamtronPlan
    from gmmvi_amd.sharded import ShardedPlan
    ctx = get_context()
    lib = _lib.load()
    for kind in (3, 7, -1):
        p = ShardedPlan()
        p.target.kind = kind
        assert lib.gmmvi_train_iter_sharded_phase(ctx.handle, C.byref(p), 1) == -2
        assert "target_kind" in ctx.lib.gmmvi_last_error(ctx.handle).decode()
        q = SamtronPlan()
        q.target.kind = kind
        assert lib.gmmvi_train_iter_samtron(ctx.handle, C.byref(q)) == -2
        assert "target_kind" in ctx.lib.gmmvi_last_error(ctx.handle).decode()
    ctx.sync()


# ---- end to end --------------------------------------------------------------------------------------------------------
def _mixture_logpdf(x, weights, means, covs):
    out = []
    for w, m, c in zip(weights, means, covs):
        L = np.linalg.cholesky(c)
        z = np.linalg.solve(L, (x - m).T)
        out.append(np.log(w) - 0.5 * (z * z).sum(0) - np.log(np.diag(L)).sum() - 0.5 * len(m) * np.log(2 * np.pi))
    return logsumexp(np.stack(out), axis=0)


def _sample_mixture(rng, n, weights, means, covs):
    comp = rng.choice(len(weights), size=n, p=weights / weights.sum())
    x = np.empty((n, means.shape[1]))
    for k in range(len(weights)):
        idx = comp == k
        x[idx] = means[k] + rng.normal(size=(idx.sum(), means.shape[1])) @ np.linalg.cholesky(covs[k]).T
    return x


def _elbo_and_logz(ref, rng, n, weights, means, covs):
    """fp64: (ELBO, its standard error, IS log Z, its standard error) with the mixture as proposal."""
    x = _sample_mixture(rng, n, weights, means, covs)
    r = ref.log_density(x) - _mixture_logpdf(x, weights, means, covs)
    elbo, elbo_se = r.mean(), r.std() / np.sqrt(n)
    logz = logsumexp(r) - np.log(n)
    w = np.exp(r - r.max())
    logz_se = w.std() / (np.sqrt(n) * w.mean())
    return elbo, elbo_se, logz, logz_se


def _run_public(tmp_path, exp_id, iters):
    from gmmvi_amd.configs import get_default_config, update_config
    from gmmvi_amd.gmmvi_runner import GmmviRunner
    cfg = update_config(get_default_config("SEMTRON", exp_id),
                        {"environment_config": {"dataset_dir": write_dataset_dir(tmp_path)}, "seed": 3})
    runner = GmmviRunner.build_from_config(cfg)
    assert runner.gmmvi._fast_path.eligible()
    for _ in range(iters):
        runner.gmmvi.train_iter()
    m = runner.gmmvi.model
    return (np.exp(m.log_weights.numpy().astype(np.float64)), m.means.numpy().astype(np.float64),
            np.einsum("kij,klj->kil", m.chol_cov.numpy().astype(np.float64), m.chol_cov.numpy().astype(np.float64)))


def test_german_credit_end_to_end(tmp_path, data):
    ref = LogRegRef(data["german_credit"])
    weights, means, covs = _run_public(tmp_path, "german_credit", 100)
    rng = np.random.default_rng(11)
    elbo, elbo_se, logz, logz_se = _elbo_and_logz(ref, rng, 20000, weights, means, covs)
    w_map, prec = _map(ref)
    lap = _elbo_and_logz(ref, rng, 20000, np.ones(1), w_map[None], np.linalg.inv(prec)[None])
    print(f"GC: ELBO(q) {elbo:.3f} +- {elbo_se:.3f}, IS log Z {logz:.3f} +- {logz_se:.3f}, Laplace ELBO {lap[0]:.3f}")
    assert elbo >= lap[0] - 3 * np.hypot(elbo_se, lap[1])
    assert elbo <= logz + 3 * np.hypot(elbo_se, logz_se)


def test_breast_cancer_end_to_end(tmp_path, data):
    A = data["breast_cancer"]
    ref = LogRegRef(A)
    weights, means, covs = _run_public(tmp_path, "breast_cancer", 100)
    rng = np.random.default_rng(12)
    elbo, elbo_se, logz, logz_se = _elbo_and_logz(ref, rng, 20000, weights, means, covs)
    # the fp64 oracle with the same algorithm settings (SEMTRON, K = 1, the yml initialisation) after as many iterations
    from gmmvi_amd.configs import get_default_config
    cfg = get_default_config("SEMTRON", "breast_cancer")
    o, _ = make_pair(A, 1, 100, 3, dict(cfg, seed=3))
    for _ in range(100):
        o.train_iter()
    om = o.model
    oel = _elbo_and_logz(ref, rng, 20000, np.asarray(om.weights, np.float64), om.means, om.covs)
    print(f"BC: ELBO(q) {elbo:.3f} +- {elbo_se:.3f}, IS log Z {logz:.3f} +- {logz_se:.3f}, oracle ELBO {oel[0]:.3f}")
    assert elbo >= oel[0] - 0.5 - 3 * np.hypot(elbo_se, oel[1])
    assert elbo <= logz + 3 * np.hypot(elbo_se, logz_se)
