"""GPU tests of the Talos target (csrc/talos.hip): the kernel and the forward kinematics against the fp64 reference walk,
the trajectory against the fp64 oracle, the single-call iteration and the sharded phases, and the experiment end to end
through the public surface."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import logsumexp

from helpers import samtron_config
from oracle import train as otrain
from talos_ref import GOLDEN_DIR, TalosRef

pytestmark = pytest.mark.gpu

CONTEXT = [0.1, 0.5, 1.0]                                # talos.yml
SIZES = (1, 63, 64, 65, 1000, 10000)


@pytest.fixture(scope="module")
def ref():
    return TalosRef(CONTEXT)


@pytest.fixture(scope="module")
def target():
    from gmmvi_amd.experiments.target_distributions.talos_ik import Talos
    return Talos(CONTEXT, dataset_dir=GOLDEN_DIR)


def _sets(rng, n):
    stand = rng.normal(size=(n, 34)) * 0.1               # near the standing pose
    stand[:, 30] += 1.08
    return {"standing": stand, "normal": rng.normal(size=(n, 34)),          # talos.yml's N(0, I) initialisation
            "large": rng.uniform(-1e3, 1e3, size=(n, 34))}


def test_kernel_matches_fp64_reference(ref, target):
    rng = np.random.default_rng(5)
    worst = {}
    for n in SIZES:
        for name, x in _sets(rng, n).items():
            x = x.astype(np.float32)
            lp_ref, g_ref = ref.log_density_and_grad(x.astype(np.float64))
            lp, g = target.log_density_and_grad(x)
            lp, g = lp.numpy().astype(np.float64), g.numpy().astype(np.float64)
            assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)), (name, n)
            err = np.abs(lp - lp_ref) / (1.0 + np.abs(lp_ref))
            gerr = np.abs(g - g_ref).max(1) / (1.0 + np.abs(g_ref).max(1))
            worst[name] = (max(worst.get(name, (0, 0))[0], float(err.max())), max(worst.get(name, (0, 0))[1], float(gerr.max())))
            assert err.max() <= 1e-5, f"{name} N={n}: lp relative error {err.max():.2e}"
            assert gerr.max() <= 1e-5, f"{name} N={n}: gradient relative error {gerr.max():.2e}"
            lp_only = target.log_density(x).numpy()
            np.testing.assert_array_equal(lp_only, lp.astype(np.float32))
    print(f"worst relative errors (lp, grad): {worst}")


def test_forward_kinematics_matches_the_reference(ref, target):
    rng = np.random.default_rng(6)
    for name, x in _sets(rng, 333).items():
        x = x.astype(np.float32)
        P, c = ref.fk(x.astype(np.float64))
        poses, com = target.forward_kinematics(x)
        scale = 1.0 + np.abs(x[:, 28:31].astype(np.float64)).max(1)
        assert poses.shape == (333, 4, 12) and com.shape == (333, 3)
        assert (np.abs(poses - P).max((1, 2)) / scale).max() <= 2e-6, name
        assert (np.abs(com - c).max(1) / scale).max() <= 2e-6, name


def test_results_are_bitwise_reproducible(target):
    x = np.random.default_rng(7).normal(size=(1000, 34)).astype(np.float32)
    a = target.log_density_and_grad(x)
    b = target.log_density_and_grad(x)
    np.testing.assert_array_equal(a[0].numpy(), b[0].numpy())
    np.testing.assert_array_equal(a[1].numpy(), b[1].numpy())


def test_metrics(target):
    x = np.zeros((10, 34), np.float32)
    m = target.expensive_metrics(None, x)
    assert m["fraction_within_joint_limits"] == 1.0
    assert m["left_gripper_error"] == pytest.approx(np.linalg.norm(np.array([0.0049, 0.294, -0.2788]) - CONTEXT), abs=1e-3)
    assert m["foot_position_error"] == pytest.approx(np.hypot(0.005, 1.083), abs=1e-3)


def test_kernel_arguments(target):
    from gmmvi_amd import _lib
    from gmmvi_amd.device import get_context
    ctx = get_context()
    T, c = target._table_dev, target._context_dev
    x = ctx.asarray(np.zeros((5, 34), np.float32))
    lp, poses, com = ctx.empty((5,)), ctx.empty((5, 4, 12)), ctx.empty((5, 3))
    lib = ctx.lib
    assert lib.gmmvi_target_talos(ctx.handle, T.ptr, c.ptr, x.ptr, 0, None, None) == 0          # N == 0: nothing to do
    assert lib.gmmvi_target_talos(ctx.handle, T.ptr, c.ptr, x.ptr, -1, lp.ptr, None) == -2
    for args in ((None, c.ptr, x.ptr), (T.ptr, None, x.ptr), (T.ptr, c.ptr, None)):
        assert lib.gmmvi_target_talos(ctx.handle, *args, 5, lp.ptr, None) == -2
    assert lib.gmmvi_target_talos(ctx.handle, T.ptr, c.ptr, x.ptr, 5, None, None) == -2
    assert lib.gmmvi_talos_fk(ctx.handle, T.ptr, x.ptr, 5, poses.ptr, None) == -2
    assert lib.gmmvi_talos_fk(ctx.handle, None, x.ptr, 5, poses.ptr, com.ptr) == -2
    assert lib.gmmvi_talos_fk(ctx.handle, T.ptr, x.ptr, 0, None, None) == 0
    ctx.sync()
    assert _lib.EXPORTED_SYMBOLS.count("gmmvi_target_talos") == 1 and _lib.EXPORTED_SYMBOLS.count("gmmvi_talos_fk") == 1


def test_target_kind_4_needs_its_model():
    from gmmvi_amd import _lib
    from gmmvi_amd.device import get_context
    from gmmvi_amd.optimization.fused import SamtronPlan
    from gmmvi_amd.sharded import ShardedPlan
    ctx = get_context()
    lib = _lib.load()
    p = ShardedPlan()
    p.target.kind = 4
    assert lib.gmmvi_train_iter_sharded_phase(ctx.handle, C.byref(p), 1) == -2
    assert "talos_model" in ctx.lib.gmmvi_last_error(ctx.handle).decode()
    q = SamtronPlan()
    q.target.kind = 4
    assert lib.gmmvi_train_iter_samtron(ctx.handle, C.byref(q)) == -2
    assert "talos_model" in ctx.lib.gmmvi_last_error(ctx.handle).decode()
    ctx.sync()


# ---- the iteration ---------------------------------------------------------------------------------------------------
def make_pair(k, s, seed, cfg):
    """fp64 oracle on TalosRef and the device GMMVI on Talos, same initial mixture (talos.yml's) and seed."""
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    from gmmvi_amd.experiments.target_distributions.talos_ik import Talos
    model = otrain.construct_initial_mixture(34, k, 0.0, 1.0, 1.0, np.random.default_rng(seed + 1))
    o = otrain.OracleGMMVI(
        TalosRef(CONTEXT), model, temperature=cfg["temperature"], seed=seed,
        desired_samples_per_component=cfg["sample_selector_config"]["desired_samples_per_component"],
        ratio_reused_samples_to_desired=cfg["sample_selector_config"]["ratio_reused_samples_to_desired"],
        ng_estimator=cfg["ng_estimator_type"], only_use_own_samples=False,
        use_self_normalized_importance_weights=cfg["ng_estimator_config"]["use_self_normalized_importance_weights"],
        updater=cfg["ng_based_updater_type"], component_stepsize_config=cfg["component_stepsize_adapter_config"],
        weight_updater=cfg["weight_updater_type"], weight_stepsize_config=cfg["weight_stepsize_adapter_config"],
        adaptive=None, max_reward_history_length=400, sample_selector=cfg["sample_selector_type"],
        max_database_size=cfg["max_database_size"], host_rng=np.random.default_rng(seed))

    def device():
        om = o.model.model
        m = FullCovGMM(om.weights, om.means.astype(np.float32), om.covs.astype(np.float32))
        m.seed = seed
        wrapper = GmmWrapper(m, cfg["component_stepsize_adapter_config"]["initial_stepsize"], 1e-12, 400)
        c = dict(cfg)
        c["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=1.0)
        return GMMVI.build_from_config(c, Talos(CONTEXT, dataset_dir=GOLDEN_DIR), wrapper)
    return o, device


def _trajectory(o, g, iters):
    for it in range(iters):
        o.train_iter()
        g.train_iter()
        om, gm = o.model, g.model
        assert gm.num_components == om.num_components, f"iteration {it}"
        tol = 5e-4 if it < 2 else 2e-3 * (1 + it)
        dm = np.abs(gm.means.numpy() - om.means).max() / max(1.0, np.abs(om.means).max())
        dc = np.abs(gm.chol_cov.numpy() - om.chol_cov).max() / np.abs(om.chol_cov).max()
        dw = np.abs(np.exp(gm.log_weights.numpy()) - om.weights).max()
        ds = np.abs(gm.stepsizes.numpy() - om.stepsizes).max()
        for name, v in (("means", dm), ("chols", dc), ("logw", dw), ("stepsizes", ds)):
            assert v <= tol, f"iteration {it}: {name} deviates by {v:.3e} (> {tol:.1e})"


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("fused", [True, False])
def test_trajectory_matches_oracle(k, fused):
    cfg = samtron_config(100, initial_stepsize=1.0)
    o, device = make_pair(k, 100, 41, cfg)
    g = device()
    if fused:
        assert g._fast_path.eligible()
    else:
        g.ng_based_updater.want_info = True
    _trajectory(o, g, 20)


def test_fast_path_equals_modular_path():
    cfg = samtron_config(100, initial_stepsize=1.0)
    _, device = make_pair(2, 100, 23, cfg)
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
    np.testing.assert_array_equal(fast.sample_db.samples.numpy(), slow.sample_db.samples.numpy())
    np.testing.assert_array_equal(fast.sample_db.target_grads.numpy(), slow.sample_db.target_grads.numpy())
    assert int(fast.num_updates) == int(slow.num_updates) == 8


@pytest.mark.parametrize("phased", [True, False])
def test_single_rank_sharded_equals_modular_gmmvi(phased, monkeypatch):
    from gmmvi_amd.device import get_context
    from gmmvi_amd.sharded import ShardedGMMVI, HipOps, LocalExchange
    k, s, seed = 3, 60, 17
    cfg = samtron_config(s)
    _, device = make_pair(k, s, seed, cfg)
    g = device()
    ctx = get_context()
    if not phased:
        monkeypatch.setenv("GMMVI_FAST_PATH", "0")
    sh = ShardedGMMVI(HipOps(ctx, g.sample_selector.target_distribution), LocalExchange(), 34, k,
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


# ---- end to end --------------------------------------------------------------------------------------------------------
def _mixture_stats(ref, rng, n, weights, means, covs):
    """fp64: (ELBO of the mixture, median left-gripper error) over n fresh draws."""
    comp = rng.choice(len(weights), size=n, p=weights / weights.sum())
    x = np.empty((n, means.shape[1]))
    logq = []
    for k in range(len(weights)):
        L = np.linalg.cholesky(covs[k])
        idx = comp == k
        x[idx] = means[k] + rng.normal(size=(idx.sum(), means.shape[1])) @ L.T
    for k in range(len(weights)):
        L = np.linalg.cholesky(covs[k])
        z = np.linalg.solve(L, (x - means[k]).T)
        logq.append(np.log(weights[k]) - 0.5 * (z * z).sum(0) - np.log(np.diag(L)).sum() - 0.5 * 34 * np.log(2 * np.pi))
    elbo = np.mean(ref.log_density(x) - logsumexp(np.stack(logq), axis=0))
    poses, _ = ref.fk(x)
    return elbo, float(np.median(np.linalg.norm(poses[:, 1, :3] - np.asarray(CONTEXT), axis=1)))


def test_talos_end_to_end(ref):
    from gmmvi_amd.configs import get_default_config, update_config
    from gmmvi_amd.gmmvi_runner import GmmviRunner
    cfg = update_config(get_default_config("SEMTRON", "talos"), {"environment_config": {"dataset_dir": GOLDEN_DIR}, "seed": 3})
    runner = GmmviRunner.build_from_config(cfg)
    assert runner.gmmvi._fast_path.eligible()

    def stats():
        m = runner.gmmvi.model
        covs = np.einsum("kij,klj->kil", m.chol_cov.numpy().astype(np.float64), m.chol_cov.numpy().astype(np.float64))
        return _mixture_stats(ref, np.random.default_rng(13), 4000, np.exp(m.log_weights.numpy().astype(np.float64)),
                              m.means.numpy().astype(np.float64), covs)
    elbo0, grip0 = stats()
    for _ in range(300):
        runner.gmmvi.train_iter()
    elbo1, grip1 = stats()
    metrics = runner.gmmvi.sample_selector.target_distribution.expensive_metrics(None, runner.gmmvi.model.means)
    print(f"Talos: ELBO {elbo0:.1f} -> {elbo1:.1f}, median left-gripper error {grip0:.3f} -> {grip1:.3f} m, "
          f"metrics at the means {metrics}")
    # first MI355X run (seed 3, 300 iterations): ELBO -17 504 -> 13.6, median gripper error 1.884 -> 0.046 m
    assert np.isfinite(elbo1) and elbo1 > elbo0 + 1e4 and elbo1 > -100.0
    assert grip1 < 0.15 and grip1 < 0.2 * grip0
