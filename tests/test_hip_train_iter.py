"""End-to-end parity: GMMVI.train_iter() on the MI355X (fp32 HIP kernels through the C ABI) against the fp64 oracle on
identical Philox draws -- the "ELBO trajectory and final component parameters within a stated fp64->fp32 tolerance on
the same seed" requirement of the north star.  Tolerances: parameters rtol 1e-3 (they drift with the
number of iterations because every iteration re-samples from the slightly different fp32 model), identical
accept/reject decisions, ELBO within Monte-Carlo noise + 1e-2 nats."""
import numpy as np
import pytest

from helpers import samtron_config, make_oracle, make_device

pytestmark = pytest.mark.gpu


def run_pair(kind, d, k, s, seed, iters, cfg, check_every=1, tol_scale=1.0, fused=False):
    """``fused``: the single-call iteration (optimization/fused.py) instead of the module-by-module path (asking the updater
    for its probe counts, ``want_info``, makes the single-call path step aside)."""
    o = make_oracle(kind, d, k, s, seed, cfg)
    g = make_device(kind, d, k, s, seed, cfg, o)
    if fused:
        assert g._fast_path.eligible(), "this configuration was expected to take the single-call path"
    else:
        g.ng_based_updater.want_info = True
    worst = {}
    for it in range(iters):
        info = o.train_iter()
        g.train_iter()
        if it % check_every:
            continue
        om = o.model
        gm = g.model
        assert gm.num_components == om.num_components
        np.testing.assert_array_equal(gm.unique_component_ids, om.unique_component_ids, err_msg=f"iteration {it}")
        # fp32 drift compounds with the iteration count (every iteration re-samples from the slightly different fp32 model);
        # before it has started (iterations 0 and 1) the parameters agree to 5e-4
        tol = tol_scale * (5e-4 if it < 2 else 2e-3 * (1 + it))
        dev = {
            "means": np.abs(gm.means.numpy() - om.means).max() / max(1.0, np.abs(om.means).max()),
            "chols": np.abs(gm.chol_cov.numpy() - om.chol_cov).max() / np.abs(om.chol_cov).max(),
            "logw": np.abs(np.exp(gm.log_weights.numpy()) - om.weights).max(),
            "stepsizes": np.abs(gm.stepsizes.numpy() - om.stepsizes).max(),
        }
        for key, v in dev.items():
            worst[key] = max(worst.get(key, 0.0), v)
            assert v <= tol, f"iteration {it}: {key} deviates by {v:.3e} (> {tol:.1e})"
        if "success" in info and g.ng_based_updater.last_success is not None:
            np.testing.assert_array_equal(g.ng_based_updater.last_success.numpy().astype(bool), info["success"],
                                          err_msg=f"iteration {it}: accept/reject decisions differ")
        np.testing.assert_allclose(gm.last_log_etas.numpy(), om.last_log_etas, rtol=5e-3 * (1 + it), atol=1e-6)
        np.testing.assert_allclose(gm.num_received_updates.numpy(), om.num_received_updates)
        np.testing.assert_allclose(gm.reward_slot(0).numpy(), om.reward_history[:, -1],
                                   rtol=tol, atol=tol * (1 + np.abs(om.reward_history[:, -1]).max()))
    return o, g, worst


@pytest.mark.parametrize("kind,d,k,s", [("stm", 4, 3, 32), ("gmm", 4, 3, 32), ("planar", 10, 4, 50),
                                        ("gauss", 3, 1, 40), ("stm", 20, 8, 64)])
def test_trajectory_matches_oracle(kind, d, k, s):
    cfg = samtron_config(s)
    o, g, worst = run_pair(kind, d, k, s, seed=11, iters=12, cfg=cfg)
    elbo_o = o.elbo(4000, seed=5)[0]
    # ELBO of the device model evaluated by the *oracle* on the same draws (matched ELBO)
    o.model.model.means = g.model.means.numpy().astype(np.float64)
    o.model.model.chol_cov = g.model.chol_cov.numpy().astype(np.float64)
    o.model.model.log_weights = g.model.log_weights.numpy().astype(np.float64)
    elbo_g = o.elbo(4000, seed=5)[0]
    assert abs(elbo_g - elbo_o) < 1e-2 + 1e-3 * abs(elbo_o), (elbo_g, elbo_o, worst)


@pytest.mark.parametrize("d,k,s", [(32, 4, 80), (40, 5, 100), (50, 4, 120), (24, 6, 60)])
@pytest.mark.parametrize("fused", [False, True], ids=["modular", "single_call"])
def test_trajectory_wide_register_kernels(d, k, s, fused):
    """24 < D <= 50 at the DEFAULT blocked threshold: the composition bench.py's C3 workload times -- tiled Stein kernel
    (stein_partial<32|40|50>), update_kl_fast<DC>, wide mixture_eval -- on both the modular and the single-call path."""
    run_pair("gmm", d, k, s, seed=17, iters=8, cfg=samtron_config(s), fused=fused)


def test_north_star_full_size():
    """The north-star shape at full size (K = 100, D = 20, 100 samples per component = 10 000 samples per iteration,
    Student-t mixture target), two iterations against the fp64 oracle: parameters to 5e-4, identical accept / reject
    decisions, identical probe counts (modular path; the single-call path is then compared with it)."""
    cfg = samtron_config(100)
    o, g, worst = run_pair("stm", 20, 100, 100, seed=31, iters=2, cfg=cfg)
    np.testing.assert_array_equal(g.ng_based_updater.last_info[1].numpy(), o.last["n_probes"])
    # single-call path with the estimate materialised as the modules do it: bit for bit; its default route (the update kernel
    # whitens the Stein moment sums directly, csrc/update_kl.hip) differs by rounding only
    for explicit in (True, False):
        f = make_device("stm", 20, 100, 100, 31, cfg, make_oracle("stm", 20, 100, 100, 31, cfg))
        assert f._fast_path.eligible()
        f._fast_path.explicit_estimate = explicit
        for _ in range(2):
            f.train_iter()
        for name in ("means", "chol_cov", "log_weights", "stepsizes", "last_log_etas"):
            a, b = getattr(f.model, name).numpy(), getattr(g.model, name).numpy()
            if explicit:
                np.testing.assert_array_equal(a, b, err_msg=name)
            else:
                np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(b).max())), err_msg=name)
        assert f.sample_db.samples.shape == (20000, 20)


def test_gmm50_config_full_size():
    """BASELINE configs[2] at full size (GMM target, D = 50, K = 100, 100 samples per component = 10 000 samples per iteration):
    two iterations against the fp64 oracle on the single-call path -- matrix-core density sweeps, moment-form Stein estimate,
    four-wave update kernel with the inverse fragments, exactly the composition `bench.py --workload c3` times."""
    cfg = samtron_config(100)
    run_pair("gmm", 50, 100, 100, seed=41, iters=2, cfg=cfg, fused=True)


def test_planar_config_full_size():
    """BASELINE configs[3] at full size on one GPU (planar-4 target, D = 10, K = 200, 100 samples per component = 20 000
    samples per iteration): two iterations against the fp64 oracle, single-call path."""
    cfg = samtron_config(100)
    run_pair("planar", 10, 200, 100, seed=37, iters=2, cfg=cfg, fused=True)


@pytest.mark.parametrize("updater,wupd", [("direct", "direct"), ("iBLR", "trust-region")])
def test_other_design_choices(updater, wupd):
    cfg = samtron_config(40, initial_stepsize=0.01, updater=updater, weight_updater=wupd, wstep=0.05)
    run_pair("gmm", 4, 3, 40, seed=3, iters=6, cfg=cfg)


def test_non_self_normalised_and_own_samples():
    run_pair("gmm", 3, 3, 60, seed=5, iters=4, cfg=samtron_config(60, snis=False, initial_stepsize=0.01),
             tol_scale=3.0)
    run_pair("gmm", 3, 3, 60, seed=5, iters=4, cfg=samtron_config(60, own=True, initial_stepsize=0.05))


@pytest.mark.parametrize("kind,d,k,s", [("gmm", 4, 3, 120), ("stm", 10, 4, 300), ("gmm", 24, 2, 1500)])
def test_more_estimator_trajectory(kind, d, k, s):
    """MORE ("Z...") instead of Stein: fp32 normal equations carry ~1e-3 relative error into (H, g) per iteration."""
    cfg = samtron_config(s, estimator="MORE", initial_stepsize=0.05)
    run_pair(kind, d, k, s, seed=13, iters=6, cfg=cfg, tol_scale=5.0)


def test_sample_reuse_and_db_growth():
    """Default component-based selector: reuse ratio 2 => ESS-driven sample counts, K_b up to 3K background comps."""
    cfg = samtron_config(30, reuse_ratio=2.0)
    o, g, _ = run_pair("stm", 4, 3, 30, seed=7, iters=8, cfg=cfg)
    assert g.sample_db.samples.shape[0] == o.sample_db.samples.shape[0]
    assert int(g.sample_db.num_samples_written) == o.sample_db.num_samples_written
    np.testing.assert_array_equal(g.sample_db.mapping.numpy(), o.sample_db.mapping)


def _assert_db_equal(g, o, rtol=2e-2):
    db, odb = g.sample_db, o.sample_db
    assert db.samples.shape[0] == odb.samples.shape[0]
    assert int(db.num_samples_written) == odb.num_samples_written
    np.testing.assert_array_equal(db.mapping.numpy(), odb.mapping)
    np.testing.assert_array_equal(db.newest_mapping_host(10 ** 9), odb.mapping)
    assert db.means.shape[0] == odb.means.shape[0]
    scale = max(1.0, np.abs(odb.samples).max())
    np.testing.assert_allclose(db.samples.numpy(), odb.samples, rtol=rtol, atol=rtol * scale)
    np.testing.assert_allclose(db.means.numpy(), odb.means, rtol=rtol, atol=rtol * scale)
    np.testing.assert_allclose(db.chols.numpy(), odb.chols, rtol=rtol, atol=rtol * np.abs(odb.chols).max())
    np.testing.assert_allclose(db.target_lnpdfs.numpy(), odb.target_lnpdfs, rtol=rtol,
                               atol=rtol * (1 + np.abs(odb.target_lnpdfs).max()))


@pytest.mark.parametrize("reuse,fused,cap", [(2.0, False, 150), (0.0, False, 400), (0.0, True, 400)],
                         ids=["reuse2_modular", "reuse0_modular", "reuse0_single_call"])
def test_db_halving(reuse, fused, cap):
    """max_database_size small enough that add_samples thins the DB out (remove_every_nth_sample(2) incl. the
    first-occurrence re-indexing of ``mapping`` and the component snapshots, sample_db.py:63-79,111-112) at least twice."""
    cfg = samtron_config(30, reuse_ratio=reuse, max_database_size=cap)
    o = make_oracle("stm", 4, 3, 30, 7, cfg)
    g = make_device("stm", 4, 3, 30, 7, cfg, o)
    if not fused:
        g._fast_path.enabled = False
    halvings, last = 0, 0
    for it in range(14):
        o.train_iter()
        g.train_iter()
        if o.sample_db.samples.shape[0] < last + 1:
            halvings += 1
        last = o.sample_db.samples.shape[0]
        _assert_db_equal(g, o, rtol=2e-3 * (2 + it))
    assert halvings >= 2
    assert last <= cap
    np.testing.assert_allclose(g.model.means.numpy(), o.model.means, rtol=0.03, atol=0.03 * np.abs(o.model.means).max())


@pytest.mark.parametrize("reuse,own", [(0.0, False), (1.0, False), (0.0, True)], ids=["fresh", "reuse1", "own_samples"])
def test_mixture_based_selector(reuse, own):
    """sample_selector_type "mixture-based" (codename letter "P", sample_selector.py:221-339): draws from the whole mixture
    (categorical + per-component normals on their own Philox streams), mixture-level effective sample size."""
    cfg = samtron_config(150, reuse_ratio=reuse, selector="mixture-based", own=own, initial_stepsize=0.05)
    o, g, _ = run_pair("gmm", 4, 3, 150, seed=19, iters=6, cfg=cfg, tol_scale=2.0)
    _assert_db_equal(g, o)


def test_adaptive_components():
    ad = {"del_iters": 6, "add_iters": 3, "max_components": 6, "thresholds_for_add_heuristic": [50., 20., 10.],
          "min_weight_for_del_heuristic": 1e-6, "num_database_samples": 200, "num_prior_samples": 0}
    cfg = samtron_config(40, adaptive=ad)
    o, g, _ = run_pair("gmm", 3, 2, 40, seed=9, iters=14, cfg=cfg, tol_scale=3.0)
    assert g.model.num_components == o.model.num_components and g.model.num_components > 2
    np.testing.assert_array_equal(g.model.unique_component_ids, o.model.unique_component_ids)


def test_single_gaussian_known_answer():
    """Device SAMTRON on one Gaussian target converges to its mean / covariance (ELBO -> log Z = 0)."""
    cfg = samtron_config(300)
    o = make_oracle("gauss", 4, 1, 300, 21, cfg)
    g = make_device("gauss", 4, 1, 300, 21, cfg, o)
    for _ in range(80):
        g.train_iter()
    np.testing.assert_allclose(g.model.means.numpy()[0], o.target.means[0], atol=5e-3)
    np.testing.assert_allclose(g.model.covs[0], o.target.covs[0], rtol=5e-3, atol=5e-3)


def test_runner_and_example_surface(tmp_path):
    """The reference's example 5 flow (configs -> GmmviRunner -> iterate_and_log) through the drop-in alias."""
    from gmmvi.gmmvi_runner import GmmviRunner
    from gmmvi.configs import update_config, get_default_experiment_config, get_default_algorithm_config
    algorithm_config = get_default_algorithm_config("SAMTRON")
    environment_config = update_config(get_default_experiment_config("stm20"), {"start_seed": 0})
    used = {"num_component_adapter_config": {"del_iters": 100, "add_iters": 4},
            "component_stepsize_adapter_config": {"initial_stepsize": 0.1, "min_stepsize": 0.001, "max_stepsize": 1.},
            "sample_selector_config": {"desired_samples_per_component": 50, "ratio_reused_samples_to_desired": 0.},
            "weight_stepsize_adapter_config": {"initial_stepsize": 1},
            "model_initialization": {"num_initial_components": 5},
            "gmmvi_runner_config": {"log_metrics_interval": 5},
            "dump_gmm_path": str(tmp_path)}
    config = update_config(environment_config, update_config(algorithm_config, used))
    runner = GmmviRunner.build_from_config(config=config)
    elbos = []
    for n in range(11):
        metrics = runner.iterate_and_log(n)
        runner.log_to_disk(n)
        assert {"walltime", "num_samples", "num_components", "max_weight", "num_db_samples",
                "num_db_components"} <= set(metrics)
        if "-elbo" in metrics:
            elbos.append(-metrics["-elbo"])
            assert {"entropy", "target_density", "algo_time", "num_detected_modes"} <= set(metrics)
    runner.finalize()
    assert runner.gmmvi.model.num_components == 5 + 2          # added at iterations 4 and 8
    assert elbos[-1] > elbos[0]
    assert metrics["num_samples"] == sum(50 * k for k in [5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7])
    import glob
    assert len(glob.glob(str(tmp_path) + "/*/gmm_dump_*.npz")) == 11


# ---- committed golden fixtures (tests/golden/*.npz: inputs + oracle outputs; generated by make_golden.py) -----------
import glob as _glob
import os as _os

_GOLDEN = sorted(_glob.glob(_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden", "samtron_*.npz")))


@pytest.mark.parametrize("path", _GOLDEN, ids=[_os.path.basename(p) for p in _GOLDEN])
def test_device_reproduces_golden_trajectory(path):
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    from gmmvi_amd.experiments.target_distributions.gmm import GMM_LNPDF
    from gmmvi_amd.experiments.target_distributions.student_t_mixture import StudentTMixture_LNPDF
    from gmmvi_amd.experiments.target_distributions.planar_robot import PlanarRobot
    g = np.load(path)
    kind, d, s, seed, iters = str(g["kind"]), int(g["d"]), int(g["s"]), int(g["seed"]), int(g["iters"])
    if kind == "stm":
        tgt = StudentTMixture_LNPDF(g["target_weights"], g["target_means"], g["target_covs"], alpha=2)
    elif kind == "gmm":
        tgt = GMM_LNPDF(g["target_weights"], g["target_means"], g["target_covs"])
    else:
        tgt = PlanarRobot(d, 4)
    model = FullCovGMM(g["init_weights"], g["init_means"].astype(np.float32), g["init_covs"].astype(np.float32))
    model.seed = seed
    cfg = samtron_config(s)
    algo = GMMVI.build_from_config(cfg, tgt, GmmWrapper(model, 0.1, 1e-12, 400))
    algo.ng_based_updater.want_info = True
    for it in range(iters):
        algo.train_iter()
        tol = 2e-3 * (1 + it)
        m = algo.model
        assert np.abs(m.means.numpy() - g["means"][it]).max() <= tol * max(1.0, np.abs(g["means"][it]).max())
        assert np.abs(m.chol_cov.numpy() - g["chols"][it]).max() <= tol * np.abs(g["chols"][it]).max()
        assert np.abs(np.exp(m.log_weights.numpy()) - np.exp(g["log_weights"][it])).max() <= tol
        np.testing.assert_array_equal(algo.ng_based_updater.last_success.numpy().astype(bool), g["success"][it])
        np.testing.assert_allclose(m.stepsizes.numpy(), g["stepsizes"][it], rtol=1e-5)
        if it < 5:
            np.testing.assert_array_equal(algo.ng_based_updater.last_info[1].numpy(), g["n_probes"][it])


def test_extended_background_equals_the_window_mixture():
    """SampleDB.get_newest_samples extends the density it returned for the reused samples (effective-sample-size step) when the
    window grows by one append, instead of evaluating the whole window's mixture again (sample_db.py:216-227): the answer must be
    that mixture's density -- checked against a from-scratch evaluation of the same window and against the fp64 oracle database."""
    from oracle.sample_db import SampleDB as OracleDB
    from gmmvi_amd.optimization.sample_db import SampleDB
    from gmmvi_amd.device import get_context
    ctx = get_context()
    rng = np.random.default_rng(5)
    d, k = 6, 4
    db, odb = SampleDB(d, False, True, ctx=ctx), OracleDB(d, False, True)
    for it in range(4):
        means = rng.normal(size=(k, d)) * 2
        a = rng.normal(size=(k, d, d)) * 0.3
        chols = np.linalg.cholesky(a @ a.transpose(0, 2, 1) + np.eye(d))
        counts = rng.integers(1, 40, k)
        mapping = np.repeat(np.arange(k, dtype=np.int32), counts)
        xs = means[mapping] + np.einsum("nij,nj->ni", chols[mapping], rng.normal(size=(len(mapping), d)))
        n_before = db.samples.shape[0]
        if it > 0:
            db.get_newest_samples(150)                   # what a selector asks first: the reused samples
            assert db._bg_cache is not None
        args = (xs.astype(np.float32), means.astype(np.float32), chols.astype(np.float32), np.zeros(len(mapping), np.float32),
                np.zeros((len(mapping), d), np.float32), mapping)
        db.add_samples(*args, counts=counts)
        odb.add_samples(*[np.asarray(v, np.float64) if v.dtype != np.int32 else v for v in args])
        n_win = min(n_before, 150) + len(mapping)
        bg = db.get_newest_samples(n_win)[0].numpy()
        if it > 0:
            assert db._bg_cache is None                  # this answer was an extension
        fresh = db.get_newest_samples(n_win)[0].numpy()  # no cache now: the whole window's mixture on all of its samples
        np.testing.assert_allclose(bg, fresh, rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(bg, odb.get_newest_samples(n_win)[0], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("new_per_append", [(3, 9), (20, 60)])
def test_sliding_window_background_equals_the_window_mixture(new_per_append):
    """Once the database is longer than the reuse window, SampleDB.get_newest_samples keeps per-append partial densities of the
    window (rows of appends that stay wholly inside are moved, not recomputed): every answer must equal the window mixture's
    density evaluated from scratch and the fp64 oracle database's; appends of very different sizes, so that the window cuts
    through an append at most offsets and several appends leave it at once."""
    from oracle.sample_db import SampleDB as OracleDB
    from gmmvi_amd.optimization.sample_db import SampleDB
    from gmmvi_amd.device import get_context
    ctx = get_context()
    rng = np.random.default_rng(11)
    d, k, window = 5, 4, 150
    db, odb = SampleDB(d, False, True, ctx=ctx), OracleDB(d, False, True)
    used_rows = 0
    for it in range(14):
        means = rng.normal(size=(k, d)) * 2
        a = rng.normal(size=(k, d, d)) * 0.3
        chols = np.linalg.cholesky(a @ a.transpose(0, 2, 1) + np.eye(d))
        counts = rng.integers(new_per_append[0], new_per_append[1], k)
        if it % 5 == 4:
            counts[rng.integers(0, k)] = 0                      # a component without a sample in this append
        mapping = np.repeat(np.arange(k, dtype=np.int32), counts)
        xs = means[mapping] + np.einsum("nij,nj->ni", chols[mapping], rng.normal(size=(len(mapping), d)))
        args = (xs.astype(np.float32), means.astype(np.float32), chols.astype(np.float32), np.zeros(len(mapping), np.float32),
                np.zeros((len(mapping), d), np.float32), mapping)
        db.add_samples(*args, counts=counts)
        odb.add_samples(*[np.asarray(v, np.float64) if v.dtype != np.int32 else v for v in args])
        bg = db.get_newest_samples(window)[0].numpy()
        if db.samples.shape[0] > window:
            assert db._pd is not None and db._pd["stop"] == db.samples.shape[0]      # the sliding route answered
            used_rows += 1
            keep, db._pd, db._bg_cache = db._pd, None, None
            scratch = db._mixture_lp(*_window_mixture(db, window))                    # all components x all samples
            np.testing.assert_allclose(bg, scratch.numpy(), rtol=3e-6, atol=3e-6)
            db._pd = keep
        np.testing.assert_allclose(bg, odb.get_newest_samples(window)[0], rtol=1e-4, atol=1e-4)
    assert used_rows >= 5


def _window_mixture(db, window):
    start = db.samples.shape[0] - window
    active, counts = db._active_components(start)
    from gmmvi_amd import hip_ops
    packed = hip_ops.gather_rows(db.ctx, db._packed.view(), active.astype(np.int32))
    logw = db.ctx.asarray(np.log(counts / counts.sum()).astype(np.float32))
    return packed, logw, db._samples.view(start)


@pytest.mark.parametrize("fused", [False, True], ids=["modular", "single_call"])
def test_sample_reuse_with_adaptive_components(fused):
    """Reuse ratio 2 AND an adaptive number of components: the appends inside the sliding reuse window then have different
    numbers of components, components are added between appends, the window cuts through appends at varying offsets -- the
    per-append partial densities of SampleDB must keep reproducing the oracle's background densities (effective sample sizes
    decide how many samples every component draws: a wrong density changes the database sizes compared below)."""
    ad = {"del_iters": 7, "add_iters": 3, "max_components": 7, "thresholds_for_add_heuristic": [50., 20., 10.],
          "min_weight_for_del_heuristic": 1e-6, "num_database_samples": 100, "num_prior_samples": 0}
    cfg = samtron_config(30, reuse_ratio=2.0, adaptive=ad)
    o = make_oracle("gmm", 3, 2, 30, 9, cfg)
    g = make_device("gmm", 3, 2, 30, 9, cfg, o)
    if not fused:
        g._fast_path.enabled = False
    slid = 0
    for it in range(18):
        o.train_iter()
        g.train_iter()
        assert g.model.num_components == o.model.num_components
        np.testing.assert_array_equal(g.model.unique_component_ids, o.model.unique_component_ids, err_msg=f"iteration {it}")
        assert g.sample_db.samples.shape[0] == o.sample_db.samples.shape[0], f"iteration {it}: different numbers of new samples"
        slid += g.sample_db._pd is not None and g.sample_db._pd["stop"] >= g.sample_db.samples.shape[0] - 400
    assert g.model.num_components > 2 and slid >= 5
    np.testing.assert_array_equal(g.sample_db.mapping.numpy(), o.sample_db.mapping)
    dev = np.abs(g.model.means.numpy() - o.model.means).max() / max(1.0, np.abs(o.model.means).max())
    assert dev <= 0.1, dev


def test_bench_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: one JSON line with the headline fields and nothing
    from the --full legs; DIR holds the mixture after W + K iterations, the same as W + K train_iter() calls on the same
    workload give here."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["metric"] == "samples_components_per_sec" and line["unit"] == "samples*components/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 3
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"ms_per_step_steady", "roofline", "kernels", "cpu_baseline", "matched_elbo"} & set(line)
    sys.path.insert(0, root)
    import bench
    algo = bench.make_gmmvi(bench.build("tiny", 1, 0), 1, 0)
    for _ in range(1 + 3):
        algo.train_iter()
    for name, arr in (("log_weights", algo.model.log_weights), ("means", algo.model.means), ("chol_cov", algo.model.chol_cov)):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, arr.numpy(), rtol=1e-5, atol=1e-6)
