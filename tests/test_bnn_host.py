"""WINE Bayesian-neural-network target on the host (no GPU): the minibatch stream, the fp64 reference against a literal
restatement of the reference's forward pass and loss, its gradient, the names and defaults of the experiment, the dataset
directory, argument errors and the expensive metrics' batching."""
import os

import numpy as np
import pytest

from bnn_ref import GOLDEN, BNNRef, literal_forward, literal_mse, load_wine, stream_rows, unpack, write_dataset_dir
from helpers import use_host_context

from gmmvi_amd.experiments.target_distributions import bnn


@pytest.fixture
def host_ctx(monkeypatch):
    use_host_context(monkeypatch, bnn)


@pytest.fixture(scope="module")
def wine():
    return load_wine()


def test_fixture_is_small_and_holds_arrays_only():
    assert os.path.getsize(GOLDEN) < 1 << 20
    with np.load(GOLDEN, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(bnn.WINE_ARRAYS)
        assert z["features_train"].shape == (2938, 11) and z["labels_train"].shape == (2938,)
        assert z["features_test"].shape == (979, 11) and z["features_vali"].shape == (981, 11)
        assert z["features_train"].dtype == np.float32 and z["labels_train"].dtype == np.int32


# ---- the minibatch stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7, 2938, 4096, 4097])
def test_every_epoch_is_a_permutation(T):
    rows = bnn.minibatch_rows(seed=17, call=3, n=3, batch_size=T, num_data=T)      # sample i is exactly epoch i
    assert rows.shape == (3, T) and rows.dtype == np.int64
    for e in range(3):
        np.testing.assert_array_equal(np.sort(rows[e]), np.arange(T))
    # a batch that straddles epochs: the stream is the concatenation of the epochs' permutations
    b = max(1, (2 * T) // 3)
    flat = bnn.minibatch_rows(17, 3, 3, b, T).ravel()
    np.testing.assert_array_equal(flat, rows.ravel()[:3 * b])


@pytest.mark.parametrize("T,B", [(1, 1), (2, 1), (7, 3), (2938, 128), (2938, 2938), (4096, 100), (4097, 4097)])
def test_product_and_reference_streams_agree(T, B):
    for seed, call in ((0, 0), (10000, 5), (2 ** 40 + 3, 2 ** 32 - 1)):
        np.testing.assert_array_equal(bnn.minibatch_rows(seed, call, 5, B, T), stream_rows(seed, call, 5, B, T))


def test_stream_is_deterministic_and_moves_with_the_call_counter():
    a = bnn.minibatch_rows(3, 0, 400, 128, 2938)
    np.testing.assert_array_equal(a, bnn.minibatch_rows(3, 0, 400, 128, 2938))
    b = bnn.minibatch_rows(3, 1, 400, 128, 2938)
    c = bnn.minibatch_rows(4, 0, 400, 128, 2938)
    assert np.mean(a != b) > 0.99 and np.mean(a != c) > 0.99
    # every row of the training set is used about equally often over many batches
    counts = np.bincount(a.ravel(), minlength=2938)
    assert counts.min() >= 17 and counts.max() <= 18                    # 400 * 128 = 17.4 epochs


def test_feistel_width():
    assert [bnn.feistel_half_bits(t) for t in (1, 2, 3, 4, 5, 7, 2938, 4096, 4097)] == [0, 1, 1, 1, 2, 2, 6, 6, 7]


# ---- the fp64 reference ------------------------------------------------------------------------------------------------
def test_reference_equals_the_literal_forward_pass_and_loss(wine):
    X, y = wine["features_train"], wine["labels_train"]
    ref = BNNRef(X, y, likelihood_scaling=0.7, prior_std=1.3)
    rng = np.random.default_rng(1)
    w = rng.normal(size=(5, 177)) * 2.0
    rows = stream_rows(0, 0, 5, 128, len(y))
    lp, _ = ref.evaluate_rows(w, rows, want_grad=False)
    for i in range(5):
        out = literal_forward(X[rows[i]], w[i])
        ll = -len(y) * literal_mse(y[rows[i]], out)                         # bnn.py:177-180
        prior = -0.5 * np.sum(np.square(w[i] / 1.3))                         # bnn.py:217-219
        np.testing.assert_allclose(lp[i], 0.7 * (ll + prior), rtol=1e-12)
    # the layout: W1 [11, 8] row-major, b1, W2 [8, 8], b2, W3 [8, 1], b3 -> D = 177
    assert [a.shape for layer in unpack(w[0], 11) for a in layer] == [(11, 8), (8,), (8, 8), (8,), (8, 1), (1,)]


@pytest.mark.parametrize("hidden,F", [((8, 8), 11), ((3, 5), 4), ((16, 1), 2)])
def test_reference_gradient_agrees_with_central_differences(hidden, F):
    rng = np.random.default_rng(F)
    X = rng.normal(size=(50, F))
    y = rng.normal(size=50) + 5.0
    ref = BNNRef(X, y, hidden_units=hidden, likelihood_scaling=0.5, prior_std=2.0, batch_size=16)
    rows = stream_rows(1, 2, 3, 16, 50)
    w = rng.normal(size=(3, ref.D))
    _, g = ref.evaluate_rows(w, rows)
    h = 1e-6
    fd = np.empty_like(w)
    for d in range(ref.D):
        e = np.zeros(ref.D)
        e[d] = h
        fd[:, d] = (ref.evaluate_rows(w + e, rows, False)[0] - ref.evaluate_rows(w - e, rows, False)[0]) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_reference_call_counter(wine):
    ref = BNNRef(wine["features_train"], wine["labels_train"], seed=2)
    w = np.zeros((3, 177))
    ref.log_density(w)
    ref.log_density_and_grad(w)
    ref.log_density(np.zeros((0, 177)))
    assert ref.call_count == 2


# ---- names, defaults, datasets -----------------------------------------------------------------------------------------
def test_wine_name_resolves():
    from gmmvi_amd.experiments import setup_experiment as se
    assert se._lookup_target("WINE") == ("bnn", "make_WINE_target", se.CONFIG_AND_SEED)
    assert se._lookup_target("WINE_small") == ("bnn", "make_WINE_target", se.CONFIG_AND_SEED)


def test_default_experiment_config_is_wine_yml():
    from gmmvi_amd.configs import get_default_experiment_config
    assert get_default_experiment_config("wine") == {
        "start_seed": 10000, "environment_name": "WINE",
        "environment_config": {"likelihood_scaling": 1., "prior_std": 1., "batch_size": 128},
        "model_initialization": {"use_diagonal_covs": False, "num_initial_components": 4, "prior_mean": 0.,
                                 "prior_scale": 1., "initial_cov": 1.},
        "gmmvi_runner_config": {"log_metrics_interval": 25},
        "use_sample_database": True, "max_database_size": 500000, "temperature": 1.}


def test_run_seed_selects_the_split_and_keys_the_stream(tmp_path, wine, host_ctx):
    from gmmvi_amd.experiments import setup_experiment as se
    write_dataset_dir(tmp_path)
    other = dict(wine, labels_train=wine["labels_train"] + 1)                 # a different file for dataset seed 1
    np.savez(os.path.join(tmp_path, "wine", "wine_seed_1.npz"), **other)
    env = {"likelihood_scaling": 1., "prior_std": 1., "batch_size": 128, "dataset_dir": str(tmp_path)}
    t = se.get_target_lnpdf("WINE", env, 10000)
    assert isinstance(t, bnn.BNN_WINE)
    assert t.dataset_seed == 10000 and t.seed == 10000 and t.call_count == 0
    np.testing.assert_array_equal(t.labels, wine["labels_train"].astype(np.float32))
    np.testing.assert_array_equal(t.features, wine["features_train"])
    np.testing.assert_array_equal(t.eval_sets["test"][0], wine["features_test"])
    np.testing.assert_array_equal(t.eval_sets["vali"][1], wine["labels_vali"].astype(np.float32))
    assert t.get_num_dimensions() == 177 and t.use_log_density_and_grad
    t1 = se.get_target_lnpdf("WINE", env, 10001)
    np.testing.assert_array_equal(t1.labels, wine["labels_train"].astype(np.float32) + 1)
    with pytest.raises(AttributeError):
        t.call_count = 3


def test_dataset_directory_from_environment(monkeypatch, tmp_path, wine, host_ctx):
    write_dataset_dir(tmp_path)
    monkeypatch.setenv(bnn.DATASET_DIR_ENV, str(tmp_path))
    t = bnn.make_WINE_target(likelihood_scaling=1., dataset_seed=20, prior_std=1., batch_size=128)
    np.testing.assert_array_equal(t.features, wine["features_train"])


def test_missing_dataset_directory_says_what_to_set(monkeypatch, tmp_path):
    monkeypatch.delenv(bnn.DATASET_DIR_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="GMMVI_DATASET_DIR") as e:
        bnn.load_wine(0)
    assert "dataset_dir" in str(e.value)
    with pytest.raises(FileNotFoundError, match="wine_seed_3.npz") as e:
        bnn.load_wine(13, str(tmp_path))
    assert "GMMVI_DATASET_DIR" in str(e.value)


@pytest.mark.parametrize("kwargs,match", [
    ({"hidden_units": (17, 8)}, "hidden"), ({"hidden_units": (8, 0)}, "hidden"), ({"hidden_units": (8,)}, "two"),
    ({"features": np.zeros((50, 33))}, "features"), ({"features": np.zeros((50, 0))}, "features"),
    ({"batch_size": 51}, "batch_size"), ({"batch_size": 0}, "batch_size"), ({"prior_std": 0.0}, "prior_std"),
    ({"labels": np.zeros(49)}, "labels")])
def test_unsupported_shapes_raise(kwargs, match):
    args = {"features": np.zeros((50, 11)), "labels": np.zeros(50), "batch_size": 16}
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        bnn.BNNRegression(**args)


def test_expensive_metrics_batching(wine, host_ctx, monkeypatch):
    """bnn.py:290-310 restated: mean prediction over the samples, per-batch MSE and RMSE (batches of B rows in stored
    order, the last one partial), averaged over the batches; upstream's key names."""
    ref = BNNRef(wine["features_train"], wine["labels_train"])
    t = bnn.BNNRegression(wine["features_train"], wine["labels_train"], batch_size=128,
                          eval_sets={"test": (wine["features_test"], wine["labels_test"]),
                                     "vali": (wine["features_vali"], wine["labels_vali"])})
    monkeypatch.setattr(t, "predict", lambda samples, features: ref.predict(samples, features))
    w = np.random.default_rng(5).normal(size=(6, 177))
    m = t.expensive_metrics(None, w)
    assert sorted(m) == ["bi_test_accuracy", "bi_test_loss", "bi_vali_loss", "bi_vali_rmse"]
    for name, key_loss, key_metric in (("test", "bi_test_loss", "bi_test_accuracy"), ("vali", "bi_vali_loss", "bi_vali_rmse")):
        X, y = wine[f"features_{name}"], wine[f"labels_{name}"]
        losses, rmses = [], []
        for b0 in range(0, len(y), 128):
            out = sum(literal_forward(X[b0:b0 + 128], wi) for wi in w) / len(w)
            losses.append(literal_mse(y[b0:b0 + 128], out))
            rmses.append(np.sqrt(losses[-1]))
        assert len(losses) == 8                                              # 979 / 981 rows: 7 full batches + 1
        np.testing.assert_allclose(m[key_loss], np.mean(losses), rtol=1e-12)
        np.testing.assert_allclose(m[key_metric], np.mean(rmses), rtol=1e-12)
