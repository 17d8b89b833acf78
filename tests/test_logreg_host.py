"""Logistic-regression targets on the host (no GPU): the preprocessing of the data tables, the fp64 reference of the
posterior and its gradient, the names and defaults of the two experiments, the dataset directory, the fixture."""
import os

import numpy as np
import pytest

from logreg_ref import GOLDEN, LogRegRef, literal_log_density, literal_preprocess, load_tables, write_dataset_dir

from gmmvi_amd.experiments.target_distributions import logistic_regression as lr


@pytest.fixture(scope="module")
def tables():
    return load_tables()


def test_fixture_is_small_and_holds_arrays_only():
    assert os.path.getsize(GOLDEN) < 1 << 20
    with np.load(GOLDEN, allow_pickle=False) as z:
        assert sorted(z.files) == ["breast_cancer", "german_credit"]
        assert z["breast_cancer"].shape == (569, 32) and z["german_credit"].shape == (1000, 25)
        assert z["breast_cancer"].dtype == np.float64 and z["german_credit"].dtype == np.float64


@pytest.mark.parametrize("dataset_id,d", [("breast_cancer", 31), ("german_credit", 25)])
def test_preprocessing_matches_the_reference_steps(tables, dataset_id, d):
    data = tables[dataset_id]
    A, D = lr.preprocess(data, dataset_id)
    assert D == d and A.shape == (data.shape[0], d) and A.dtype == np.float32
    X, labels = literal_preprocess(data, dataset_id)
    assert set(np.unique(labels)) == {0.0, 1.0}
    s = np.where(labels == 1, -1.0, 1.0)
    np.testing.assert_array_equal(A.astype(np.float64), s[:, None] * X)     # exact: sign flip of the f32 values
    np.testing.assert_array_equal(np.abs(A[:, 0]), 1.0)                     # bias first
    np.testing.assert_array_equal(A[:, 0], s)
    # ddof 0: every standardised feature column has population std 1
    np.testing.assert_allclose(np.std(X[:, 1:], 0), 1.0, rtol=1e-6)


@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_signed_form_equals_the_literal_formula(tables, dataset_id):
    data = tables[dataset_id]
    A, D = lr.preprocess(data, dataset_id)
    X, labels = literal_preprocess(data, dataset_id)
    ref = LogRegRef(A)
    rng = np.random.default_rng(3)
    for scale in (0.1, 1.0, 10.0):
        w = rng.normal(size=(9, D)) * scale
        lit = literal_log_density(X, labels, w)
        np.testing.assert_allclose(ref.log_density(w), lit, rtol=1e-11, atol=1e-9 * (1 + ref.abs_terms(w)).max())


@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_gradient_agrees_with_central_differences(tables, dataset_id):
    A, D = lr.preprocess(tables[dataset_id], dataset_id)
    ref = LogRegRef(A)
    rng = np.random.default_rng(4)
    w = rng.normal(size=(3, D)) * 0.5
    _, g = ref.log_density_and_grad(w)
    h = 1e-5
    fd = np.empty_like(w)
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd[:, d] = (ref.log_density(w + e) - ref.log_density(w - e)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_large_arguments_stay_finite():
    A = np.array([[1.0, 0.0], [-1.0, 0.0], [0.5, 0.5]])
    ref = LogRegRef(A)
    w = np.array([[1e4, 0.0], [-1e4, 0.0], [1e4, 1e4]])
    lp, g = ref.log_density_and_grad(w)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    # log sigma(-1e4) = -1e4 exactly in fp64; log sigma(1e4) = 0
    t = w @ A.T
    np.testing.assert_allclose(lp - ref._prior(w), np.minimum(t, 0).sum(1), rtol=1e-12)


@pytest.mark.parametrize("exp_id,name,interval", [("breast_cancer", "breastCancer", 50), ("german_credit", "GermanCredit", 20)])
def test_default_experiment_configs(exp_id, name, interval):
    from gmmvi_amd.configs import get_default_experiment_config
    c = get_default_experiment_config(exp_id)
    assert c["environment_name"] == name and c["environment_config"] == {}
    assert c["start_seed"] == 10000
    assert c["model_initialization"] == {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0.,
                                         "prior_scale": 10., "initial_cov": 100.}
    assert c["gmmvi_runner_config"]["log_metrics_interval"] == interval
    assert c["use_sample_database"] is True and c["max_database_size"] == 10000000 and c["temperature"] == 1.


def test_names_resolve_and_minibatch_variants_are_refused():
    from gmmvi_amd.experiments import setup_experiment as se
    assert se._lookup_target("breastCancer") == ("logistic_regression", "make_breast_cancer", True)
    assert se._lookup_target("GermanCredit") == ("logistic_regression", "make_german_credit", True)
    for name in ("breastCancer_mb", "GermanCredit_mb"):
        with pytest.raises(ValueError) as e:
            se.get_target_lnpdf(name, {}, 0)
        msg = str(e.value)
        assert "minibatch" in msg and "not supported" in msg and name in msg and "unknown" not in msg


def test_missing_dataset_directory_says_what_to_set(monkeypatch, tmp_path):
    monkeypatch.delenv(lr.DATASET_DIR_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="GMMVI_DATASET_DIR") as e:
        lr.load_table("breast_cancer")
    assert "dataset_dir" in str(e.value)
    with pytest.raises(FileNotFoundError, match="breast_cancer.data"):
        lr.load_table("breast_cancer", str(tmp_path))


def test_dataset_directory_from_environment(monkeypatch, tmp_path, tables):
    write_dataset_dir(tmp_path)
    monkeypatch.setenv(lr.DATASET_DIR_ENV, str(tmp_path))
    for key in ("breast_cancer", "german_credit"):
        np.testing.assert_array_equal(lr.load_table(key), tables[key])
    np.testing.assert_array_equal(lr.load_table("german_credit", str(tmp_path)), tables["german_credit"])


def test_unknown_dataset_id():
    with pytest.raises(ValueError, match="logistic-regression dataset"):
        lr.split_table(np.zeros((3, 4)), "wine")
