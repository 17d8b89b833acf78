"""Minibatch logistic-regression targets on the host (no GPU): the batch map of DESIGN.md 6 against an independent
restatement and against upstream's literal ``start`` loop, its bijection and disjointness properties, the holdout and the
argument errors, the names and the defaults."""
import numpy as np
import pytest

from logreg_mb_ref import LogRegMbRef, batch_rows, rho, upstream_start_loop_rows
from logreg_ref import LogRegRef, load_tables

from gmmvi_amd.experiments.target_distributions import minibatch_stream
from gmmvi_amd.experiments.target_distributions import logistic_regression as lr

CASES = [(seed, call, T, B, own)
         for seed, call in ((0, 0), (10000, 7), (2 ** 40 + 3, 2 ** 32 - 1))
         for T in (569, 1000)
         for B in (1, 64, T)
         for own in (True, False)]


@pytest.mark.parametrize("seed,call,T,B,own", CASES)
def test_minibatch_rows_match_the_reference_restatement(seed, call, T, B, own):
    nb = lr.num_batches(T, B, own)
    assert nb == (T // B if own else 1)
    n = min(3 * nb + 5, 2000)
    rows = lr.minibatch_rows(seed, call, n, B, T, nb)
    assert rows.shape == (n, B) and rows.dtype == np.int64
    np.testing.assert_array_equal(rows, batch_rows(seed, call, n, B, T, nb))


@pytest.mark.parametrize("seed,call,T,B,own", CASES)
def test_upstream_start_loop_on_the_same_permutation_gives_the_same_rows(seed, call, T, B, own):
    nb = lr.num_batches(T, B, own)
    perm = rho(seed, call, np.arange(T), T)                  # the call's shuffled order of the training rows
    n = min(2 * nb + 3, 1500)
    np.testing.assert_array_equal(lr.minibatch_rows(seed, call, n, B, T, nb),
                                  upstream_start_loop_rows(perm, n, B, own))


@pytest.mark.parametrize("T", [1, 2, 5, 64, 569, 1000, 4097])
def test_each_call_permutes_the_training_rows(T):
    for seed, call in ((0, 0), (3, 1), (10000, 12)):
        perm = lr.minibatch_rows(seed, call, 1, T, T, 1)[0]
        np.testing.assert_array_equal(np.sort(perm), np.arange(T))


@pytest.mark.parametrize("T,B", [(569, 64), (1000, 64), (1000, 7), (569, 1)])
def test_batches_of_a_call_are_disjoint_and_vary_with_call_and_seed(T, B):
    nb = T // B
    rows = lr.minibatch_rows(5, 3, nb, B, T, nb)
    assert len(np.unique(rows)) == nb * B                    # the nb classes cover nb B distinct rows
    more = lr.minibatch_rows(5, 3, 3 * nb, B, T, nb)
    np.testing.assert_array_equal(more[nb:2 * nb], rows)     # sample n takes batch n mod nb
    other_call = lr.minibatch_rows(5, 4, nb, B, T, nb)
    other_seed = lr.minibatch_rows(6, 3, nb, B, T, nb)
    assert np.mean(other_call != rows) > 0.9 and np.mean(other_seed != rows) > 0.9


def test_stream_ids_are_separate_and_wine_keeps_its_own():
    p = np.arange(569)
    wine = minibatch_stream.permute_rows(7, 2, np.zeros_like(p), p, 569)
    np.testing.assert_array_equal(wine, minibatch_stream.permute_rows(7, 2, np.zeros_like(p), p, 569, stream=3))
    mb = minibatch_stream.permute_rows(7, 2, np.zeros_like(p), p, 569, stream=lr.STREAM_MINIBATCH)
    np.testing.assert_array_equal(mb, rho(7, 2, p, 569))
    assert np.mean(mb != wine) > 0.9


@pytest.mark.parametrize("dataset_id", ["breast_cancer", "german_credit"])
def test_reference_at_full_batch_equals_the_full_data_posterior(dataset_id):
    A, D = lr.preprocess(load_tables()[dataset_id], dataset_id)
    ref = LogRegMbRef(A, A.shape[0], use_own_batch_per_sample=False, seed=4)
    w = np.random.default_rng(0).normal(size=(6, D))
    lp, g = ref.evaluate_rows(w, ref.rows(0, 6))
    lp_fb, g_fb = LogRegRef(A).log_density_and_grad(w)
    np.testing.assert_allclose(lp, lp_fb, rtol=1e-12)
    np.testing.assert_allclose(g, g_fb, rtol=1e-10, atol=1e-10 * np.abs(g_fb).max())
    np.testing.assert_allclose(ref.log_density_fb(w), lp_fb, rtol=1e-12)


def test_reference_gradient_agrees_with_central_differences():
    A, D = lr.preprocess(load_tables()["breast_cancer"], "breast_cancer")
    ref = LogRegMbRef(A, 64, seed=1)
    w = np.random.default_rng(2).normal(size=(10, D)) * 0.5
    rows = ref.rows(3, 10)
    _, g = ref.evaluate_rows(w, rows)
    h = 1e-5
    fd = np.empty_like(w)
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd[:, d] = (ref.evaluate_rows(w + e, rows, False)[0] - ref.evaluate_rows(w - e, rows, False)[0]) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())


# ---- holdout and argument errors (host-side checks, before anything reaches the device) ------------------------------
def _minibatch(monkeypatch, **kw):
    """LogisticRegressionMinibatch with the device calls stubbed: the constructor's checks and bookkeeping only."""
    monkeypatch.setattr(lr, "get_context", lambda: _NoDevice())
    return lr.LogisticRegressionMinibatch(**kw)


class _NoDevice:
    def asarray(self, a):
        return a


@pytest.mark.parametrize("dataset_id,rows", [("breast_cancer", 569), ("german_credit", 1000)])
def test_holdout_keeps_the_first_rows_in_file_order(monkeypatch, dataset_id, rows):
    data = load_tables()[dataset_id]
    A, D = lr.preprocess(data, dataset_id)
    for s in (0, 1, 100):
        t = _minibatch(monkeypatch, dataset_id=dataset_id, data=data, batch_size=64, size_test_set=s,
                       use_own_batch_per_sample=True, seed=9)
        assert t.num_data == rows - s and t.get_num_dimensions() == D
        np.testing.assert_array_equal(t.A, A[:rows - s])
        np.testing.assert_array_equal(t.A_test, A[rows - s:])
        assert t.num_batches == (rows - s) // 64 and t.call_count == 0 and t.seed == 9
    t = _minibatch(monkeypatch, dataset_id=dataset_id, data=data, batch_size=64, size_test_set=0,
                   use_own_batch_per_sample=False)
    assert t.num_batches == 1
    assert not hasattr(t, "_fast_path_target")               # the single-call iteration must not take it


def test_argument_errors(monkeypatch):
    data = load_tables()["breast_cancer"]
    kw = dict(dataset_id="breast_cancer", data=data, use_own_batch_per_sample=True)
    with pytest.raises(ValueError, match="batch_size"):
        _minibatch(monkeypatch, batch_size=570, size_test_set=0, **kw)
    with pytest.raises(ValueError, match="batch_size"):
        _minibatch(monkeypatch, batch_size=500, size_test_set=100, **kw)       # B > T = 469
    with pytest.raises(ValueError, match="batch_size"):
        _minibatch(monkeypatch, batch_size=0, size_test_set=0, **kw)
    for s in (569, 600, -1):
        with pytest.raises(ValueError, match="size_test_set"):
            _minibatch(monkeypatch, batch_size=1, size_test_set=s, **kw)
    with pytest.raises(ValueError, match="prior_std"):
        _minibatch(monkeypatch, batch_size=64, size_test_set=0, prior_std=0.0, **kw)
    with pytest.raises(ValueError, match="dimensions"):
        _minibatch(monkeypatch, X=np.ones((10, 129)), labels=np.zeros(10), batch_size=5, size_test_set=0)
    t = _minibatch(monkeypatch, batch_size=569, size_test_set=0, **kw)          # B = T: one batch
    assert t.num_batches == 1


# ---- names and defaults ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exp_id,name", [("breast_cancer_mb", "breastCancer_mb"), ("german_credit_mb", "GermanCredit_mb")])
def test_default_experiment_configs_are_the_yml_values(exp_id, name):
    from gmmvi_amd.configs import get_default_experiment_config
    c = get_default_experiment_config(exp_id)
    assert c == {"start_seed": 10000, "environment_name": name,
                 "environment_config": {"batch_size": 64, "size_test_set": 0, "use_own_batch_per_sample": True},
                 "model_initialization": {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0.,
                                          "prior_scale": 10., "initial_cov": 100.},
                 "gmmvi_runner_config": {"log_metrics_interval": 20},
                 "use_sample_database": True, "max_database_size": 10000000, "temperature": 1.}


def test_names_resolve_exactly_and_take_the_run_seed(monkeypatch):
    from gmmvi_amd.experiments import setup_experiment as se
    assert se._lookup_target("breastCancer_mb") == ("logistic_regression", "make_breast_cancer_mb", se.CONFIG_AND_RUN_SEED)
    assert se._lookup_target("GermanCredit_mb") == ("logistic_regression", "make_german_credit_mb", se.CONFIG_AND_RUN_SEED)
    assert se._lookup_target("breastCancer_mbx") is None and se._lookup_target("GermanCredit_m") is None
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return "target"
    monkeypatch.setattr(lr, "make_german_credit_mb", fake)
    env = {"batch_size": 32, "size_test_set": 10, "use_own_batch_per_sample": False, "dataset_dir": "d"}
    assert se.get_target_lnpdf("GermanCredit_mb", env, 77) == "target"
    assert seen == dict(env, seed=77)


def test_missing_minibatch_keys_are_refused_before_the_factory():
    from gmmvi_amd.experiments import setup_experiment as se
    for name in ("breastCancer_mb", "GermanCredit_mb"):
        with pytest.raises(ValueError) as e:
            se.get_target_lnpdf(name, {"batch_size": 64, "size_test_set": 0}, 0)
        msg = str(e.value)
        assert "use_own_batch_per_sample" in msg and "batch_size" not in msg.split("needs")[1].split("in env")[0]
        assert "minibatch" in msg and "not supported" in msg and name in msg and "unknown" not in msg
