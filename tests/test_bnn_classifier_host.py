"""MNIST-style Bayesian-neural-network classification target on the host (no GPU): the fp64 reference against a literal
restatement of the reference's forward pass and loss, its gradient and log-softmax, the parameter layout, the MNIST loader,
argument errors, the expensive metrics' batching and the declared symbols."""
import os
import re

import numpy as np
import pytest

from bnn_classifier_ref import (BNNClassifierRef, literal_cross_entropy, literal_forward, log_softmax, num_parameters,
                                offsets, separable_data, unpack, write_mnist_dir)
from bnn_ref import stream_rows
from helpers import use_host_context

from gmmvi_amd.experiments.target_distributions import bnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def host_ctx(monkeypatch):
    use_host_context(monkeypatch, bnn)


# ---- the fp64 reference ------------------------------------------------------------------------------------------------
def test_reference_equals_the_literal_forward_pass_and_loss():
    rng = np.random.default_rng(0)
    X, y = separable_data(90, 13, 4, rng)
    ref = BNNClassifierRef(X, y, 4, hidden=6, likelihood_scaling=0.7, prior_std=1.3, batch_size=32)
    w = rng.normal(size=(5, ref.D))
    rows = stream_rows(0, 0, 5, 32, 90)
    lp, _ = ref.evaluate_rows(w, rows, want_grad=False)
    for i in range(5):
        out = literal_forward(X[rows[i]], w[i], 6, 4)
        ll = -90 * literal_cross_entropy(y[rows[i]], out)                    # bnn.py:177-180 with BNN_MNIST's loss
        prior = -0.5 * np.sum(np.square(w[i] / 1.3))                         # bnn.py:228-230
        np.testing.assert_allclose(lp[i], 0.7 * (ll + prior), rtol=1e-12)
    np.testing.assert_allclose(ref.predict(w, X[:7])[2], literal_forward(X[:7], w[2], 6, 4), rtol=1e-13)


@pytest.mark.parametrize("F,H,C", [(5, 4, 3), (2, 7, 2), (9, 3, 16)])
def test_reference_gradient_agrees_with_central_differences(F, H, C):
    rng = np.random.default_rng(F)
    X, y = separable_data(50, F, C, rng)
    ref = BNNClassifierRef(X, y, C, hidden=H, likelihood_scaling=0.5, prior_std=2.0, batch_size=16)
    rows = stream_rows(1, 2, 3, 16, 50)
    while True:                                                               # stay away from the ReLU kink
        w = rng.normal(size=(3, ref.D))
        if ref.min_abs_preactivation(w, rows) >= 1e-3:
            break
    _, g = ref.evaluate_rows(w, rows)
    h = 1e-6
    fd = np.empty_like(w)
    for d in range(ref.D):
        e = np.zeros(ref.D)
        e[d] = h
        fd[:, d] = (ref.evaluate_rows(w + e, rows, False)[0] - ref.evaluate_rows(w - e, rows, False)[0]) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_reference_log_softmax_is_scipys():
    from scipy import special
    l = np.random.default_rng(2).normal(size=(40, 10)) * 30.0
    np.testing.assert_allclose(log_softmax(l), special.log_softmax(l, axis=-1), rtol=1e-13, atol=1e-13)


def test_parameter_count_and_layout():
    assert num_parameters(784, 128, 10) == 101770
    assert bnn.classifier_num_parameters(784, 128, 10) == 101770
    assert offsets(784, 128, 10) == (0, 100352, 100480, 101760, 101770)
    w = np.arange(num_parameters(3, 2, 4), dtype=np.float64)
    W1, b1, W2, b2 = unpack(w, 3, 2, 4)
    np.testing.assert_array_equal(W1, [[0, 1], [2, 3], [4, 5]])               # [F, H] row-major
    np.testing.assert_array_equal(b1, [6, 7])
    np.testing.assert_array_equal(W2, [[8, 9, 10, 11], [12, 13, 14, 15]])     # [H, C] row-major
    np.testing.assert_array_equal(b2, [16, 17, 18, 19])


def test_reference_call_counter():
    X, y = separable_data(40, 3, 2, np.random.default_rng(0))
    ref = BNNClassifierRef(X, y, 2, hidden=2, batch_size=8, seed=2)
    w = np.zeros((3, ref.D))
    ref.log_density(w)
    ref.log_density_and_grad(w)
    ref.log_density(np.zeros((0, ref.D)))
    assert ref.call_count == 2


# ---- the loader --------------------------------------------------------------------------------------------------------
def test_loader_normalises_and_splits(tmp_path, host_ctx):
    d, arrays = write_mnist_dir(tmp_path, 64, 10000)
    data = bnn.load_mnist(d)
    assert data["features_train"].dtype == np.float32 and data["features_train"].shape == (64, 784)
    np.testing.assert_array_equal(data["features_train"],
                                  arrays["x_train"].reshape(64, 784).astype(np.float32) / np.float32(255))   # true division
    assert not np.array_equal(data["features_train"],
                              arrays["x_train"].reshape(64, 784).astype(np.float32) * np.float32(1 / 255))
    assert data["labels_train"].dtype == np.int32
    np.testing.assert_array_equal(data["labels_train"], arrays["y_train"])
    assert data["features_test"].shape == (5000, 784) and data["features_vali"].shape == (5000, 784)
    np.testing.assert_array_equal(data["labels_test"], arrays["y_test"][:5000])            # take(5000)
    np.testing.assert_array_equal(data["labels_vali"], arrays["y_test"][5000:])            # skip(5000)
    np.testing.assert_array_equal(data["features_vali"][0], arrays["x_test"][5000].ravel() / np.float32(255))


def test_loader_splits_a_short_file_in_halves(tmp_path, host_ctx, monkeypatch):
    d, arrays = write_mnist_dir(tmp_path, 40, 30)
    monkeypatch.setenv(bnn.DATASET_DIR_ENV, d)
    t = bnn.make_MNIST_target(likelihood_scaling=2., prior_std=3., batch_size=8, seed=5)
    assert isinstance(t, bnn.BNN_MNIST) and isinstance(t, bnn.BNNClassification)
    assert t.get_num_dimensions() == 101770 and t.train_size == 40 and t.call_count == 0 and t.seed == 5
    assert t.hidden_units == (128,) and t.num_classes == 10 and t.use_log_density_and_grad
    assert (t.likelihood_scaling, t.prior_std, t.batch_size) == (2., 3., 8)
    assert t.eval_sets["test"][0].shape == (15, 784) and t.eval_sets["vali"][0].shape == (15, 784)
    np.testing.assert_array_equal(t.eval_sets["test"][1], arrays["y_test"][:15])
    np.testing.assert_array_equal(t.eval_sets["vali"][1], arrays["y_test"][15:])
    with pytest.raises(AttributeError):
        t.call_count = 3


def test_missing_dataset_says_what_to_set(monkeypatch, tmp_path):
    monkeypatch.delenv(bnn.DATASET_DIR_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="GMMVI_DATASET_DIR") as e:
        bnn.load_mnist()
    assert "dataset_dir" in str(e.value) and "mnist.npz" in str(e.value)
    with pytest.raises(FileNotFoundError, match="mnist.npz") as e:
        bnn.load_mnist(str(tmp_path))
    assert "GMMVI_DATASET_DIR" in str(e.value) and "x_train" in str(e.value)


def test_mnist_has_no_experiment_name():
    from gmmvi_amd.experiments import setup_experiment as se
    assert se._lookup_target("MNIST") is None
    with pytest.raises(ValueError, match="unknown experiment name"):
        se.get_target_lnpdf("MNIST", {}, 0)


# ---- arguments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,match", [
    ({"features": np.zeros((50, 1025))}, "1024"), ({"features": np.zeros((50, 0))}, "1024"),
    ({"hidden_units": (129,)}, "128"), ({"hidden_units": (0,)}, "128"), ({"hidden_units": (8, 8)}, "one hidden"),
    ({"num_classes": 1}, r"\[2, 16\]"), ({"num_classes": 17}, r"\[2, 16\]"),
    ({"batch_size": 51}, r"\[1, 50\]"), ({"batch_size": 0}, "batch_size"),
    ({"features": np.zeros((1100, 11)), "labels": np.zeros(1100), "batch_size": 1025}, "1024"),
    ({"labels": np.full(50, 3)}, r"\[0, 3\)"), ({"labels": np.full(50, -1)}, r"\[0, 3\)"),
    ({"prior_std": 0.0}, "prior_std"), ({"labels": np.zeros(49)}, "labels")])
def test_unsupported_shapes_raise(kwargs, match):
    args = {"features": np.zeros((50, 11)), "labels": np.zeros(50), "num_classes": 3, "hidden_units": (8,),
            "batch_size": 16}
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        bnn.BNNClassification(**args)


# ---- metrics -----------------------------------------------------------------------------------------------------------
def test_expensive_metrics_batching(host_ctx, monkeypatch):
    """bnn.py:290-310 restated: mean logits over the samples, per-batch cross-entropy and accuracy (batches of B rows in
    stored order, the last one partial), averaged over the batches; BNN_MNIST's key names."""
    rng = np.random.default_rng(4)
    X, y = separable_data(60, 5, 3, rng)
    sets = {"test": separable_data(70, 5, 3, rng), "vali": separable_data(33, 5, 3, rng)}
    ref = BNNClassifierRef(X, y, 3, hidden=4)
    t = bnn.BNNClassification(X, y, 3, hidden_units=(4,), batch_size=32, eval_sets=sets)
    monkeypatch.setattr(t, "predict", lambda samples, features: ref.predict(samples, features))
    w = rng.normal(size=(6, ref.D))
    m = t.expensive_metrics(None, w)
    assert sorted(m) == ["bi_test_accuracy", "bi_test_loss", "bi_vali_accuracy", "bi_vali_loss"]
    for name, batches in (("test", 3), ("vali", 2)):                          # 70 = 32 + 32 + 6, 33 = 32 + 1
        Xe, ye = sets[name]
        losses, accuracies = [], []
        for b0 in range(0, len(ye), 32):
            out = sum(literal_forward(Xe[b0:b0 + 32], wi, 4, 3) for wi in w) / len(w)
            losses.append(literal_cross_entropy(ye[b0:b0 + 32], out))
            accuracies.append(np.mean(np.argmax(out, 1) == ye[b0:b0 + 32]))
        assert len(losses) == batches
        np.testing.assert_allclose(m[f"bi_{name}_loss"], np.mean(losses), rtol=1e-12)
        np.testing.assert_allclose(m[f"bi_{name}_accuracy"], np.mean(accuracies), rtol=1e-12)
    assert 0.0 <= m["bi_test_accuracy"] <= 1.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_new_symbols():
    from gmmvi_amd import _lib
    with open(os.path.join(ROOT, "include", "gmmvi_hip.h")) as f:
        header = f.read()
    for name in ("gmmvi_target_bnn_classifier", "gmmvi_bnn_classifier_predict"):
        assert len(re.findall(rf"\bint {name}\(", header)) == 1
        assert _lib.EXPORTED_SYMBOLS.count(name) == 1
    # the regression entry points keep their limits
    assert (bnn.MAX_FEATURES, bnn.MAX_HIDDEN) == (32, 16)
