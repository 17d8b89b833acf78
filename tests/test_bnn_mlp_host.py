"""Generic Bayesian-neural-network target on the host (no GPU): the fp64 reference's gradient against central differences,
the ReLU margin of every committed case, the reference against the two specialised references on their network shapes,
argument errors, the parameter count, the metrics' keys and the declared symbols."""
import os
import re

import numpy as np
import pytest

import bnn_mlp_cases as cases
from bnn_classifier_ref import BNNClassifierRef
from bnn_mlp_ref import BNNMlpRef, num_parameters, unpack
from bnn_ref import BNNRef, stream_rows
from helpers import use_host_context

from gmmvi_amd.experiments.target_distributions import bnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSE, CE = cases.MSE, cases.CE


@pytest.fixture
def host_ctx(monkeypatch):
    use_host_context(monkeypatch, bnn)


# ---- the fp64 reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,acts,loss,C", [
    ((4,), ("linear",), MSE, 1), ((4,), ("sigmoid",), MSE, 1), ((4,), ("relu",), MSE, 1), ((4,), ("tanh",), MSE, 1),
    ((4,), ("linear",), CE, 3), ((4,), ("sigmoid",), CE, 3), ((4,), ("relu",), CE, 3), ((4,), ("tanh",), CE, 3),
    ((5, 3), ("tanh", "relu"), CE, 2), ((3, 4, 2), ("relu", "sigmoid", "tanh"), MSE, 1),
    ((3, 4, 2), ("sigmoid", "linear", "relu"), CE, 16)])
def test_reference_gradient_agrees_with_central_differences(hidden, acts, loss, C):
    rng = np.random.default_rng(len(hidden) * 100 + C)
    X = rng.normal(size=(50, 6))
    y = rng.normal(size=50) if loss == MSE else rng.integers(0, C, size=50)
    ref = BNNMlpRef(X, y, hidden, acts + ("linear",), loss, num_classes=C, likelihood_scaling=0.5, prior_std=2.0,
                    batch_size=16)
    rows = bnn.minibatch_rows(1, 2, 2, 16, 50)
    w = rng.normal(size=(2, ref.D)) * 0.5
    assert ref.min_abs_relu_preactivation(w, rows) > 1e-3            # the differences below stay on one side of the kink
    lp, g = ref.evaluate_rows(w, rows)
    eps = 1e-6
    for i in range(2):
        for d in range(ref.D):
            e = np.zeros(ref.D)
            e[d] = eps
            up = ref.evaluate_rows(w[i] + e, rows[i:i + 1], want_grad=False)[0][0]
            dn = ref.evaluate_rows(w[i] - e, rows[i:i + 1], want_grad=False)[0][0]
            assert abs((up - dn) / (2 * eps) - g[i, d]) <= 1e-6 * max(1.0, np.abs(g[i]).max()), (i, d)


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=lambda c: c["name"])
def test_every_committed_case_keeps_the_relu_margin(case):
    b = cases.build(case)
    assert b["W"].dtype == np.float32 and b["W"].shape == (case["N"], b["ref"].D)
    margin = b["ref"].min_abs_relu_preactivation(b["W"].astype(np.float64), b["rows"])
    print(f"{case['name']}: margin {margin:.3e} after {b['redraws']} redraws")
    assert margin >= cases.RELU_MARGIN
    assert np.all(np.isfinite(b["lp64"])) and np.all(np.isfinite(b["g64"]))
    if "relu" not in case["acts"]:
        assert b["redraws"] == 0 and margin == np.inf


def test_rows_are_the_products_minibatch_rows():
    np.testing.assert_array_equal(bnn.minibatch_rows(7, 3, 5, 37, 300), stream_rows(7, 3, 5, 37, 300))
    ref = BNNMlpRef(np.zeros((40, 2)), np.zeros(40), (2,), ("tanh", "linear"), MSE, batch_size=8, seed=2)
    np.testing.assert_array_equal(ref.next_rows(3), stream_rows(2, 0, 3, 8, 40))
    np.testing.assert_array_equal(ref.next_rows(3), stream_rows(2, 1, 3, 8, 40))
    ref.next_rows(0)
    assert ref.call_count == 2


def test_reference_equals_the_regression_reference_on_the_wine_shape():
    b = cases.build(cases.WINE_CASE)
    old = BNNRef(b["X"], b["y"], hidden_units=(8, 8), likelihood_scaling=cases.SCALING, prior_std=cases.PRIOR_STD,
                 batch_size=cases.WINE_CASE["B"], seed=cases.SEED)
    lp, g = old.evaluate_rows(b["W"].astype(np.float64), b["rows"])
    np.testing.assert_allclose(b["lp64"], lp, rtol=1e-12)
    np.testing.assert_allclose(b["g64"], g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
    np.testing.assert_allclose(b["ref"].predict(b["W"], b["X"][:9]), old.predict(b["W"], b["X"][:9].astype(np.float64)),
                               rtol=1e-12)


def test_reference_equals_the_classifier_reference_on_the_mnist_shape():
    b = cases.build(cases.MNIST_CASE)
    old = BNNClassifierRef(b["X"], b["y"], 10, hidden=128, likelihood_scaling=cases.SCALING, prior_std=cases.PRIOR_STD,
                           batch_size=cases.MNIST_CASE["B"], seed=cases.SEED)
    lp, g = old.evaluate_rows(b["W"].astype(np.float64), b["rows"])
    np.testing.assert_allclose(b["lp64"], lp, rtol=1e-12)
    np.testing.assert_allclose(b["g64"], g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
    np.testing.assert_allclose(b["ref"].predict(b["W"], b["X"][:9]), old.predict(b["W"], b["X"][:9]), rtol=1e-12,
                               atol=1e-12)


def test_fp32_mode_stays_in_single_precision():
    b = cases.build(cases.CASES[5])
    assert b["lp32"].dtype == np.float32 and b["g32"].dtype == np.float32
    e_lp, e_g = cases.errors(b["lp32"].astype(np.float64), b["g32"].astype(np.float64), b["lp64"], b["g64"])
    assert 0 < e_lp < 1e-5 and 0 < e_g < 1e-5


# ---- the parameter layout ----------------------------------------------------------------------------------------------
def test_num_parameters_against_the_layouts_by_hand():
    assert bnn.num_parameters(11, (8, 8)) == 11 * 8 + 8 + 8 * 8 + 8 + 8 + 1 == 177           # WINE, the default output width
    assert bnn.num_parameters(784, (128,), 10) == 784 * 128 + 128 + 128 * 10 + 10 == 101770  # MNIST
    assert bnn.num_parameters(784, (128, 64), 10) == 784 * 128 + 128 + 128 * 64 + 64 + 64 * 10 + 10
    assert bnn.num_parameters(3, (2, 4, 5), 1) == 3 * 2 + 2 + 2 * 4 + 4 + 4 * 5 + 5 + 5 + 1
    assert num_parameters(3, (2, 4, 5), 1) == bnn.num_parameters(3, (2, 4, 5), 1)
    (W1, b1), (W2, b2) = unpack(np.arange(bnn.num_parameters(3, (2,), 4), dtype=np.float64), 3, (2,), 4)
    np.testing.assert_array_equal(W1, [[0, 1], [2, 3], [4, 5]])                              # [in, out] row-major
    np.testing.assert_array_equal(b1, [6, 7])
    np.testing.assert_array_equal(W2, [[8, 9, 10, 11], [12, 13, 14, 15]])
    np.testing.assert_array_equal(b2, [16, 17, 18, 19])


# ---- arguments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,match", [
    ({"features": np.zeros((50, 1025))}, "1024"), ({"features": np.zeros((50, 0))}, "1024"),
    ({"hidden_units": (129,)}, "128"), ({"hidden_units": (8, 0)}, "128"), ({"hidden_units": ()}, "1 to 3 hidden"),
    ({"hidden_units": (8, 8, 8, 8), "activations": ("relu",) * 4 + ("linear",)}, "1 to 3 hidden"),
    ({"activations": ("relu",)}, "one activation per layer"), ({"activations": ("swish", "linear")}, "swish"),
    ({"activations": ("relu", "tanh")}, "'linear'"), ({"loss": "hinge"}, "loss"),
    ({"num_classes": None}, "num_classes is required"), ({"num_classes": 1}, r"\[2, 16\]"),
    ({"num_classes": 17}, r"\[2, 16\]"), ({"batch_size": 51}, r"\[1, 50\]"), ({"batch_size": 0}, "batch_size"),
    ({"features": np.zeros((1100, 11)), "labels": np.zeros(1100), "batch_size": 1025}, "1024"),
    ({"features": np.zeros((50, 1024)), "hidden_units": (128, 128)}, "131072"),
    ({"labels": np.full(50, 3)}, r"\[0, 3\)"), ({"labels": np.full(50, -1)}, r"\[0, 3\)"),
    ({"prior_std": 0.0}, "prior_std"), ({"labels": np.zeros(49)}, "labels")])
def test_unsupported_arguments_raise(kwargs, match):
    args = {"features": np.zeros((50, 11)), "labels": np.zeros(50), "num_classes": 3, "hidden_units": (8,),
            "activations": ("relu", "linear"), "loss": CE, "batch_size": 16}
    args.update(kwargs)
    if len(args["hidden_units"]) == 2 and len(args["activations"]) == 2:
        args["activations"] = ("relu", "relu", "linear")
    with pytest.raises(ValueError, match=match):
        bnn.BNN_LNPDF(**args)


def test_constructor_keeps_its_arguments_and_prepare_data_is_the_subclass_hook(host_ctx):
    X, y = np.zeros((50, 11)), np.arange(50) % 3
    t = bnn.BNN_LNPDF(likelihood_scaling=2., prior_std=3., batch_size=16, hidden_units=[8, 6], loss=CE,
                      activations=["tanh", "relu", "linear"], features=X, labels=y, num_classes=3, seed=5)
    assert t.hidden_units == (8, 6) and t.activations == ("tanh", "relu", "linear") and t.num_classes == 3
    assert (t.likelihood_scaling, t.prior_std, t.batch_size, t.seed, t.call_count) == (2., 3., 16, 5, 0)
    assert t.get_num_dimensions() == bnn.num_parameters(11, (8, 6), 3) and t.train_size == 50
    assert t.labels.dtype == np.int32 and t.use_log_density_and_grad
    with pytest.raises(AttributeError):
        t.call_count = 3
    r = bnn.BNN_LNPDF(features=X, labels=np.zeros(50), hidden_units=(4,), activations=("sigmoid", "linear"), batch_size=8)
    assert r.loss == MSE and r.num_classes is None and r.labels.dtype == np.float32
    assert r.get_num_dimensions() == bnn.num_parameters(11, (4,))
    with pytest.raises(NotImplementedError):
        bnn.BNN_LNPDF(hidden_units=(4,), activations=("sigmoid", "linear"))

    class Mine(bnn.BNN_LNPDF):
        def prepare_data(self):
            return X, np.zeros(50), {"test": (X[:5], np.zeros(5))}

    m = Mine(batch_size=8, hidden_units=(4,), loss=MSE, activations=("tanh", "linear"), dataset_seed=4)
    assert m.train_size == 50 and m.dataset_seed == 4 and sorted(m.eval_sets) == ["test"]


# ---- metrics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [MSE, CE])
def test_expensive_metrics_keys_and_batching(host_ctx, monkeypatch, loss):
    rng = np.random.default_rng(4)

    def data(n):
        return rng.normal(size=(n, 5)), (rng.normal(size=n) if loss == MSE else rng.integers(0, 3, size=n))

    X, y = data(60)
    sets = {"test": data(70), "vali": data(33)}
    acts = ("tanh", "relu", "linear")
    ref = BNNMlpRef(X, y, (4, 3), acts, loss, num_classes=3)
    t = bnn.BNN_LNPDF(features=X, labels=y, hidden_units=(4, 3), activations=acts, loss=loss, num_classes=3, batch_size=32,
                      eval_sets=sets)
    monkeypatch.setattr(t, "predict", lambda samples, features: ref.predict(samples, features))
    w = rng.normal(size=(6, ref.D))
    m = t.expensive_metrics(None, w)
    assert sorted(m) == ["bi_test_accuracy", "bi_test_loss", "bi_vali_accuracy", "bi_vali_loss"]
    for name, batches in (("test", 3), ("vali", 2)):                          # 70 = 32 + 32 + 6, 33 = 32 + 1
        Xe, ye = sets[name]
        out = ref.predict(w, Xe.astype(np.float32)).mean(0)                   # the target keeps its features in f32
        losses, seconds = [], []
        for b0 in range(0, len(ye), 32):
            o, yy = out[b0:b0 + 32], ye[b0:b0 + 32]
            if loss == MSE:
                losses.append(np.mean((yy.astype(np.float32) - o) ** 2))
                seconds.append(np.sqrt(losses[-1]))
            else:
                lse = np.log(np.exp(o).sum(1))
                losses.append(np.mean(lse - o[np.arange(len(yy)), yy]))
                seconds.append(np.mean(o.argmax(1) == yy))
        assert len(losses) == batches
        np.testing.assert_allclose(m[f"bi_{name}_loss"], np.mean(losses), rtol=1e-12)
        np.testing.assert_allclose(m[f"bi_{name}_accuracy"], np.mean(seconds), rtol=1e-12)
    assert t.expensive_metrics(None, w) == m and t.call_count == 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_new_symbols():
    import ctypes
    from gmmvi_amd import _lib, hip_ops
    with open(os.path.join(ROOT, "include", "gmmvi_hip.h")) as f:
        header = f.read()
    for name in ("gmmvi_target_mlp", "gmmvi_mlp_predict"):
        assert len(re.findall(rf"\bint {name}\(", header)) == 1
        assert _lib.EXPORTED_SYMBOLS.count(name) == 1
    assert "typedef struct gmmvi_mlp_desc" in header
    assert ctypes.sizeof(_lib.MlpDesc) == 4 * (1 + 5 + 4 + 1)                 # the header's field order, all int32
    d = hip_ops.mlp_desc(784, (128, 64), ("relu", "tanh", "linear"), CE, 10)
    assert d.n_layers == 3 and list(d.widths) == [784, 128, 64, 10, 0] and list(d.activations) == [2, 3, 0, 0] and d.loss == 1
    d = hip_ops.mlp_desc(11, (8, 8), ("sigmoid", "sigmoid", "linear"), MSE)
    assert d.n_layers == 3 and list(d.widths) == [11, 8, 8, 1, 0] and list(d.activations) == [1, 1, 0, 0] and d.loss == 0
    # the specialised entry points keep their limits
    assert (bnn.MAX_FEATURES, bnn.MAX_HIDDEN, bnn.MAX_CLASSIFIER_HIDDEN) == (32, 16, 128)
