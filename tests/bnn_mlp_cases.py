"""Case builders of the generic BNN tests: seeded small data sets and weight draws.

Every factor of the kernel (csrc/bnn_mlp.hip) is swept once, in combined cases rather than a full product: depth 1 - 3,
each activation in a hidden layer and mixed per layer, both losses with C = 2 and 16, F around the 32-feature tile
(1, 31, 32, 33, 65) and at the cap, H around the 16-wide MFMA tile and at the cap (1, 15, 16, 17, 64, 128), B around the
64-row chunk (63, 64, 65) and around two chunks (1, 127, 128, 129, 300), T = 37 and 300 (no power of two: the Feistel walk
cycles), B = T, N = 1 and 5.

ReLU cases: a weight vector whose fp64 pre-activation of a ReLU layer comes within ``RELU_MARGIN`` of zero on its batch is
redrawn from the next seed of a fixed sequence, so no comparison depends on which side of the kink fp32 lands."""
import numpy as np

from bnn_mlp_ref import BNNMlpRef
from gmmvi_amd.experiments.target_distributions.bnn import minibatch_rows

RELU_MARGIN = 1e-4
MAX_REDRAWS = 400
SEED, CALL = 7, 3
SCALING, PRIOR_STD = 0.5, 2.0

MSE, CE = "mse", "sparse_categorical_crossentropy"


def _case(name, F, hidden, acts, loss, C, T, B, N, wscale=0.3):
    return {"name": name, "F": F, "hidden": tuple(hidden), "acts": tuple(acts) + ("linear",), "loss": loss,
            "C": C if loss == CE else 1, "T": T, "B": B, "N": N, "wscale": wscale}


CASES = [
    _case("d1-sigmoid-mse-F1-H17-BeqT", 1, (17,), ("sigmoid",), MSE, 1, 37, 37, 5),
    _case("d1-tanh-mse-F31-H1-B1", 31, (1,), ("tanh",), MSE, 1, 300, 1, 5),
    _case("d1-linear-mse-F5-H4-B63", 5, (4,), ("linear",), MSE, 1, 300, 63, 1),
    _case("d1-sigmoid-ce16-F32-H16-B64", 32, (16,), ("sigmoid",), CE, 16, 300, 64, 5),
    _case("d2-tanh-relu-ce2-F32-H15-16-B127", 32, (15, 16), ("tanh", "relu"), CE, 2, 300, 127, 1),
    _case("d3-relu-linear-sigmoid-ce16-F33-B128", 33, (16, 17, 15), ("relu", "linear", "sigmoid"), CE, 16, 300, 128, 5),
    _case("d2-relu-mse-F65-H64-128-B129", 65, (64, 128), ("relu", "relu"), MSE, 1, 300, 129, 1, wscale=0.15),
    _case("d1-relu-ce10-F65-H128-BeqT300", 65, (128,), ("relu",), CE, 10, 300, 300, 5, wscale=0.15),
    _case("d3-tanh-ce3-F33-H128-B65", 33, (128, 128, 128), ("tanh", "tanh", "tanh"), CE, 3, 300, 65, 1, wscale=0.1),
    _case("d1-sigmoid-mse-F1024-H64-B128", 1024, (64,), ("sigmoid",), MSE, 1, 300, 128, 1, wscale=0.05),
]
WINE_CASE = _case("wine-shape", 11, (8, 8), ("sigmoid", "sigmoid"), MSE, 1, 300, 128, 5)
MNIST_CASE = _case("mnist-shape", 784, (128,), ("relu",), CE, 10, 512, 128, 2, wscale=0.05)
ALL_CASES = CASES + [WINE_CASE, MNIST_CASE]

_built = {}


def make_data(case):
    """Features f32 [T, F] and labels (f32 for the MSE, int32 classes otherwise) from the case's own seed."""
    rng = np.random.default_rng([11, case["F"], case["T"], case["C"]])
    X = rng.normal(size=(case["T"], case["F"])).astype(np.float32)
    if case["loss"] == MSE:
        y = rng.normal(size=case["T"]).astype(np.float32)
    else:
        y = rng.integers(0, case["C"], size=case["T"]).astype(np.int32)
    return X, y


def make_ref(case, X, y, dtype=np.float64, batch_size=None, seed=SEED, likelihood_scaling=SCALING, prior_std=PRIOR_STD):
    return BNNMlpRef(X, y, case["hidden"], case["acts"], case["loss"], num_classes=case["C"],
                     likelihood_scaling=likelihood_scaling, prior_std=prior_std,
                     batch_size=case["B"] if batch_size is None else batch_size, seed=seed, dtype=dtype)


def draw_weights(case, ref, rows):
    """f32 [N, D]: sample i from the seed sequence (index of the case's name, i, attempt), the first attempt whose ReLU
    pre-activations on its batch all keep the margin.  -> (weights, redraws)."""
    key = sum(ord(ch) * (k + 1) for k, ch in enumerate(case["name"]))
    W = np.empty((case["N"], ref.D), np.float32)
    redraws = 0
    for i in range(case["N"]):
        for attempt in range(MAX_REDRAWS):
            wi = (np.random.default_rng([key, i, attempt]).normal(size=ref.D) * case["wscale"]).astype(np.float32)
            if ref.min_abs_relu_preactivation(wi.astype(np.float64), rows[i:i + 1]) >= RELU_MARGIN:
                break
            redraws += 1
        else:
            raise AssertionError(f"{case['name']}: no draw of sample {i} keeps the ReLU margin")
        W[i] = wi
    return W, redraws


def build(case):
    """The case's data, stream rows, weights and its fp64 / fp32 references with their results (computed once)."""
    if case["name"] in _built:
        return _built[case["name"]]
    X, y = make_data(case)
    ref, ref32 = make_ref(case, X, y), make_ref(case, X, y, dtype=np.float32)
    rows = minibatch_rows(SEED, CALL, case["N"], case["B"], case["T"])
    W, redraws = draw_weights(case, ref, rows)
    lp64, g64 = ref.evaluate_rows(W.astype(np.float64), rows)
    lp32, g32 = ref32.evaluate_rows(W, rows)
    for a in (lp64, g64, lp32, g32):
        a.setflags(write=False)
    built = {"X": X, "y": y, "rows": rows, "W": W, "ref": ref, "ref32": ref32, "lp64": lp64, "g64": g64, "lp32": lp32,
             "g32": g32, "redraws": redraws}
    _built[case["name"]] = built
    return built


def errors(lp, g, lp_ref, g_ref):
    """test_hip_bnn_classifier.py's measures: lp relative to max(|lp|, 1), the gradient's largest deviation relative to its
    largest entry, each the worst over the samples."""
    err = np.abs(lp - lp_ref) / np.maximum(np.abs(lp_ref), 1.0)
    gerr = np.abs(g - g_ref).max(1) / np.maximum(np.abs(g_ref).max(1), 1e-30)
    return float(err.max()), float(gerr.max())
