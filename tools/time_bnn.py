"""Developer tool: HIP-event timings of the WINE Bayesian-neural-network target (csrc/bnn.hip) and of a SAMTRON iteration on it.

  python tools/time_bnn.py [--json OUT]

1. gmmvi_target_bnn (log density + gradient, B = 128 rows per sample) at N in {400, 1e4} samples, weights at the yml
   initialisation's scale; the rate of the ~2 B (2 F H1 + 2 H1 H2 + ...) flops the forward and backward passes need,
   and the fraction of the f32 vector peak (157.3 TFLOP/s) that makes.
2. gmmvi_bnn_predict of 2000 samples on the 979 test rows (what one expensive-metrics evaluation launches for the test set).
3. train_iter() of SAMTRON on WINE (K = 4, 100 samples per component, the modular path: D = 177), the mean over 30
   iterations after 10 of warm-up.
The dataset is the fixture tests/golden/wine_seed_0.npz."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402
from bnn_ref import load_wine, write_dataset_dir  # noqa: E402

PEAK_F32 = 157.3e12


def flops_per_row(F=11, H1=8, H2=8):
    """Forward (2 F H1 + 2 H1 H2 + 2 H2) + backward deltas (2 H1 H2 + 3 H2 + 3 H1) + gradient contractions (2 D)."""
    d = F * H1 + H1 + H1 * H2 + H2 + H2 + 1
    return 2 * F * H1 + 2 * H1 * H2 + 2 * H2 + 2 * H1 * H2 + 3 * H2 + 3 * H1 + 2 * d


def time_target(ctx, X, y, n, reps=50):
    rng = np.random.default_rng(0)
    x = ctx.asarray(rng.normal(size=(n, 177)).astype(np.float32))
    for c in range(5):
        hip_ops.target_bnn(ctx, X, y, (8, 8), 0, c, 128, 1.0, 1.0, x, want_grad=True)
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for c in range(reps):
        hip_ops.target_bnn(ctx, X, y, (8, 8), 0, c, 128, 1.0, 1.0, x, want_grad=True)
    ctx.record(e1)
    ctx.sync()
    us = ctx.elapsed_ms(e0, e1) * 1e3 / reps
    flops = n * 128.0 * flops_per_row()
    return us, flops, flops / (us * 1e-6) / PEAK_F32


def time_predict(ctx, data, reps=20):
    W = ctx.asarray(np.random.default_rng(1).normal(size=(2000, 177)).astype(np.float32))
    X = ctx.asarray(data["features_test"])
    hip_ops.bnn_predict(ctx, (8, 8), W, X)
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        hip_ops.bnn_predict(ctx, (8, 8), W, X)
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / reps


def time_iter(ctx, dataset_dir, warmup=10, iters=30):
    from gmmvi_amd.configs import get_default_config, update_config
    from gmmvi_amd.gmmvi_runner import GmmviRunner
    cfg = update_config(get_default_config("SAMTRON", "wine"), {"environment_config": {"dataset_dir": dataset_dir},
                                                                 "seed": 10000})
    g = GmmviRunner.build_from_config(cfg).gmmvi
    for _ in range(warmup):
        g.train_iter()
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(iters):
        g.train_iter()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = get_context()
    data = load_wine()
    X, y = ctx.asarray(data["features_train"]), ctx.asarray(data["labels_train"].astype(np.float32))
    out = {"target_bnn": [], "bnn_predict": [], "train_iter": []}
    for n in (400, 10000):
        us, flops, frac = time_target(ctx, X, y, n)
        out["target_bnn"].append({"N": n, "B": 128, "us": round(us, 2), "gflop": round(flops / 1e9, 3),
                                  "f32_vector_peak_fraction": round(frac, 4)})
        print(f"target_bnn WINE B = 128  N = {n:6d}: {us:8.1f} us  ({flops / 1e9:.3f} GFLOP, {100 * frac:.2f} % of f32 peak)")
    us = time_predict(ctx, data)
    out["bnn_predict"].append({"S": 2000, "M": 979, "us": round(us, 2)})
    print(f"bnn_predict S = 2000 M = 979: {us:8.1f} us")
    with tempfile.TemporaryDirectory() as d:
        us = time_iter(ctx, write_dataset_dir(d))
    out["train_iter"].append({"codename": "SAMTRON", "K": 4, "path": "modular", "us": round(us, 1)})
    print(f"train_iter SAMTRON WINE (K = 4, modular): {us:8.1f} us")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
