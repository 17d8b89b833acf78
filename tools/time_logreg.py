"""Developer tool: HIP-event timings of the logistic-regression target (csrc/logreg.hip) and of a SEMTRON iteration on it.

  python tools/time_logreg.py [--json OUT]

1. gmmvi_target_logreg (log density + gradient) at N in {3100, 1e4, 1e5} samples for Breast Cancer (M = 569, D = 31) and
   German Credit (M = 1000, D = 25), samples at the yml initialisation's scale; the fraction of the f32 matrix-core peak
   (157.3 TFLOP/s) that the two contractions' 4 N M D flops make of it.
2. train_iter() of SEMTRON (K = 1, 100 samples per component, reuse ratio 2) on both datasets, the single-call iteration
   against the module-by-module path, as the mean over 50 iterations after 20 of warm-up.
The datasets are the fixture tables of tests/golden/logreg_datasets.npz."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402
from gmmvi_amd.experiments.target_distributions.logistic_regression import LogisticRegression, preprocess  # noqa: E402
from logreg_ref import load_tables  # noqa: E402

PEAK_F32 = 157.3e12


def time_target(ctx, A_dev, m, d, n, reps=50):
    rng = np.random.default_rng(0)
    x = ctx.asarray((rng.normal(size=(n, d)) * 10.0).astype(np.float32))
    for _ in range(5):
        hip_ops.target_logreg(ctx, A_dev, 0.0, 10.0, x, want_grad=True)
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        hip_ops.target_logreg(ctx, A_dev, 0.0, 10.0, x, want_grad=True)
    ctx.record(e1)
    ctx.sync()
    us = ctx.elapsed_ms(e0, e1) * 1e3 / reps
    return us, 4.0 * n * m * d / (us * 1e-6) / PEAK_F32


def time_iter(ctx, data, dataset_id, fast, warmup=20, iters=50):
    from gmmvi_amd.configs import get_default_config
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    cfg = get_default_config("SEMTRON", dataset_id)
    tgt = LogisticRegression(dataset_id, data=data)
    d = tgt.get_num_dimensions()
    model = FullCovGMM(np.ones(1), np.zeros((1, d), np.float32), (100.0 * np.eye(d, dtype=np.float32))[None])
    model.seed = 1
    g = GMMVI.build_from_config(cfg, tgt, GmmWrapper(model, 1.0, 1e-12, 400))
    g._fast_path.enabled = fast
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
    tables = load_tables()
    out = {"target_logreg": [], "train_iter": []}
    for key, data in tables.items():
        A, d = preprocess(data, key)
        A_dev = ctx.asarray(A)
        for n in (3100, 10000, 100000):
            us, frac = time_target(ctx, A_dev, A.shape[0], d, n)
            out["target_logreg"].append({"dataset": key, "N": n, "us": round(us, 2), "f32_mfma_peak_fraction": round(frac, 4)})
            print(f"target_logreg {key:13s} M = {A.shape[0]:4d} D = {d}  N = {n:6d}: {us:8.1f} us  ({100 * frac:.1f} % of f32 peak)")
    for key, data in tables.items():
        for fast in (True, False):
            us = time_iter(ctx, data, key, fast)
            out["train_iter"].append({"dataset": key, "path": "single-call" if fast else "modular", "us": round(us, 1)})
            print(f"train_iter SEMTRON {key:13s} {'single-call' if fast else 'modular':11s}: {us:8.1f} us")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
