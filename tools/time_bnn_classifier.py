"""Developer tool: HIP-event timings of the Bayesian-neural-network classification target (csrc/bnn_classifier.hip) at
MNIST's shape.

  python tools/time_bnn_classifier.py [--json profiles/bnn_classifier_timing.json]

F, H, C, B = 784, 128, 10, 128 on synthetic data of T = 60 000 rows (188 MB of f32 features, as the real training set):
1. gmmvi_target_bnn_classifier at N in {100, 1000} samples, with and without the gradient;
2. gmmvi_bnn_classifier_predict of S = 100 weight vectors on M = 5000 rows.
Every figure is the median of 30 launches, each between two HIP events (a new minibatch call per launch).  An entry carries
the algorithmic FLOPs N (4 B F H + 6 B H C) (forward and backward contraction of both layers; predict: S (2 M F H + 2 M H C))
and bytes N (8 D + 4 B F) (weights read, gradient written, batch rows read; predict: S (4 D + 4 M F + 4 M C)), the rate they
make and its share of the two rooflines: 157.3 TFLOP/s (f32 matrix cores) and 8 TB/s (HBM)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

PEAK_F32_MATRIX, PEAK_HBM = 157.3e12, 8e12
F, H, C, B, T = 784, 128, 10, 128, 60000
D = hip_ops.bnn_classifier_num_parameters(F, H, C)
REPS, WARMUP = 30, 3


def _median_us(ctx, launch):
    for c in range(WARMUP):
        launch(c)
    times = []
    for c in range(REPS):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        launch(WARMUP + c)
        ctx.record(e1)
        ctx.sync()
        times.append(ctx.elapsed_ms(e0, e1) * 1e3)
    return float(np.median(times))


def _entry(us, flops, nbytes, **shape):
    rate, bw = flops / (us * 1e-6), nbytes / (us * 1e-6)
    return dict(shape, us=round(us, 1), gflop=round(flops / 1e9, 3), mbyte=round(nbytes / 1e6, 2),
                tflops=round(rate / 1e12, 2), f32_matrix_peak_fraction=round(rate / PEAK_F32_MATRIX, 4),
                tbytes_per_s=round(bw / 1e12, 3), hbm_peak_fraction=round(bw / PEAK_HBM, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = get_context()
    rng = np.random.default_rng(0)
    X = ctx.asarray(rng.random((T, F), dtype=np.float32))
    y = ctx.asarray(rng.integers(0, C, size=T).astype(np.int32), np.int32)
    out = {"shape": {"F": F, "H": H, "C": C, "B": B, "T": T, "D": D}, "target_bnn_classifier": [],
           "bnn_classifier_predict": []}
    for n in (100, 1000):
        x = ctx.asarray((rng.normal(size=(n, D)) * 0.1).astype(np.float32))
        for want_grad in (True, False):
            us = _median_us(ctx, lambda c: hip_ops.target_bnn_classifier(ctx, X, y, H, C, 0, c, B, 1.0, 1.0, x,
                                                                         want_grad=want_grad))
            if want_grad:
                flops, nbytes = n * (4.0 * B * F * H + 6.0 * B * H * C), n * (8.0 * D + 4.0 * B * F)
            else:                                                          # forward only: half the work, no gradient row
                flops, nbytes = n * (2.0 * B * F * H + 2.0 * B * H * C), n * (4.0 * D + 4.0 * B * F)
            e = _entry(us, flops, nbytes, N=n, gradient=want_grad)
            out["target_bnn_classifier"].append(e)
            print(f"target_bnn_classifier N = {n:5d} gradient = {want_grad!s:5}: {us:9.1f} us  {e['tflops']:6.2f} TFLOP/s "
                  f"({100 * e['f32_matrix_peak_fraction']:.1f} % of the f32 matrix peak)  {e['tbytes_per_s']:.3f} TB/s "
                  f"({100 * e['hbm_peak_fraction']:.1f} % of 8 TB/s)")
    s, m = 100, 5000
    W = ctx.asarray((rng.normal(size=(s, D)) * 0.1).astype(np.float32))
    Xe = X.rows(0, m)
    us = _median_us(ctx, lambda c: hip_ops.bnn_classifier_predict(ctx, H, C, W, Xe))
    e = _entry(us, s * (2.0 * m * F * H + 2.0 * m * H * C), s * (4.0 * D + 4.0 * m * F + 4.0 * m * C), S=s, M=m)
    out["bnn_classifier_predict"].append(e)
    print(f"bnn_classifier_predict S = {s} M = {m}: {us:9.1f} us  {e['tflops']:6.2f} TFLOP/s "
          f"({100 * e['f32_matrix_peak_fraction']:.1f} % of the f32 matrix peak)")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
