"""Developer tool: HIP-event timings of the minibatch logistic-regression target (csrc/logreg_mb.hip).

  python tools/time_logreg_mb.py [--json OUT]

gmmvi_target_logreg_mb (log density + gradient) at B = 64 and N in {400, 1e4, 1e5} samples for Breast Cancer (T = 569,
D = 31) and German Credit (T = 1000, D = 25), with own batches per sample (nb = floor(T / 64)) and with one shared batch
(nb = 1), each next to gmmvi_target_logreg (the full-data kernel) at the same N.  Samples at the yml initialisation's
scale; every shape is warmed up before it is timed.  The datasets are the fixture tables of
tests/golden/logreg_datasets.npz."""
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
from gmmvi_amd.experiments.target_distributions.logistic_regression import preprocess  # noqa: E402
from logreg_ref import load_tables  # noqa: E402

B = 64


def time_us(ctx, fn, warmup=10, reps=100):
    for _ in range(warmup):
        fn()
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        fn()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = get_context()
    out = []
    for key, table in load_tables().items():
        A, d = preprocess(table, key)
        T = A.shape[0]
        A_dev = ctx.asarray(A)
        for n in (400, 10000, 100000):
            x = ctx.asarray((np.random.default_rng(0).normal(size=(n, d)) * 10.0).astype(np.float32))
            full = time_us(ctx, lambda: hip_ops.target_logreg(ctx, A_dev, 0.0, 10.0, x, want_grad=True))
            for own in (True, False):
                nb = T // B if own else 1
                call = iter(range(1 << 30))          # a fresh call per launch, as in a run
                mb = time_us(ctx, lambda: hip_ops.target_logreg_mb(ctx, A_dev, B, nb, 1, next(call), 0.0, 10.0, x,
                                                                   want_grad=True))
                out.append({"dataset": key, "T": T, "D": d, "N": n, "B": B, "own_batches": own, "nb": nb,
                            "logreg_mb_us": round(mb, 2), "logreg_full_us": round(full, 2)})
                print(f"{key:13s} T = {T:4d} D = {d}  N = {n:6d}  B = {B} nb = {nb:2d}: logreg_mb {mb:8.2f} us   "
                      f"full-data logreg {full:8.2f} us")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
