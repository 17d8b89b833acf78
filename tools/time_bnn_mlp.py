"""Developer tool: HIP-event timings of the generic Bayesian-neural-network target (csrc/bnn_mlp.hip) next to the two
specialised kernels on the networks they take.

  python tools/time_bnn_mlp.py [--json profiles/bnn_mlp_timing.json]

N = 1000 samples, B = 128, synthetic data, with the gradient:
1. the WINE network, F = 11, hidden (8, 8), sigmoid, MSE: gmmvi_target_mlp and gmmvi_target_bnn;
2. the MNIST network, F = 784, hidden (128,), ReLU, C = 10: gmmvi_target_mlp and gmmvi_target_bnn_classifier;
3. a network only the generic kernel takes, F = 784, hidden (128, 64), ReLU, C = 10: gmmvi_target_mlp.
Every figure is the median of 30 launches, each between two HIP events (a new minibatch call per launch).  An entry carries
the algorithmic FLOPs of the contractions, N B (4 F H1 + sum over the later layers of 6 in out), and the ratio of the generic
to the specialised kernel's time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

N, B, REPS, WARMUP = 1000, 128, 30, 3
MSE, CE = "mse", "sparse_categorical_crossentropy"
NETWORKS = [
    {"name": "wine", "F": 11, "hidden": (8, 8), "acts": ("sigmoid", "sigmoid", "linear"), "loss": MSE, "C": 1, "T": 2938},
    {"name": "mnist", "F": 784, "hidden": (128,), "acts": ("relu", "linear"), "loss": CE, "C": 10, "T": 60000},
    {"name": "mnist-two-hidden", "F": 784, "hidden": (128, 64), "acts": ("relu", "relu", "linear"), "loss": CE, "C": 10,
     "T": 60000},
]


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


def _flops(net):
    widths = [net["F"]] + list(net["hidden"]) + [net["C"]]
    per_row = 4.0 * widths[0] * widths[1] + sum(6.0 * a * b for a, b in zip(widths[1:-1], widths[2:]))
    return N * B * per_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = get_context()
    rng = np.random.default_rng(0)
    out = {"N": N, "B": B, "reps": REPS, "networks": []}
    for net in NETWORKS:
        f, hidden, c, t = net["F"], net["hidden"], net["C"], net["T"]
        d = hip_ops.mlp_num_parameters(f, hidden, c)
        X = ctx.asarray(rng.random((t, f), dtype=np.float32))
        if net["loss"] == MSE:
            y = ctx.asarray(rng.normal(size=t).astype(np.float32))
        else:
            y = ctx.asarray(rng.integers(0, c, size=t).astype(np.int32), np.int32)
        x = ctx.asarray((rng.normal(size=(N, d)) * 0.1).astype(np.float32))
        entry = {"name": net["name"], "F": f, "hidden": list(hidden), "C": c, "T": t, "D": d, "loss": net["loss"],
                 "gflop": round(_flops(net) / 1e9, 3)}
        us = _median_us(ctx, lambda call: hip_ops.target_mlp(ctx, X, y, hidden, net["acts"], net["loss"], c, 0, call, B, 1.0,
                                                             1.0, x))
        entry["target_mlp_us"] = round(us, 1)
        entry["target_mlp_tflops"] = round(_flops(net) / (us * 1e-6) / 1e12, 2)
        special = None
        if net["name"] == "wine":
            special = ("target_bnn", lambda call: hip_ops.target_bnn(ctx, X, y, hidden, 0, call, B, 1.0, 1.0, x))
        elif net["name"] == "mnist":
            special = ("target_bnn_classifier",
                       lambda call: hip_ops.target_bnn_classifier(ctx, X, y, hidden[0], c, 0, call, B, 1.0, 1.0, x))
        if special:
            us_s = _median_us(ctx, special[1])
            entry[special[0] + "_us"] = round(us_s, 1)
            entry["generic_over_specialised"] = round(us / us_s, 2)
        out["networks"].append(entry)
        print(json.dumps(entry))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
