"""Developer tool: HIP-event timings of the Talos target (csrc/talos.hip).

  python tools/time_talos.py [--json OUT]

gmmvi_target_talos (log density + gradient, and log density only) at N = 400 (talos.yml: one component, the SEMTRON
sample count with reuse) and N = 1e4, on talos.yml's N(0, I) draws; the mean over 200 launches after 10 of warm-up.
The robot description is the fixture tests/golden/talos_reduced.urdf."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402
from gmmvi_amd.experiments.target_distributions.talos_ik import Talos  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def time_target(ctx, t, n, want_grad, reps=200):
    x = ctx.asarray(np.random.default_rng(0).normal(size=(n, 34)).astype(np.float32))
    for _ in range(10):
        hip_ops.target_talos(ctx, t._table_dev, t._context_dev, x, want_grad=want_grad)
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        hip_ops.target_talos(ctx, t._table_dev, t._context_dev, x, want_grad=want_grad)
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = get_context()
    t = Talos([0.1, 0.5, 1.0], dataset_dir=GOLDEN_DIR)
    out = []
    for n in (400, 10000):
        for want_grad in (True, False):
            us = time_target(ctx, t, n, want_grad)
            out.append({"N": n, "grad": want_grad, "us": round(us, 2)})
            print(f"target_talos N = {n:6d} {'lp + grad' if want_grad else 'lp only  '}: {us:8.2f} us")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
