"""Developer tool: what the predictive density of a data-set target (the predictive kernels of csrc/custom_target_data.inc,
``hip_ops.custom_data_predictive``) costs beside the value call of the same target on as many row-term evaluations.

  python tools/time_custom_predictive.py [--json profiles/custom_predictive_timing.json]

The protocol of tools/time_custom_data.py: one process, HIP events on the context's stream, median of 30 after 3 warm-up calls.
``logit`` of tests/custom_data_cases.py at D = 32, N = 2 000 samples: the predictive call on M = 1 000 evaluation rows, and
``target_custom_data`` (value only) on T = 1 000 data rows, each on the automatic plan and forced to one chunk."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import custom_data_cases as cases  # noqa: E402
from time_custom_target import REPS, event_ms  # noqa: E402
from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = get_context()
    rng = np.random.default_rng(0)
    d, n, m = 32, 2000, 1000
    rows = np.concatenate([rng.normal(size=(m, d)) / np.sqrt(d), rng.choice([-1.0, 1.0], size=(m, 1))], axis=1).astype(np.float32)
    x = ctx.asarray(rng.normal(size=(n, d)).astype(np.float32))
    rows_dev, prior = ctx.asarray(rows), ctx.asarray(np.array([0.25, 2.0], np.float32))
    handle = hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data")

    def predictive(chunks):
        return hip_ops.custom_data_predictive(ctx, handle, prior, rows_dev, x, chunks=chunks)

    def value(chunks):
        return hip_ops.target_custom_data(ctx, handle, prior, rows_dev, x, False, chunks=chunks)

    # the two see the same row terms before they are timed: the sum over the rows of the per-row mean is the mean over the samples
    # of the data sum
    mean = predictive(0)[1].numpy().astype(np.float64)
    lp = value(0)[0].numpy().astype(np.float64)
    x_h = x.numpy().astype(np.float64)
    prior_lp = -0.5 * np.sum(((x_h - 0.25) / 2.0) ** 2, axis=1) - d * (np.log(2.0) + cases.HALF_LOG_2PI)
    assert abs(mean.sum() - (lp - prior_lp).mean()) <= 1e-3 * abs(mean.sum())
    tiles, chunks, per = hip_ops.custom_data_predictive_plan(n, m)
    res = {"protocol": "tools/time_custom_predictive.py: one process, HIP events on the context's stream, median of 30 after 3 "
                       "warm-up calls; logit, value call of target_custom_data on the same N and T = M rows as the yardstick",
           "reps": REPS, "D": d, "N": n, "M": m, "tiles": tiles, "chunks": chunks, "rows_per_chunk": per,
           "value_plan": list(hip_ops.custom_data_plan(n, m)),
           "predictive_us": event_ms(ctx, lambda: predictive(0)),
           "predictive_one_chunk_us": event_ms(ctx, lambda: predictive(1)),
           "value_us": event_ms(ctx, lambda: value(0)),
           "value_one_chunk_us": event_ms(ctx, lambda: value(1))}
    res["predictive_over_value"] = round(res["predictive_us"] / res["value_us"], 2)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
