"""Developer tool: what the gradient of a differentiated user-defined target (csrc/custom_target_autodiff.inc) costs against
the hand-written gradient of the same target.

  python tools/time_custom_autodiff.py [--json profiles/custom_autodiff_timing.json]

The protocol of tools/time_custom_target.py: one process, HIP events on the context's stream, median of 30 after 3 warm-up
calls.  The planar-robot density at D = 10, N = 2 * 10^4 and the quartic density at D = 50, N = 10^4 (tests/custom_target_cases.py
and tests/custom_autodiff_cases.py hold the two texts of each): lp + gradient and lp alone, route 0."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import custom_autodiff_cases as auto  # noqa: E402
import custom_target_cases as hand  # noqa: E402
from time_custom_target import REPS, event_ms  # noqa: E402
from gmmvi_amd import _lib, hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--tangents", type=int, default=_lib.CUSTOM_AUTODIFF_TANGENTS,
                    help="W of the library that is loaded (for the record; the library's own constant decides)")
    a = ap.parse_args()
    ctx = get_context()
    rng = np.random.default_rng(0)
    rows = []
    for name, d, n in (("planar", 10, 20000), ("quartic", 50, 10000)):
        tgt, _ = hand.build_case(name, d, 8)
        params = ctx.asarray(tgt.params())
        scale = tgt.prior_stds if name == "planar" else 1.0
        centre = 0.0 if name == "planar" else tgt.m
        x = ctx.asarray((centre + rng.normal(size=(n, d)) * scale).astype(np.float32))
        h_hand = hip_ops.custom_target_compile(ctx, hand.SOURCES[name])
        h_auto = hip_ops.custom_target_compile(ctx, auto.SOURCES[name], autodiff=True)
        # the two gradients agree before they are timed
        g_hand = hip_ops.target_custom(ctx, h_hand, params, x, True)[1].numpy()
        g_auto = hip_ops.target_custom(ctx, h_auto, params, x, True)[1].numpy()
        assert np.abs(g_hand - g_auto).max() <= 1e-3 * np.abs(g_hand).max()
        row = {"target": name, "D": d, "N": n, "tangents": a.tangents,
               "passes": math.ceil(d / a.tangents), "model_value_evaluations": math.ceil(d / a.tangents) * (1 + a.tangents),
               "hand_grad_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_hand, params, x, True)),
               "autodiff_grad_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_auto, params, x, True)),
               "hand_value_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_hand, params, x, False)),
               "autodiff_value_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_auto, params, x, False))}
        row["autodiff_over_hand"] = round(row["autodiff_grad_us"] / row["hand_grad_us"], 2)
        rows.append(row)
    res = {"reps": REPS, "gradient_calls": rows}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
