"""Developer tool: what a user-defined device target (csrc/custom_target.hip) costs against a built-in target kernel.

  python tools/time_custom_target.py [--json profiles/custom_target_timing.json]

One process, HIP events on the context's stream, median of 30 after 3 warm-up calls.
  kernels   -- the planar-robot density as a user function (tests/custom_target_cases.py) against the built-in
               gmmvi_target_planar at D = 10, N = 10^4 and 2 * 10^4, lp + gradient, staged and direct route; the quartic user
               function at D = 50 and D = 120, N = 10^4, both routes
  iteration -- one train_iter at the README's planar shape (D = 10, K = 200, N = 2 * 10^4 samples per iteration, single-call
               path), the user-function planar target and the built-in one, ms per iteration"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import custom_target_cases as cases  # noqa: E402
from helpers import samtron_config  # noqa: E402
from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

REPS, WARMUP = 30, 3


def event_ms(ctx, fn):
    start, stop = ctx.event(), ctx.event()
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPS):
        ctx.record(start)
        fn()
        ctx.record(stop)
        ctx.check(ctx.lib.gmmvi_event_synchronize(ctx.handle, stop))
        ms.append(ctx.elapsed_ms(start, stop))
    return round(statistics.median(ms) * 1e3, 2)           # microseconds


def time_kernels(ctx):
    out = []
    planar = cases.Planar(10)
    h_planar = hip_ops.custom_target_compile(ctx, cases.PLANAR_SRC)
    p_planar = ctx.asarray(planar.params())
    prior, goals = ctx.asarray(planar.prior_stds), ctx.asarray(planar.goals)
    rng = np.random.default_rng(0)
    for n in (10000, 20000):
        x = ctx.asarray((rng.normal(size=(n, 10)) * planar.prior_stds).astype(np.float32))
        row = {"target": "planar", "D": 10, "N": n,
               "builtin_us": event_ms(ctx, lambda: hip_ops.target_planar(ctx, prior, goals, float(planar.likelihood_std), x)),
               "staged_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_planar, p_planar, x, True, 1)),
               "direct_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_planar, p_planar, x, True, 2))}
        row["staged_over_builtin"] = round(row["staged_us"] / row["builtin_us"], 2)
        row["direct_over_builtin"] = round(row["direct_us"] / row["builtin_us"], 2)
        out.append(row)
    h_quartic = hip_ops.custom_target_compile(ctx, cases.QUARTIC_SRC)
    for d in (50, 120):
        tgt = cases.Quartic.random(d, 0.05, 1)
        params = ctx.asarray(tgt.params())
        x = ctx.asarray((tgt.m + rng.normal(size=(10000, d))).astype(np.float32))
        out.append({"target": "quartic", "D": d, "N": 10000,
                    "staged_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_quartic, params, x, True, 1)),
                    "direct_us": event_ms(ctx, lambda: hip_ops.target_custom(ctx, h_quartic, params, x, True, 2))})
    return out


def time_iteration(ctx, user):
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceLNPDF
    from gmmvi_amd.experiments.target_distributions.planar_robot import PlanarRobot
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi import GMMVI
    d, k, s = 10, 200, 100
    planar = cases.Planar(d)
    target = DeviceLNPDF(cases.PLANAR_SRC, d, params=planar.params()) if user else PlanarRobot(d, 4)
    rng = np.random.default_rng(3)
    prior_scale = np.array([1.0] + [0.2] * (d - 1))
    means = (rng.normal(size=(k, d)) * prior_scale).astype(np.float32)
    covs = np.broadcast_to(np.diag([0.0625] + [0.0025] * (d - 1)).astype(np.float32), (k, d, d))
    model = FullCovGMM(np.ones(k) / k, means, covs)
    model.seed = 7
    cfg = samtron_config(s)
    cfg["model_initialization"] = dict(cfg["model_initialization"], prior_mean=0.0, initial_cov=0.0625)
    g = GMMVI.build_from_config(cfg, target, GmmWrapper(model, 0.1, 1e-12, 400))
    assert g._fast_path.eligible()
    return round(event_ms(ctx, g.train_iter) / 1e3, 4)    # ms per iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = get_context()
    res = {"reps": REPS, "kernels": time_kernels(ctx),
           "train_iter_ms": {"shape": "D=10 K=200 N=20000 (single-call path)", "builtin_planar": time_iteration(ctx, False),
                             "user_planar": time_iteration(ctx, True)}}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
