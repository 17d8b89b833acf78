"""Developer tool: timings of the MORE estimate for blocked-path dimensions (csrc/more_blocked.hip).

  python tools/time_more_blocked.py [--json OUT] [--skip-large]

1. gmmvi_more at D = 63 against gmmvi_more_blocked at D = 64, K = 8, N = 8 192 (F + 1 = 2 081 against 2 146), same
   process, alternating, one warm-up call and 7 timed calls each between stream synchronisations; the median.
2. gmmvi_more_blocked at D = 100 and D = 128, K = 8, N = 3 F: one warm-up call, 3 timed calls (median), then one call with
   gmmvi_profile_enable for the per-kernel sums, and the Gram kernel's fp64 rate (all 128 x 128 blocks of the lower triangle
   it computes, 2 flops per multiply-add)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402


def make_inputs(ctx, k, d, n, seed=0):
    rng = np.random.default_rng(seed)
    means = rng.normal(size=(k, d)) * 3.0
    chols = np.stack([np.linalg.cholesky(a @ a.T / d + 0.3 * np.eye(d)) for a in rng.normal(size=(k, d, d))])
    comp = np.repeat(np.arange(k), -(-n // k))[:n]
    x = means[comp] + np.einsum("nij,nj->ni", chols[comp], rng.normal(size=(n, d)))
    means_d, chols_d, xd = ctx.asarray(means), ctx.asarray(chols), ctx.asarray(x)
    packed, _ = hip_ops.pack_components(ctx, means_d, chols_d)
    logw = ctx.asarray(np.full(k, -np.log(k)))
    ld, lp, _ = hip_ops.mixture_eval(ctx, packed, logw, xd, d, want_ld=True, want_lp=True)
    tlp = ctx.asarray(-0.5 * np.sum((x / 4.0) ** 2, axis=1) + np.sin(x[:, 0]))
    l2 = ctx.asarray(np.full(k, 1e-6))
    return packed, chols_d, xd, ld, lp, lp, tlp, l2, d           # background densities = the mixture itself


def timed(ctx, fn, args, reps):
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn(ctx, *args)
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_sums(ctx, fn, args):
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 1))
    fn(ctx, *args)
    buf = ctypes.create_string_buffer(1 << 16)
    ctx.check(ctx.lib.gmmvi_profile_report(ctx.handle, buf, len(buf)))
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 0))
    return {line.split()[0]: round(float(line.split()[2]), 3) for line in buf.value.decode().splitlines()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    ctx = get_context()
    res = {}

    k, n = 8, 8192
    old, new = make_inputs(ctx, k, 63, n), make_inputs(ctx, k, 64, n)
    hip_ops.more(ctx, *old); hip_ops.more_blocked(ctx, *new)
    t_old, t_new = [], []
    for _ in range(7):
        t_old += timed(ctx, hip_ops.more, old, 1)
        t_new += timed(ctx, hip_ops.more_blocked, new, 1)
    res["more_d63_ms"] = round(statistics.median(t_old), 3)
    res["more_blocked_d64_ms"] = round(statistics.median(t_new), 3)
    res["ratio"] = round(res["more_blocked_d64_ms"] / res["more_d63_ms"], 3)
    res["more_d63_kernels_ms"] = kernel_sums(ctx, hip_ops.more, old)
    res["more_blocked_d64_kernels_ms"] = kernel_sums(ctx, hip_ops.more_blocked, new)
    print(json.dumps(res), flush=True)

    for d in () if a.skip_large else (100, 128):
        f = d * (d + 1) // 2 + d + 1
        n = 3 * f
        args = make_inputs(ctx, k, d, n)
        hip_ops.more_blocked(ctx, *args)
        ms = timed(ctx, hip_ops.more_blocked, args, 3)
        sums = kernel_sums(ctx, hip_ops.more_blocked, args)
        nblk = -(-(f + 1) // 128)
        flops = 2.0 * k * (-(-n // 64) * 64) * (nblk * (nblk + 1) // 2) * 128 * 128
        res[f"d{d}"] = {"K": k, "N": n, "F": f, "call_ms": round(statistics.median(ms), 2), "kernels_ms": sums,
                        "gram_tflops": round(flops / (sums["more_blocked_gram"] * 1e-3) / 1e12, 2)}
        print(json.dumps(res[f"d{d}"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
