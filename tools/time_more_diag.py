"""Developer tool: time of the MORE estimate for diagonal mixtures (csrc/more_diag.hip) at the shape the diagonal Stein figure
of DESIGN.md 4b is quoted at.

  python tools/time_more_diag.py [--json OUT] [--k 64 --d 300 --n 20000]

One process, two warm-up calls, 20 timed calls between stream synchronisations (median, minimum, maximum), then one call with
gmmvi_profile_enable for the per-kernel sums and the Gram kernel's fp64 rate (all 128 x 128 blocks of the lower triangle it
computes, 2 flops per multiply-add)."""
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
    sigma = rng.random((k, d)) + 0.5
    comp = np.repeat(np.arange(k), -(-n // k))[:n]
    x = means[comp] + sigma[comp] * rng.normal(size=(n, d))
    xd = ctx.asarray(x)
    packed = hip_ops.diag_pack(ctx, ctx.asarray(means), ctx.asarray(sigma))
    ld, lp, _ = hip_ops.diag_mixture_eval(ctx, packed, ctx.asarray(np.full(k, -np.log(k))), xd, d, want_ld=True, want_lp=True)
    tlp = ctx.asarray(-0.5 * np.sum((x / 4.0) ** 2, axis=1) + np.sin(x[:, 0]))
    return packed, xd, ld, lp, lp, tlp, ctx.asarray(np.full(k, 1e-6)), d       # background densities = the mixture itself


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--d", type=int, default=300)
    ap.add_argument("--n", type=int, default=20000)
    a = ap.parse_args()
    ctx = get_context()
    args = make_inputs(ctx, a.k, a.d, a.n)
    for _ in range(2):
        h, g = hip_ops.more_diag(ctx, *args)
    assert np.all(np.isfinite(h.numpy())) and np.all(np.isfinite(g.numpy()))
    ms = []
    for _ in range(20):
        ctx.sync()
        t0 = time.perf_counter()
        hip_ops.more_diag(ctx, *args)
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 1))
    hip_ops.more_diag(ctx, *args)
    buf = ctypes.create_string_buffer(1 << 16)
    ctx.check(ctx.lib.gmmvi_profile_report(ctx.handle, buf, len(buf)))
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 0))
    sums = {line.split()[0]: round(float(line.split()[2]), 3) for line in buf.value.decode().splitlines()}
    f = 2 * a.d + 1
    nblk = -(-(f + 1) // 128)
    flops = 2.0 * a.k * (-(-a.n // 64) * 64) * (nblk * (nblk + 1) // 2) * 128 * 128
    res = {"K": a.k, "D": a.d, "N": a.n, "F": f, "call_ms_median": round(statistics.median(ms), 3),
           "call_ms_min": round(min(ms), 3), "call_ms_max": round(max(ms), 3), "kernels_ms": sums}
    if sums.get("more_diag_gram"):
        res["gram_tflops"] = round(flops / (sums["more_diag_gram"] * 1e-3) / 1e12, 2)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
