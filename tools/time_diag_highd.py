"""Developer tool: HIP-event timings of the diagonal kernels above D = 512 (csrc/diag_sweep.hip, csrc/diag.hip).

  python tools/time_diag_highd.py [--json profiles/diag_highd_timing.json] [--reps 30]
  python tools/time_diag_highd.py --d300 [--json OUT]     # only DESIGN.md 4b's K = 64, D = 300, N = 2e4 rows

Per shape (K = 10, N = 1 000, D in 512, 1 024, 8 192, 101 770): the density + gradient sweep (gmmvi_diag_mixture_eval with ld, lp
and the gradient), the Stein launch (gmmvi_diag_stein, self-normalised) and both component updates (cold bracket), each call
between two events on the library's stream, one warm-up call, the median of --reps calls.  Next to each time: the bytes the
launch must move at least (every operand read once, every result written once, computed from the shapes) and the share of the
MI355X's 8 TB/s that this is."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def event_ms(ctx, fn, reps, before=None):
    """Median (and min / max) of `reps` calls of fn(), each between two events; before() runs untimed ahead of every call."""
    start, stop = ctx.event(), ctx.event()
    out = []
    for i in range(reps + 1):                      # the first call is the warm-up
        if before is not None:
            before()
        ctx.record(start)
        fn()
        ctx.record(stop)
        ctx.sync()
        if i:
            out.append(ctx.elapsed_ms(start, stop))
    return statistics.median(out), min(out), max(out)


def entry(ms, nbytes):
    med, lo, hi = ms
    return {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "bytes_min": int(nbytes),
            "hbm_share": round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4)}


def time_shape(ctx, k, d, n, reps, updates=True, seed=0):
    rng = np.random.default_rng(seed)
    means = (rng.normal(size=(k, d)) * 3.0).astype(np.float32)
    sigma = np.sqrt(rng.uniform(0.3, 3.0, size=(k, d))).astype(np.float32)
    comp = np.repeat(np.arange(k), -(-n // k))[:n]
    x = (means[comp] + sigma[comp] * rng.normal(size=(n, d)).astype(np.float32)).astype(np.float32)
    md, sd, xd = ctx.asarray(means), ctx.asarray(sigma), ctx.asarray(x)
    logw = ctx.asarray(np.full(k, -np.log(k), np.float32))
    packed = hip_ops.diag_pack(ctx, md, sd)
    res = {"K": k, "D": d, "N": n}
    f = 4                                                               # bytes per float
    res["pack"] = entry(event_ms(ctx, lambda: hip_ops.diag_pack(ctx, md, sd), reps), f * 5 * k * d)
    sweep = lambda: hip_ops.diag_mixture_eval(ctx, packed, logw, xd, d, want_ld=True, want_lp=True, want_grad=True)  # noqa: E731
    # densities: x, [mu | 1/sigma] read, ld + lp written; gradient: x, [mu | 1/sigma^2], ld, lp read, grad written
    res["sweep"] = entry(event_ms(ctx, sweep, reps), f * (3 * n * d + 4 * k * d + 2 * k * n + 2 * n))
    ld, lp, grad = sweep()
    tgrad = ctx.asarray(rng.normal(size=(n, d)).astype(np.float32))
    stein = lambda: hip_ops.diag_stein(ctx, packed, xd, ld, grad, lp, tgrad, d)  # noqa: E731
    res["stein"] = entry(event_ms(ctx, stein, reps), f * (3 * n * d + 4 * k * d + k * n + n))
    if updates:
        scale = np.sqrt(512.0 / d) if d > 512 else 1.0
        hs = ctx.asarray(((rng.normal(size=(k, d)) * 0.5 + 0.3) * scale).astype(np.float32))
        gs = ctx.asarray((rng.normal(size=(k, d)) * scale).astype(np.float32))
        steps = ctx.asarray(np.linspace(0.05, 0.5, k).astype(np.float32))
        m2, s2 = ctx.empty((k, d)), ctx.empty((k, d))
        last_eta, l2, nupd = ctx.empty((k,)), ctx.empty((k,)), ctx.empty((k,))
        probes = [None]

        def reset():
            m2.copy_from(md); s2.copy_from(sd)
            last_eta.set(np.full(k, -1.0, np.float32)); l2.set(np.full(k, 1e-12, np.float32)); nupd.set(np.ones(k, np.float32))

        def kl():
            probes[0] = hip_ops.update_components_diag(ctx, "kl", m2, s2, hs, gs, steps, 1.0, 1e-12, last_eta, l2, nupd,
                                                       want_info=True)[2]

        res["update_kl"] = entry(event_ms(ctx, kl, reps, before=reset), f * 6 * k * d)
        res["update_kl"]["probes"] = [int(p) for p in probes[0].numpy()]
        iblr = lambda: hip_ops.update_components_diag(ctx, "iblr", m2, s2, hs, gs, steps, 0.0, 1e-12, None, l2, nupd)  # noqa: E731
        res["update_iblr"] = entry(event_ms(ctx, iblr, reps, before=reset), f * 6 * k * d)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--d300", action="store_true", help="only the K = 64, D = 300, N = 20 000 rows of DESIGN.md 4b")
    a = ap.parse_args()
    ctx = get_context()
    res = {}
    if a.d300:
        res["d300"] = time_shape(ctx, 64, 300, 20000, a.reps, updates=False)
        print(json.dumps(res["d300"]), flush=True)
    else:
        for d in (512, 1024, 8192, 101770):
            res[f"d{d}"] = time_shape(ctx, 10, d, 1000, a.reps)
            print(json.dumps(res[f"d{d}"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
