"""Developer tool: what the gradient of a user-defined target summed over a data set costs in forward mode
(csrc/custom_target_data.inc, DeviceDataLNPDF's route) and in reverse mode (csrc/custom_target_data_tape.inc,
DeviceDataTapeLNPDF's route), the same logit text and the same data through both.

  python tools/time_custom_data_tape.py [--dims 32,128,512,2048,16384] [--batches 0,64] [--scratch-gib 0]
                                        [--json profiles/custom_data_tape_timing.json]

One process; the library's own HIP-event profile (gmmvi_profile_enable) brackets every kernel of a call, a call's time is the
sum over its kernels, and the median over the timed calls is reported.  After the call that sizes the tape and one warm-up call,
up to 20 timed calls or as many as fit into --seconds, at least one.  logit of tests/custom_data_cases.py, N = 10^4 samples, T =
1000 rows, full data (batch 0) and minibatches of 64.  Forward mode is timed up to its cap of 512.  --scratch-gib is the budget of
tapes and accumulators (0: the library's default); the plan under it is recorded."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import custom_data_cases as cases  # noqa: E402
from gmmvi_amd import _lib, hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

REPS = 20


def report(ctx):
    buf = C.create_string_buffer(1 << 16)
    ctx.check(ctx.lib.gmmvi_profile_report(ctx.handle, buf, len(buf)))
    return {f[0]: float(f[2]) for f in (line.split() for line in buf.value.decode().splitlines()) if len(f) >= 3}


def timed_us(ctx, fn, seconds, totals=None):
    """-> (median microseconds of a call, by kernel tag and in total; timed calls).  totals: a list that receives every timed
    call's total in microseconds."""
    fn()
    ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 1))
    calls, t0 = [], time.time()
    try:
        while len(calls) < REPS and (not calls or time.time() - t0 < seconds):
            fn()
            calls.append(report(ctx))
    finally:
        ctx.check(ctx.lib.gmmvi_profile_enable(ctx.handle, 0))
    if totals is not None:
        totals.extend(round(sum(c.values()) * 1e3, 1) for c in calls)
    tags = sorted(calls[0])
    by_tag = {t: round(statistics.median(c[t] for c in calls) * 1e3, 1) for t in tags}
    return round(statistics.median(sum(c.values()) for c in calls) * 1e3, 1), by_tag, len(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--dims", default="32,128,512,2048,16384")
    ap.add_argument("--batches", default="0,64", help="0: full data")
    ap.add_argument("--scratch-gib", type=float, default=0.0)
    ap.add_argument("--seconds", type=float, default=6.0, help="time the timed calls of one entry may take")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    ctx = get_context()
    n, t = a.samples, a.rows
    scratch = int(a.scratch_gib * (1 << 30))
    h_rev = hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data_tape")
    h_fwd = hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data")
    out = []
    for d in (int(v) for v in a.dims.split(",")):
        tgt, x = cases.build_case(cases.Case("logit", d, n, t, 0, None, 0))
        params, data, x = ctx.asarray(tgt.params()), ctx.asarray(tgt.data), ctx.asarray(x)
        for batch in (int(v) for v in a.batches.split(",")):
            kw = dict(batch_size=batch or None, seed=9, call=3)
            row = {"target": "logit", "D": d, "N": n, "T": t, "batch": batch}
            g_rev = hip_ops.target_custom_data_tape(ctx, h_rev, params, data, x, True, scratch_bytes=scratch, **kw)[1]   # sizes the tape
            length = hip_ops.custom_tape_length(ctx, h_rev, d)
            row["tape_length"] = length
            row["plan_chunks_rows_slabs_tiles"] = hip_ops.custom_data_tape_plan(n, batch or t, d, length, 0, scratch)
            row["reverse_grad_us"], row["reverse_by_kernel_us"], row["reverse_reps"] = timed_us(
                ctx, lambda: hip_ops.target_custom_data_tape(ctx, h_rev, params, data, x, True, scratch_bytes=scratch, **kw), a.seconds)
            row["value_us"], _, _ = timed_us(ctx, lambda: hip_ops.target_custom_data_tape(ctx, h_rev, params, data, x, False, **kw),
                                             a.seconds)
            if d <= _lib.CUSTOM_AUTODIFF_MAX_DIM:
                g_fwd = hip_ops.target_custom_data(ctx, h_fwd, params, data, x, True, **kw)[1].numpy()
                assert np.abs(g_fwd - g_rev.numpy()).max() <= 1e-3 * np.abs(g_fwd).max()      # the two agree before they are timed
                row["forward_grad_us"], row["forward_by_kernel_us"], row["forward_reps"] = timed_us(
                    ctx, lambda: hip_ops.target_custom_data(ctx, h_fwd, params, data, x, True, **kw), a.seconds)
                row["reverse_over_forward"] = round(row["reverse_grad_us"] / row["forward_grad_us"], 2)
            out.append(row)
            print(json.dumps(row), flush=True)
    res = {"max_reps": REPS, "seconds_per_entry": a.seconds, "scratch_bytes": scratch or _lib.CUSTOM_TAPE_SCRATCH_BYTES,
           "gradient_calls": out}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
