"""Developer tool: what the gradient of a user-defined target costs in forward mode (csrc/custom_target_autodiff.inc) and on a
tape (csrc/custom_target_tape.inc), the same density text through both.

  python tools/time_custom_tape.py [--scratch-gib 32] [--json profiles/custom_tape_timing.json]

The protocol of tools/time_custom_target.py (one process, HIP events on the context's stream, the median) with a cap on the
time a row may take: after the call that sizes the tape and one warm-up call, up to 30 timed calls or as many as fit into
--seconds, at least one.  The quartic density (O(D^2) operations, so O(D^2) records) at D = 16, 50, 120, 300, 512 and the chain
density of tests/custom_tape_cases.py (O(D) operations) at D = 512 and 4096, N = 10^4.  A tape call is timed as a user pays for
it: every slab's launch, the 4-byte readback and the stream synchronisation.  --scratch-gib is the budget of the tape scratch
(0: the library's default); the slab count under it and under the default are both recorded."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import custom_tape_cases as cases  # noqa: E402
from gmmvi_amd import _lib, hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

REPS = 30


def timed_us(ctx, fn, seconds):
    start, stop = ctx.event(), ctx.event()
    fn()
    ms, t0 = [], time.time()
    while len(ms) < REPS and (not ms or time.time() - t0 < seconds):
        ctx.record(start)
        fn()
        ctx.record(stop)
        ctx.check(ctx.lib.gmmvi_event_synchronize(ctx.handle, stop))
        ms.append(ctx.elapsed_ms(start, stop))
    return round(statistics.median(ms) * 1e3, 1), len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--scratch-gib", type=float, default=0.0, help="budget of the tape scratch; 0: the library's default")
    ap.add_argument("--seconds", type=float, default=8.0, help="time the timed calls of one entry may take")
    ap.add_argument("--samples", type=int, default=10000)
    a = ap.parse_args()
    ctx = get_context()
    n = a.samples
    scratch = int(a.scratch_gib * (1 << 30))
    rows = []
    for name, d in [("quartic", d) for d in (16, 50, 120, 300, 512)] + [("chain", 512), ("chain", 4096)]:
        tgt, x = cases.build_case(name, d, n)
        params, x = ctx.asarray(tgt.params()), ctx.asarray(x)
        h_tape = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode="tape")
        row = {"target": name, "D": d, "N": n}
        g_tape = hip_ops.target_custom_tape(ctx, h_tape, params, x, True, scratch_bytes=scratch)[1].numpy()   # sizes the tape
        length = hip_ops.custom_tape_length(ctx, h_tape, d)
        row["tape_length"] = length
        row["tape_bytes_per_sample"] = length * _lib.CUSTOM_TAPE_RECORD_BYTES
        row["slabs"] = hip_ops.custom_tape_plan(n, length, scratch)[0]
        row["slabs_at_default_budget"] = hip_ops.custom_tape_plan(n, length, 0)[0]
        row["tape_grad_us"], row["tape_reps"] = timed_us(
            ctx, lambda: hip_ops.target_custom_tape(ctx, h_tape, params, x, True, scratch_bytes=scratch), a.seconds)
        row["value_us"], _ = timed_us(ctx, lambda: hip_ops.target_custom_tape(ctx, h_tape, params, x, False), a.seconds)
        if d <= _lib.CUSTOM_AUTODIFF_MAX_DIM:
            h_fwd = hip_ops.custom_target_compile(ctx, cases.SOURCES[name], mode="autodiff")
            g_fwd = hip_ops.target_custom(ctx, h_fwd, params, x, True)[1].numpy()
            assert np.abs(g_fwd - g_tape).max() <= 1e-3 * np.abs(g_fwd).max()       # the two gradients agree before they are timed
            row["forward_grad_us"], row["forward_reps"] = timed_us(
                ctx, lambda: hip_ops.target_custom(ctx, h_fwd, params, x, True), a.seconds)
            row["tape_over_forward"] = round(row["tape_grad_us"] / row["forward_grad_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"max_reps": REPS, "seconds_per_entry": a.seconds, "scratch_bytes": scratch or _lib.CUSTOM_TAPE_SCRATCH_BYTES,
           "gradient_calls": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
