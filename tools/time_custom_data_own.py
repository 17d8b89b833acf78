"""Developer tool: what an own minibatch per sample costs a user-defined target summed over a data set: a gradient call of the
forward-mode route (DeviceDataLNPDF's) and of the tape route (DeviceDataTapeLNPDF's) with the batch shared by all samples, with
a batch per sample and on the full data, and the run-time compile of a handle of either data mode.

  python tools/time_custom_data_own.py [--dims 32,128,600] [--batch 64] [--root TREE] [--json profiles/custom_data_own_timing.json]

The protocol of tools/time_custom_data_tape.py: one process; the library's own HIP-event profile (gmmvi_profile_enable) brackets
every kernel of a call, a call's time is the sum over its kernels, and the median over the timed calls is reported; after the
call that sizes the tape and one warm-up call, up to 20 timed calls or as many as fit into --seconds, at least one.  logit of
tests/custom_data_cases.py, N = 10^4 samples, T = 1000 rows.  Forward mode is timed up to its cap of 512.  The compile time is a
host clock around gmmvi_custom_target_compile_* on a text the context has not seen, median of --compiles; the run-time compiler
keeps a cache on disk, so only the first process of a machine that sees these texts measures a compile.
--root: the tree whose gmmvi_amd package and library are timed (default: this one); a tree whose library has no own-batch
entries is timed without them, which is how the shared-batch and full-data figures of two commits are compared."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--dims", default="32,128,600")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0, help="time the timed calls of one entry may take")
    ap.add_argument("--compiles", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import numpy as np
    import custom_data_cases as cases
    from gmmvi_amd import _lib, hip_ops
    from gmmvi_amd.device import get_context
    from time_custom_data_tape import timed_us

    ctx = get_context()
    has_own = "gmmvi_target_custom_data_own_batches" in _lib.EXPORTED_SYMBOLS
    n, t = a.samples, a.rows
    res = {"root": os.path.relpath(root, HERE), "own_batch_entries": has_own, "max_reps": 20, "seconds_per_entry": a.seconds,
           "compile_s": {}, "gradient_calls": []}
    for mode in ("data", "data_tape"):
        times = []
        for i in range(a.compiles):
            t0 = time.perf_counter()
            hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC + f"\n// compile timing {mode} {i}\n", mode=mode)
            times.append(time.perf_counter() - t0)
        res["compile_s"][mode] = {"median": round(statistics.median(times), 3), "all": [round(v, 3) for v in times]}
        print(json.dumps({"compile": mode, **res["compile_s"][mode]}), flush=True)
    routes = {"forward": (hip_ops.target_custom_data, hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data")),
              "tape": (hip_ops.target_custom_data_tape, hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data_tape"))}
    lists = {"full": dict(batch_size=None), "shared": dict(batch_size=a.batch)}
    if has_own:
        lists["own"] = dict(batch_size=a.batch, own_batches=True)
    for d in (int(v) for v in a.dims.split(",")):
        tgt, x = cases.build_case(cases.Case("logit", d, n, t, 0, None, 0))
        params, data, x = ctx.asarray(tgt.params()), ctx.asarray(tgt.data), ctx.asarray(x)
        for route, (op, handle) in routes.items():
            if route == "forward" and d > _lib.CUSTOM_AUTODIFF_MAX_DIM:
                continue
            row = {"target": "logit", "D": d, "N": n, "T": t, "B": a.batch, "route": route}
            grads = {}
            for name, kw in lists.items():
                call = lambda: op(ctx, handle, params, data, x, True, seed=9, call=3, **kw)      # noqa: E731
                grads[name] = call()[1].numpy()                                                  # sizes the tape
                row[name + "_grad_us"], row[name + "_by_kernel_us"], row[name + "_reps"] = timed_us(ctx, call, a.seconds)
            if has_own:
                # sample 0 of the own-batch call sees the shared batch: the two routes agree there before the ratio is reported
                assert np.abs(grads["own"][0] - grads["shared"][0]).max() <= 1e-3 * np.abs(grads["shared"][0]).max()
                row["own_over_shared"] = round(row["own_grad_us"] / row["shared_grad_us"], 2)
            res["gradient_calls"].append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
