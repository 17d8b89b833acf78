"""Developer tool: what the vector primitives of user-defined targets (gmmvi_dot, gmmvi_sumsq) gain a logistic regression summed
over a data set, and what the vector branch of the sweep costs a source that does not use them.

  python tools/time_custom_vector.py [--root TREE] [--entries tape:loop:512,tape:vec:512,...] [--json FILE]

An entry is route:source:D.  route: ``tape`` (gmmvi_target_custom_data_tape) or ``forward`` (gmmvi_target_custom_data); source:
``loop`` (logit of tests/custom_data_cases.py, scalar loops) or ``vec`` (logit_vec of tests/custom_vector_cases.py).  The
protocol of tools/time_custom_data_tape.py (its timed_us): one process; the library's own HIP-event profile brackets every
kernel of a call, a call's time is the sum over its kernels; after the call that sizes the tape and one warm-up call, up to 20
timed calls or as many as fit into --seconds, at least one; the median and every call's total are reported.  Full data, N = 4096
samples, T = 1000 rows.  --root: the tree whose gmmvi_amd package and library are timed (default: this one), which is how two
commits are compared: run this file once per tree, alternating, and take the spread from the repeats of one tree.  A tree
without the primitives times ``loop`` entries only."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--entries", default="tape:loop:512,tape:vec:512,forward:loop:512,forward:vec:512,tape:vec:4096,tape:loop:4096")
    ap.add_argument("--seconds", type=float, default=3.0, help="time the timed calls of one entry may take")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import numpy as np
    import custom_data_cases as loop_cases
    import custom_vector_cases as vec_cases
    import time_custom_data_tape as protocol
    from gmmvi_amd import _lib, hip_ops
    from gmmvi_amd.device import get_context

    ctx = get_context()
    has_vector = hasattr(_lib, "VECTOR_OPS")
    sources = {"loop": loop_cases.LOGIT_SRC, "vec": vec_cases.LOGIT_VEC_SRC}
    ops = {"tape": (hip_ops.target_custom_data_tape, "data_tape"), "forward": (hip_ops.target_custom_data, "data")}
    n, t = a.samples, a.rows
    out = {"root": os.path.relpath(root, HERE), "vector_primitives": has_vector, "N": n, "T": t, "seconds_per_entry": a.seconds,
           "entries": []}
    inputs, grads = {}, {}
    for entry in a.entries.split(","):
        route, source, d = entry.split(":")
        d = int(d)
        if source == "vec" and not has_vector:
            continue
        if d not in inputs:
            tgt, x = vec_cases.build_data_case(vec_cases.Case("logit_vec", d, n, t, 0, None, 0))
            inputs[d] = (ctx.asarray(tgt.params()), ctx.asarray(tgt.data), ctx.asarray(x))
        params, data, x = inputs[d]
        op, mode = ops[route]
        handle = hip_ops.custom_target_compile(ctx, sources[source], mode=mode)
        call = lambda: op(ctx, handle, params, data, x, True)          # noqa: E731
        g = call()[1].numpy()                                           # sizes the tape
        if d in grads:                                                  # the sources are the same function: the entries agree
            assert np.abs(g - grads[d]).max() <= 1e-3 * np.abs(grads[d]).max(), entry
        grads[d] = g
        # timed_us keeps the median; every call's total is kept here as well, for the spread within one process
        totals = []
        report = protocol.report

        def recording(c):
            r = report(c)
            totals.append(round(sum(r.values()) * 1e3, 1))
            return r

        protocol.report = recording
        try:
            us, by_kernel, reps = protocol.timed_us(ctx, call, a.seconds)
        finally:
            protocol.report = report
        row = {"route": route, "source": source, "D": d, "grad_us": us, "by_kernel_us": by_kernel, "reps": reps, "calls_us": totals}
        if mode == "data_tape":
            row["tape_length"] = hip_ops.custom_tape_length(ctx, handle, d)
        out["entries"].append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
