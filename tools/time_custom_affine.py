"""Developer tool: what gmmvi_affine gains a network summed over a data set, and what its branch of the sweep costs a source that
does not name it.

  python tools/time_custom_affine.py [--root TREE] [--entries tape:mlp2_vec:16x32x32x8,tape:mlp2_affine:16x32x32x8,...] [--json FILE]

An entry is route:source:shape.  route: ``tape`` (gmmvi_target_custom_data_tape) or ``forward`` (gmmvi_target_custom_data, which
stops at D = 512).  source: ``mlp2_vec`` / ``mlp2_affine`` (shape FxH1xH2xK) and ``keras_loop`` / ``keras_affine`` (shape FxHxK) of
tests/custom_affine_cases.py, and the four sources of tools/time_custom_nodes.py, none of which names gmmvi_affine: ``mlp_loop`` /
``mlp_vec`` (FxHxK), ``logit`` / ``logit_vec`` (D).  The protocol of tools/time_custom_nodes.py: one process per tree; the library's
own HIP-event profile brackets every kernel of a call, a call's time is the sum over its kernels; after the call that sizes the
tape and one warm-up call, up to 20 timed calls or as many as fit into --seconds, at least one; the median and every call's total
are reported.  Full data, N = 4096 samples, T = 1000 rows, lp + gradient.  --root: the tree whose gmmvi_amd package and library
are timed (default: this one), which is how two commits are compared: run this file once per tree, alternating, and take the
spread from the repeats of one tree.  A tree without gmmvi_affine times the other entries only.  Before an entry is timed its
gradient is compared with that of the other source of the same function in the same process, and its sums go into the output,
so that two trees can be compared."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT_ENTRIES = ("tape:logit:512,tape:logit_vec:512,tape:mlp_loop:16x32x8,tape:mlp_vec:16x32x8,"
                   "tape:mlp2_vec:16x32x32x8,tape:mlp2_affine:16x32x32x8,forward:mlp2_vec:8x12x12x4,forward:mlp2_affine:8x12x12x4,"
                   "tape:keras_loop:16x32x8,tape:keras_affine:16x32x8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--entries", default=DEFAULT_ENTRIES)
    ap.add_argument("--seconds", type=float, default=3.0, help="time the timed calls of one entry may take")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import numpy as np
    from gmmvi_amd import _lib, hip_ops                                 # the tree's own package, before anything else imports one
    from gmmvi_amd.device import get_context
    assert os.path.abspath(_lib.__file__).startswith(root + os.sep), _lib.__file__
    sys.path.insert(1, os.path.join(HERE, "tests"))
    sys.path.insert(1, os.path.join(HERE, "tools"))
    import custom_affine_cases as affine_cases
    import custom_data_cases as loop_cases
    import custom_nodes_cases as nodes_cases
    import custom_vector_cases as vec_cases
    import time_custom_data_tape as protocol

    ctx = get_context()
    has_affine = "gmmvi_tape_probe_affine" in _lib.EXPORTED_SYMBOLS
    sources = {"mlp_loop": nodes_cases.SOURCES["mlp_loop"], "mlp_vec": nodes_cases.SOURCES["mlp_vec"],
               "logit": loop_cases.LOGIT_SRC, "logit_vec": vec_cases.LOGIT_VEC_SRC}
    sources.update({name: affine_cases.SOURCES[name] for name in ("mlp2_vec", "mlp2_affine", "keras_loop", "keras_affine")})
    ops = {"tape": (hip_ops.target_custom_data_tape, "data_tape"), "forward": (hip_ops.target_custom_data, "data")}
    n, t = a.samples, a.rows
    out = {"root": os.path.relpath(root, HERE), "package": os.path.relpath(os.path.dirname(_lib.__file__), HERE),
           "affine": has_affine, "N": n, "T": t, "seconds_per_entry": a.seconds, "entries": []}
    inputs, grads = {}, {}
    for entry in a.entries.split(","):
        route, source, shape = entry.split(":")
        if source.endswith("_affine") and not has_affine:
            continue
        family = source.split("_")[0]
        if (family, shape) not in inputs:
            dims = tuple(int(v) for v in shape.split("x"))
            if family in ("mlp2", "keras"):
                d = affine_cases.dim(source, dims)
                tgt, x = affine_cases.build_data_case(affine_cases.Case(family + "_affine", d, n, t, 0, None, 0), dims)
            elif family == "mlp":
                d = nodes_cases.mlp_dim(*dims)
                tgt, x = nodes_cases.build_data_case(nodes_cases.Case("mlp_vec", d, n, t, 0, None, 0), dims)
            else:
                d = dims[0]
                tgt, x = vec_cases.build_data_case(vec_cases.Case("logit_vec", d, n, t, 0, None, 0))
            inputs[(family, shape)] = (d, ctx.asarray(tgt.params()), ctx.asarray(tgt.data), ctx.asarray(x))
        d, params, data, x = inputs[(family, shape)]
        op, mode = ops[route]
        handle = hip_ops.custom_target_compile(ctx, sources[source], mode=mode)
        call = lambda: op(ctx, handle, params, data, x, True)          # noqa: E731
        g = call()[1].numpy()                                           # sizes the tape
        if (family, shape) in grads:                                    # the sources are the same function: the entries agree
            assert np.abs(g - grads[(family, shape)]).max() <= 1e-3 * np.abs(grads[(family, shape)]).max(), entry
        grads[(family, shape)] = g
        totals = []
        us, by_kernel, reps = protocol.timed_us(ctx, call, a.seconds, totals)
        row = {"route": route, "source": source, "shape": shape, "D": d, "grad_us": us, "by_kernel_us": by_kernel, "reps": reps,
               "calls_us": totals, "grad_sum": float(g.astype(np.float64).sum()), "grad_abs_sum": float(np.abs(g.astype(np.float64)).sum())}
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
