"""Child process of test_hip_more.py (not a test module): the library reads GMMVI_BLOCKED_ABOVE once per process, so D = 51 and
63 packed in the register layout (the DP = 64 instance of the tiled route without the re-packing) run here, in a fresh
interpreter with the knob in its environment; so does the blocked call whose workspace budget (GMMVI_MORE_WS_GB, set around the
call from the case) leaves a ragged last group.

    python more_route_child.py OUT.npz CASE_ID ...

The cases are rebuilt from more_cases.py by their ids; OUT receives, per case c, c{c}_h / _g of a first call, c{c}_h2 / _g2 of a
second one and c{c}_packed, the component blocks the kernels read.  The parent computes the residuals."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import more_cases as cases  # noqa: E402


def run_case(ctx, case):
    """-> (H_neg, g_neg, packed) of the device for one case, as NumPy arrays; packed are the component blocks of the call."""
    from gmmvi_amd import hip_ops
    d = case["d"]
    means, x = ctx.asarray(case["means"]), ctx.asarray(case["x"])
    kw = dict(self_normalized=case["snis"], own_samples_only=case["own"])
    if case["own"]:
        ld = bg = None
        kw.update(mapping=ctx.asarray(case["mapping"], np.int32), map_offset=case["map_offset"])
    else:
        ld, bg = ctx.asarray(case["ld"]), ctx.asarray(case["bg"])
    tail = (x, ld, ctx.asarray(case["logq"]), bg, ctx.asarray(case["tlp"]), ctx.asarray(case["l2"]), d)
    saved = os.environ.get("GMMVI_MORE_WS_GB")
    if "ws_gb" in case:
        os.environ["GMMVI_MORE_WS_GB"] = repr(case["ws_gb"])
    try:
        if case["route"] == "diag":
            packed = hip_ops.diag_pack(ctx, means, ctx.asarray(case["sigma"]))
            h, g = hip_ops.more_diag(ctx, packed, *tail, **kw)
        else:
            chols = ctx.asarray(case["chols"])
            packed, _ = hip_ops.pack_components(ctx, means, chols)
            fn = hip_ops.more_blocked if case["route"] == "blocked" else hip_ops.more
            h, g = fn(ctx, packed, chols, *tail, **kw)
        return h.numpy(), g.numpy(), packed.numpy()
    finally:
        if "ws_gb" in case:
            if saved is None:
                del os.environ["GMMVI_MORE_WS_GB"]
            else:
                os.environ["GMMVI_MORE_WS_GB"] = saved


def main(dst, ids):
    from gmmvi_amd.device import get_context
    ctx = get_context()
    res = {}
    for c, case_id in enumerate(ids):
        case = cases.make_case(cases.spec_by_id(case_id))
        res[f"c{c}_h"], res[f"c{c}_g"], res[f"c{c}_packed"] = run_case(ctx, case)
        res[f"c{c}_h2"], res[f"c{c}_g2"], _ = run_case(ctx, case)
    np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
