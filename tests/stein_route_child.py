"""Child process of test_hip_stein.py (not a test module): the library reads GMMVI_BLOCKED_ABOVE once per process, so the
DP = 64 instance of the register-resident Stein kernels (D = 51 ... 63) runs here, in a fresh interpreter with the knob in its
environment.

    python stein_route_child.py OUT.npz CASE_ID ...

The cases are rebuilt from stein_cases.py by their ids; OUT receives, per case c and weighting s (1 self-normalised, 0 plain),
c{c}_s{s}_h / _g of a first call and c{c}_s{s}_h2 / _g2 of a second one.  The parent computes the references."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stein_cases as cases  # noqa: E402


def run_case(ctx, case, snis):
    """-> (H_neg, g_neg) of the device for one case and weighting, as NumPy arrays."""
    from gmmvi_amd import hip_ops
    d = case["d"]
    means, x = ctx.asarray(case["means"]), ctx.asarray(case["x"])
    args = (x, ctx.asarray(case["ld"]), ctx.asarray(case["qgrad"]), ctx.asarray(case["bg"]), ctx.asarray(case["tgrad"]), d)
    kw = dict(self_normalized=snis, own_samples_only=case["own"])
    if case["own"]:
        kw.update(mapping=ctx.asarray(case["mapping"], np.int32), map_offset=case["map_offset"])
    if case["route"] == "diag":
        h, g = hip_ops.diag_stein(ctx, hip_ops.diag_pack(ctx, means, ctx.asarray(case["sigma"])), *args, **kw)
    else:
        packed, _ = hip_ops.pack_components(ctx, means, ctx.asarray(case["chols"]))
        h, g = hip_ops.stein(ctx, packed, *args, **kw)
    return h.numpy(), g.numpy()


def main(dst, ids):
    from gmmvi_amd.device import get_context
    ctx = get_context()
    res = {}
    for c, case_id in enumerate(ids):
        case = cases.make_case(cases.spec_by_id(case_id))
        for snis in (True, False):
            for rep in ("", "2"):
                res[f"c{c}_s{int(snis)}_h{rep}"], res[f"c{c}_s{int(snis)}_g{rep}"] = run_case(ctx, case, snis)
    np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
