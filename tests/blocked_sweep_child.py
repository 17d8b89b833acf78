"""The device side of test_hip_blocked_sweep.py, and its child process (not a test module): the library reads GMMVI_BLOCKED_F32
once per process, so the f32 matrix-core route of the blocked density sweep at D >= 160 runs here, in a fresh interpreter with
the knob in its environment.

    python blocked_sweep_child.py IN.npz OUT.npz

IN holds, per case c, c{c}_block / _logw / _logw2 / _x and c{c}_meta = (family, nu, D); OUT receives c{c}_{call}_{output} for the
eight calls of CALLS.  The parent builds the cases and computes the references."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SENTINEL = np.float32(-1.2345e30)            # what every output array holds before a call: no element may keep it
# name -> (ld, lp, grad, dual): the combinations of outputs gmmvi_blocked_mixture_eval carves its scratch by.  The dual form
# (gmmvi_mixture_eval_dual) always returns lp and lp2
CALLS = {"ld": (True, False, False, False), "lp": (False, True, False, False), "ld_lp": (True, True, False, False),
         "lp_grad": (False, True, True, False), "grad": (False, False, True, False), "ld_lp_grad": (True, True, True, False),
         "dual_ld_grad": (True, True, True, True), "dual": (False, True, False, True)}


def upload(ctx, case):
    """The inputs of a case on the device, once: the component block as a plain [K, stride] array."""
    from gmmvi_amd import hip_ops
    block, x = np.asarray(case["block"]), np.asarray(case["x"])
    assert block.dtype == np.float32 and block.shape[1] == hip_ops.packed_stride(int(case["d"])), "not the library's block stride"
    assert x.ndim == 2 and x.shape[1] == int(case["d"]) and len(case["logw"]) == len(case["logw2"]) == block.shape[0]
    return dict(block=ctx.asarray(case["block"]), logw=ctx.asarray(case["logw"]), logw2=ctx.asarray(case["logw2"]),
                x=ctx.asarray(case["x"]), family=int(case["family_id"]), nu=float(case["nu"]), d=int(case["d"]))


def run_call(ctx, dev, call):
    """One call straight through ctx.lib, with the output arrays filled with SENTINEL before -> {output: NumPy array}."""
    want_ld, want_lp, want_grad, dual = CALLS[call]
    k, n, d = dev["block"].shape[0], dev["x"].shape[0], dev["d"]
    out = {}
    if want_ld:
        out["ld"] = ctx.full((k, n), SENTINEL)
    if want_lp:
        out["lp"] = ctx.full((n,), SENTINEL)
    if want_grad:
        out["grad"] = ctx.full((n, d), SENTINEL)
    if dual:
        out["lp2"] = ctx.full((n,), SENTINEL)
    ptr = lambda key: out[key].ptr if key in out else None                             # noqa: E731
    if dual:
        rc = ctx.lib.gmmvi_mixture_eval_dual(ctx.handle, dev["family"], dev["nu"], k, d, dev["block"].ptr, dev["logw"].ptr,
                                             dev["logw2"].ptr, dev["x"].ptr, n, ptr("ld"), ptr("lp"), ptr("grad"), ptr("lp2"))
    else:
        rc = ctx.lib.gmmvi_mixture_eval(ctx.handle, dev["family"], dev["nu"], k, d, dev["block"].ptr, dev["logw"].ptr,
                                        dev["x"].ptr, n, ptr("ld"), ptr("lp"), ptr("grad"))
    ctx.check(rc)
    return {key: a.numpy() for key, a in out.items()}


def run_calls(ctx, dev, calls=tuple(CALLS)):
    return {call: run_call(ctx, dev, call) for call in calls}


def main(src, dst):
    from gmmvi_amd.device import get_context
    ctx = get_context()
    data = np.load(src)
    res = {}
    for c in range(int(data["ncases"])):
        family, nu, d = data[f"c{c}_meta"]
        case = dict(block=data[f"c{c}_block"], logw=data[f"c{c}_logw"], logw2=data[f"c{c}_logw2"], x=data[f"c{c}_x"],
                    family_id=int(family), nu=float(nu), d=int(d))
        for call, out in run_calls(ctx, upload(ctx, case)).items():
            for key, a in out.items():
                res[f"c{c}_{call}_{key}"] = a
    np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
