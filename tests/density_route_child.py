"""Child process of test_hip_density_routes.py (not a test module): the library reads the GMMVI_ME_PK* knobs once per
process, so the sweeps with the packed route forced run here, in a fresh interpreter with the knobs in its environment.

    python density_route_child.py IN.npz OUT.npz

IN holds ncases and, per case c, c{c}_family / means / chols / logw / logw2 / x; OUT receives per case the component log
densities (c{c}_ld, and c{c}_ld1 from the ld-only sweep), the mixture log density (c{c}_lp), the gradient sweep (c{c}_lpg,
c{c}_grad; padded D <= 40) and the dual sweep (c{c}_lpd, c{c}_lp2d, c{c}_gradd).  The parent computes the references."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gmmvi_amd import _lib, hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

NU = 2.0


def padded_dim(d):
    return next(dp for dp in (2, 4, 8, 10, 12, 16, 20, 24, 32, 40, 50, 64) if d <= dp)


def run_case(ctx, family, means, chols, logw, logw2, x):
    k, d = means.shape
    n = x.shape[0]
    nu = NU if family == _lib.STUDENT_T else 0.0
    grad_ok = padded_dim(d) <= 40
    packed, _ = hip_ops.pack_components(ctx, ctx.asarray(means), ctx.asarray(chols), family=family, nu=nu)
    lw, lw2, xd = ctx.asarray(logw), ctx.asarray(logw2), ctx.asarray(x)
    out = {}
    ld, lp, _ = hip_ops.mixture_eval(ctx, packed, lw, xd, d, family=family, nu=nu, want_ld=True, want_lp=True)
    out["ld"], out["lp"] = ld.numpy(), lp.numpy()
    out["ld1"] = hip_ops.mixture_eval(ctx, packed, lw, xd, d, family=family, nu=nu, want_ld=True, want_lp=False)[0].numpy()
    if grad_ok:
        _, lpg, grad = hip_ops.mixture_eval(ctx, packed, lw, xd, d, family=family, nu=nu, want_grad=True)
        out["lpg"], out["grad"] = lpg.numpy(), grad.numpy()
    lpd, lp2d = ctx.empty((n,)), ctx.empty((n,))
    gradd = ctx.empty((n, d)) if grad_ok else None
    ctx.check(ctx.lib.gmmvi_mixture_eval_dual(ctx.handle, family, nu, k, d, packed.ptr, lw.ptr, lw2.ptr, xd.ptr, n, None,
                                              lpd.ptr, None if gradd is None else gradd.ptr, lp2d.ptr))
    out["lpd"], out["lp2d"] = lpd.numpy(), lp2d.numpy()
    if grad_ok:
        out["gradd"] = gradd.numpy()
    return out


def main(src, dst):
    ctx = get_context()
    inp = np.load(src)
    res = {}
    for c in range(int(inp["ncases"])):
        args = [inp[f"c{c}_{key}"] for key in ("means", "chols", "logw", "logw2", "x")]
        for key, v in run_case(ctx, int(inp[f"c{c}_family"]), *args).items():
            res[f"c{c}_{key}"] = v
    np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
