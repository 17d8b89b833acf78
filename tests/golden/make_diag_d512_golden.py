"""Records the diagonal kernels' outputs at D = 512 (fixed seed) into diag_d512_parent.npz.

Run ONCE on the commit before the D > 512 diagonal path existed (python tests/golden/make_diag_d512_golden.py, on the GPU);
tests/test_hip_diag_highd.py::test_d512_bitwise_unchanged replays inputs() on the current build and compares bit for bit.
The fixture is this project's own output."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

K, D, N, SEED = 3, 512, 70, 512


def inputs():
    rng = np.random.default_rng(SEED)
    means = (rng.normal(size=(K, D)) * 3.0).astype(np.float32)
    sigma = np.sqrt(rng.uniform(0.3, 3.0, size=(K, D))).astype(np.float32)
    w = rng.random(K) + 0.1
    logw = np.log(w / w.sum()).astype(np.float32)
    x = (means[rng.integers(0, K, N)] + rng.normal(size=(N, D)) * 1.5).astype(np.float32)
    hs = (rng.normal(size=(K, D)) * 0.5 + 0.3).astype(np.float32)
    gs = rng.normal(size=(K, D)).astype(np.float32)
    steps = np.linspace(0.05, 0.5, K).astype(np.float32)
    return means, sigma, logw, x, hs, gs, steps


def run(ctx):
    """-> dict of the outputs the fixture holds."""
    from gmmvi_amd import hip_ops
    means, sigma, logw, x, hs, gs, steps = inputs()
    md, sd = ctx.asarray(means), ctx.asarray(sigma)
    packed = hip_ops.diag_pack(ctx, md, sd)
    ld, lp, grad = hip_ops.diag_mixture_eval(ctx, packed, ctx.asarray(logw), ctx.asarray(x), D, want_ld=True, want_lp=True,
                                             want_grad=True)
    out = {"packed": packed.numpy(), "ld": ld.numpy(), "lp": lp.numpy(), "grad": grad.numpy()}
    last_eta, l2, nupd = ctx.asarray(np.full(K, -1.0, np.float32)), ctx.full((K,), 1e-12), ctx.zeros((K,))
    for r in range(2):
        succ, kl, probes = hip_ops.update_components_diag(ctx, "kl", md, sd, ctx.asarray(hs), ctx.asarray(gs), ctx.asarray(steps),
                                                          1.0, 1e-12, last_eta, l2, nupd, want_info=True)
        out.update({f"kl{r}_means": md.numpy(), f"kl{r}_sigma": sd.numpy(), f"kl{r}_eta": last_eta.numpy(),
                    f"kl{r}_success": succ.numpy(), f"kl{r}_kl": kl.numpy(), f"kl{r}_probes": probes.numpy()})
    mi, si = ctx.asarray(means), ctx.asarray(sigma)
    l2i, nupdi = ctx.full((K,), 1e-12), ctx.zeros((K,))
    for r in range(2):
        succ, _, _ = hip_ops.update_components_diag(ctx, "iblr", mi, si, ctx.asarray(hs), ctx.asarray(gs),
                                                    ctx.asarray(np.full(K, 0.3, np.float32)), 0.0, 1e-12, None, l2i, nupdi)
        out.update({f"iblr{r}_means": mi.numpy(), f"iblr{r}_sigma": si.numpy(), f"iblr{r}_success": succ.numpy()})
    return out


if __name__ == "__main__":
    from gmmvi_amd.device import get_context
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "diag_d512_parent.npz")
    np.savez_compressed(dst, **run(get_context()))
    print("wrote", dst)
