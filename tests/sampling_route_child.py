"""Device calls of test_hip_sampling.py, and its child process (not a test module): the library reads GMMVI_BLOCKED_ABOVE once
per process, so the DP = 64 instance of the register sampling route (D = 51 ... 63) runs here, in a fresh interpreter with the
knob in its environment.

    python sampling_route_child.py OUT.npz

runs the cases of sampling_cases.register64_table() through the stand-alone launch and the twins of the single-call iteration
at sampling_cases.TWIN64_SHAPE.  OUT receives c{i}_{name} per case i (the arrays of run_case) and twin_{name} (the arrays of
run_twins); a call the library refuses is recorded as c{i}_error / twin_error (its message) and the run goes on, unless the message
names a device fault.  The parent computes the references and asserts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_cases as cases  # noqa: E402

PAD = 3                                   # rows behind the N the kernels are given
SENTINEL = -7.0e7
SENTINEL_MAP = -12345
TWIN_SEED = 23
TWIN_ITERS = 3
MODEL_ARRAYS = ("means", "chol_cov", "log_weights", "stepsizes")


def draw(ctx, case, eps=None, mapping=True):
    """gmmvi_sample_components / gmmvi_diag_sample called directly on buffers PAD rows longer than N and pre-filled with a
    sentinel -> (x [N + PAD, D], mapping [N + PAD] or None, the supplied eps buffer re-read after the call or None).
    ``eps``: an [N, D] array (host or device) of normals to use; None: the device's Philox stream of the case."""
    k, d, n = case["k"], case["d"], case["n"]
    diag = case["route"] == "diag"
    means, fac = ctx.asarray(case["means"]), ctx.asarray(case["sigma" if diag else "chols"])
    offsets = ctx.asarray(case["offsets"], np.int32)
    x = ctx.full((n + PAD, d), SENTINEL)
    mp = ctx.full((n + PAD,), SENTINEL_MAP, np.int32) if mapping else None
    eps_dev = None if eps is None else ctx.asarray(eps)
    fn = ctx.lib.gmmvi_diag_sample if diag else ctx.lib.gmmvi_sample_components
    ctx.check(fn(ctx.handle, k, d, means.ptr, fac.ptr, offsets.ptr, n, case["seed"], case["first_index"], case["stream_id"],
                 None if eps_dev is None else eps_dev.ptr, x.ptr, None if mp is None else mp.ptr))
    return x.numpy(), None if mp is None else mp.numpy(), None if eps_dev is None else eps_dev.numpy()


def run_case(ctx, case):
    """-> dict: x_eps, map_eps, eps_after (eps supplied); x_nomap (the same call with mapping_out = NULL); x_dev, map_dev (the
    device's Philox stream); normals (gmmvi_philox_normals of the same seed, first index and stream) and x_fed (the call fed
    those)."""
    from gmmvi_amd import hip_ops
    out = {}
    out["x_eps"], out["map_eps"], out["eps_after"] = draw(ctx, case, eps=case["eps"])
    out["x_nomap"], _, _ = draw(ctx, case, eps=case["eps"], mapping=False)
    out["x_dev"], out["map_dev"], _ = draw(ctx, case)
    normals = hip_ops.philox_normals(ctx, case["seed"], case["first_index"], case["n"], case["d"], case["stream_id"])
    out["normals"] = normals.numpy()
    out["x_fed"], _, _ = draw(ctx, case, eps=normals)
    return out


def run_twins(d, per_component, k=cases.TWIN_K, seed=TWIN_SEED, iters=TWIN_ITERS):
    """Two GMMVI objects on the single-call iteration, ``early`` drawing the next iteration's samples as a rider of the
    expected-log-ratio launch (csrc/riders.h) and ``plain`` in the sampling launch -> dict: means0, chols0 (the initial
    components), first0, per twin t in (early, plain): {t}_{model array}, {t}_samples, {t}_mapping; eligible, presampled."""
    from helpers import samtron_config, make_oracle, make_device
    cfg = samtron_config(per_component)
    o = make_oracle("gmm", d, k, per_component, seed, cfg)
    early = make_device("gmm", d, k, per_component, seed, cfg, o)
    plain = make_device("gmm", d, k, per_component, seed, cfg, o)
    plain._fast_path.presample = False
    out = dict(means0=early.model.means.numpy().copy(), chols0=early.model.chol_cov.numpy().copy(),
               first0=np.int64(int(early.sample_db.num_samples_written)), seed=np.int64(seed))
    eligible = True
    for g in (early, plain):
        g._fast_path.explicit_estimate = True
    for _ in range(iters):
        for g in (early, plain):
            eligible = eligible and bool(g._fast_path.eligible())
            g.train_iter()
    out["eligible"] = np.bool_(eligible)
    out["presampled"] = np.bool_(early._fast_path._presample_token is not None and plain._fast_path._presample_token is None)
    for tag, g in (("early", early), ("plain", plain)):
        for name in MODEL_ARRAYS:
            out[f"{tag}_{name}"] = getattr(g.model, name).numpy()
        out[f"{tag}_samples"] = g.sample_db.samples.numpy()
        out[f"{tag}_mapping"] = g.sample_db.mapping.numpy()
    return out


def _device_fault(message):
    m = message.lower()
    return any(w in m for w in ("illegal", "fault", "abort", "unspecified", "hardware", "hang"))


def main(dst):
    from gmmvi_amd.device import get_context
    from gmmvi_amd._lib import GmmviError
    ctx = get_context()
    res = {}
    try:
        for i, spec in enumerate(cases.register64_table()):
            try:
                res.update({f"c{i}_{name}": v for name, v in run_case(ctx, cases.make_case(spec)).items()})
            except GmmviError as e:
                res[f"c{i}_error"] = np.asarray(str(e))
                if _device_fault(str(e)):
                    return
        try:
            res.update({f"twin_{name}": v for name, v in run_twins(*cases.TWIN64_SHAPE).items()})
        except GmmviError as e:
            res["twin_error"] = np.asarray(str(e))
    finally:
        np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1])
