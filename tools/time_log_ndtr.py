"""Developer tool: what gmmvi_log_ndtr costs per row next to the plain form log(0.5f * erfc(.)), by HIP events.

  python tools/time_log_ndtr.py

The probit target of tests/custom_normal_cases.py (without its planted row) and the same source with the plain form, compiled in the
data mode (forward-mode gradients) at D = 16, T = 4096 rows, N = 1024 samples, full data: the value call and the gradient call of
gmmvi_target_custom_data, each the median of 30 launches between two HIP events after 3 warm-up launches.  One JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import custom_normal_cases as cases  # noqa: E402
from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402

D, T, N, REPS, WARMUP = 16, 4096, 1024, 30, 3


def _median_us(ctx, launch):
    for _ in range(WARMUP):
        launch()
    times = []
    for _ in range(REPS):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        launch()
        ctx.record(e1)
        ctx.sync()
        times.append(ctx.elapsed_ms(e0, e1) * 1e3)
    return float(np.median(times))


def main():
    ctx = get_context()
    rng = np.random.default_rng(0)
    features = rng.normal(size=(T, D)) / np.sqrt(D)
    labels = rng.integers(0, 2, size=(T, 1)).astype(np.float64)
    data = ctx.asarray(np.concatenate([features, labels], axis=1).astype(np.float32))
    x = ctx.asarray(rng.normal(size=(N, D)).astype(np.float32))
    params = ctx.asarray(np.array([0.25, 2.0], np.float32))
    lp, grad = ctx.full((N,), 0.0), ctx.full((N, D), 0.0)
    out = {"D": D, "T": T, "N": N, "reps": REPS}
    for name, source in (("log_ndtr", cases.PROBIT_SRC), ("plain_erfc", cases.PROBIT_PLAIN_SRC)):
        handle = hip_ops.custom_target_compile(ctx, source, mode="data")
        for call, g in (("lp", None), ("grad", grad.ptr)):
            def launch():
                rc = ctx.lib.gmmvi_target_custom_data(ctx.handle, handle.handle, D, params.ptr, data.ptr, T, D + 1, 0, T, 0, 0, x.ptr, N,
                                                      lp.ptr, g, 0)
                assert rc == 0, ctx.lib.gmmvi_last_error(ctx.handle).decode()
            us = _median_us(ctx, launch)
            out[f"{name}_{call}_us"] = round(us, 1)
            out[f"{name}_{call}_ns_per_row_and_sample"] = round(us * 1e3 / (T * N), 4)
        out[f"{name}_finite"] = bool(np.all(np.isfinite(lp.numpy())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
