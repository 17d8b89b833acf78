"""Developer tool: what a user-defined target summed over a data set (csrc/custom_target_data.inc, DeviceDataLNPDF) costs
against the same posterior written for a differentiated target whose density loops over the rows itself.

  python tools/time_custom_data.py [--json profiles/custom_data_timing.json]

The protocol of tools/time_custom_autodiff.py: one process, HIP events on the context's stream, median of 30 after 3 warm-up
calls.  Logistic regression at D = 31: the breast-cancer rows of tests/golden/logreg_datasets.npz (T = 569) at N = 300 and
N = 10^4, and T = 20 000 synthetic rows at N = 300.  The data-mode text is ``logit`` of tests/custom_data_cases.py; the baseline
is the text below, a ``gmmvi_user_density`` with the data in ``params``, one lane per sample.  Each shape: lp + gradient and lp
alone, on the automatic plan and forced to one chunk."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import custom_data_cases as cases  # noqa: E402
import logreg_ref  # noqa: E402
from time_custom_target import REPS, event_ms  # noqa: E402
from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402
from gmmvi_amd.experiments.target_distributions import logistic_regression as lr  # noqa: E402

# params = [prior mean, prior std, T, rows (T * (D + 1))]: the formulas of cases.LOGIT_SRC, the row loop inside the density
BASELINE_SRC = r"""
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    const int rows = (int)params[2];
    const float* data = params + 3;
    T sum = 0.f;
    for (int r = 0; r < rows; ++r) {
        const float* row = data + (size_t)r * (D + 1);
        T z = 0.f;
        for (int i = 0; i < D; ++i) z += row[i] * x[i];
        z *= row[D];
        sum += -(fmax(-z, 0.f) + log1p(exp(-fabs(z))));
    }
    T q = 0.f;
    for (int i = 0; i < D; ++i) {
        const T r = (x[i] - m) / s;
        q += r * r;
    }
    return sum + (-0.5f * q - D * (logf(s) + 0.9189385332046727f));
}
"""


def breast_cancer_rows():
    table = logreg_ref.load_tables()["breast_cancer"]
    A, _ = lr.preprocess(table, "breast_cancer")
    s = np.where(lr.split_table(table, "breast_cancer")[1] == 1, -1.0, 1.0).astype(np.float32)
    return np.concatenate([A * s[:, None], s[:, None]], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = get_context()
    rng = np.random.default_rng(0)
    real = breast_cancer_rows()
    d = real.shape[1] - 1
    synthetic = np.concatenate([rng.normal(size=(20000, d)) / np.sqrt(d), rng.choice([-1.0, 1.0], size=(20000, 1))], axis=1).astype(np.float32)
    prior = np.array([lr.PRIOR_MEAN, lr.PRIOR_STD], np.float32)
    h_data = hip_ops.custom_target_compile(ctx, cases.LOGIT_SRC, mode="data")
    h_base = hip_ops.custom_target_compile(ctx, BASELINE_SRC, mode="autodiff")
    rows = []
    for label, data, n in (("breast_cancer", real, 300), ("breast_cancer", real, 10000), ("synthetic", synthetic, 300)):
        t = data.shape[0]
        x = ctx.asarray((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
        data_dev, prior_dev = ctx.asarray(data), ctx.asarray(prior)
        base_params = ctx.asarray(np.concatenate([prior, [t], data.ravel()]).astype(np.float32))

        def run_data(want_grad, chunks):
            return hip_ops.target_custom_data(ctx, h_data, prior_dev, data_dev, x, want_grad, chunks=chunks)

        def run_base(want_grad):
            return hip_ops.target_custom(ctx, h_base, base_params, x, want_grad)

        # the two agree before they are timed
        lp_d, g_d = run_data(True, 0)
        lp_b, g_b = run_base(True)
        assert np.abs(lp_d.numpy() - lp_b.numpy()).max() <= 1e-4 * np.abs(lp_b.numpy()).max()
        assert np.abs(g_d.numpy() - g_b.numpy()).max() <= 1e-3 * np.abs(g_b.numpy()).max()
        chunks, per = hip_ops.custom_data_plan(n, t)
        row = {"data": label, "D": d, "T": t, "N": n, "chunks": chunks, "rows_per_chunk": per,
               "data_grad_us": event_ms(ctx, lambda: run_data(True, 0)),
               "data_grad_one_chunk_us": event_ms(ctx, lambda: run_data(True, 1)),
               "baseline_grad_us": event_ms(ctx, lambda: run_base(True)),
               "data_value_us": event_ms(ctx, lambda: run_data(False, 0)),
               "data_value_one_chunk_us": event_ms(ctx, lambda: run_data(False, 1)),
               "baseline_value_us": event_ms(ctx, lambda: run_base(False))}
        row["baseline_over_data_grad"] = round(row["baseline_grad_us"] / row["data_grad_us"], 2)
        row["baseline_over_data_value"] = round(row["baseline_value_us"] / row["data_value_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"protocol": "tools/time_custom_data.py: one process, HIP events on the context's stream, median of 30 after 3 warm-up "
                       "calls; baseline: a DeviceAutodiffLNPDF density that loops over the rows itself, data in params",
           "reps": REPS, "shapes": rows}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
