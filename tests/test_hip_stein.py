"""GPU parity of the three Stein estimators against fp64 ON THEIR OWN INPUTS and at their seams: the matrix-core moment kernel
with stein_finalize (csrc/stein.hip, stein_finalize.h), the blocked route (gmmvi_blocked_stein, csrc/blocked.hip) and the
diagonal kernel (diag_stein_kernel, csrc/diag_sweep.hip).

The model-level tests (test_hip_kernels.test_stein, test_hip_blocked, the diagonal tests) let the oracle recompute ld and
grad log q in fp64, so their tolerance has to absorb the fp32 density error amplified by exp(ld - bg): 3e-3 of the largest
element.  Here the device and the reference read the same fp32-representable ld, qgrad, bg, tgrad and mapping
(stein_cases.py), and every element of H and g is held to

    |device - reference| <= C * EPS32 * B,

B the same sums over absolute values (stein_cases.abs_bound) and C = 128 = 8 x the worst error of the float32 NumPy evaluation
of the same formulas, in the same units, measured on the reference alone.  test_stein_cases_cpu.py shows that every planted
fault -- one seam sample left out, a range left out, a chunk not rescaled, the wrong symmetrisation, orientation, mean or
divisor -- lies ten times outside that bound on every case.  Two calls on the same inputs must agree bit for bit (the kernels
promise a fixed summation order)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stein_cases as cases
from stein_route_child import run_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = cases.case_table()
PARTIAL = [s for s in TABLE if "-R" in s["id"]]
FIXED = [s for s in TABLE if "-R" not in s["id"]]


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def _check(case, snis, got, again):
    ref, bound = cases.reference(case, snis), cases.abs_bound(case, snis)
    ratios = [cases.error_ratio([g], [r], [b]) for g, r, b in zip(got, ref, bound)]
    print(f"{case['id']} snis={snis}: H {ratios[0]:.2f}  g {ratios[1]:.2f}  (EPS32 B; bound {cases.C:.0f})")
    for g, r, b, name in zip(got, ref, bound, ("H", "g")):
        live = (b > 0) & np.isfinite(r)
        # the empty own set: zeros / NaN, exactly
        np.testing.assert_array_equal(g[~live], r[~live].astype(np.float32), err_msg=f"{name} {case['id']} snis={snis}")
        excess = np.abs(g.astype(np.float64) - r)[live] / (cases.C * cases.EPS32 * b[live])
        assert not np.isnan(excess).any() and np.all(excess <= 1.0), \
            f"{name} {case['id']} snis={snis}: {excess.max() * cases.C:.1f} EPS32 B at the worst element, bound {cases.C:.0f}"
    for g, g2, name in zip(got, again, ("H", "g")):
        assert np.array_equal(g, g2, equal_nan=True), f"{name} {case['id']} snis={snis}: two calls differ"
    return ratios


def _run(ctx, case):
    for snis in cases.modes(case):
        _check(case, snis, run_case(ctx, case, snis), run_case(ctx, case, snis))


@pytest.mark.parametrize("spec", FIXED, ids=[s["id"] for s in FIXED])
def test_stein_on_its_own_inputs(ctx, spec):
    """Every case of stein_cases.case_table() whose shape does not depend on the device, both weightings."""
    _run(ctx, cases.make_case(spec))


@pytest.mark.parametrize("spec", PARTIAL, ids=[s["id"] for s in PARTIAL])
def test_stein_partial_counts(ctx, spec):
    """One stack summed from R = 1, 7, 8, 9, 16, 17 partials (the eight chains of stein_slab_sum and its clamped tail): N is
    recomputed from the compute units of this device."""
    r = int(spec["id"].split("-R")[1].split("-")[0])
    n = cases.n_for_partials(r, spec["d"], ctx.num_cus)
    if n is None:
        pytest.skip(f"{ctx.num_cus} compute units cannot give one stack {r} partials")
    assert cases.register_geometry(spec["d"], 1, n, ctx.num_cus)["R"] == r
    _run(ctx, cases.make_case(spec, n=n))


def test_stein_register_instance_for_d_51_to_63(tmp_path):
    """GMMVI_BLOCKED_ABOVE=64 sends D = 51 and 63 to the DP = 64 instance of the register route: one child process
    (stein_route_child.py) runs the cases, the parent compares."""
    table = cases.register64_table()
    dst = tmp_path / "stein64.npz"
    env = dict(os.environ, GMMVI_BLOCKED_ABOVE="64")
    r = subprocess.run([sys.executable, os.path.join(HERE, "stein_route_child.py"), str(dst)] + [s["id"] for s in table], env=env,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    out = np.load(dst)
    for c, spec in enumerate(table):
        case = cases.make_case(spec)
        for snis in cases.modes(spec):
            key = f"c{c}_s{int(snis)}_"
            _check(case, snis, (out[key + "h"], out[key + "g"]), (out[key + "h2"], out[key + "g2"]))
