"""GPU test of the MORE estimators against fp64 ON THEIR OWN INPUTS and at their seams: the register-resident route and the
tiled route of csrc/more.hip, gmmvi_more_blocked (csrc/more_blocked.hip) and gmmvi_more_diag (csrc/more_diag.hip).

The model-level tests (test_hip_kernels.test_more*, test_hip_more_blocked, test_hip_more_diag) let the oracle recompute ld and
log q in fp64 and compare the estimate itself, whose forward error grows with the conditioning of the regression: 1e-2 of the
largest entry.  Here the device and the reference read the same fp32-representable arrays (more_cases.py) and the device's
(H, g) is held to the normal equations it claims to solve: mapped back to whitened coefficients theta in fp64, every row but the
bias must satisfy

    |Phi^T (w (Phi theta - r)) + Lambda theta|_f <= C * 2^-24 * B_f,

B the same sums over absolute values plus the fp32 rounding of the outputs (more_cases.residual_ratio), C = 8 x the worst ratio
of the float32 NumPy model of the kernels' formulation, per law class, measured on the reference alone (register 8, tiled
0.4, blocked 0.2, diagonal 6.4; rewards offset by -1e4: tiled 1.6, blocked 3.2).  test_more_cases_cpu.py shows that every
planted fault -- a seam sample, a tile or a chunk partial left out, weights not normalised, the ridge on the bias, the
neighbour's mean, L for L^T, the diagonal factor, the feature order, the sign of g, map_offset off by one, ld for log q in the
reward -- lies ten times outside that bound on every case designated for it.  Two calls on the same inputs must agree bit for bit; a component without a weighted sample is NaN in every element;
non-finite x, tlp and log q on samples without weight must not change a bit of the result.  The forward deviation from the fp64
solve is printed where that solve is cheap, never asserted.

Largest ratio per route on an MI355X (256 compute units), in units of 2^-24 B: DESIGN.md, "MORE estimators on their own inputs"."""
import os
import subprocess
import sys

import numpy as np
import pytest

import more_cases as cases
from more_route_child import run_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = cases.case_table()
CHUNKS = [s for s in TABLE if "chunk_shape" in s]
FIXED = [s for s in TABLE if "chunk_shape" not in s]
CHEAP_FEATURES = 700                     # the fp64 reference solve is printed up to this feature count


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def _check(case, got, again, packed):
    h, g = got
    wh = cases.whitening(case, packed if case["route"] in ("blocked", "diag") else None)
    c = cases.bound_constant(case)
    per_comp = cases.residual_ratio(case, wh, h, g, per_component=True)
    note = ""
    if cases.n_features(case["d"], case["diag"]) <= CHEAP_FEATURES and case["k"] <= 8:
        dev = cases.forward_deviation(h, g, cases.estimate(case, wh))
        note = f"  forward deviation H {dev[0]:.1e} g {dev[1]:.1e}"
    print(f"{case['id']} [{case['route']}]: {max(per_comp):.3f} (2^-24 B; bound {c:g}){note}")
    for i in range(case["k"]):
        w = cases.weights(cases.log_weights(case, i), case["snis"])
        if not (w > 0).any():
            assert np.isnan(h[i]).all() and np.isnan(g[i]).all(), f"{case['id']}: component {i} has no weighted sample, expected NaN"
        else:
            assert np.isfinite(h[i]).all() and np.isfinite(g[i]).all(), f"{case['id']}: component {i} is not finite"
        assert per_comp[i] <= c, f"{case['id']}: component {i}: {per_comp[i]:.3f} 2^-24 B at the worst row, bound {c:g}"
    for a, b, name in zip(got, again, ("H", "g")):
        assert np.array_equal(a, b, equal_nan=True), f"{name} {case['id']}: two calls differ"
    return max(per_comp)


def _run(ctx, case):
    h, g, packed = run_case(ctx, case)
    h2, g2, _ = run_case(ctx, case)
    _check(case, (h, g), (h2, g2), packed)
    if case["dead"].any():
        hn, gn, _ = run_case(ctx, cases.with_nonfinite(case))
        assert np.array_equal(h, hn, equal_nan=True) and np.array_equal(g, gn, equal_nan=True), \
            f"{case['id']}: NaN / inf in x, tlp, logq of samples without weight changed the result"


@pytest.mark.parametrize("spec", FIXED, ids=[s["id"] for s in FIXED])
def test_more_on_its_own_inputs(ctx, spec):
    """Every case of more_cases.case_table() whose shape does not depend on the device."""
    _run(ctx, cases.make_case(spec))


@pytest.mark.parametrize("spec", CHUNKS, ids=[s["id"] for s in CHUNKS])
def test_more_chunk_shapes(ctx, spec):
    """One more_gram launch with 1, 2 and 3 chunks of 4, 5, 7, 8, 9 and 17 tiles, the last one full or short: K and N are
    computed from the compute units of this device."""
    if ctx.num_cus <= 0:
        pytest.skip("the number of compute units of this device is not available")
    resolved = cases.resolve(spec, ctx.num_cus)
    if resolved is None:
        pytest.skip(f"{ctx.num_cus} compute units cannot give one launch the chunk shape {spec['chunk_shape']}")
    g = cases.register_geometry(resolved["d"], resolved["k"], resolved["n"], ctx.num_cus)
    assert (g["chunks"], g["tpc"], bool(g["short"])) == spec["chunk_shape"]
    _run(ctx, cases.make_case(resolved))


def test_more_routes_of_the_child_process(tmp_path):
    """GMMVI_BLOCKED_ABOVE=64: D = 51 and 63 packed in the register layout (no re-packing), and a blocked call at D = 65 whose
    workspace budget makes groups of two components out of three.  One child process (more_route_child.py) runs the cases, the
    parent compares."""
    table = cases.child_table()
    dst = tmp_path / "more_child.npz"
    env = dict(os.environ, GMMVI_BLOCKED_ABOVE="64")
    env.pop("GMMVI_MORE_WS_GB", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "more_route_child.py"), str(dst)] + [s["id"] for s in table], env=env,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    out = np.load(dst)
    for c, spec in enumerate(table):
        key = f"c{c}_"
        _check(cases.make_case(spec), (out[key + "h"], out[key + "g"]), (out[key + "h2"], out[key + "g2"]), out[key + "packed"])
