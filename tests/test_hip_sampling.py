"""GPU parity of component-ordered sampling x = mu_k + L_k eps against fp64 at its tile, wave and chunk seams, on all four routes:
the register route (csrc/sample_block.h) in its three forms -- the stand-alone launch (csrc/sampling.hip), extra blocks of that
launch in the single-call iteration, a rider of the 1024-thread expected-log-ratio launch (csrc/riders.h) --, the blocked
contraction for D > 50 (gmmvi_blocked_sample) and the diagonal kernel (gmmvi_diag_sample).

The inputs, the reference and the bounds are those of sampling_cases.py; none of them is tuned on the device, and
test_sampling_cases_cpu.py shows that every planted fault -- a term dropped, L transposed, a stale eps row at a tile / wave /
chunk seam, the neighbour's mean, the Philox index off by one, the ragged Philox block taken from block 0 -- fails the
assertions below on every case.  Per case, with eps supplied: |x - reference| <= bound element-wise, the mapping exact, three
sentinel rows behind X and the mapping intact, the eps buffer unchanged, the same call with mapping_out = NULL bit-equal.  From the
device's Philox stream: bit-equal to the same call fed gmmvi_philox_normals of the same seed, first index and stream (both
inline philox_normal4 and then run the same arithmetic), within bound of the fp64 reference on those device normals, and within
philox_bound of the reference on the oracle's normals.

Largest |x - reference| / bound observed on the MI355X (the assertion is <= 1):
    route                                          eps supplied            device stream / philox_bound
    register, scalar branch (D = 1 ... 24)         0.184  (D = 3)          0.271  (D = 1)
    register, matrix cores  (D = 25 ... 50)        0.046  (D = 25)         0.325  (D = 33)
    register, DP = 64       (D = 51 ... 63)        0.026  (D = 52, 53)     0.165  (D = 52)
    blocked                 (D = 51 ... 161)       0.027  (D = 65)         0.133  (D = 64)
    diagonal                (D = 1 ... 513)        0.500  (every D)        0.713  (D = 513)
    first draw of the twins (D = 24 ... 53)        --                      0.552  (D = 41)
(the float32 NumPy evaluation of test_sampling_cases_cpu.py reaches 0.233 at D = 2 and 0.03 ... 0.1 from D = 23 on; 0.5 on the
diagonal route is the half ulp of a correctly rounded fmaf.)  The device stream is bit-equal to the fed call on every case.

What the first run of these tests found:
  * the launches above 64 KB of dynamic LDS (65,720 B at D = 53, 80,640 B at D = 63, under GMMVI_BLOCKED_ABOVE=64; none of the
    three launchers raises the limit) are accepted by the runtime and compute within the bounds above -- nothing to fix
    (DESIGN.md);
  * the device's normals missed the tolerance of test_philox_bits_and_normals for about 6 in 10^5 draws, all with a radius below
    0.015: u = (k + 0.5) 2^-24 was rounded to fp32 before its logarithm, up to 1.9e-5 absolute at r = 0.002 (r = 0 for the last
    k), and the D = 51 case reached 1.012 of philox_bound.  csrc/philox.h philox_log_u01 takes the logarithm of the unrounded
    value.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import philox
import sampling_cases as cases
from sampling_route_child import PAD, SENTINEL, SENTINEL_MAP, MODEL_ARRAYS, TWIN_ITERS, run_case, run_twins

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = cases.case_table()


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def check_case(case, out):
    n, tag = case["n"], case["id"]
    ref, mapping = cases.reference(case)
    bnd, pbnd = cases.bound(case), cases.philox_bound(case)
    # ---- eps supplied
    r_eps = cases.excess(out["x_eps"][:n], ref, bnd)
    print(f"{tag}: eps supplied {r_eps:.3f} of the bound")
    assert r_eps <= 1.0, f"{tag}: eps supplied, {r_eps:.3f} of the bound at the worst element"
    np.testing.assert_array_equal(out["map_eps"][:n], mapping, err_msg=tag)
    assert np.all(out["x_eps"][n:] == np.float32(SENTINEL)) and np.all(out["map_eps"][n:] == SENTINEL_MAP), f"{tag}: rows behind N"
    np.testing.assert_array_equal(out["eps_after"], case["eps"].astype(np.float32), err_msg=f"{tag}: the eps buffer")
    np.testing.assert_array_equal(out["x_nomap"], out["x_eps"], err_msg=f"{tag}: mapping_out = NULL")
    # ---- the device's Philox stream
    np.testing.assert_array_equal(out["map_dev"][:n], mapping, err_msg=tag)
    assert np.all(out["x_dev"][n:] == np.float32(SENTINEL)) and np.all(out["map_dev"][n:] == SENTINEL_MAP), f"{tag}: rows behind N"
    np.testing.assert_allclose(out["normals"], philox.normals(case["seed"], case["first_index"], n, case["d"], case["stream_id"]),
                               rtol=cases.PHILOX_RTOL, atol=cases.PHILOX_ATOL, err_msg=f"{tag}: gmmvi_philox_normals")
    np.testing.assert_array_equal(out["x_dev"], out["x_fed"], err_msg=f"{tag}: device stream against the call fed philox_normals")
    dev_eps = out["normals"].astype(np.float64)
    r_fed = cases.excess(out["x_fed"][:n], cases.reference(case, dev_eps)[0], cases.bound(case, dev_eps))
    r_dev = cases.excess(out["x_dev"][:n], ref, pbnd)
    print(f"{tag}: fed the device normals {r_fed:.3f} of the bound, device stream {r_dev:.3f} of the Philox bound")
    assert r_fed <= 1.0, f"{tag}: fed the device normals, {r_fed:.3f} of the bound"
    assert r_dev <= 1.0, f"{tag}: device stream, {r_dev:.3f} of the Philox bound"
    return r_eps, r_dev


def check_twins(out, d, per_component, k=cases.TWIN_K):
    tag = f"twins D={d} S={per_component}"
    assert bool(out["eligible"]), f"{tag}: not on the single-call path"
    assert bool(out["presampled"]), f"{tag}: the early twin drew nothing early"
    for name in MODEL_ARRAYS + ("samples", "mapping"):
        np.testing.assert_array_equal(out[f"early_{name}"], out[f"plain_{name}"], err_msg=f"{tag}: {name}")
    n = k * per_component
    assert out["early_samples"].shape == (TWIN_ITERS * n, d)
    case, x, comp = cases.twin_reference(out["means0"], out["chols0"], int(out["seed"]), int(out["first0"]), per_component)
    r = cases.excess(out["early_samples"][:n], x, cases.philox_bound(case))
    print(f"{tag}: first draw {r:.3f} of the Philox bound")
    assert r <= 1.0, f"{tag}: first draw, {r:.3f} of the Philox bound"
    # the database's mapping holds component + the number of snapshots appended before (mapping_base)
    np.testing.assert_array_equal(out["early_mapping"], np.concatenate([comp + it * k for it in range(TWIN_ITERS)]), err_msg=tag)


@pytest.mark.parametrize("spec", TABLE, ids=[s["id"] for s in TABLE])
def test_sampling_at_its_seams(ctx, spec):
    """Every case of sampling_cases.case_table(): register route (scalar and matrix-core branch), blocked and diagonal route."""
    case = cases.make_case(spec)
    check_case(case, run_case(ctx, case))


@pytest.mark.parametrize("d,per_component", cases.TWIN_SHAPES)
def test_rider_and_in_launch_draws_of_the_single_call_iteration(d, per_component):
    """sample_block at 1024 threads inside the expected-log-ratio launch (the early twin's draws from the second iteration on)
    against the 256-thread sampling launch (the plain twin): models and databases bit-equal after three iterations; the first
    iteration's draw -- uniform_count and mapping_base of gmmvi_sample_components_prep -- against the fp64 reference built from
    the initial components."""
    check_twins(run_twins(d, per_component), d, per_component)


@pytest.mark.parametrize("stream", [0, 1])
def test_philox_streams_across_the_32_bit_index_boundary(ctx, stream):
    """philox_normals at D = 1, 3, 4, 5, 8 (ragged and full blocks of four) and philox_uniforms over sample indices
    2^32 - 2^14 ... 2^32 + 2^14 - 1: the high counter word changes inside the range.  Uniforms bit for bit, normals to the
    tolerance of test_hip_kernels.test_philox_bits_and_normals.  2^15 samples: some 700,000 normals per stream, of which about
    one in 10^4 has a radius below 0.015 -- there u = (k + 0.5) 2^-24 close to 1 must not be rounded to fp32 before its
    logarithm is taken (csrc/philox.h philox_log_u01; with the rounding about 40 of these normals miss the tolerance)."""
    from gmmvi_amd import hip_ops
    n, first, seed = 1 << 15, (1 << 32) - (1 << 14), cases.SEED
    u = hip_ops.philox_uniforms(ctx, seed, first, n, stream_id=stream).numpy()
    np.testing.assert_array_equal(u, philox.uniform01(seed, first, n, stream, dtype=np.float32))
    for d in (1, 3, 4, 5, 8):
        e = hip_ops.philox_normals(ctx, seed, first, n, d, stream_id=stream).numpy()
        np.testing.assert_allclose(e, philox.normals(seed, first, n, d, stream), rtol=cases.PHILOX_RTOL, atol=cases.PHILOX_ATOL,
                                   err_msg=f"D = {d}")


def test_register_route_for_d_51_to_63(tmp_path):
    """GMMVI_BLOCKED_ABOVE=64 sends D = 51, 52, 53, 63 to the DP = 64 instance of the register route, whose launches ask for
    62,832 / 65,296 / 65,720 / 80,640 B of dynamic LDS: one child process (sampling_route_child.py) runs the cases of the
    stand-alone launch and the twins at D = 53, the parent compares.  A launch the runtime refuses is a failure here."""
    table = cases.register64_table()
    dst = tmp_path / "sampling64.npz"
    env = dict(os.environ, GMMVI_BLOCKED_ABOVE="64")
    r = subprocess.run([sys.executable, os.path.join(HERE, "sampling_route_child.py"), str(dst)], env=env, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    out = np.load(dst)
    errors = {key: str(out[key]) for key in out.files if key.endswith("error")}
    for key, message in errors.items():
        d = "twins" if key.startswith("twin") else f"D = {table[int(key[1:].split('_')[0])]['d']}"
        print(f"{d}: {message}")
    assert not errors, errors
    for i, spec in enumerate(table):
        check_case(cases.make_case(spec), {key[len(f"c{i}_"):]: out[key] for key in out.files if key.startswith(f"c{i}_")})
    check_twins({key[5:]: out[key] for key in out.files if key.startswith("twin_")}, *cases.TWIN64_SHAPE)
