"""Host-side guard of tests/test_hip_diag_sweep.py (no GPU needed): the reference of diag_sweep_cases.py alone satisfies every
condition the GPU test relies on -- it is the oracle's diagonal mixture density and gradient, its float32 evaluation stays within
C / 8 of it in units of EPS32 B on every case, every planted fault is an order of magnitude outside the GPU test's bound, the
responsibilities are mixed, and the cases reach the branches of gmmvi_diag_mixture_eval the table names."""
import time

import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import gmm as ogmm
import diag_sweep_cases as cases

ALL = cases.case_table()
G = cases.geometry


@pytest.mark.parametrize("case_id", ["dim-K3-D5-N65-normal", "dim-K3-D36-N65-normal", "comp-K33-D33-N65-normal",
                                     "dim-K3-D545-N65-normal", "K48-D5-N65-far_weights", "K9-D33-N129-far"])
def test_reference_is_the_oracle(case_id):
    """reference() with the block's three vectors not rounded against oracle.gmm.DiagonalGMM.log_density_and_grad on normalised
    weights: the same component densities, the same log density up to log sum w, the same gradient, to 1e-9.  The rounded vectors
    the device reads are the fp32 neighbours of those."""
    case = cases.make_case(cases.spec_by_id(case_id))
    exact = cases.exact_case(case)
    for key in ("isig", "isig2", "c"):
        np.testing.assert_allclose(case[key], exact[key], rtol=cases.EPS32 / 2, atol=0)
    ref = cases.reference(exact)
    for lw, key in ((case["logw"], "lp"), (case["logw2"], "lp2")):
        lse_w = logsumexp(lw)
        m = ogmm.DiagonalGMM(np.exp(lw - lse_w), case["mu"], np.square(case["sigma"]))
        olp, og, old = m.log_density_and_grad(case["x"])
        np.testing.assert_allclose(ref["ld"], old, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(ref[key] - lse_w, olp, rtol=1e-9, atol=1e-9)
        if key == "lp":
            np.testing.assert_allclose(ref["grad"], og, rtol=1e-9, atol=1e-9 * np.abs(og).max())


def test_the_block_has_the_documented_layout():
    """[mu | 1 / sigma | 1 / sigma^2 | log-normaliser | zeros], one piece of padding, a multiple of four floats."""
    for case_id in ("dim-K3-D5-N65-normal", "dim-K3-D545-N65-normal"):
        case = cases.make_case(cases.spec_by_id(case_id))
        k, d = case["k"], case["d"]
        blk = case["block"]
        stride = cases.block_stride(d)
        assert blk.dtype == np.float32 and blk.shape == (k, stride) and stride % 4 == 0 and 3 * d + 33 <= stride < 3 * d + 37
        assert np.array_equal(blk[:, :d], case["mu"]) and np.array_equal(blk[:, d:2 * d], case["isig"])
        assert np.array_equal(blk[:, 2 * d:3 * d], case["isig2"]) and np.array_equal(blk[:, 3 * d], case["c"])
        assert not blk[:, 3 * d + 1:].any()


_seen = dict(ratio={r: {o: (0.0, "") for o in cases.OUTPUTS} for r in cases.ROUTES}, shift=(np.inf, ""), slowest=(0.0, ""),
             sequential={})


@pytest.mark.parametrize("spec", ALL, ids=[s["id"] for s in ALL])
def test_case_is_fit_for_the_gpu_test(spec):
    t0 = time.perf_counter()
    case = cases.make_case(spec)
    k, n, kind, rt = case["k"], case["n"], case["kind"], cases.route(spec)
    geo = cases.case_geometry(case)
    for name in ("mu", "sigma", "isig", "isig2", "c", "logw", "logw2", "x"):
        assert np.array_equal(case[name], cases.f32(case[name])), name
    assert not np.array_equal(case["logw"], case["logw2"])
    assert k == 1 or np.argmax(case["logw"]) != np.argmax(case["logw2"])
    ref, bound = cases.reference(case), cases.abs_bound(case)
    t_ref = time.perf_counter() - t0
    # -inf exactly where every contributing weight is -inf: nowhere in ld, lp and lp2 (never all K), in the chunk partials
    # exactly for a chunk whose components all have none
    assert all(np.isfinite(ref[o]).all() and np.isfinite(bound[o]).all() and (bound[o] > 0).all() for o in cases.OUTPUTS)
    dead_chunk = np.array([np.isneginf(case["logw"][lo:hi]).all() for lo, hi in geo["chunks"]])
    assert np.array_equal(np.isneginf(ref["parts"]), np.broadcast_to(dead_chunk[:, None], ref["parts"].shape))
    assert not np.isnan(ref["parts"]).any()
    r = cases._resp(case["logw"][:, None] + ref["ld"], ref["lp"])
    if kind == "normal" and k >= 2:
        # mixed responsibilities: at least half of the samples have a second component above 1e-3
        assert np.mean(np.sort(r, axis=0)[-2] >= 1e-3) >= 0.5
    if kind == "neginf":
        dead, whole, (other, wave) = cases.neginf_components(geo)
        assert np.array_equal(np.flatnonzero(np.isneginf(case["logw"])), dead) and k / 3 <= len(dead) < k and k - 1 not in dead
        assert np.isfinite(case["logw2"]).all() and np.all(r[dead] == 0) and np.isfinite(ref["ld"][dead]).all()
        assert (whole is None) == (geo["ky"] == 1) and (whole is None or (dead_chunk[whole] and dead_chunk.sum() == 1))
        lo, hi = geo["chunks"][other]
        assert other != whole and set(range(lo + wave, hi, geo["nw"])) <= set(dead) and geo["per_wave"][other][wave] >= 1
    if kind == "far_weights" and k > 1:
        assert case["logw"][k - 1] == 0.0 and case["logw2"][0] == 0.0 and case["logw"].min() == cases.f32(cases.LOG_FLOOR)
    if kind == "far":
        assert np.abs(ref["ld"][:, 2::3]).min() > 1e5 and np.abs(ref["ld"][:, 0::3]).max() < 1e4
    got = cases.reference_f32(case)
    for o in cases.OUTPUTS:
        ratio = cases.error_ratio(got[o], ref[o], bound[o])
        if ratio > _seen["ratio"][rt][o][0]:
            _seen["ratio"][rt][o] = (ratio, spec["id"])
        assert ratio <= cases.RATIO_F32[rt][o] <= cases.C[rt] / 8, (o, ratio)
    faults = cases.planted_faults(case)
    assert faults
    for fault in faults:
        wrong = cases.evaluate(case, fault)
        shift = max(cases.error_ratio(wrong[o], ref[o], bound[o]) for o in cases.OUTPUTS)
        if shift < _seen["shift"][0]:
            _seen["shift"] = (shift, f"{spec['id']} {fault}")
        assert shift >= cases.FAULT_FACTOR * cases.C[rt], (fault, shift)
    if rt == "hd":
        # not asserted (module docstring): the pieces added in order in float32
        wrong = cases.reference_f32(case, sequential_f32=True)
        _seen["sequential"][spec["id"]] = max(cases.error_ratio(wrong[o], ref[o], bound[o]) for o in cases.OUTPUTS)
    if t_ref > _seen["slowest"][0]:
        _seen["slowest"] = (t_ref, spec["id"])
    assert t_ref < 10.0, "the fp64 reference and bound of a case must stay within a few seconds"


def test_report_the_measured_figures():
    """Prints what the docstring of diag_sweep_cases.py records (run with -s); the assertions are in the test above."""
    for rt, per in _seen["ratio"].items():
        for o, (ratio, where) in per.items():
            print(f"{rt:4s} {o:5s} {ratio:6.2f}  {where}")
    print("smallest planted-fault shift: %.3g EPS32 B  %s" % _seen["shift"])
    for where, shift in sorted(_seen["sequential"].items(), key=lambda kv: -kv[1])[:3]:
        print(f"sequential float32 piece sums: {shift:.2f} EPS32 B  {where}")
    print("slowest reference + bound: %.2f s  %s" % _seen["slowest"])


def test_every_planted_fault_is_in_the_table():
    """Each fault of the issue's list applies to some case, and the chunk, wave and piece faults to cases of both routes."""
    by_fault = {}
    for s in ALL:
        logw = np.zeros(s["k"])                                    # (of the inputs, only which chunks carry weight matters)
        if s["kind"] == "neginf":
            logw[cases.neginf_components(G(s["k"], s["d"], s["n"]))[0]] = -np.inf
        for name, _ in cases.planted_faults(dict(s, logw=logw)):
            by_fault.setdefault(name, set()).add(cases.route(s))
    both = {"ragged_piece_left_out", "last_dimension_left_out", "mask_missing", "last_row_read_for_the_one_before",
            "last_component_left_out_of_lp", "chunk_dropped", "lp2_from_logw", "gradient_with_inverse_sigma",
            "gradient_wave_missing", "gradient_by_chunk_lp", "gradient_last_piece_not_written"}
    assert set(by_fault) == both | {"empty_wave_counts_one"}
    assert all(by_fault[name] == {"f32", "hd"} for name in both)


def test_the_table_reaches_what_it_names():
    """The geometry of the issue's table at 256 compute units, by the restated dispatch arithmetic."""
    ids = [s["id"] for s in ALL]
    assert len(set(ids)) == len(ids)
    for rt in cases.ROUTES:
        assert cases.C[rt] == 8 * max(cases.RATIO_F32[rt].values()) and all(float(v).is_integer() for v in cases.RATIO_F32[rt].values())
    assert cases.FAULT_FACTOR == 10
    shapes = {(s["k"], s["d"], s["n"], s["kind"]) for s in ALL}
    sizes = lambda g: [hi - lo for lo, hi in g["chunks"]]                                 # noqa: E731
    # dimension classes at K = 3, N = 65
    for d in cases.DIMS_F32 + cases.DIMS_HD:
        g = G(3, d, 65)
        assert (3, d, 65, "normal") in shapes and g["nw"] == 3 and g["ky"] == 1 and g["tiles"] == 2
        assert g["pieces"] == -(-d // 32) and g["ragged"] == d % 32 and g["one_piece"] == (d <= 32) and g["hd"] == (d > 512)
        assert g["pack_threads"] == (256 if d > 512 else 64) and g["stride"] == (3 * d + 33 + 3) // 4 * 4
    assert [d for d in cases.DIMS_F32 if G(3, d, 65)["one_piece"]] == [1, 2, 3, 4, 5, 31, 32]
    assert [d for d in cases.DIMS_F32 + cases.DIMS_HD if G(3, d, 65)["vec4"]] == [4, 32, 36, 64, 96, 128, 512, 516, 544, 1024]
    # vec4 whole pieces only; vec4 with a ragged last piece (read by the scalar form); the scalar path; the 64-thread pack stride
    assert [d for d in cases.DIMS_F32 + cases.DIMS_HD if G(3, d, 65)["vec4"] and G(3, d, 65)["ragged"]] == [4, 36, 516]
    assert G(3, 36, 65)["pieces"] == 2 and G(3, 516, 65)["pieces"] == 17 and G(3, 545, 65)["ragged"] == 1
    assert {63, 64, 65} <= set(cases.DIMS_F32) and {513, 516} <= set(cases.DIMS_HD)
    assert all(G(3, d, 65)["hd"] for d in cases.DIMS_HD) and not any(G(3, d, 65)["hd"] for d in cases.DIMS_F32)
    # the extremes
    g, h = G(2, 131072, 65), G(2, 131071, 3)
    assert g["hd"] and h["hd"] and g["vec4"] and not h["vec4"] and g["pieces"] == h["pieces"] == 4096 and h["ragged"] == 31
    assert g["nw"] == 2 and g["ky"] == 1
    # component classes at D = 5 and D = 33, N = 65
    for d in (5, 33):
        assert all((k, d, 65, "normal") in shapes for k in cases.COMPONENTS)
        for k in (1, 2, 7):
            assert G(k, d, 65)["nw"] == k and G(k, d, 65)["per_wave"] == [[1] * k]
        assert G(8, d, 65)["per_wave"] == [[1] * 8] and G(9, d, 65)["per_wave"] == [[2, 1, 1, 1, 1, 1, 1, 1]]
        assert [G(k, d, 65)["ky"] for k in (15, 16, 17, 31)] == [1, 1, 1, 1]
        assert G(32, d, 65)["ky"] == 2 and sizes(G(32, d, 65)) == [16, 16]
        assert sizes(G(33, d, 65)) == [17, 16] and sizes(G(47, d, 65)) == [24, 23] and sizes(G(48, d, 65)) == [16, 16, 16]
        assert sizes(G(100, d, 65)) == [17] * 5 + [15] and sizes(G(255, d, 65)) == [17] * 15
        assert G(256, d, 65)["ky"] == 16 and sizes(G(256, d, 65)) == [16] * 16
        g = G(257, d, 65)
        assert g["ky"] == 16 and sizes(g) == [17] * 15 + [2] and g["per_wave"][-1] == [1, 1, 0, 0, 0, 0, 0, 0]
        assert g["per_wave"][0] == [3, 2, 2, 2, 2, 2, 2, 2]
        assert sizes(G(300, d, 65)) == [19] * 15 + [15]
    # sample classes: tiles and the ragged last tile
    for k in (9, 33):
        assert all((k, 33, n, "normal") in shapes for n in cases.SAMPLES)
        assert [G(k, 33, n)["tiles"] for n in cases.SAMPLES] == [1, 1, 1, 1, 2, 2, 2, 3, 5]
        assert {G(k, 33, n)["ky"] for n in cases.SAMPLES} == {1 if k == 9 else 2}
    # tile count against chunk count
    assert [(G(64, 8, n)["tiles"], G(64, 8, n)["ky"]) for n in cases.TILES] == [(128, 4), (300, 2), (383, 1), (384, 1)]
    assert 2 * 383 < 3 * 256 <= 2 * 384
    # the kinds
    for kind in ("far", "far_weights", "neginf"):
        assert all((k, d, n, kind) in shapes for k, d, n in cases.KIND_SHAPES)
    assert [G(*s)["ky"] for s in cases.KIND_SHAPES] == [1, 2, 16, 3, 1, 2]
    assert [G(*s)["hd"] for s in cases.KIND_SHAPES] == [False, False, False, False, True, True]
    # what the GPU test requires of the table as a whole
    for what in ("chunked", "unequal_last_chunk", "empty_wave"):
        assert any(cases.reaches(G(s["k"], s["d"], s["n"]))[what] for s in ALL), what


def test_the_geometry_follows_the_compute_units():
    """The GPU test recomputes the geometry from the device: the chunk count depends on the compute units only through the rule
    of two workgroups per unit."""
    assert G(64, 8, 8192, num_cus=64)["ky"] == 1 and G(64, 8, 8192, num_cus=304)["ky"] == 4
    assert G(64, 8, 24576, num_cus=304)["ky"] == 2 and G(257, 5, 65, num_cus=1)["ky"] == 1 and G(257, 5, 65, num_cus=8)["ky"] == 8


@pytest.mark.parametrize("d", cases.PACK_DIMS)
def test_pack_in_float32_is_within_the_bound(d):
    """gmmvi_diag_pack restated in float32 stays within C / 8 of the fp64 values in units of EPS32 times their own scale."""
    mu, sigma = cases.pack_inputs(d)
    want, scale = cases.pack_reference(sigma)
    got = cases.pack_f32(sigma)
    rt = "hd" if d > cases.MAX_DIM_F32 else "f32"
    for key in ("isig", "isig2", "c"):
        ratio = np.max(np.abs(got[key] - want[key]) / (cases.EPS32 * scale[key]))
        print(f"pack D={d} {key}: {ratio:.2f} EPS32 scale")
        assert ratio <= cases.C[rt] / 8, (key, ratio)
