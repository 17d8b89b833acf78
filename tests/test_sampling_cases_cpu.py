"""Host-side guard of tests/test_hip_sampling.py (no GPU needed): the reference of sampling_cases.py alone satisfies every
condition the GPU test relies on -- it is the oracle's sample_from_components_no_shuffle, its float32 evaluation stays within
half of the bound in two orders of summation, every planted fault fails the GPU test's assertion on every case it applies to,
and the cases reach the seams their ids claim."""
import numpy as np
import pytest

from oracle import gmm as ogmm, philox
import sampling_cases as cases

ALL = cases.case_table() + cases.register64_table()
IDS = [s["id"] for s in ALL]


@pytest.fixture(scope="module")
def built():
    """make_case and reference once per case for the whole module (read-only)."""
    store = {}

    def get(spec):
        if spec["id"] not in store:
            case = cases.make_case(spec)
            for v in case.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            store[spec["id"]] = (case, cases.reference(case), cases.bound(case))
        return store[spec["id"]]
    return get


@pytest.mark.parametrize("spec", ALL, ids=IDS)
def test_reference_is_the_oracle_sampler(spec, built):
    case, (x, mapping), _ = built(spec)
    k, d = case["k"], case["d"]
    if case["route"] == "diag":
        m = ogmm.DiagonalGMM(np.ones(k) / k, case["means"], case["sigma"] ** 2)
        m.chol_cov = case["sigma"].copy()
    else:
        m = ogmm.FullCovGMM(np.ones(k) / k, case["means"], np.broadcast_to(np.eye(d), (k, d, d)))
        m.chol_cov = case["chols"].copy()
    rx, rmap = m.sample_from_components_no_shuffle(case["counts"], case["eps"])
    np.testing.assert_array_equal(mapping, rmap)
    np.testing.assert_allclose(x, rx, rtol=1e-12, atol=1e-12)
    for name in ("means", "eps", "sigma" if case["route"] == "diag" else "chols"):
        assert np.array_equal(case[name], cases.f32(case[name])), name
    if case["route"] != "diag":
        # lower triangular, the upper triangle exactly zero, the corner L[D - 1, 0] there: a transposed read is visible
        assert not np.triu(case["chols"], 1).any() and (d == 1 or np.all(case["chols"][:, d - 1, 0] != 0))
    np.testing.assert_array_equal(case["eps"], cases.f32(philox.normals(case["seed"], case["first_index"], case["n"], d,
                                                                         case["stream_id"])))


@pytest.mark.parametrize("spec", ALL, ids=IDS)
def test_float32_evaluation_and_planted_faults(spec, built):
    """The float32 NumPy evaluation in two orders stays within half of the bound (on the diagonal route: the exact result rounded
    once, half an ulp); every planted fault exceeds the bound it is tested against."""
    case, (x, _), bnd = built(spec)
    assert np.all(bnd > 0)
    for order in ("mean_first_ascending", "mean_last_descending"):
        ratio = cases.excess(cases.evaluate_f32(case, order), x, bnd)
        print(f"{spec['id']} {order}: fp32 NumPy {ratio:.3f} of the bound")
        assert ratio <= 0.5
    pb = cases.philox_bound(case)
    assert np.all(pb > bnd)
    faults = cases.planted_faults(case)
    names = {f[0] for f in faults}
    assert {"stale_eps", "next_mean", "philox_index"} <= names
    assert ("transposed" in names) == (case["route"] != "diag" and case["d"] >= 2)
    assert ("philox_ragged_block" in names) == (case["d"] % 4 != 0 and case["d"] > 4)
    for fault in faults:
        shift = cases.excess(cases.faulty(case, fault), x, bnd if fault[2] == "eps" else pb)
        assert shift > 1.0, (fault, shift)


def test_the_table_holds_what_it_names():
    """The count vectors, dimensions, Philox indices and LDS sizes of the issue, restated from the kernels' arithmetic."""
    assert len(set(IDS)) == len(IDS)
    rc, bc = np.asarray(cases.REGISTER_COUNTS), np.asarray(cases.BLOCKED_COUNTS)
    assert len(rc) == 15 and rc.sum() == 1522 and len(bc) == 8 and bc.sum() == 685
    # empty components in front, behind and next to one another
    for c in (rc, bc):
        assert c[0] == 0 and c[-1] == 0
    assert rc[5] == rc[6] == 0
    # one sample short of, on and one past the 16-row tile, the 64-sample wave, the 256-sample chunk; three chunks
    live = rc[rc > 0]
    for m in (16, 64, 256):
        assert {m - 1, m, m + 1} <= set(live.tolist())
    assert sorted(set((live % 16).tolist())) == [0, 1, 15] and set((live % 64).tolist()) >= {0, 1, 63}
    assert set((live % 256).tolist()) >= {0, 1, 255} and (live.max() + 255) // 256 == 3 and live.max() % 256 == 1
    assert sorted((bc[bc > 0] % cases.BLOCKED_BM).tolist()) == [0, 1, 1, 44, 127] and (bc.max() + 127) // 128 == 3
    # dimensions: both parities of the LDS row stride on the scalar branch; D == DP and D == previous DP + 1 on the matrix cores,
    # ragged 16-column tiles and a ragged last k-step of four
    assert all(cases.padded_dim(d) < 32 for d in cases.REGISTER_SCALAR_DIMS)
    assert {(d | 1) == d for d in cases.REGISTER_SCALAR_DIMS} == {True, False}
    assert {cases.padded_dim(d) for d in cases.REGISTER_MFMA_DIMS} == {32, 40, 50}
    assert {cases.padded_dim(d) for d in cases.REGISTER64_DIMS} == {64}
    for prev, dp in ((24, 32), (32, 40), (40, 50)):
        assert prev + 1 in cases.REGISTER_MFMA_DIMS and dp in cases.REGISTER_MFMA_DIMS
    mfma = cases.REGISTER_MFMA_DIMS + cases.REGISTER64_DIMS
    assert {d % 16 == 0 for d in mfma} == {True, False} and {d % 4 == 0 for d in mfma} == {True, False}
    assert {d % 4 for d in cases.REGISTER_MFMA_DIMS} == {0, 1, 2}
    assert cases.BLOCKED_DIMS == (51, 64, 65, 161) and 161 >= 160 and (161 * 4) % 16 != 0
    assert {(d + 3) // 4 for d in cases.DIAG_DIMS} == {1, 2, 9, 129} and {d % 4 for d in cases.DIAG_DIMS} == {0, 1, 3}
    # dynamic LDS of the register-route launches
    assert [cases.lds_bytes(d) for d in (50, 52, 53, 63)] == [62424, 65296, 65720, 80640]
    assert cases.lds_bytes(52) <= 64 * 1024 < cases.lds_bytes(53)
    # one case per route wraps the low word of the Philox sample index inside its largest component, one uses stream 2
    for route in cases.ROUTES:
        specs = [s for s in ALL if s["route"] == route]
        wraps = [s for s in specs if "wrap" in s["id"]]
        assert wraps and any(s["stream_id"] == 2 for s in specs)
        for s in wraps:
            counts = np.asarray(s["counts"])
            big = int(np.argmax(counts))
            lo = s["first_index"] + int(counts[:big].sum())
            assert lo >> 32 == cases.WRAP_HI - 1 and (lo + int(counts[big]) - 1) >> 32 == cases.WRAP_HI
            assert (lo & 0xFFFFFFFF) + int(counts[big]) > 1 << 32
    # the twins: two chunks, the second with 44 or 4 samples; one shape on the scalar branch, three on the matrix cores
    assert [(s - 256) for _, s in cases.TWIN_SHAPES] == [44, 44, 44, 4]
    assert [cases.padded_dim(d) for d, _ in cases.TWIN_SHAPES] == [24, 32, 50, 50]
    assert cases.lds_bytes(cases.TWIN64_SHAPE[0]) > 64 * 1024
