"""Host-side guard of tests/test_hip_stein.py (no GPU needed): the reference of stein_cases.py alone satisfies every condition
the GPU test relies on -- it is the oracle's estimate, its float32 evaluation stays within C / 8 of it in units of EPS32 B on
every case, every planted fault is an order of magnitude outside the GPU test's bound, and the cases reach the seams their
names claim."""
import numpy as np
import pytest

from oracle import gmm as ogmm, stein as ostein
import diag_highd_cases
import stein_cases as cases
from test_oracle_math import random_gmm

ALL = cases.case_table() + cases.register64_table()


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("snis", [True, False])
def test_reference_is_the_oracle_estimate(rng, diag, own, snis):
    """reference() fed the model's own fp64 ld, bg and gradients against get_expected_hessian_and_grad, which evaluates the
    model itself: 1e-10.  Pins the argument order, the signs, the map_offset convention and the zeros of an empty own set."""
    k, d, n = (5, 17, 300) if diag else (4, 5, 200)
    m = diag_highd_cases.random_diag_gmm(rng, k, d) if diag else random_gmm(rng, k, d)
    mapping = rng.integers(0, k - 1, size=n)
    if snis:
        mapping[mapping == 1] = 0                  # component 1 has no sample (the oracle's plain estimator refuses an empty set)
    mapping[n - 1] = k - 1
    x = m.means[mapping] + rng.normal(size=(n, d))
    _, qgrad, cld = m.log_density_and_grad(x)
    bg = rng.normal(size=n) - 12.0
    tgrad, tlp = rng.normal(size=(n, d)), rng.normal(size=n)
    case = dict(route="diag" if diag else "register", d=d, k=k, n=n, kind="own" if own else "normal", own=own, means=m.means,
                x=x, tgrad=tgrad, qgrad=qgrad, ld=cld, bg=bg, mapping=mapping + cases.MAP_BASE, map_offset=-cases.MAP_BASE)
    case["sigma" if diag else "chols"] = m.chol_cov
    rh, rg = ostein.get_expected_hessian_and_grad(m, x, mapping + cases.MAP_BASE, bg, tlp, tgrad, own, snis)
    for got in (cases.reference(case, snis), cases.estimate(case, snis)):
        for g, r in zip(got, (rh, rg)):
            live = np.isfinite(r)
            assert np.array_equal(np.isnan(g), np.isnan(r))
            np.testing.assert_allclose(g[live], r[live], rtol=1e-10, atol=1e-10 * np.abs(r[live]).max())
    if own and snis:
        assert np.all(rh[1] == 0) and np.all(rg[1] == 0)


def test_plain_reference_at_d512_is_the_oracle_estimate():
    """Above 2^24 elements of the oracle's [n, D, D] array reference() evaluates the plain-weight estimate with estimate():
    once, at D = 512, against the oracle's function itself."""
    case = cases.make_case(cases.spec_by_id("blocked-D512-K1-N255-normal"))
    assert case["n"] * case["d"] ** 2 > cases._ORACLE_PLAIN_ELEMS
    ref = cases.reference(case, False, force_oracle=True)
    assert cases.error_ratio(cases.reference(case, False), ref, cases.abs_bound(case, False)) * cases.EPS32 <= 1e-10


@pytest.mark.parametrize("spec", ALL, ids=[s["id"] for s in ALL])
def test_case_is_fit_for_the_gpu_test(spec):
    case = cases.make_case(spec)
    k, n = case["k"], case["n"]
    for name in ("means", "x", "tgrad", "qgrad", "ld", "bg", "sigma" if case["route"] == "diag" else "chols"):
        assert np.array_equal(case[name], cases.f32(case[name])), name
    a = cases.log_weights(case)
    if spec["kind"] == "wide":
        # about [-120, 60]; chunks of 64 and ranges of 256 without a seam sample lie tens of nats below the others
        assert a.min() < -115.0 and 59.9 < a.max() < 60.1
        tops = np.array([a[:, c:c + 64].max() for c in range(0, n, 64)])
        assert np.all(a[:, case["seams"]] > 56.9) and (n <= 512 or np.ptp(tops) > 10.0)
        assert n <= 768 or np.ptp([a[:, c:c + 256].max() for c in range(0, n, 256)]) > 10.0
    elif spec["kind"] == "neginf":
        dead = np.isneginf(case["ld"])
        assert 0.2 * n < dead[k // 2].sum() < 0.45 * n and dead.sum() == dead[k // 2].sum() and not dead[:, case["seams"]].any()
    elif spec["kind"] == "own":
        counts = np.bincount(case["mapping"] + case["map_offset"], minlength=k)
        assert case["map_offset"] != 0 and counts[1] == 0 and counts[k - 1] == 1 and case["mapping"][n - 1] == k - 1 + cases.MAP_BASE
    for snis in cases.modes(spec):
        ref, bound = cases.reference(case, snis), cases.abs_bound(case, snis)
        assert cases.error_ratio(cases.estimate(case, snis), ref, bound) * cases.EPS32 <= 1e-10
        ratio = cases.error_ratio(cases.reference_f32(case, snis), ref, bound)
        print(f"{spec['id']} snis={snis}: fp32 NumPy {ratio:.2f} EPS32 B")
        assert ratio <= cases.RATIO_F32[spec["route"].replace("64", "")] <= cases.C / 8
        faults = cases.planted_faults(case, snis)
        assert [f for f in faults if f[0] == "drop_sample"]
        for fault in faults:
            shift = cases.error_ratio(cases.estimate(case, snis, fault=fault), ref, bound)
            assert shift >= cases.FAULT_FACTOR * cases.C, (fault, snis, shift)


def test_the_table_holds_what_it_names():
    """The case lists of the issue, and the seams the comments of stein_cases.py place by the kernels' dispatch arithmetic."""
    ids = [s["id"] for s in ALL]
    assert len(set(ids)) == len(ids)
    assert cases.C == 8 * max(cases.RATIO_F32.values())
    # padded classes: D == DP and D == PREV + 1 of every class
    dps = cases.PADDED_DIMS[:-1]
    assert {cases.padded_dim(d) for d in cases.REGISTER_CLASS_DIMS} == set(dps)
    for prev, dp in zip((0,) + dps, dps):
        assert dp in cases.REGISTER_CLASS_DIMS and prev + 1 in cases.REGISTER_CLASS_DIMS
    assert [cases.stein_tile(dp)[2] for dp in dps] == [5, 3, 5, 4, 1, 5, 3, 3, 2, 1, 2]
    assert all(7 % nb for nb in (2, 3, 4, 5))                             # K = 7: a partly filled stack for every NB > 1
    assert [cases.stein_tile(dp)[0] for dp in (16, 20, 32, 40, 50, 64)] == [2, 2, 3, 3, 4, 4]      # both forms of the wave merge
    # sample seams
    geo = {n: cases.register_geometry(20, 3, n) for n in cases.REGISTER_SEAM_NS}
    assert [geo[n]["wave_range"] for n in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)] == \
        [4, 4, 4, 4, 16, 16, 20, 64, 64, 36, 64, 52]
    assert [geo[n]["R"] for n in (255, 256, 257, 1023, 1025)] == [1, 1, 2, 4, 5]
    # partial counts and the bump R0 = 0 -> 1
    for d in (4, 20):
        assert [cases.register_geometry(d, 1, cases.n_for_partials(r, d))["R"] for r in cases.PARTIAL_COUNTS] == list(cases.PARTIAL_COUNTS)
    assert cases.n_for_partials(17, 20, num_cus=8) is None
    for d, k, n in cases.MANY_STACKS:
        g = cases.register_geometry(d, k, n)
        assert g["stacks"] > 256 and g["R0"] == 0 and g["R"] == 1
    # blocked: the row stride, the sample ranges, both routes of the contraction
    assert [cases.blocked_geometry(d, 256)["LP"] for d in cases.BLOCKED_DIMS] == [52, 64, 68, 68, 128, 132, 132, 516]
    assert [cases.blocked_geometry(64, n)["S"] for n in cases.BLOCKED_NS + (4097,)] == [1, 1, 1, 2, 2, 16]
    assert [cases.blocked_geometry(64, n)["split"] for n in (511, 512)] == [False, True]
    assert [cases.blocked_geometry(d, 256)["split"] for d in (155, 156)] == [False, True]
    assert "blocked-D64-K1-N4097-normal" in ids and "blocked-f32-D155-K1-N256-normal" in ids
    # every route has every weight shape
    for route in ("register", "blocked", "diag"):
        for kind in cases.KINDS:
            assert sum(s["route"] == route and s["kind"] == kind for s in ALL) >= 2, (route, kind)
        assert any(s["route"] == route and s["kind"] == "wide" and s["n"] > 768 for s in ALL)
    assert {(s["d"], s["n"]) for s in ALL if s["d"] == 131072} == {(131072, 8)}
    assert {s["d"] for s in cases.register64_table()} == {51, 63}
