"""Host-side guard of tests/test_hip_more.py (no GPU needed): the reference quantities of more_cases.py alone satisfy every
condition the GPU test relies on -- estimate() is the oracle's MORE estimate, the float32 model of the kernels' formulation and
the fp32-rounded reference stay within C / 8 of a zero normal-equation residual in units of EPS B on every case, every planted
fault lies an order of magnitude outside the GPU test's bound on every case designated for it, and the cases reach the seams
their names claim."""
import numpy as np
import pytest

from oracle import more as omore
import more_cases as cases
import more_diag_ref
from test_oracle_math import random_gmm

ALL = cases.case_table() + cases.child_table()


def _fault_case(spec):
    """The cases the planted faults are run on: every weight, ridge, reward and factor shape, the register route (the chunk
    shapes at D = 4), and on the other routes the dimensions at and beside a seam of the feature count -- what a host solves in
    a second or two."""
    route, d, n = spec["route"], spec["d"], spec["n"]
    if n < 15:
        # the bias is no output: the measure takes it from the bias row, and with one sample that row leaves no residual for
        # any (H, g) but lambda theta -- the N = 1 cases hold the device to the law, to NaN-freedom and to reproducibility
        return False
    if "-shape-" in spec["id"] or "groups2" in spec["id"]:
        return True
    if route == "register":
        return "chunk_shape" not in spec or d == 4
    if route == "tiled":
        return d in (22, 30, 31, 43, 44) or (d == 63 and n == 257)
    if route == "blocked":
        return d <= 65
    return d <= 129 or (d == 1024 and n == 65)


@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("snis", [True, False])
def test_estimate_is_the_oracle_estimate(rng, own, snis):
    """estimate() fed the model's own fp64 ld and log q against oracle.more.get_expected_hessian_and_grad, which evaluates the
    model itself: 1e-8.  Pins the argument order, the signs, the feature order, the un-whitening and the map_offset convention."""
    k, d, n = 3, 4, 90
    m = random_gmm(rng, k, d)
    mapping = rng.integers(0, k, size=n)
    x = m.means[mapping] + rng.normal(size=(n, d))
    logq, cld = m.log_densities_also_individual(x)
    bg = rng.normal(size=n) - 12.0
    tlp = rng.normal(size=n) * 3.0
    l2 = np.full(k, 1e-6)
    case = dict(route="register", d=d, k=k, n=n, kind="own" if own else "normal", own=own, snis=snis, diag=False,
                means=m.means, chols=m.chol_cov, x=x, ld=cld, bg=bg, tlp=tlp, logq=logq, mapping=mapping + cases.MAP_BASE,
                map_offset=-cases.MAP_BASE, l2=l2)
    rh, rg = omore.get_expected_hessian_and_grad(m, l2, x, mapping + cases.MAP_BASE, bg, tlp, own, snis)
    h, g = cases.estimate(case, cases.whitening(case))
    np.testing.assert_allclose(h, rh, rtol=1e-8, atol=1e-8 * np.abs(rh).max())
    np.testing.assert_allclose(g, rg, rtol=1e-8, atol=1e-8 * np.abs(rg).max())


def test_diagonal_estimate_is_the_diagonal_reference(rng):
    """The diagonal route of estimate() against tests/more_diag_ref.py on one of its own cases."""
    case = cases.make_case(cases.spec_by_id("diag-D65-K2-N200-normal"))
    wh = cases.whitening(case)
    h, g = cases.estimate(case, wh)
    for i in range(case["k"]):
        iw = more_diag_ref.importance_weights(case["ld"][i] - case["bg"], True)
        mu, sigma = case["means"][i], 1.0 / wh["winv"][i]
        quad, lin, _ = more_diag_ref.fit_diag_quadratic(case["l2"][i], case["x"], case["tlp"] - case["logq"], iw, mu, sigma)
        np.testing.assert_allclose(h[i], quad, rtol=1e-7, atol=1e-7 * np.abs(quad).max())
        np.testing.assert_allclose(g[i], quad * mu - lin, rtol=1e-7, atol=1e-7 * np.abs(lin).max())


@pytest.mark.parametrize("spec", ALL, ids=[s["id"] for s in ALL])
def test_case_is_fit_for_the_gpu_test(spec):
    spec = cases.resolve(spec)
    assert spec is not None
    case = cases.make_case(spec)
    k, n, kind = case["k"], case["n"], case["kind"]
    for name in ("means", "ld", "bg", "l2", "sigma" if case["diag"] else "chols"):
        assert np.array_equal(case[name], cases.f32(case[name])), name
    for name in ("x", "tlp", "logq"):
        assert np.isfinite(case[name]).all() and np.array_equal(case[name], cases.f32(case[name])), name
    a = np.stack([cases.log_weights(case, i) for i in range(k)])
    w = np.stack([cases.weights(ai, case["snis"]) for ai in a])
    r = np.abs(case["tlp"] - case["logq"])
    # the seam samples: at least the mean weight of the weighted samples, a reward of ordinary size
    if not case["own"]:
        assert np.all(w[:, case["seams"]] >= w.sum(axis=1, keepdims=True) / np.maximum((w > 0).sum(axis=1, keepdims=True), 1))
    assert np.all(r[case["seams"]] >= (4.0 if kind != "offset" else 9.0e3))
    if kind in ("wide", "wideplain"):
        top, bottom = (60.0, -120.0) if kind == "wide" else (40.0, -60.0)
        assert abs(a.min() - bottom) < 1e-4 and abs(a.max() - top) < 1e-4
    elif kind == "neginf":
        gone = np.isneginf(case["ld"])
        assert 0.2 * n < gone[k // 2].sum() < 0.45 * n and gone.sum() == gone[k // 2].sum() and not gone[:, case["seams"]].any()
    elif kind in ("nonfinite", "nonfiniteown"):
        bad = cases.with_nonfinite(case)
        dead = case["dead"]
        assert 0.2 * n < dead.sum() < 0.45 * n and np.all(w[:, dead] == 0) and not dead[case["seams"]].any()
        for name in ("x", "tlp", "logq"):
            assert not np.isfinite(bad[name][dead]).any() and np.array_equal(bad[name][~dead], case[name][~dead])
            assert np.isnan(bad[name][dead]).any() and np.isposinf(bad[name][dead]).any() and np.isneginf(bad[name][dead]).any()
    elif kind == "lam12":
        assert n < cases.n_features(case["d"], case["diag"]) and case["l2"][0] == cases.f32(1e-12)
    elif kind == "cond":
        f = case["sigma"] if case["diag"] else case["chols"]
        conds = [s.max() / s.min() if case["diag"] else np.linalg.cond(s) for s in f]
        assert case["d"] == 1 or all(500.0 < c < 2000.0 for c in conds), conds
    if case["own"]:
        counts = np.bincount(np.clip(case["mapping"] + case["map_offset"], 0, k), minlength=k + 1)
        assert case["map_offset"] != 0 and counts[1] == 0 and counts[k - 1] == 1 and case["mapping"][n - 1] == k - 1 + cases.MAP_BASE

    wh = cases.whitening(case)
    c = cases.bound_constant(spec)
    ref = cases.estimate(case, wh)
    empty = [i for i in range(k) if not (w[i] > 0).any()]
    assert all(np.isnan(ref[0][i]).all() and np.isnan(ref[1][i]).all() for i in empty) and (bool(empty) == case["own"])
    ratio = cases.residual_ratio(case, wh, *cases.model_f32(case, wh))
    rounded = cases.residual_ratio(case, wh, ref[0].astype(np.float32), ref[1].astype(np.float32))
    print(f"{spec['id']}: float32 model {ratio:.3f}, fp32-rounded reference {rounded:.3f} EPS B (C / 8 = {c / 8:.3f})")
    assert ratio <= cases.RATIO_F32[cases.law_class(spec)] == c / 8
    assert rounded <= c / 8
    if not _fault_case(spec):
        return
    faults = cases.planted_faults(case)
    assert [f for f in faults if f[0] == "drop_sample"]
    for fault in faults:
        h, g = cases.estimate(case, wh, fault=fault)
        shift = cases.residual_ratio(case, wh, h.astype(np.float32), g.astype(np.float32))
        assert shift >= cases.FAULT_FACTOR * c, (fault, shift)


def test_every_fault_has_its_cases():
    """A fault that no case can show would be a gap in the table: each is planted on several routes."""
    seen = {}
    for spec in ALL:
        spec = cases.resolve(spec)
        if _fault_case(spec):
            for name, _ in cases.planted_faults(cases.make_case(spec)):
                seen.setdefault(name, set()).add(spec["route"])
    dense = {"register", "tiled", "blocked"}
    everywhere = dense | {"diag"}
    for name in ("drop_sample", "drop_tile", "weights_not_normalised", "ridge_on_bias", "neighbour_mean", "diagonal_factor", "g_sign",
                 "map_offset", "ld_in_reward"):
        assert seen[name] == everywhere, name
    assert seen["l_for_lt"] == dense and seen["feature_order"] == dense and seen["drop_chunk"] == {"register"}
    # the two faults that show through the ridge alone are planted on the lambda = 0.5 cases only
    for spec in ALL:
        names = {f[0] for f in cases.planted_faults(cases.make_case(cases.resolve(spec)))}
        assert bool(names & {"weights_not_normalised", "ridge_on_bias"}) == (spec["kind"] == "lam05")


def test_the_table_holds_what_it_names():
    """The case lists of the issue, and the seams the comments of more_cases.py place by the routes' dispatch arithmetic."""
    ids = [s["id"] for s in ALL]
    assert len(set(ids)) == len(ids)
    assert all(cases.C[cls] == 8 * cases.RATIO_F32[cls] for cls in cases.RATIO_F32) and set(cases.ROUTES) <= set(cases.C)
    reg = cases.register_geometry
    # register route: every (DP, PP) instance, at D = DP and D = PREV + 1 where the class has more than one dimension
    assert {reg(d, 1, 64)["DP"] for d in cases.REGISTER_DIMS} == set(cases.REGISTER_PP)
    assert cases.REGISTER_DIMS == (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21)
    for d in range(1, cases.REGISTER_MAX_DIM + 1):
        g = reg(d, 1, 64)
        assert g["pairs"] <= 8 * g["PP"]
    assert reg(20, 1, 64)["pairs"] == 120 == 8 * 15 and reg(21, 1, 64)["pairs"] == 136 == 8 * 17      # the full tile-pair budget
    assert {(s["k"], s["n"]) for s in ALL if s["route"] == "register" and s["d"] == 13 and s["kind"] == "normal"} == \
        {(k, n) for k in (1, 3) for n in (1, 63, 64, 65)}
    # the chunk shapes with 256 compute units: 1, 2, 3 chunks; 4, 7, 8, 9, 17 tiles per chunk; a short last chunk
    shapes = [cases.shape_for_chunks(*cs, d=4) for cs in cases.CHUNK_SHAPES]
    assert all(s is not None for s in shapes)
    geo = [reg(4, k, n) for k, n in shapes]
    assert {g["chunks"] for g in geo} == {1, 2, 3} and {g["tpc"] for g in geo} >= {4, 7, 8, 9, 17}
    assert any(g["short"] for g in geo) and [(g["chunks"], g["tpc"], bool(g["short"])) for g in geo] == list(cases.CHUNK_SHAPES)
    assert cases.shape_for_chunks(1, 17, False, d=4, num_cus=256)[0] == 256          # one chunk of 17 tiles needs K = CUs
    assert cases.pick_chunks(1, 256, 3) == 1 and cases.pick_chunks(1, 256, 8) == 2 and cases.pick_chunks(256, 256, 17) == 1
    # a shape that no K and N of the search gives returns None (the GPU test skips it)
    assert cases.shape_for_chunks(2, 50, False, d=4) is None
    # tiled route: every padded class, and F + 1 across a multiple of 128 at 30 -> 31 and 43 -> 44
    tg = cases.tiled_geometry
    assert {tg(d, 64)["DP"] for d in cases.TILED_DIMS + cases.REPACKED_DIMS} == set(cases.TILED_CLASSES)
    assert [tg(d, 64)["nblk"] for d in (30, 31, 43, 44)] == [4, 5, 8, 9]
    assert tg(30, 64)["F"] + 1 <= 512 < tg(31, 64)["F"] + 1 and tg(43, 64)["F"] + 1 <= 1024 < tg(44, 64)["F"] + 1
    assert [tg(22, n)["tiles"] for n in cases.TILED_NS] == [1, 1, 3, 4, 5, 9] and [n % 64 for n in cases.TILED_NS] == [1, 63, 0, 0, 1, 63]
    assert [tg(22, n)["passes"] for n in cases.TILED_NS] == [1, 1, 1, 1, 2, 3]
    assert {s["d"] for s in cases.child_table() if s["route"] == "tiled"} == {51, 63}
    # blocked route: the shapes of the issue, the panel count, and the ragged last group of the child's case
    assert {(d, k, n) for d, k, n in cases.BLOCKED_SHAPES} == \
        {(d, 2 if d <= 67 else 1, n) for d in (64, 65, 67, 96, 127) for n in (64, 65, 257)} | {(128, 1, 130)}
    pg = cases.panel_geometry
    assert [pg("blocked", d, 1, 64)["panels"] for d in (64, 128)] == [17, 66] and pg("blocked", 128, 1, 64)["LDG"] == 8448
    grp = next(s for s in cases.child_table() if "groups2" in s["id"])
    g = pg("blocked", grp["d"], grp["k"], grp["n"], grp["ws_gb"])
    assert (g["KG"], g["groups"], g["last"]) == (2, 2, 1) and pg("blocked", grp["d"], grp["k"], grp["n"])["KG"] == 3
    # diagonal route: F + 1 at and just past one and two panels, the 64-dimension pieces of md_stage_kernel, the cap
    assert cases.DIAG_DIMS == (1, 2, 63, 64, 65, 127, 128, 129, 300, 1023, 1024) and cases.DIAG_NS == (1, 64, 65, 200)
    assert [pg("diag", d, 1, 64)["nblk"] for d in (63, 64, 127, 128)] == [1, 2, 2, 3]
    assert [pg("diag", d, 1, 64)["panels"] for d in (63, 64, 127, 128, 1024)] == [1, 2, 2, 3, 17]
    # every route has every shape of weights, ridge, rewards and factor
    for route in cases.ROUTES:
        assert {s["kind"] for s in ALL if s["route"] == route} == set(cases.KINDS), route
