"""Host-side guard of tests/test_hip_blocked_sweep.py (no GPU needed): the reference of blocked_sweep_cases.py alone satisfies
every condition the GPU test relies on -- it is the oracle's mixture density and gradient, its float32 evaluation (plain and
through the three bf16 planes) stays within C / 8 of it in units of EPS32 B on every case, every planted fault is an order of
magnitude outside the GPU test's bound, and the cases reach the branches of gmmvi_blocked_mixture_eval their comments claim."""
import time

import numpy as np
import pytest
from scipy.linalg import solve_triangular
from scipy.special import logsumexp

from oracle import gmm as ogmm, targets as otargets
import blocked_sweep_cases as cases

ALL = cases.case_table() + cases.f32_table()
G = cases.geometry


@pytest.mark.parametrize("case_id", ["K8-D51-N129-normal-gauss", "K9-D72-N257-normal-student_t", "K9-D161-N129-neginf-gauss",
                                     "K9-D72-N257-far_weights-gauss", "K9-D72-N257-far-gauss"])
def test_reference_is_the_oracle(case_id):
    """reference() against oracle.gmm.FullCovGMM / oracle.targets.StudentTMixtureTarget, which take covariances and normalised
    weights: the same log density up to log sum w, the same gradient, to 1e-9 relative.  The oracle factorises
    Sigma = (L^-1)^-1 (L^-1)^-T itself; the component log densities follow from it with one-hot weights."""
    case = cases.make_case(cases.spec_by_id(case_id))
    k, d = case["k"], case["d"]
    sub = np.unique(np.concatenate([np.arange(min(case["n"], 24)), [case["n"] - 1]]))
    ref = cases.reference(case)
    chols = np.stack([solve_triangular(li, np.eye(d), lower=True) for li in case["linv"]])
    covs = chols @ np.transpose(chols, (0, 2, 1))
    # the block's log-normaliser is the fp32 rounding of the oracle's: the densities differ by that rounding, component-wise
    logdet = np.log(np.diagonal(chols, axis1=1, axis2=2)).sum(axis=1)
    if case["family"] == "gauss":
        c64 = -logdet - 0.5 * d * np.log(2 * np.pi)
    else:
        from scipy.special import gammaln
        c64 = gammaln(0.5 * (cases.NU + d)) - gammaln(0.5 * cases.NU) - 0.5 * d * np.log(cases.NU * np.pi) - logdet
    np.testing.assert_allclose(case["c"], c64, rtol=2 * cases.EPS32)
    for lw, key in ((case["logw"], "lp"), (case["logw2"], "lp2")):
        live = np.isfinite(lw)                                   # the oracle takes log w: a component without weight is left out
        lse_w = logsumexp(lw + case["c"] - c64)              # the oracle's weights carry the rounding of c
        w = np.exp(lw + case["c"] - c64 - lse_w)
        x = case["x"][sub]
        if case["family"] == "gauss":
            olp, og, old = ogmm.FullCovGMM(w[live], case["mu"][live], covs[live]).log_density_and_grad(x)
            scale = max(1.0, np.abs(old).max())
            np.testing.assert_allclose(ref["ld"][live][:, sub] - (case["c"] - c64)[live, None], old, rtol=1e-9, atol=1e-9 * scale)
        else:
            olp, og = otargets.StudentTMixtureTarget(w, case["mu"], covs, cases.NU).log_density_and_grad(x)
        np.testing.assert_allclose(ref[key][sub] - lse_w, olp, rtol=1e-9, atol=1e-9 * np.abs(olp).max())
        if key == "lp":
            np.testing.assert_allclose(ref["grad"][sub], og, rtol=1e-7, atol=1e-9 * np.abs(og).max())


def test_the_block_has_the_documented_layout():
    """[mu (D) | log-normaliser | pad to 4 | L^-1 dense row-major D x D], zeros above the diagonal and in the padding."""
    for case_id in ("K8-D51-N129-normal-gauss", "K9-D161-N129-normal-gauss"):
        case = cases.make_case(cases.spec_by_id(case_id))
        k, d = case["k"], case["d"]
        lo = cases.ceil4(d + 1)
        blk = case["block"]
        assert blk.dtype == np.float32 and blk.shape == (k, lo + d * d) and lo % 4 == 0 and d + 1 <= lo < d + 5
        assert np.array_equal(blk[:, :d], case["mu"]) and np.array_equal(blk[:, d], case["c"]) and not blk[:, d + 1:lo].any()
        linv = blk[:, lo:].reshape(k, d, d)
        assert np.array_equal(linv, case["linv"]) and not np.triu(linv, 1).any() and np.all(np.diagonal(linv, axis1=1, axis2=2) > 0)


def test_bf16_planes_are_the_device_split():
    """The three planes are bf16 values (16 low bits clear), each the round-to-nearest-even of the running remainder, and
    leave a residual below 2^-24 |x| (csrc/bf16_split.h states 2^-27 |x| for the bounds of the planes it lists)."""
    rng = np.random.default_rng(5)
    x = (rng.normal(size=4096) * np.exp(rng.uniform(-20, 20, size=4096))).astype(np.float32)
    x[:4] = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], np.float32)      # ties: to even
    p1, p2, p3 = cases._planes(x)
    for p in (p1, p2, p3):
        assert not (p.view(np.uint32) & 0xFFFF).any()
    assert list(p1[:4]) == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0]
    assert np.all(np.abs(x - p1) <= 2.0 ** -8 * np.abs(x)) and np.all(np.abs((x - p1) - p2) <= 2.0 ** -8 * np.abs(x - p1))
    total = p1.astype(np.float64) + p2 + p3
    assert np.all(np.abs(total - x) <= 2.0 ** -24 * np.abs(x))


_seen = dict(ratio={v: {o: (0.0, "") for o in cases.OUTPUTS} for v in ("plain", "split")}, shift=(np.inf, ""), slowest=(0.0, ""))


@pytest.mark.parametrize("spec", ALL, ids=[s["id"] for s in ALL])
def test_case_is_fit_for_the_gpu_test(spec):
    t0 = time.perf_counter()
    case = cases.make_case(spec)
    k, n = case["k"], case["n"]
    for name in ("mu", "linv", "c", "logw", "logw2", "x"):
        assert np.array_equal(case[name], cases.f32(case[name])), name
    assert not np.array_equal(case["logw"], case["logw2"])
    ref, bound = cases.reference(case), cases.abs_bound(case)
    t_ref = time.perf_counter() - t0
    assert all(np.isfinite(ref[o]).all() and np.isfinite(bound[o]).all() and (bound[o] > 0).all() for o in cases.OUTPUTS)
    r = cases._resp(case["logw"][:, None] + ref["ld"], ref["lp"])
    if spec["kind"] in ("normal", "neginf") and n >= 100:
        # mixed responsibilities: the median sample has a second component above 1e-3 and an owner above 0.3
        top = np.sort(r, axis=0)
        assert np.median(top[-1]) > 0.3 and np.median(top[-2]) > 1e-3
    if spec["kind"] == "neginf":
        assert np.isneginf(case["logw"]).sum() == 1 and np.all(r[k // 2] == 0) and np.isfinite(ref["ld"][k // 2]).all()
    if spec["kind"] == "far_weights":
        # components 0 (log weight -100) and 1 (the floor) alone near their own samples: the others more than 150 nats lower
        assert case["logw"][0] == -100.0 and case["logw"][1] == cases.f32(cases.LOG_FLOOR) and case["logw2"][2] == -100.0
        a = case["logw"][:, None] + ref["ld"]
        for i in (0, 1):
            own = case["comp"] == i
            assert own.any() and np.all(a[i, own][None, :] - np.delete(a[:, own], i, axis=0) > 150.0)
    if spec["kind"] == "far":
        assert np.abs(case["x"]).max() > 500.0
    for variant in ("plain", "split"):
        got = cases.reference_f32(case, variant == "split")
        for o in cases.OUTPUTS:
            ratio = cases.error_ratio(got[o], ref[o], bound[o])
            if ratio > _seen["ratio"][variant][o][0]:
                _seen["ratio"][variant][o] = (ratio, spec["id"])
            assert ratio <= cases.RATIO_F32[variant][o] <= cases.C / 8, (variant, o, ratio)
    faults = cases.planted_faults(case)
    assert faults or n == 1 or n % 128 == 0
    for fault in faults:
        wrong = cases.evaluate(case, fault)
        shift = max(cases.error_ratio(wrong[o], ref[o], bound[o]) for o in cases.OUTPUTS)
        if shift < _seen["shift"][0]:
            _seen["shift"] = (shift, f"{spec['id']} {fault}")
        assert shift >= cases.FAULT_FACTOR * cases.C, (fault, shift)
    if t_ref > _seen["slowest"][0]:
        _seen["slowest"] = (t_ref, spec["id"])
    assert t_ref < 10.0, "the fp64 reference and bound of a case must stay within a few seconds"


def test_report_the_measured_figures():
    """Prints what the docstring of blocked_sweep_cases.py records (run with -s); the assertions are in the test above."""
    for variant, per in _seen["ratio"].items():
        for o, (ratio, where) in per.items():
            print(f"{variant:6s} {o:5s} {ratio:6.2f}  {where}")
    print("smallest planted-fault shift: %.3g EPS32 B  %s" % _seen["shift"])
    print("slowest reference + bound: %.2f s  %s" % _seen["slowest"])


def test_the_table_reaches_what_it_names():
    """The geometry of the issue's table at 256 compute units, by the restated dispatch arithmetic."""
    ids = [s["id"] for s in ALL]
    assert len(set(ids)) == len(ids)
    assert cases.C == 8 * max(v for per in cases.RATIO_F32.values() for v in per.values())
    assert all(float(v).is_integer() for per in cases.RATIO_F32.values() for v in per.values())
    ch = lambda *a, **kw: G(*a, **kw)["chunks"]                                        # noqa: E731
    ranges = lambda kn, inner, nz, last: [inner] * (nz - 1) + [last]                    # noqa: E731
    # the smallest blocked D, N = 1: S = 2, ranges 4 + 4
    for k, d, n in ((8, 51, 129), (8, 64, 1)):
        g = G(k, d, n)
        assert not g["split"] and g["S"] == 2 and ranges(*g["chunks"][0]) == [4, 4] and g["Kc"] == k
    assert G(8, 51, 129)["LP"] == 52 and G(8, 64, 1)["row_tiles"] == 1
    g = G(9, 72, 257)
    assert g["S"] == 2 and ranges(*g["chunks"][0]) == [5, 4] and g["row_tiles"] == 3 and 257 - 2 * 128 == 1
    g = G(13, 130, 128)
    assert g["NT"] == 5 and g["S"] == 3 and ranges(*g["chunks"][0]) == [5, 5, 3] and g["row_tiles"] == 1
    g = G(25, 96, 127)                             # nz < S: a slab nobody writes
    assert g["S"] == 6 and g["chunks"][0][1:3] == (5, 5)
    assert G(64, 65, 130)["S"] == 16 and ch(64, 65, 130)[0][1:3] == (4, 16)
    g = G(9, 161, 129)
    assert g["split"] and g["NT"] == 6 and g["ctiles"] == 1 and 161 % 4 == 1 and g["S"] == 2 and ranges(*g["chunks"][0]) == [5, 4]
    g = G(17, 201, 257)
    assert g["split"] and g["NT"] == 8 and g["S"] == 4 and ranges(*g["chunks"][0]) == [5, 5, 5, 2]
    g = G(12, 324, 130)                            # 192 + 132 columns (NT = 10 would leave 4, but pads to 640 against 384)
    assert g["split"] and (g["NT"], g["ctiles"]) == (6, 2) and g["S"] == 3
    g = G(10, 512, 129)
    assert g["split"] and g["ctiles"] == 2 and g["S"] == 2
    g = G(40, 161, 1000)
    assert g["split"] and g["wtiles"] == 320 > 256 and g["S"] == 10
    # chunks with S > 1 and a shorter last chunk, both routes
    for (k, d, n, zb), split in zip(cases.CHUNKED, (False, True)):
        g = G(k, d, n, zbytes=zb)
        assert g["split"] == split and g["Kc"] == 8 and g["S"] == 2 and [c[0] for c in g["chunks"]] == [8, 8, 3]
        assert ranges(*g["chunks"][0]) == [4, 4] and ranges(*g["chunks"][2]) == [2, 1]
        assert G(k, d, n)["Kc"] == k
    # the f32 route with two column tiles
    assert [(G(9, d, 129, f32_route=True)["NT"], G(9, d, 129, f32_route=True)["ctiles"]) for d in (161, 300)] == [(3, 2), (5, 2)]
    assert not any(G(9, d, 129, f32_route=True)["split"] for d in (161, 300))
    # the sweeps: every NT instance of both routes, all four D % 4, the sample seams
    seen = {(G(3, d, 129)["split"], G(3, d, 129)["NT"]) for d in cases.SWEEP_D} | {(G(s["k"], s["d"], s["n"])["split"],
                                                                                   G(s["k"], s["d"], s["n"])["NT"]) for s in ALL
                                                                                  if not s["f32"]}
    # (the split route's NT = 4 is never the least padded width of a D x D launch: 128 m columns tie with NT = 8 for even m and
    # with NT = 6 at 384, and ties go to the wider tile; D = 257 ... 288 takes NT = 3 in three column tiles)
    reachable = {cases.tile_width(d, True)[0] for d in range(160, 513)}
    assert reachable == {3, 5, 6, 8, 10}
    assert seen == {(False, 3), (False, 4), (False, 5)} | {(True, nt) for nt in reachable}
    assert G(3, 257, 129)["ctiles"] == 3 and G(3, 321, 129)["ctiles"] == 2
    for split in (False, True):
        assert {s["d"] % 4 for s in ALL if (s["d"] >= 160) == split and not s["f32"]} == {0, 1, 2, 3}
    for d in (72, 161):
        assert {s["n"] for s in ALL if s["k"] == 9 and s["d"] == d and s["kind"] == "normal" and s["family"] == "gauss"
                and not s["f32"]} >= set(cases.SWEEP_N)
    # S > 1 on both routes, a ragged last range, every kind of input on both routes, Student-t where the issue asks for it
    assert any(G(s["k"], s["d"], s["n"])["S"] > 1 for s in ALL if s["d"] < 160)
    assert any(G(s["k"], s["d"], s["n"])["S"] > 1 for s in ALL if s["d"] >= 160 and not s["f32"])
    for kind in cases.KINDS:
        assert {s["d"] >= 160 for s in ALL if s["kind"] == kind and not s["f32"]} == {False, True}, kind
    t = [s for s in ALL if s["family"] == "student_t"]
    assert any(s["zbytes"] for s in t) and any(cases.case_geometry(s)["ctiles"] == 2 for s in t)
    assert any(cases.case_geometry(s)["S"] > 1 and cases.case_geometry(s)["split"] == sp for s in t for sp in (False, True))
    # the table does not depend on the seed of the budget knob: the unchunked twin of a chunked case has the same inputs
    spec = next(s for s in ALL if s["zbytes"])
    a, b = cases.make_case(spec), cases.make_case(cases.unchunked(spec))
    assert all(np.array_equal(a[key], b[key]) for key in ("block", "logw", "logw2", "x"))


def test_the_geometry_follows_the_compute_units():
    """The GPU test recomputes the geometry from the device: the rule for S depends on the compute units only through the
    number of resident tiles (f32 route: 8 per unit; split route: whole rounds of one workgroup per unit)."""
    assert G(9, 72, 257, num_cus=1)["S"] == 2 and G(64, 65, 130 * 40, num_cus=4)["S"] == 1
    assert G(40, 161, 1000, num_cus=8)["S"] in range(1, 11) and G(40, 161, 1000, num_cus=304)["wtiles"] == 320
