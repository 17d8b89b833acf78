"""GPU parity of the component updates against fp64 ON THEIR OWN INPUTS, on every route and seam: update_kl_fast_kernel and the
kernel in the reference's arithmetic (csrc/update_kl.hip, csrc/update.hip), update_plain_kernel (direct, iBLR) and the blocked
route (gmmvi_blocked_update_kl / gmmvi_blocked_update_plain, csrc/blocked_update.hip).

The device and oracle.updaters read the same fp32-representable state and rewards in every round (update_cases.py); the warm
round starts from the fp64 result of the cold one rounded to fp32, on both sides.  Asserted per round:

    success, num_updates, probe counts            exact
    last_eta                                      rtol 1e-5
    l2                                            rtol 1e-6
    E_L  = max |L'_ref^-1 L'_dev - I|             <= C_L
    E_mu = max |L'_ref^-1 (mu_dev - mu_ref)|      <= C_mu
    |KL_dev - KL_ref(eta_dev)|                    <= C_kl EPS32 B_kl
    rejected components                           old parameters bit for bit, last_eta = -1
    packed blocks                                 gmmvi_pack_components of the device's own result, rtol 2e-6 / atol 1e-6

The constants are 8 x the worst error of the float32 NumPy evaluation of the same formulas against fp64, measured on the
reference alone (update_cases.F32_WORST -> C_L, C_mu, C_kl):

    KL update, register routes      C_L 3.2e-6   C_mu 5.6e-6   C_kl 12
    KL update, illcond law          C_L 5.6e-4   C_mu 3.2e-6   C_kl 12
    KL update, blocked route        C_L 2.4e-6   C_mu 5.6e-6   C_kl 20
    KL update, reference arithmetic C_L 1.6e-5   C_mu 4.0e-5   C_kl 28   (update_kl_kernel, measured on the oracle's float32
                                    arithmetic; run on the cases whose decision margins hold under C_kl 28 -- none of the
                                    illcond law, where float32 inversion at condition 1e6 leaves C_kl 4.8e6)
    plain updates, register         C_L 4.8e-6   C_mu 4.8e-5
    plain updates, illcond law      C_L 2.8e-3   C_mu 5.6e-4
    plain updates, blocked route    C_L 8.0e-6   C_mu 8.0e-5

test_update_cases_cpu.py shows that every case keeps the decision margins under which an fp32 kernel within these bounds must
take the oracle's path, and that every planted fault of update_cases.fault() lies ten times outside them.  Every check prints the
achieved ratios (1 = the bound); the worst seen on an MI355X are 0.80 / 0.26 / 0.38 (E_L, E_mu, E_kl) on the register routes, 0.18 /
0.11 / 0.52 on the blocked route, 0.12 / 0.17 / 0.38 for the reference arithmetic, 0.16 / 0.15 and 0.12 / 0.29 for the plain updates
on the register and the blocked route, 0.01 / 0.09 for the update from the Stein slab."""
import os
import subprocess
import sys

import numpy as np
import pytest

import update_cases as cases
from update_device import run_round, run_slab

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = cases.case_table()


def _pick(pred):
    t = [s for s in TABLE if pred(s)]
    return pytest.mark.parametrize("spec", t, ids=[s["id"] for s in t])


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def _check(case, rnd, got, what="device", packed=True, group=None):
    r = case["rounds"][rnd]
    ref = r["ref"]
    tag = f"{case['id']} round {rnd} ({what})"
    ratios = cases.compare(case, rnd, got, group)
    print(f"{tag}: E_L {ratios['E_L']:.3f}  E_mu {ratios['E_mu']:.3f}  E_kl {ratios['E_kl']:.3f}  (1 = the bound)")
    decided = ~ref.get("undecided", np.zeros(case["k"], bool))
    np.testing.assert_array_equal(got["success"][decided], ref["success"][decided], err_msg=tag)
    np.testing.assert_array_equal(got["num_updates"], ref["num_updates"], err_msg=tag)
    np.testing.assert_allclose(got["l2"], cases.l2_rule(r["l2"], got["success"]), rtol=cases.RTOL_L2, atol=0, err_msg=tag)
    bad = ~got["success"]
    np.testing.assert_array_equal(got["means"][bad], r["means"][bad].astype(np.float32), err_msg=tag)
    np.testing.assert_array_equal(got["chols"][bad], r["chols"][bad].astype(np.float32), err_msg=tag)
    assert np.all(np.isfinite(got["means"][~bad])) and np.all(np.isfinite(got["chols"][~bad])), tag
    if case["mode"] == "kl":
        resolved = ref["probes"] <= cases.MAX_EXACT_PROBES
        np.testing.assert_array_equal(got["probes"][resolved], ref["probes"][resolved], err_msg=tag)
        assert np.all(got["probes"][~resolved] > cases.MAX_EXACT_PROBES), tag
        np.testing.assert_allclose(got["last_eta"], ref["last_eta"], rtol=cases.RTOL_ETA, atol=0, err_msg=tag)
        np.testing.assert_array_equal(got["last_eta"][bad], -1.0, err_msg=tag)
    assert ratios["E_L"] <= 1.0 and ratios["E_mu"] <= 1.0 and ratios["E_kl"] <= 1.0, f"{tag}: {ratios}"
    if packed and "packed" in got:
        np.testing.assert_allclose(got["packed"], got["packed_ref"], rtol=2e-6, atol=1e-6, err_msg=tag)
    return ratios


def _run(ctx, case, reference=False):
    for rnd in range(len(case["rounds"])):
        _check(case, rnd, run_round(ctx, case, rnd))
        if reference and cases.reference_kernel_holds(case):
            _check(case, rnd, run_round(ctx, case, rnd, reference=True), "reference arithmetic", group=cases.reference_group(case))
        elif reference:
            # its decision margins do not hold under its own C_kl (the illcond law): the kernel may take another path than the
            # oracle.  It is run all the same and held to what does not depend on the path
            got, r = run_round(ctx, case, rnd, reference=True), case["rounds"][rnd]
            ratios = cases.compare(case, rnd, got, cases.reference_group(case))
            print(f"{case['id']} round {rnd} (reference arithmetic, margins do not hold: decisions {got['success'].astype(int)} "
                  f"against {r['ref']['success'].astype(int)}, probes {got['probes']} against {r['ref']['probes']}): {ratios}")
            bad = ~got["success"]
            np.testing.assert_array_equal(got["means"][bad], r["means"][bad].astype(np.float32))
            np.testing.assert_array_equal(got["chols"][bad], r["chols"][bad].astype(np.float32))
            np.testing.assert_array_equal(got["last_eta"][bad], -1.0)
            assert np.all(np.isfinite(got["means"])) and np.all(np.isfinite(got["chols"])) and np.all(got["last_eta"][~bad] >= 1.0)
            np.testing.assert_array_equal(got["num_updates"], r["ref"]["num_updates"])
            np.testing.assert_allclose(got["l2"], cases.l2_rule(r["l2"], got["success"]), rtol=cases.RTOL_L2, atol=0)


@_pick(lambda s: s["route"] == "register" and s["mode"] == "kl" and s["law"] in ("benign", "illcond", "nonsym"))
def test_update_kl_on_every_instance(ctx, spec):
    """Static instances <4,1> <10,1> <20,1> <32,4> <40,4> <50,4>, the generic one on one wave (D <= 24) and on four (the 24 | 25
    switch, D = 33, 49), D = 1 and 2 without a reflector: cold and warm round, both kernels held to fp64, packed blocks."""
    _run(ctx, cases.make_case(spec), reference=True)


@_pick(lambda s: s["route"] == "register" and s["law"] in ("diag", "blockdiag2", "arrow", "zero", "zerog", "scale", "smallstep"))
def test_update_kl_structure_and_scale(ctx, spec):
    """Columns that are already tridiagonal (the early exit of every reflector step), H = 0 and g = 0, rewards scaled by
    2^-80 ... 2^30 (the device must accept wherever fp64 does), the smallest and the largest stepsize."""
    case = cases.make_case(spec)
    _run(ctx, case, reference=True)
    if spec["law"] == "zero":
        # eta = exp(5) from the cold bracket; the parameters come back within 4 EPS32 of the old ones
        got, r = run_round(ctx, case, 0), case["rounds"][0]
        np.testing.assert_allclose(got["last_eta"], np.exp(5.0), rtol=cases.RTOL_ETA)
        np.testing.assert_allclose(got["means"], r["means"], rtol=4 * cases.EPS32, atol=0)
        np.testing.assert_allclose(got["chols"], r["chols"], rtol=4 * cases.EPS32, atol=0)


@_pick(lambda s: s["law"] == "search")
def test_update_kl_search_paths(ctx, spec):
    """Searches that end at the last node of a six-level round and at the first node of the next (6, 7, 12, 13 probes), an
    immediate accept at the root, the warm bracket's max(0, ln eta - 3) clamp, a bracket without a feasible eta, and eta raised
    to the temperature: probe counts, accepted eta, success and the KL at the accepted (raised) eta, on both kernels."""
    case = cases.make_case(spec)
    _run(ctx, case, reference=True)


@_pick(lambda s: s["law"] == "fail")
def test_update_kl_failures_and_bookkeeping(ctx, spec):
    """NaN in H, NaN in g only, +inf in H and H = -1e6 I between succeeding neighbours: the neighbours' outputs equal those of a
    run in which the bad components are benign, bit for bit; old parameters kept exactly, last_eta = -1, the l2 cap
    min(1e-6, 10 l2) and floor max(l2 / 2, l2_init), num_updates.  (Inputs the kernels are documented to accept.)"""
    case = cases.make_case(spec)
    bad = [i for i, _ in cases.FAIL_BAD["fail" + spec["tag"]]]
    h, g = case["H_neg"].copy(), case["g_neg"].copy()
    for i in bad:
        h[i], g[i] = case["H_neg"][0], case["g_neg"][0]
    good = [i for i in range(case["k"]) if i not in bad]
    for rnd in range(2):
        got = run_round(ctx, case, rnd)
        _check(case, rnd, got)
        clean = run_round(ctx, case, rnd, h_neg=h, g_neg=g)
        for name in ("means", "chols", "kls", "last_eta", "l2", "num_updates", "success", "probes"):
            np.testing.assert_array_equal(got[name][good], clean[name][good], err_msg=f"{case['id']} round {rnd}: {name}")
        np.testing.assert_array_equal(got["packed"][good], clean["packed"][good], err_msg=f"{case['id']} round {rnd}: packed")
        r = case["rounds"][rnd]
        np.testing.assert_allclose(got["l2"], cases.l2_rule(r["l2"], r["ref"]["success"]), rtol=cases.RTOL_L2, atol=0)


@_pick(lambda s: s["route"] == "blocked" and s["mode"] == "kl")
def test_blocked_update_kl_at_its_instance_seams(ctx, spec):
    """blk_tridiag_instance changes at D = 64 | 65, 128 | 129, 192 | 193, 256 | 257, 304 | 305; above 320 the global
    tridiagonalisation and one thread per row; D = 51 and 512 are the ends of the route.  Two cases with rewards scaled by 2^-66
    (column tails in the fp32 subnormal range) run the register-resident and the global-memory tridiagonalisation."""
    _run(ctx, cases.make_case(spec))


@_pick(lambda s: s["route"] == "blocked" and s["mode"] != "kl")
def test_blocked_update_plain_at_its_instance_seams(ctx, spec):
    _run(ctx, cases.make_case(spec))


@_pick(lambda s: s["route"] == "register" and s["mode"] != "kl")
def test_update_plain_on_the_register_route(ctx, spec):
    """direct and iBLR, two rounds (iBLR keeps the mean on a component's first update and moves it afterwards), one failing
    component under the onefail law."""
    _run(ctx, cases.make_case(spec))


SLAB = cases.slab_table()


@pytest.mark.parametrize("spec", SLAB, ids=[s["id"] for s in SLAB])
def test_update_from_stein_slab(ctx, spec):
    """The component-update step of the single-call iteration (gmmvi_stein_update_kl = gmmvi_stein_partials +
    gmmvi_update_components_kl_from_slab) against the fp64 Stein estimate fed to the fp64 updater: the direct route (M whitened
    from the moment sums; ukl_block_product and L^-1 from the packed fragments at D = 32 / 40 / 50) under self-normalised
    weights, the in-kernel finalize prologue (D <= 24) and the finalize launch (D = 32 / 40 / 50) under plain weights, and D = 33,
    which is not fused; from one partial per component and from three.  The bound is the update bound plus the Stein bound
    propagated through the step (update_cases: spread_L, spread_mu)."""
    import stein_cases
    n = cases.slab_n(spec, ctx.num_cus)
    if n is None:
        pytest.skip(f"{ctx.num_cus} compute units cannot give every component {spec['r']} partials")
    case = cases.make_slab_case(spec, n)
    r = case["rounds"][0]
    ref = r["ref"]
    got = run_slab(ctx, case)
    d, snis = spec["d"], spec["snis"]
    assert got["R"] == spec["r"] == stein_cases.register_geometry(d, spec["k"], n, ctx.num_cus)["R"]
    branch = cases.slab_branch(d, snis, got["R"])
    assert branch == ("direct" if snis and d != 33 else "prologue" if d <= 24 else "finalize"), branch
    ratios = cases.compare_slab(case, got)
    print(f"{spec['id']} (N = {n}, {branch}): E_L {ratios['E_L']:.3f}  E_mu {ratios['E_mu']:.3f}  (1 = the bound)")
    if branch == "direct":
        # the estimate is never written on this route: the scratch keeps the NaN it was filled with
        assert np.isnan(got["h_scratch"]).all() and np.isnan(got["g_scratch"]).all()
    else:
        sc = case["stein"]
        for dev, want, b in zip((got["h_scratch"], got["g_scratch"]), stein_cases.reference(sc, snis), stein_cases.abs_bound(sc, snis)):
            assert np.all(np.abs(dev - want) <= stein_cases.C * stein_cases.EPS32 * b), spec["id"]
    np.testing.assert_array_equal(got["success"], ref["success"])
    np.testing.assert_array_equal(got["num_updates"], ref["num_updates"])
    np.testing.assert_allclose(got["l2"], ref["l2"], rtol=cases.RTOL_L2, atol=0)
    np.testing.assert_allclose(got["last_eta"], ref["last_eta"], rtol=cases.RTOL_ETA, atol=0)
    bad = ~ref["success"]
    np.testing.assert_array_equal(got["means"][bad], r["means"][bad].astype(np.float32))
    np.testing.assert_array_equal(got["chols"][bad], r["chols"][bad].astype(np.float32))
    assert ratios["E_L"] <= 1.0 and ratios["E_mu"] <= 1.0, ratios
    np.testing.assert_allclose(got["packed"], got["packed_ref"], rtol=2e-6, atol=1e-6)


def test_update_routes_for_d_51_to_64(tmp_path):
    """GMMVI_BLOCKED_ABOVE=64 sends D = 51 ... 64 to the register kernels: the generic four-wave instance of the KL update, whose
    dynamic LDS passes 64 KB between D = 54 and 55, and update_plain_kernel, which passes it between 56 and 57.  One child
    process (update_route_child.py) runs the cases, the parent compares; a child that dies is not started again."""
    table = cases.route64_table()
    dst = tmp_path / "update64.npz"
    env = dict(os.environ, GMMVI_BLOCKED_ABOVE="64")
    r = subprocess.run([sys.executable, os.path.join(HERE, "update_route_child.py"), str(dst)] + [s["id"] for s in table], env=env,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    out = np.load(dst)
    for c, spec in enumerate(table):
        case = cases.make_case(spec)
        for rnd in range(len(case["rounds"])):
            key = f"c{c}_r{rnd}_"
            _check(case, rnd, {n[len(key):]: out[n] for n in out.files if n.startswith(key)})
