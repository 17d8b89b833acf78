"""GPU parity of the density sweep of the blocked path (gmmvi_blocked_mixture_eval, csrc/blocked.hip with the contractions of
blocked_gemm.hip) against fp64 ON ITS OWN INPUTS, at its component ranges, chunks, tile and sample seams.

test_hip_blocked.py lets the device pack the components and compares at 1e-3 of the largest gradient element, with at most five
components: the component-range split of the gradient (S > 1), its slab sum, the chunked accumulation and most combinations of
outputs never ran there.  Here the component block is built on the host (blocked_sweep_cases.py), the device and the reference
read the same fp32-representable numbers, and every element of ld, lp, lp2 and the gradient is held to

    |device - reference| <= C * EPS32 * B,

B the same sums over absolute values (blocked_sweep_cases.abs_bound) and C = 16 = 8 x the worst error of the float32 NumPy
evaluation of the same formulas, plain and through the three bf16 planes, in the same units, measured on the reference alone.
test_blocked_sweep_cases_cpu.py shows that every planted fault -- a component range left out or added twice, a chunk that
overwrites, a column tile's |z|^2 left out, a ragged row given its neighbour's values, the wrong weights, coefficient or lp --
lies ten times outside that bound on every case it applies to.

Every case runs the eight combinations of outputs of blocked_sweep_child.CALLS on the shared context; the output arrays hold a
sentinel before each call.  Outputs that are mathematically the same across the calls agree to the same bound (not bit for bit:
ld of the ld-only call comes from the launch that does not store Z)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blocked_sweep_cases as cases
from blocked_sweep_child import CALLS, SENTINEL, run_call, run_calls, upload

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = cases.case_table()
PLAIN = [s for s in TABLE if not s["zbytes"]]
CHUNKED = [s for s in TABLE if s["zbytes"]]


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def _assert_geometry(spec, num_cus):
    geo = cases.case_geometry(spec, num_cus)
    for what, holds in cases.requirements(spec):
        assert holds(geo, num_cus), f"{spec['id']}: '{what}' does not hold with {num_cus} compute units: {geo}"


def _within(got, want, bound, what):
    """|got - want| <= C EPS32 B element-wise, -inf in the same places -> the largest ratio in units of EPS32 B."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert not np.isnan(got).any(), what + ": NaN"
    ninf = np.isneginf(want)
    np.testing.assert_array_equal(np.isneginf(got), ninf, err_msg=what + ": -inf places")
    ratio = cases.error_ratio(got, want, bound)
    assert ratio <= cases.C, f"{what}: {ratio:.1f} EPS32 B at the worst element, bound {cases.C:.0f}"
    return ratio


def _check(case, outs):
    """Every output of every call against the reference, and the calls against each other."""
    ref, bound = cases.reference(case), cases.abs_bound(case)
    worst = {o: 0.0 for o in cases.OUTPUTS}
    first = {}
    for call, out in outs.items():
        want_ld, want_lp, want_grad, dual = CALLS[call]
        assert sorted(out) == sorted(o for o, w in zip(cases.OUTPUTS, (want_ld, want_lp, dual, want_grad)) if w), call
        for o, got in out.items():
            what = f"{case['id']} call {call}: {o}"
            assert got.dtype == np.float32 and not (got == SENTINEL).any(), what + ": an element was not written"
            worst[o] = max(worst[o], _within(got, ref[o], bound[o], what))
            if o in first:
                _within(got, first[o][1], bound[o], f"{what} against call {first[o][0]}")
            else:
                first[o] = (call, got)
    print(f"{case['id']}: " + "  ".join(f"{o} {worst[o]:.2f}" for o in cases.OUTPUTS) + f"  (EPS32 B; bound {cases.C:.0f})")
    return worst


def _check_wrappers(ctx, case, dev, outs):
    """hip_ops.mixture_eval / mixture_eval_dual (which allocate their outputs themselves) give what the direct calls gave: the
    sweep sums in a fixed order."""
    from gmmvi_amd import hip_ops
    ld, lp, grad = hip_ops.mixture_eval(ctx, dev["block"], dev["logw"], dev["x"], dev["d"], family=dev["family"], nu=dev["nu"],
                                        want_ld=True, want_lp=True, want_grad=True)
    for o, a in (("ld", ld), ("lp", lp), ("grad", grad)):
        np.testing.assert_array_equal(a.numpy(), outs["ld_lp_grad"][o], err_msg=f"{case['id']}: hip_ops.mixture_eval {o}")
    if case["family"] == "gauss":
        _, lp, _, lp2 = hip_ops.mixture_eval_dual(ctx, dev["block"], dev["logw"], dev["logw2"], dev["x"], dev["d"], want_ld=False,
                                                  want_grad=False)
        for o, a in (("lp", lp), ("lp2", lp2)):
            np.testing.assert_array_equal(a.numpy(), outs["dual"][o], err_msg=f"{case['id']}: hip_ops.mixture_eval_dual {o}")


@pytest.mark.parametrize("spec", PLAIN, ids=[s["id"] for s in PLAIN])
def test_sweep_on_its_own_inputs(ctx, spec, monkeypatch):
    monkeypatch.delenv("GMMVI_BLOCKED_ZBYTES", raising=False)
    _assert_geometry(spec, ctx.num_cus)
    case = cases.make_case(spec)
    dev = upload(ctx, case)
    outs = run_calls(ctx, dev)
    _check(case, outs)
    _check_wrappers(ctx, case, dev, outs)


@pytest.mark.parametrize("spec", CHUNKED, ids=[s["id"] for s in CHUNKED])
def test_sweep_in_component_chunks(ctx, spec, monkeypatch):
    """GMMVI_BLOCKED_ZBYTES (read per call) leaves room for eight components: chunks 8 + 8 + 3 with two component ranges each, the
    slab sum accumulating from the second chunk on.  Against fp64, and against the same case in one chunk: the densities bit
    for bit, the gradient (summed in another order) within the bound."""
    _assert_geometry(spec, ctx.num_cus)
    assert len(cases.case_geometry(cases.unchunked(spec), ctx.num_cus)["chunks"]) == 1
    case = cases.make_case(spec)
    dev = upload(ctx, case)
    monkeypatch.setenv("GMMVI_BLOCKED_ZBYTES", str(spec["zbytes"]))
    outs = run_calls(ctx, dev)
    monkeypatch.delenv("GMMVI_BLOCKED_ZBYTES")
    whole = {call: run_call(ctx, dev, call) for call in ("ld_lp_grad", "dual_ld_grad")}
    _check(case, outs)
    bound = cases.abs_bound(case)
    for call, out in whole.items():
        for o, a in out.items():
            what = f"{case['id']} call {call}: {o} in chunks against one chunk"
            if o == "grad":
                _within(outs[call][o], a, bound[o], what)
            else:
                np.testing.assert_array_equal(outs[call][o], a, err_msg=what)


def test_sweep_on_the_f32_route(tmp_path):
    """GMMVI_BLOCKED_F32=1 keeps the contractions of D >= 160 on the f32 matrix-core instruction, where they take two column
    tiles of 96 / 160 columns: one child process (blocked_sweep_child.py) runs the cases, the parent compares."""
    table = cases.f32_table()
    built = [cases.make_case(s) for s in table]
    src, dst = tmp_path / "f32_in.npz", tmp_path / "f32_out.npz"
    arrays = {"ncases": np.array(len(built))}
    for c, case in enumerate(built):
        _assert_geometry(case, 256)
        for key in ("block", "logw", "logw2", "x"):
            arrays[f"c{c}_{key}"] = np.asarray(case[key], np.float32)
        arrays[f"c{c}_meta"] = np.array([case["family_id"], case["nu"], case["d"]], np.float64)
    np.savez(src, **arrays)
    env = {v: s for v, s in os.environ.items() if not v.startswith("GMMVI_BLOCKED_")}
    env["GMMVI_BLOCKED_F32"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "blocked_sweep_child.py"), str(src), str(dst)], env=env, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    got = np.load(dst)
    for c, case in enumerate(built):
        outs = {call: {} for call in CALLS}
        for name in got.files:
            if name.startswith(f"c{c}_"):
                call, o = name[len(f"c{c}_"):].rsplit("_", 1)
                outs[call][o] = got[name]
        _check(case, outs)
