"""GPU parity of the density sweep of diagonal-covariance mixtures (gmmvi_diag_mixture_eval, csrc/diag_sweep.hip, with the chunk
merge of csrc/combine.h) against fp64 ON ITS OWN INPUTS, at its wave, chunk, piece, tile and sample seams, and of gmmvi_diag_pack
in front of it.

test_diag_sweep_kernels and test_highd_sweep_kernels let the device pack the components and compare eleven random shapes at
1e-3: the waves that stride over the components, the component chunks and their merge, the ragged last piece and its selects, the
vec4 loads and the three scratch layouts are never placed there.  Here the component block is built on the host
(diag_sweep_cases.py), the device and the reference read the same fp32-representable numbers, and every element of ld, lp, lp2
and the gradient is held to

    |device - reference| <= C[route] * EPS32 * B,

B the same sums over absolute values (diag_sweep_cases.abs_bound) and C = 8 x the worst error of the float32 NumPy evaluation
of the same formulas in the same units, per route (D <= 512: 16; above: 8), measured on the reference alone.
test_diag_sweep_cases_cpu.py shows that every planted fault -- a piece, a dimension or the selects left out, a component, a wave's
share or a chunk missing, an empty wave that counts, the wrong weights, scale or lp in the gradient, a row read for its
neighbour -- lies ten times outside that bound on every case it applies to.

Measured on the MI355X (256 compute units), the worst error over all cases and calls as a fraction of the bound:
    D <= 512:  ld 0.105 (K48-D5-N65-far)   lp 0.035   lp2 0.043   grad 0.017
    D >  512:  ld 0.084 (K3-D545-N65-far)  lp 0.053   lp2 0.050   grad 0.040 (D = 131072)
gmmvi_diag_pack: 0.044 (1 / sigma^2) up to D = 512, 0.093 above."""
import numpy as np
import pytest

import diag_sweep_cases as cases

pytestmark = pytest.mark.gpu

TABLE = cases.case_table()
SENTINEL = np.float32(-1.2345e30)            # what every output array holds before a call through the C entry
PAD = 64                                     # floats behind every output there: they keep the sentinel
# name -> (ld, lp, grad, dual): the combinations of outputs gmmvi_diag_mixture_eval carves its scratch by (gradient without ld:
# ld in the workspace; without lp: lp too; chunks: the partials behind them)
CALLS = {"ld": (True, False, False, False), "lp": (False, True, False, False), "grad": (False, False, True, False),
         "lp_grad": (False, True, True, False), "dual": (False, True, False, True), "all": (True, True, True, True)}
# one case per class of the table
VARIANT_CASES = ("dim-K3-D36-N65-normal", "dim-K3-D545-N65-normal", "comp-K257-D5-N65-normal", "comp-K33-D33-N65-normal",
                 "samp-K33-D33-N129-normal", "tile-K64-D8-N8192-normal", "K48-D5-N65-neginf")


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def upload(ctx, case):
    from gmmvi_amd import hip_ops
    assert case["block"].dtype == np.float32 and case["block"].shape[1] == hip_ops.diag_packed_stride(case["d"])
    return dict(block=ctx.asarray(case["block"]), logw=ctx.asarray(case["logw"]), logw2=ctx.asarray(case["logw2"]),
                x=ctx.asarray(case["x"]), k=case["k"], d=case["d"], n=case["n"])


def run_call(ctx, dev, call, x_ptr=None):
    """One call straight through the C entry, every output over-allocated by PAD floats and filled with SENTINEL before ->
    {output: NumPy array}; the PAD floats behind each output must keep the sentinel."""
    want_ld, want_lp, want_grad, dual = CALLS[call]
    k, d, n = dev["k"], dev["d"], dev["n"]
    shapes = dict(ld=(k, n), lp=(n,), grad=(n, d), lp2=(n,))
    bufs = {o: ctx.full((int(np.prod(shapes[o])) + PAD,), SENTINEL)
            for o, w in zip(cases.OUTPUTS, (want_ld, want_lp, dual, want_grad)) if w}
    ptr = lambda o: bufs[o].ptr if o in bufs else None                                   # noqa: E731
    ctx.check(ctx.lib.gmmvi_diag_mixture_eval(ctx.handle, k, d, dev["block"].ptr, dev["logw"].ptr, dev["logw2"].ptr if dual else None,
                                              dev["x"].ptr if x_ptr is None else x_ptr, n, ptr("ld"), ptr("lp"), ptr("grad"),
                                              ptr("lp2")))
    out = {}
    for o, buf in bufs.items():
        flat = buf.numpy()
        assert np.all(flat[-PAD:] == SENTINEL), f"call {call}: written behind {o}"
        out[o] = flat[:-PAD].reshape(shapes[o])
        assert not (out[o] == SENTINEL).any(), f"call {call}: an element of {o} was not written"
    return out


def _within(got, want, bound, c, what):
    """|got - want| <= c EPS32 B element-wise, -inf in the same places, no NaN -> the largest ratio in units of EPS32 B."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert not np.isnan(got).any(), what + ": NaN"
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want), err_msg=what + ": -inf places")
    ratio = cases.error_ratio(got, want, bound)
    assert ratio <= c, f"{what}: {ratio:.2f} EPS32 B at the worst element, bound {c:.0f}"
    return ratio


def _check(case, out, what=""):
    """-> {output: worst error as a fraction of its bound}, printed before it is asserted."""
    ref, bound, c = cases.reference(case), cases.abs_bound(case), cases.C[cases.route(case)]
    assert np.isfinite(ref["lp"]).all()          # the gradient is compared on every sample: the table has none without weight
    ratios = {o: cases.error_ratio(out[o], ref[o], bound[o]) for o in out}
    print(f"{case['id']}{what}: " + "  ".join(f"{o} {r / c:.3f}" for o, r in ratios.items()) + f"  (of the bound {c:.0f} EPS32 B)")
    for o in out:
        assert out[o].dtype == np.float32
        _within(out[o], ref[o], bound[o], c, f"{case['id']}{what}: {o}")
    return {o: r / c for o, r in ratios.items()}


def test_the_table_reaches_the_seams_on_this_device(ctx):
    """The chunk count follows the compute units: on the device the suite runs on some case must still run in several chunks,
    with an unequal last chunk, and with a wave that has no component."""
    hit = {}
    for spec in TABLE:
        for what, holds in cases.reaches(cases.case_geometry(spec, ctx.num_cus)).items():
            if holds:
                hit.setdefault(what, []).append(spec["id"])
    print(f"{ctx.num_cus} compute units: " + ", ".join(f"{what}: {len(ids)} cases" for what, ids in hit.items()))
    assert set(hit) == {"chunked", "unequal_last_chunk", "empty_wave"}, hit.keys()


@pytest.mark.parametrize("spec", TABLE, ids=[s["id"] for s in TABLE])
def test_sweep_on_its_own_inputs(ctx, spec):
    from gmmvi_amd import hip_ops
    geo = cases.case_geometry(spec, ctx.num_cus)
    print(f"{spec['id']}: " + ", ".join(f"{key} {geo[key]}" for key in ("nw", "tiles", "ky", "kchunk", "pieces", "ragged", "vec4",
                                                                          "one_piece", "hd"))
          + f", components per (chunk, wave) {geo['per_wave'] if geo['ky'] <= 3 else [geo['per_wave'][0], '...', geo['per_wave'][-1]]}")
    case = cases.make_case(spec)
    dev = upload(ctx, case)
    ld, lp, grad, lp2 = hip_ops.diag_mixture_eval(ctx, dev["block"], dev["logw"], dev["x"], dev["d"], want_ld=True, want_lp=True,
                                                  want_grad=True, logw2=dev["logw2"])
    _check(case, dict(ld=ld.numpy(), lp=lp.numpy(), lp2=lp2.numpy(), grad=grad.numpy()))


@pytest.mark.parametrize("case_id", VARIANT_CASES)
def test_output_variants_are_bit_equal(ctx, case_id):
    """The six combinations of outputs (three scratch layouts, each with and without the chunk partials) give the same bits,
    within the bound, and write nothing behind their outputs."""
    case = cases.make_case(cases.spec_by_id(case_id))
    dev = upload(ctx, case)
    outs = {call: run_call(ctx, dev, call) for call in CALLS}
    for call, out in outs.items():
        want_ld, want_lp, want_grad, dual = CALLS[call]
        assert sorted(out) == sorted(o for o, w in zip(cases.OUTPUTS, (want_ld, want_lp, dual, want_grad)) if w), call
        _check(case, out, f" call {call}")
        for o, got in out.items():
            np.testing.assert_array_equal(got, outs["all"][o], err_msg=f"{case_id}: {o} of call {call} against all outputs")


def test_gradient_only_on_a_fresh_context(ctx):
    """A fresh context has no workspace: the gradient-only call (ld, lp and the chunk partials all in scratch) grows it inside the
    call, twice (the second case needs more than the slack of the first).  The same bits as on the shared context."""
    from gmmvi_amd.device import Context
    fresh = Context()
    for case_id in ("samp-K9-D33-N129-normal", "comp-K257-D33-N65-normal"):
        case = cases.make_case(cases.spec_by_id(case_id))
        got = run_call(fresh, upload(fresh, case), "grad")
        _check(case, got, " fresh context")
        np.testing.assert_array_equal(got["grad"], run_call(ctx, upload(ctx, case), "grad")["grad"])


@pytest.mark.parametrize("k,d,n", [(9, 33, 65), (33, 33, 65), (257, 5, 129)])
def test_all_weights_without_mass(ctx, k, d, n):
    """Every log weight -inf, lp only, in one chunk and in several (the merge sees -inf in every chunk): -inf, not NaN."""
    from gmmvi_amd import hip_ops
    case = cases.make_case(dict(k=k, d=d, n=n, kind="normal", id=f"K{k}-D{d}-N{n}-no-mass"))
    dev = upload(ctx, case)
    _, lp, _ = hip_ops.diag_mixture_eval(ctx, dev["block"], ctx.full((k,), -np.inf), dev["x"], d)
    assert np.all(np.isneginf(lp.numpy()))


@pytest.mark.parametrize("k", [9, 33])
@pytest.mark.parametrize("n", [1, 65, 129])
def test_nothing_outside_the_outputs_is_written(ctx, k, n):
    """ld, lp, lp2 and the gradient over-allocated by 64 floats of sentinel each: the lanes past N clamp to row N - 1 and write
    nothing, in one chunk (K = 9) and in two (K = 33)."""
    assert cases.geometry(k, 33, n, ctx.num_cus)["ky"] == (1 if k == 9 else 2)
    case = cases.make_case(dict(k=k, d=33, n=n, kind="normal", id=f"tails-K{k}-D33-N{n}"))
    dev = upload(ctx, case)
    for call in ("all", "grad"):
        _check(case, run_call(ctx, dev, call), f" call {call}")                          # (run_call asserts the tails)


@pytest.mark.parametrize("d", [32, 64])
def test_x_off_the_16_byte_alignment(ctx, d):
    """X once at a 16-byte-aligned address and once 4 bytes further on, where the kernels take the scalar loads by their own
    check: both within the bound, ld bit for bit the same."""
    from gmmvi_amd.device import DeviceArray
    case = cases.make_case(cases.spec_by_id(f"dim-K3-D{d}-N65-normal"))
    dev = upload(ctx, case)
    n = case["n"]
    buf = ctx.zeros((n * d + 4,))
    outs = []
    for shift in (0, 1):
        view = DeviceArray._view(buf, buf.ptr + 4 * shift, (n, d))
        view.set(case["x"])
        assert buf.ptr % 16 == 0 and (view.ptr % 16 == 0) == (shift == 0)
        outs.append(run_call(ctx, dev, "all", x_ptr=view.ptr))
        _check(case, outs[-1], f" X at +{4 * shift} bytes")
    np.testing.assert_array_equal(outs[0]["ld"], outs[1]["ld"])


@pytest.mark.parametrize("d", cases.PACK_DIMS)
def test_pack_against_fp64(ctx, d):
    """gmmvi_diag_pack: mu bit-exact; 1 / sigma, 1 / sigma^2 and the log-normaliser within C[route] EPS32 of their own
    absolute-value scale; zeros up to the stride; a guard row behind the last block untouched."""
    from gmmvi_amd import hip_ops
    k = 3
    mu, sigma = cases.pack_inputs(d, k)
    want, scale = cases.pack_reference(sigma)
    stride = hip_ops.diag_packed_stride(d)
    assert stride == cases.block_stride(d)
    packed = ctx.full((k + 1, stride), SENTINEL)
    means_dev, sigma_dev = ctx.asarray(mu), ctx.asarray(sigma)
    ctx.check(ctx.lib.gmmvi_diag_pack(ctx.handle, k, d, means_dev.ptr, sigma_dev.ptr, packed.ptr))
    got = packed.numpy()
    assert np.all(got[k] == SENTINEL), "the guard row was written"
    np.testing.assert_array_equal(got[:k, :d], mu.astype(np.float32))
    assert not got[:k, 3 * d + 1:].any(), "the padding is not zero"
    c = cases.C["hd" if d > cases.MAX_DIM_F32 else "f32"]
    parts = dict(isig=got[:k, d:2 * d], isig2=got[:k, 2 * d:3 * d], c=got[:k, 3 * d])
    ratios = {key: float(np.max(np.abs(parts[key].astype(np.float64) - want[key]) / (cases.EPS32 * scale[key]))) for key in parts}
    print(f"pack D={d}: " + "  ".join(f"{key} {r / c:.3f}" for key, r in ratios.items()) + f"  (of the bound {c:.0f} EPS32 scale)")
    for key, r in ratios.items():
        assert r <= c, f"pack D={d} {key}: {r:.2f} EPS32 scale, bound {c:.0f}"
