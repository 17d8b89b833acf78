"""GPU parity of gmmvi_more_blocked (csrc/more_blocked.hip: the MORE estimate for 64 <= D <= 128 from the blocked component
blocks) against the fp64 oracle, through the C ABI (gmmvi_amd.hip_ops).

Bounds.  The project's bound for the tiled MORE sizes (test_hip_kernels.py, F <= 1 654) is 1e-2 of the per-component
magnitude + 1e-5 for H and g; it is asserted here unchanged for every case up to F = 8 385.  Every test prints the measured
deviation before it asserts; the figures measured on an MI355X are in DESIGN.md section 4 and next to each bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import philox, gmm as ogmm, targets as otargets, more as omore
from helpers import samtron_config, make_oracle, make_device

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def ops():
    from gmmvi_amd import hip_ops
    return hip_ops


def random_gmm(rng, k, d, spread=3.0, scale=1.0):
    means = rng.normal(size=(k, d)) * spread
    covs = []
    for _ in range(k):
        a = rng.normal(size=(d, d))
        covs.append(scale * (a @ a.T / d + 0.3 * np.eye(d)))
    w = rng.random(k) + 0.1
    return ogmm.FullCovGMM(w / w.sum(), means, np.stack(covs))


def upload_model(ctx, m):
    return ctx.asarray(m.log_weights), ctx.asarray(m.means), ctx.asarray(m.chol_cov)


def _stein_inputs(rng, k, d, n):
    """The input pattern of test_hip_kernels.py: samples of the model's own components, a GMM target, background densities
    of the mixture that drew the samples."""
    m = random_gmm(rng, k, d)
    n_k = rng.multinomial(n, np.ones(k) / k)
    x, mapping = m.sample_from_components_no_shuffle(n_k, philox.normals(5, 0, n, d))
    x = x.astype(np.float32).astype(np.float64)
    tgt = otargets.make_gmm_target(d, rng, 3)
    tlp, _ = tgt.log_density_and_grad(x)
    cnt = np.maximum(n_k, 1e-9)
    bg = logsumexp(m.component_log_densities(x) + np.log(cnt / cnt.sum())[:, None], axis=0)
    return m, x, mapping, tlp, bg


def _device_inputs(ctx, m, x, d):
    logw, means, chols = upload_model(ctx, m)
    packed, _ = ops().pack_components(ctx, means, chols)
    assert packed.shape[1] == ((d + 1 + 3) // 4) * 4 + d * d            # the blocked block [mu | log-normaliser | pad | L^-1]
    xd = ctx.asarray(x)
    ld, lp, _ = ops().mixture_eval(ctx, packed, logw, xd, d, want_ld=True, want_lp=True)
    return packed, chols, xd, ld, lp


def _deviation(h, g, rh, rg):
    """Largest |device - oracle| per component, relative to the component's largest |oracle| entry."""
    scale_h = np.abs(rh).max(axis=(1, 2))
    scale_g = np.abs(rg).max(axis=1)
    return (np.abs(h - rh).max(axis=(1, 2)) / scale_h).max(), (np.abs(g - rg).max(axis=1) / scale_g).max()


def _assert_bound(h, g, rh, rg, bound, what):
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(g)), what
    dev_h, dev_g = _deviation(h, g, rh, rg)
    print(f"\n[more_blocked] {what}: deviation H {dev_h:.3e}  g {dev_g:.3e}  (bound {bound:.1e})")
    scale_h = np.abs(rh).max(axis=(1, 2), keepdims=True)
    scale_g = np.abs(rg).max(axis=1, keepdims=True)
    assert np.all(np.abs(h - rh) <= bound * scale_h + 1e-5), (what, dev_h)
    assert np.all(np.abs(g - rg) <= bound * scale_g + 1e-5), (what, dev_g)


# (k, d, n): N about 3 F, F = d (d + 1) / 2 + d + 1 = 2 145, 2 556, 5 151, 8 385.  The fp64 oracle alone takes 2 s, 1 s, 8 s
# and 23 s for these on 8 CPU threads and returns finite values.
PARITY_SHAPES = [(2, 64, 6500), (1, 70, 7700), (1, 100, 15500), (1, 128, 25200)]


@pytest.mark.parametrize("k,d,n", PARITY_SHAPES)
@pytest.mark.parametrize("snis", [True, False])
def test_more_blocked_matches_the_oracle(ctx, rng, k, d, n, snis):
    """First blocked dimension (64), a dimension that is no multiple of 16 (70: the shape gmmvi_more refuses), gmm100's
    dimension and the largest one (128), both weightings, ridge 1e-6, well-posed regime (N about 3 F).
    Bound: 1e-2 of the per-component magnitude (+ 1e-5), the project's bound for the tiled MORE sizes, unchanged.
    Measured on an MI355X (H / g): d = 64 1.7e-6 / 9.5e-7, d = 70 8.5e-7 / 2.3e-7, d = 100 7.9e-7 / 5.1e-7,
    d = 128 9.1e-7 / 9.3e-7 (the larger of the two weightings)."""
    m, x, mapping, tlp, bg = _stein_inputs(rng, k, d, n)
    packed, chols, xd, ld, lp = _device_inputs(ctx, m, x, d)
    l2 = np.full(k, 1e-6)
    h, g = ops().more_blocked(ctx, packed, chols, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(l2), d,
                              self_normalized=snis)
    rh, rg = omore.get_expected_hessian_and_grad(m, l2, x, mapping, bg, tlp, False, snis)
    _assert_bound(h.numpy(), g.numpy(), rh, rg, 1e-2, f"k={k} d={d} n={n} snis={snis}")


def test_more_blocked_own_samples_and_shifted_mapping(ctx, rng):
    """only_use_own_samples with data-base style mapping values (shifted by 5, map_offset brings the newest to K - 1):
    every component regresses on its own about 3 F samples with plain weights.  Measured: H 1.1e-6, g 4.1e-7."""
    k, d, n = 2, 64, 13000
    m, x, mapping, tlp, bg = _stein_inputs(rng, k, d, n)
    packed, chols, xd, ld, lp = _device_inputs(ctx, m, x, d)
    mp = mapping + 5
    l2 = np.full(k, 1e-6)
    h, g = ops().more_blocked(ctx, packed, chols, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(l2), d,
                              mapping=ctx.asarray(mp, np.int32), map_offset=k - 1 - int(mp.max()), own_samples_only=True)
    rh, rg = omore.get_expected_hessian_and_grad(m, l2, x, mp, bg, tlp, True, True)
    _assert_bound(h.numpy(), g.numpy(), rh, rg, 1e-2, f"own samples k={k} d={d} n={n}")


def test_more_blocked_quadratic_reward_is_exact(ctx, rng):
    """A reward that IS quadratic is recovered whatever the weights (the form of test_more_quadratic_reward_is_exact, same
    3e-2 bound), at d = 72.  Measured: H 2.7e-6, g 1.5e-7."""
    k, d, n = 2, 72, 8200
    m, x, mapping, _, bg = _stein_inputs(rng, k, d, n)
    packed, chols, xd, ld, lp = _device_inputs(ctx, m, x, d)
    b = rng.normal(size=(d, d)); q = b @ b.T / d + np.eye(d)
    lin = rng.normal(size=d)
    x32 = xd.numpy().astype(np.float64)
    rew = -0.5 * np.einsum("ni,ij,nj->n", x32, q, x32) + x32 @ lin + 0.3
    tlp = rew + lp.numpy().astype(np.float64)              # reward = tlp - logq
    l2 = np.full(k, 1e-10)
    h, g = ops().more_blocked(ctx, packed, chols, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(l2), d)
    for i in range(k):
        want_g = q @ m.means[i] - lin
        print(f"\n[more_blocked] quadratic reward, component {i}: H {np.abs(h.numpy()[i] - q).max() / np.abs(q).max():.3e}"
              f"  g {np.abs(g.numpy()[i] - want_g).max() / np.abs(want_g).max():.3e}  (bound 3.0e-02)")
        np.testing.assert_allclose(h.numpy()[i], q, rtol=0, atol=3e-2 * np.abs(q).max())
        np.testing.assert_allclose(g.numpy()[i], want_g, rtol=0, atol=3e-2 * np.abs(want_g).max())


def test_more_blocked_result_does_not_depend_on_the_group_size():
    """GMMVI_MORE_WS_GB small enough to force one component per group gives bit-identical H, g (a child process per
    setting: tests/more_blocked_group_child.py writes the two arrays of the same seeded call)."""
    import tempfile
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, gb in (("default", None), ("one_per_group", "0.01")):
            env = dict(os.environ)
            env.pop("GMMVI_MORE_WS_GB", None)
            if gb is not None:
                env["GMMVI_MORE_WS_GB"] = gb
            path = os.path.join(tmp, name + ".npz")
            r = subprocess.run([sys.executable, os.path.join(HERE, "more_blocked_group_child.py"), path], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            outs.append(dict(np.load(path)))
    assert np.all(np.isfinite(outs[0]["h"])) and np.all(np.isfinite(outs[0]["g"]))
    np.testing.assert_array_equal(outs[0]["h"], outs[1]["h"])
    np.testing.assert_array_equal(outs[0]["g"], outs[1]["g"])


def test_more_estimator_takes_the_blocked_route(ctx, rng):
    """MoreNgEstimator on a FullCovGMM of d = 72 returns what hip_ops.more_blocked returns."""
    from gmmvi_amd.models.full_cov_gmm import FullCovGMM
    from gmmvi_amd.models.gmm_wrapper import GmmWrapper
    from gmmvi_amd.optimization.gmmvi_modules.ng_estimator import MoreNgEstimator
    k, d, n = 2, 72, 8200
    m, x, mapping, tlp, bg = _stein_inputs(rng, k, d, n)
    model = FullCovGMM(m.weights, m.means.astype(np.float32), m.covs.astype(np.float32))
    w = GmmWrapper(model, 0.1, 1e-6, 4)
    est = MoreNgEstimator(1.0, w, False, 1e-6, True)
    xd, bgd, tlpd = ctx.asarray(x), ctx.asarray(bg), ctx.asarray(tlp)
    h, g = est.get_expected_hessian_and_grad(xd, mapping, bgd, tlpd)
    lp, ld = w.log_densities_also_individual(xd)
    h2, g2 = ops().more_blocked(ctx, w.packed, w.chol_cov, xd, ld, lp, bgd, tlpd, w.l2_regularizers, d)
    assert np.all(np.isfinite(h.numpy()))
    np.testing.assert_array_equal(h.numpy(), h2.numpy())
    np.testing.assert_array_equal(g.numpy(), g2.numpy())


def test_more_training_on_a_blocked_dimension_follows_the_oracle():
    """Three train_iter of a GMMVI built from a config with ng_estimator_type "MORE" on a GMM target of d = 72, k = 2
    (4 100 samples per component: N about 3 F, F = 2 701) keep every parameter finite and follow the fp64 oracle's
    trajectory.  Bounds: those of test_hip_train_iter.py::test_more_estimator_trajectory (tol_scale 5: 2.5e-3 in iterations
    0 and 1, 1e-2 (1 + it) afterwards), unchanged.  Measured: means 3.8e-7, 7.8e-7, 1.2e-6; factors 6.1e-7, 9.7e-7, 1.3e-6."""
    kind, d, k, s = "gmm", 72, 2, 4100
    cfg = samtron_config(s, estimator="MORE", initial_stepsize=0.05)
    o = make_oracle(kind, d, k, s, 13, cfg)
    g = make_device(kind, d, k, s, 13, cfg, o)
    for it in range(3):
        o.train_iter()
        g.train_iter()
        om, gm = o.model, g.model
        tol = 5.0 * (5e-4 if it < 2 else 2e-3 * (1 + it))
        vals = {"means": gm.means.numpy(), "chols": gm.chol_cov.numpy(), "logw": gm.log_weights.numpy(),
                "stepsizes": gm.stepsizes.numpy()}
        for key, v in vals.items():
            assert np.all(np.isfinite(v)), f"iteration {it}: {key} is not finite"
        dev = {
            "means": np.abs(vals["means"] - om.means).max() / max(1.0, np.abs(om.means).max()),
            "chols": np.abs(vals["chols"] - om.chol_cov).max() / np.abs(om.chol_cov).max(),
            "logw": np.abs(np.exp(vals["logw"]) - om.weights).max(),
            "stepsizes": np.abs(vals["stepsizes"] - om.stepsizes).max(),
        }
        print(f"\n[more_blocked] training d={d} iteration {it}: " + "  ".join(f"{a} {b:.3e}" for a, b in dev.items())
              + f"  (bound {tol:.1e})")
        for key, v in dev.items():
            assert v <= tol, f"iteration {it}: {key} deviates by {v:.3e} (> {tol:.1e})"


def test_more_blocked_argument_errors(ctx, rng):
    """d = 63, d = 129 and a null X_dev return GMMVI_ERR_ARG (-2) with a message that names the range, before any launch;
    the context then still serves a valid call."""
    k, d, n = 1, 64, 6500
    m, x, mapping, tlp, bg = _stein_inputs(rng, k, d, n)
    packed, chols, xd, ld, lp = _device_inputs(ctx, m, x, d)
    bgd, tlpd, l2d = ctx.asarray(bg), ctx.asarray(tlp), ctx.asarray(np.full(k, 1e-6))
    hh, gg = ctx.empty((k, d, d)), ctx.empty((k, d))

    def call(dim, xptr):
        return ctx.lib.gmmvi_more_blocked(ctx.handle, k, dim, packed.ptr, chols.ptr, xptr, n, ld.ptr, lp.ptr, bgd.ptr,
                                          tlpd.ptr, None, 0, 1, l2d.ptr, hh.ptr, gg.ptr)

    for dim, xptr in ((63, xd.ptr), (129, xd.ptr), (d, None)):
        assert call(dim, xptr) == -2                                     # GMMVI_ERR_ARG (include/gmmvi_hip.h)
        msg = ctx.lib.gmmvi_last_error(ctx.handle).decode()
        assert "64 <= D <= 128" in msg, msg
    for bad in (63, 129):
        with pytest.raises(ValueError, match="64 <= D <= 128"):
            ops().more_blocked(ctx, packed, chols, xd, ld, lp, bgd, tlpd, l2d, bad)
    assert call(d, xd.ptr) == 0
    l2 = np.full(k, 1e-6)
    rh, rg = omore.get_expected_hessian_and_grad(m, l2, x, mapping, bg, tlp, False, True)
    _assert_bound(hh.numpy(), gg.numpy(), rh, rg, 1e-2, "valid call after the refused ones")
