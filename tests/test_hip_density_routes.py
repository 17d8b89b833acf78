"""The packed two-samples-per-lane mixture sweep (density_pk.hip mixture_eval_pk_kernel) and the small log-sum-exp merges
against fp64 NumPy / SciPy.

From (N + 127) / 128 * K >= 4096 passes on, gmmvi_mixture_eval(_dual) runs the packed kernel: every padded dimension it is
instantiated for, both families, with and without the gradient, the ld-only form the sample database calls, and the dual
sweep.  The fp64 reference is computed on a fixed subset of the samples only (the first and the last 128-sample tile, lanes
63 / 64 of every few tiles, 1 000 more at random): a sample's outputs depend on that sample and all K components alone.
The edges (tiny and ragged N, forced chunk counts and wave counts) need the route forced through environment knobs the
library reads once per process: they run in child processes (density_route_child.py).

Tolerances are those of test_hip_kernels.assert_parity: log densities 1e-5 relative / 1e-6 * scale, gradients 1e-4 /
1e-5 * scale (scale = max(1, max |reference|)); a looser bound carries its reason next to it."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.linalg import solve_triangular
from scipy.special import gammaln, logsumexp

from oracle import gmm as ogmm, targets as otargets

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GAUSS, STUDENT_T = 0, 1                                     # include/gmmvi_hip.h
NU = 2.0
PADDED = (2, 4, 8, 10, 12, 16, 20, 24, 32, 40, 50)          # common.h gmmvi_padded_dim, register path


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def ops():
    from gmmvi_amd import hip_ops
    return hip_ops


def padded_dim(d):
    return next(dp for dp in PADDED + (64,) if d <= dp)


def packed_route(k, n, d, grad):
    """The route choice of density.hip sweep_route (the block under "enough (128-sample tile, component) passes") with no
    GMMVI_ME_PK* knob set: the packed kernel from 4 096 passes on, at padded D <= 50, with the gradient only up to padded
    D = 40."""
    dp = padded_dim(d)
    if dp > 50 or (grad and dp > 40):
        return False
    return (n + 127) // 128 * k >= 4096


def pk_knobs_set():
    return sorted(v for v in os.environ if v.startswith("GMMVI_ME_PK"))


# ---- fp64 reference ------------------------------------------------------------------------------------------------------

def component_terms(means, chols, x, family, nu=NU, want_grad=True):
    """fp64 per-component log densities [K, n] and, per component, the generator of their gradients in x."""
    k, d = means.shape
    for i in range(k):
        z = solve_triangular(chols[i], (x - means[i]).T, lower=True)
        q = np.sum(z * z, axis=0)
        logdet = np.sum(np.log(np.diag(chols[i])))
        if family == GAUSS:
            ld = -0.5 * q - logdet - 0.5 * d * np.log(2 * np.pi)
            coef = -np.ones_like(q)
        else:       # multivariate Student-t with scale factor L (oracle/targets.py StudentTMixtureTarget._components)
            ld = (gammaln(0.5 * (nu + d)) - gammaln(0.5 * nu) - 0.5 * d * np.log(nu * np.pi) - logdet
                  - 0.5 * (nu + d) * np.log1p(q / nu))
            coef = -(nu + d) / (nu + q)
        y = solve_triangular(chols[i], z, lower=True, trans='T').T if want_grad else None
        yield ld, (coef[:, None] * y if want_grad else None)


def reference(means, chols, logws, x, family, want_grad=True):
    """-> (ld [K, n], [log sum_k exp(logw_k + ld_k) for logw in logws], gradient of the first mixture [n, D])."""
    ld = np.stack([t[0] for t in component_terms(means, chols, x, family, want_grad=False)])
    lps = [logsumexp(ld + np.asarray(lw, np.float64)[:, None], axis=0) for lw in logws]
    grad = None
    if want_grad:
        grad = np.zeros_like(x)
        for i, (ldi, gi) in enumerate(component_terms(means, chols, x, family)):
            grad += np.exp(ldi + logws[0][i] - lps[0])[:, None] * gi
    return ld, lps, grad


def assert_reference_is_the_oracle(means, chols, logw, x, family):
    """The fp64 reference above (arbitrary log weights, Student-t component densities) against oracle.gmm.FullCovGMM and
    oracle.targets.StudentTMixtureTarget, which normalise the weights: same log density up to log sum w, same gradient."""
    lse_w = logsumexp(logw)
    covs = chols @ np.transpose(chols, (0, 2, 1))
    if family == GAUSS:
        olp, og, _ = ogmm.FullCovGMM(np.exp(logw - lse_w), means, covs).log_density_and_grad(x)
    else:
        olp, og = otargets.StudentTMixtureTarget(np.exp(logw - lse_w), means, covs, NU).log_density_and_grad(x)
    _, (rlp,), rg = reference(means, chols, [logw], x, family)
    np.testing.assert_allclose(rlp - lse_w, olp, rtol=1e-9, atol=1e-9 * np.abs(olp).max())
    np.testing.assert_allclose(rg, og, rtol=1e-7, atol=1e-9 * np.abs(og).max())


def assert_parity(actual, desired, rtol, atol, what):
    """test_hip_kernels.assert_parity, with -inf allowed in the reference: the same places must hold -inf, the scale is
    taken over the finite values."""
    actual, desired = np.asarray(actual, np.float64), np.asarray(desired, np.float64)
    ninf = np.isneginf(desired)
    np.testing.assert_array_equal(np.isneginf(actual), ninf, err_msg=what + ": -inf places")
    a, r = actual[~ninf], desired[~ninf]
    scale = max(1.0, float(np.max(np.abs(r)))) if r.size else 1.0
    np.testing.assert_allclose(a, r, rtol=rtol, atol=atol * scale, err_msg=what)


def sample_subset(n, rng):
    tiles = (n + 127) // 128
    idx = set(range(min(n, 128))) | set(range((tiles - 1) * 128, n))
    for t in range(0, tiles, max(1, tiles // 8)):
        idx |= {i for i in (t * 128 + 63, t * 128 + 64) if i < n}
    idx |= set(rng.choice(n, min(n, 1000), replace=False).tolist())
    return np.array(sorted(idx))


def random_components(rng, k, d, spread=3.0):
    means = rng.normal(size=(k, d)) * spread
    a = rng.normal(size=(k, d, d))
    covs = a @ np.transpose(a, (0, 2, 1)) / d + 0.3 * np.eye(d)
    return means, np.linalg.cholesky(covs)


def near_samples(rng, means, n):
    return means[rng.integers(0, means.shape[0], n)] + rng.normal(size=(n, means.shape[1])) * 1.5


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def dual_eval(ctx, packed, logw, logw2, x, d, family, want_ld=False, want_grad=True):
    """gmmvi_mixture_eval_dual for either family (hip_ops.mixture_eval_dual is the model's Gaussian form)."""
    k, n = packed.shape[0], x.shape[0]
    ld = ctx.empty((k, n)) if want_ld else None
    lp, lp2 = ctx.empty((n,)), ctx.empty((n,))
    grad = ctx.empty((n, d)) if want_grad else None
    ctx.check(ctx.lib.gmmvi_mixture_eval_dual(ctx.handle, family, NU if family == STUDENT_T else 0.0, k, d, packed.ptr,
                                              logw.ptr, logw2.ptr, x.ptr, n, None if ld is None else ld.ptr, lp.ptr,
                                              None if grad is None else grad.ptr, lp2.ptr))
    return ld, lp, grad, lp2


def pack(ctx, means, chols, family):
    return ops().pack_components(ctx, ctx.asarray(means), ctx.asarray(chols), family=family,
                                 nu=NU if family == STUDENT_T else 0.0)[0]


def check_all_sweeps(ctx, rng, means, chols, logw, logw2, x, family, sub, what, grad_bound=(1e-4, 1e-5)):
    """ld + lp, lp + gradient (padded D <= 40), ld alone, the dual sweep: each against fp64 on the samples `sub`."""
    k, d = means.shape
    n = x.shape[0]
    nu = NU if family == STUDENT_T else 0.0
    grad_ok = padded_dim(d) <= 40
    packed = pack(ctx, means, chols, family)
    lw_d, lw2_d, x_d = ctx.asarray(logw), ctx.asarray(logw2), ctx.asarray(x)
    rld, (rlp, rlp2), rgrad = reference(f32(means), f32(chols), [f32(logw), f32(logw2)], f32(x[sub]), family,
                                        want_grad=grad_ok)
    ld, lp, _ = ops().mixture_eval(ctx, packed, lw_d, x_d, d, family=family, nu=nu, want_ld=True, want_lp=True)
    assert_parity(ld.numpy()[:, sub], rld, 1e-5, 1e-6, what + ": component log densities")
    assert_parity(lp.numpy()[sub], rlp, 1e-5, 1e-6, what + ": mixture log density")
    ld1, _, _ = ops().mixture_eval(ctx, packed, lw_d, x_d, d, family=family, nu=nu, want_ld=True, want_lp=False)
    assert_parity(ld1.numpy()[:, sub], rld, 1e-5, 1e-6, what + ": component log densities alone")
    if grad_ok:
        _, lpg, grad = ops().mixture_eval(ctx, packed, lw_d, x_d, d, family=family, nu=nu, want_grad=True)
        assert_parity(lpg.numpy()[sub], rlp, 1e-5, 1e-6, what + ": mixture log density (gradient sweep)")
        assert_parity(grad.numpy()[sub], rgrad, *grad_bound, what + ": gradient")
    _, lpd, gradd, lp2d = dual_eval(ctx, packed, lw_d, lw2_d, x_d, d, family, want_grad=grad_ok)
    assert_parity(lpd.numpy()[sub], rlp, 1e-5, 1e-6, what + ": dual sweep, first mixture")
    assert_parity(lp2d.numpy()[sub], rlp2, 1e-5, 1e-6, what + ": dual sweep, second mixture")
    if grad_ok:
        assert_parity(gradd.numpy()[sub], rgrad, *grad_bound, what + ": dual sweep, gradient")
    return ld, lp


# ---- 1. the packed route as shipped --------------------------------------------------------------------------------------

# (D, K, N): just at or above 4 096 passes at every padded dimension; dimensions below their padding (3 / 4, 7 / 8, 11 / 12,
# 17 / 20, 27 / 32, 37 / 40, 45 / 50), ragged last tiles (N = 16 257: one sample in the last tile), and chunk counts from 2
# (128 tiles) to 32 (8 tiles, K = 512: the run-time branch of the partial merge) on the 256 CUs of an MI355X
PK_SHAPES = [(2, 32, 16257), (3, 256, 2047), (7, 128, 4001), (10, 103, 5100), (11, 41, 12800), (16, 64, 8191),
             (17, 512, 1024), (24, 128, 4097), (27, 64, 8100), (37, 60, 10001), (45, 64, 9000)]


def test_the_shapes_cover_every_packed_instance():
    assert sorted({padded_dim(d) for d, _, _ in PK_SHAPES}) == list(PADDED)
    assert all(packed_route(k, n, d, grad=False) for d, k, n in PK_SHAPES)
    assert all(packed_route(k, n, d, grad=True) for d, k, n in PK_SHAPES if padded_dim(d) <= 40)


@pytest.mark.parametrize("family", [GAUSS, STUDENT_T], ids=["gauss", "student_t"])
@pytest.mark.parametrize("d,k,n", PK_SHAPES)
def test_packed_sweep_against_fp64(ctx, rng, d, k, n, family):
    if pk_knobs_set():
        pytest.skip(f"{', '.join(pk_knobs_set())} set in the environment: these shapes may not take the packed kernel")
    means, chols = random_components(rng, k, d)
    logw = np.log(rng.dirichlet(np.ones(k)))
    logw2 = np.log(rng.integers(1, 50, k) / 1.0) - np.log(50.0 * k)       # background weights (counts), unnormalised
    x = near_samples(rng, means, n)
    assert_reference_is_the_oracle(means, chols, logw, x[:16], family)
    check_all_sweeps(ctx, rng, means, chols, logw, logw2, x, family, sample_subset(n, rng), f"D {d} K {k} N {n}")


# ---- 2. the route boundary -----------------------------------------------------------------------------------------------

def test_route_boundary_4095_and_4096_passes(ctx, rng):
    """K = 65, N = 8 064 (63 tiles: 4 095 passes, the one-sample kernel) against K = 64, N = 8 192 (64 tiles: 4 096, the
    packed kernel), the same mixture on both sides: A's components 0 and 64 are B's component 0, each at half its weight.
    Both sides match fp64, and each other on the 8 064 shared samples to the same bound."""
    if pk_knobs_set():
        pytest.skip(f"{', '.join(pk_knobs_set())} set in the environment: the route choice is not the shipped one")
    d = 20
    means, chols = random_components(rng, 64, d)
    logw = np.log(rng.dirichlet(np.ones(64)))
    x = near_samples(rng, means, 8192)
    sides = {"A": (np.concatenate([means, means[:1]]), np.concatenate([chols, chols[:1]]),
                   np.concatenate([logw, logw[:1]]) - np.log(2.0) * (np.arange(65) % 64 == 0), x[:8064]),
             "B": (means, chols, logw, x)}
    assert not packed_route(65, 8064, d, True) and packed_route(64, 8192, d, True)
    sub = sample_subset(8064, rng)
    out = {}
    for name, (mu, ch, lw, xs) in sides.items():
        packed = pack(ctx, mu, ch, GAUSS)
        ld, lp, grad = ops().mixture_eval(ctx, packed, ctx.asarray(lw), ctx.asarray(xs), d, want_ld=True, want_lp=True,
                                          want_grad=True)
        out[name] = ld.numpy()[:64, :8064], lp.numpy()[:8064], grad.numpy()[:8064]
        rld, (rlp,), rg = reference(f32(mu), f32(ch), [f32(lw)], f32(xs[sub]), GAUSS)
        assert_parity(out[name][0][:, sub], rld[:64], 1e-5, 1e-6, name + ": component log densities")
        assert_parity(out[name][1][sub], rlp, 1e-5, 1e-6, name + ": mixture log density")
        assert_parity(out[name][2][sub], rg, 1e-4, 1e-5, name + ": gradient")
    for i, what in enumerate(("component log densities", "mixture log density", "gradient")):
        bound = (1e-4, 1e-5) if what == "gradient" else (1e-5, 1e-6)
        assert_parity(out["B"][i], out["A"][i], *bound, "B against A: " + what)


# ---- 3. edges with the route forced (child processes) --------------------------------------------------------------------

def _edge_cases(rng):
    """Tiny and ragged N against K in {1, 3, 5, 7}, both families, dimensions across the padded set, far samples."""
    cases = []
    dims = [2, 5, 10, 13, 17, 24, 27, 40, 45]
    i = 0
    for n in (1, 2, 3, 127, 128, 129, 257):
        for k in (1, 3, 5, 7):
            d = dims[i % len(dims)]
            family = (GAUSS, STUDENT_T)[i % 2]
            far = i % 5 == 4
            i += 1
            means, chols = random_components(rng, k, d)
            x = rng.normal(size=(n, d)) * 200 if far else near_samples(rng, means, n)
            cases.append(dict(family=family, means=means, chols=chols, logw=np.log(rng.dirichlet(np.ones(k))),
                              logw2=np.log(rng.dirichlet(np.ones(k))), x=x, far=far))
    return cases


def _run_child(tmp_path, name, env_knobs, cases):
    src, dst = tmp_path / f"{name}_in.npz", tmp_path / f"{name}_out.npz"
    arrays = {"ncases": np.array(len(cases))}
    for c, case in enumerate(cases):
        for key in ("family", "means", "chols", "logw", "logw2", "x"):
            arrays[f"c{c}_{key}"] = np.asarray(case[key])
    np.savez(src, **arrays)
    env = {v: s for v, s in os.environ.items() if not v.startswith("GMMVI_ME_")}
    env.update(env_knobs)
    r = subprocess.run([sys.executable, os.path.join(HERE, "density_route_child.py"), str(src), str(dst)], env=env,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"child {name} ({env_knobs}) exited with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return np.load(dst)


def _check_child(out, cases, what):
    for c, case in enumerate(cases):
        d = case["means"].shape[1]
        family, x = int(case["family"]), case["x"]
        grad_ok = padded_dim(d) <= 40
        tag = f"{what}, case {c} (K {case['means'].shape[0]}, D {d}, N {x.shape[0]}, family {family})"
        rld, (rlp, rlp2), rg = reference(f32(case["means"]), f32(case["chols"]), [f32(case["logw"]), f32(case["logw2"])],
                                         f32(x), family, want_grad=grad_ok)
        assert_parity(out[f"c{c}_ld"], rld, 1e-5, 1e-6, tag + ": component log densities")
        assert_parity(out[f"c{c}_lp"], rlp, 1e-5, 1e-6, tag + ": mixture log density")
        assert_parity(out[f"c{c}_ld1"], rld, 1e-5, 1e-6, tag + ": component log densities alone")
        assert_parity(out[f"c{c}_lpd"], rlp, 1e-5, 1e-6, tag + ": dual sweep, first mixture")
        assert_parity(out[f"c{c}_lp2d"], rlp2, 1e-5, 1e-6, tag + ": dual sweep, second mixture")
        if grad_ok:
            # far samples (|x| ~ 200 x sqrt(D)): |ld| ~ 1e4 .. 1e5, whose fp32 rounding (~1e-2) moves the responsibilities of
            # nearly tied components by as much; the bound of test_hip_kernels.test_mixture_eval_far_samples_and_empty
            gb = (2e-3, 1e-2 / max(1.0, float(np.abs(rg).max()))) if case["far"] else (1e-4, 1e-5)
            assert_parity(out[f"c{c}_lpg"], rlp, 1e-5, 1e-6, tag + ": mixture log density (gradient sweep)")
            assert_parity(out[f"c{c}_grad"], rg, *gb, tag + ": gradient")
            assert_parity(out[f"c{c}_gradd"], rg, *gb, tag + ": dual sweep, gradient")


def test_packed_sweep_forced_at_the_edges(ctx, rng, tmp_path):
    """GMMVI_ME_PK=1 in three children: the launch's own geometry (at most (K + 3) / 4 chunks: K = 5 / 7 in chunks of
    3 + 2 / 4 + 3 components, as many waves as the chunk has components), then the chunk count forced to 4 with one wave
    per workgroup (K = 5: 2 + 2 + 1, K = 7: 2 + 2 + 2 + 1) and to 3 with two waves (K = 5: 2 + 2 + 1, K = 7: 3 + 3 + 1:
    a wave without a component in the last chunk).  The partials of every split go through combine_partials.  Far
    samples and log weights far from 0 go along (test_log_weights_far_from_zero has their reasons)."""
    cases = _edge_cases(rng)
    cases += _far_weight_cases(rng, n=300)
    for name, knobs in (("geometry", {"GMMVI_ME_PK": "1"}),
                        ("ky4_nw1", {"GMMVI_ME_PK": "1", "GMMVI_ME_PK_KY": "4", "GMMVI_ME_PK_NW": "1"}),
                        ("ky3_nw2", {"GMMVI_ME_PK": "1", "GMMVI_ME_PK_KY": "3", "GMMVI_ME_PK_NW": "2"})):
        _check_child(_run_child(tmp_path, name, knobs, cases), cases, name)


# ---- 4. log weights far from 0 -------------------------------------------------------------------------------------------

def _far_weight_cases(rng, n):
    """Six well separated components, Gaussian at D = 10 and Student-t at D = 27 (padded 32): component 0 at log weight -100
    and component 1 at the model floor log(1e-30) = -69.07 (weights.hip), each alone near its own samples (the other
    components lie more than 150 nats lower there: the Student-t tails need the means 1 000 apart for that).  The second
    weights (dual sweep) put -100 on component 2 and 0 on component 0."""
    cases = []
    for d, family, spacing in ((10, GAUSS, 60.0), (27, STUDENT_T, 1000.0)):
        k = 6
        means = np.zeros((k, d))
        for i in range(k):
            means[i, i] = spacing
        chols = np.stack([np.eye(d) * (0.7 + 0.1 * i) for i in range(k)])
        logw = np.log(np.full(k, 1.0 / k))
        logw[0], logw[1] = -100.0, np.log(1e-30)
        logw2 = np.log(np.full(k, 0.2))
        logw2[2], logw2[0] = -100.0, 0.0
        x = means[np.arange(n) % k] + rng.normal(size=(n, d))
        cases.append(dict(family=family, means=means, chols=chols, logw=logw, logw2=logw2, x=x, far=False))
    return cases


@pytest.mark.parametrize("route", ["packed", "default"])
def test_log_weights_far_from_zero(ctx, rng, route):
    """The contract of every route: lp = fp64 log sum_k exp(logw_k + ld_k) for any finite log weight.  A weight taken as the
    factor exp(-100) underflows fp32 (a component that alone covers a sample would vanish: lp = -inf); the model floor
    -69.07 stays in range.  route "packed": N = 8 192 at K = 6 (64 tiles: 384 passes -- forced in the child of
    test_packed_sweep_forced_at_the_edges) is below the threshold, so the in-process packed case repeats the six
    components to K = 66 (4 224 passes) with the copies at weights 1e-3 of the originals; "default": N = 300."""
    if pk_knobs_set():
        pytest.skip(f"{', '.join(pk_knobs_set())} set in the environment: the route choice is not the shipped one")
    for case in _far_weight_cases(rng, 8192 if route == "packed" else 300):
        means, chols, logw, logw2, x, family = (case[key] for key in ("means", "chols", "logw", "logw2", "x", "family"))
        if route == "packed":
            reps = 11
            means, chols = np.tile(means, (reps, 1)), np.tile(chols, (reps, 1, 1))
            extra = np.log(1e-3) * (np.arange(6 * reps) >= 6)
            logw, logw2 = np.tile(logw, reps) + extra, np.tile(logw2, reps) + extra
        k, d = means.shape
        n = x.shape[0]
        assert packed_route(k, n, d, grad=True) == (route == "packed")
        sub = sample_subset(n, rng) if route == "packed" else np.arange(n)
        check_all_sweeps(ctx, rng, means, chols, logw, logw2, x, family, sub, f"{route} route, D {d}")


# ---- 5. the merges -------------------------------------------------------------------------------------------------------

def lse_rows(v):
    """log sum exp over axis 0 in fp64, -inf for an empty or all -inf column."""
    v = np.asarray(v, np.float64)
    if v.shape[0] == 0:
        return np.full(v.shape[1:], -np.inf)
    m = np.max(v, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = m + np.log(np.sum(np.exp(v - np.where(np.isneginf(m), 0.0, m)), axis=0))
    return np.where(np.isneginf(m), -np.inf, out)


@pytest.mark.parametrize("r", [2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 9, 11, 20])    # unrolled cases of combine.h, then the loop
@pytest.mark.parametrize("with_grad", [True, False])
def test_combine_partials(ctx, rng, r, with_grad):
    """Partials spread over 200 nats, a whole -inf partial (a chunk that covers none of the samples), columns where all
    partials are -inf but one, and one column where all are -inf (lp = -inf; its gradient, that of log 0, is not checked)."""
    n, d = 333, 7
    lp = rng.normal(size=(r, n)) * 50 - 20
    lp[r // 2] = -np.inf
    lp[:, 5] = -np.inf
    lp[r - 1, 5] = 3.0
    lp[:, 7] = -np.inf
    g = rng.normal(size=(r, n, d))
    lp32, g32 = f32(lp), f32(g)
    out_lp, out_g = ops().combine_partials(ctx, ctx.asarray(lp32), ctx.asarray(g32) if with_grad else None, d)
    ref_lp = lse_rows(lp32)
    assert_parity(out_lp.numpy(), ref_lp, 1e-5, 1e-6, "merged log values")
    if with_grad:
        keep = np.isfinite(ref_lp)
        resp = np.exp(lp32[:, keep] - ref_lp[None, keep])
        assert_parity(out_g.numpy()[keep], np.einsum("rn,rnd->nd", resp, g32[:, keep]), 1e-4, 1e-5, "merged gradients")
    else:
        assert out_g is None


def test_segment_lse_into(ctx, rng):
    """Segment lengths 0, 1, 7, 8, 9, 17 and 3 000 (the loop takes eight components per round), N = 300 (not a multiple of
    the 256-thread block), col0 = 3 inside a row of 311, -inf log weights (one segment all -inf).  The cells the launch
    does not own keep their contents."""
    lengths = [0, 1, 7, 8, 9, 17, 3000, 0, 5]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    kw, n, col0, width = int(offs[-1]), 300, 3, 311
    ld = f32(rng.normal(size=(kw, n)) * 20 - 50)
    logw = f32(np.log(rng.dirichlet(np.ones(kw))))
    logw[rng.choice(kw, 40, replace=False)] = -np.inf
    logw[offs[2]:offs[3]] = -np.inf                               # the segment of seven: no weight at all
    logw[offs[6] + 5] = -100.0
    out = ctx.asarray(np.full((len(lengths) + 2, width), 7.0, np.float32))
    ops().segment_lse_into(ctx, out, col0, ctx.asarray(offs, np.int32), ctx.asarray(logw), ctx.asarray(ld))
    got = out.numpy()
    g = len(lengths)
    ref = np.stack([lse_rows(logw[offs[i]:offs[i + 1], None] + ld[offs[i]:offs[i + 1]]) for i in range(g)])
    assert np.isneginf(ref[[0, 2, 7]]).all()
    assert_parity(got[:g, col0:col0 + n], ref, 1e-5, 1e-6, "segment log-sum-exp")
    untouched = np.ones(got.shape, bool)
    untouched[:g, col0:col0 + n] = False
    assert (got[untouched] == 7.0).all()


def test_logaddexp(ctx, rng):
    """log(exp(a + ca) + exp(b + cb)) with -inf in one operand, in both (-inf, not NaN), and offsets ca / cb of -100."""
    n = 1000
    a = f32(rng.normal(size=n) * 30)
    b = f32(rng.normal(size=n) * 30)
    a[::7] = -np.inf
    b[::5] = -np.inf                                              # both -inf at every 35th element
    for ca, cb in ((0.0, 0.0), (-100.0, 0.0), (0.0, -100.0), (-100.0, -100.0), (2.5, -1.0)):
        out = ops().logaddexp(ctx, ctx.asarray(a), ca, ctx.asarray(b), cb).numpy()
        ref = np.logaddexp(a + np.float32(ca), b + np.float32(cb))
        assert not np.isnan(out).any(), (ca, cb)
        assert_parity(out, ref, 1e-5, 1e-6, f"logaddexp ca {ca} cb {cb}")
