"""Temperature != 1 on the GPU: the component KL update on every route at eta = max(lo, temperature) with both branches taken
(weight_step_cases.py, guarded by test_weight_step_cpu.py), and whole trajectories against the fp64 oracle at temperature 0.5
and 3.  Assertions and tolerances are those of test_update_components_kl / test_blocked_update_components_kl /
test_diag_update_kl and of test_hip_train_iter.run_pair."""
import numpy as np
import pytest

from oracle import gmm as ogmm, updaters as oupd
import weight_step_cases as cases
from helpers import samtron_config
from test_hip_train_iter import run_pair
from test_hip_diag_mmd import _run_pair as run_diag_pair

pytestmark = pytest.mark.gpu

KL_RTOL = {"dense": 5e-3, "reference": 5e-3, "blocked": 1e-2, "diag": 5e-3}


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


@pytest.mark.parametrize("route,d,temperature", cases.kl_case_ids())
def test_update_components_kl_at_temperature(ctx, route, d, temperature):
    """Cold round, then warm round: in the warm one, at temperature 30, half of the components are raised to eta = temperature,
    where a kernel can no longer return the KL its search holds and factorises at an eta it never probed."""
    from gmmvi_amd import hip_ops
    m, hs, gs, stepsizes = cases.kl_update_inputs(route, d, temperature)
    k = cases.KL_K
    w = ogmm.GmmWrapper(m, 0.1, 1e-12, 4)
    w.stepsizes = stepsizes
    means, chols = ctx.asarray(m.means), ctx.asarray(m.chol_cov)
    last_eta = ctx.asarray(w.last_log_etas); l2 = ctx.asarray(w.l2_regularizers)
    nupd = ctx.asarray(w.num_received_updates); steps = ctx.asarray(w.stepsizes)
    raised_seen = kept_seen = 0
    for round_ in range(2):
        if route == "diag":
            succ, kl, probes = hip_ops.update_components_diag(ctx, "kl", means, chols, ctx.asarray(hs), ctx.asarray(gs), steps,
                                                              temperature, 1e-12, last_eta, l2, nupd, want_info=True)
        else:
            succ, kl, probes = hip_ops.update_components_kl(ctx, means, chols, ctx.asarray(hs), ctx.asarray(gs), steps,
                                                            temperature, 1e-12, last_eta, l2, nupd, want_info=True,
                                                            reference=(route == "reference"))
        rs, retas, rkls, rprobes = oupd.apply_ng_update_kl(w, hs, gs, w.stepsizes, temperature, traces=[])
        raised_seen += int(np.sum(rs & (retas == temperature)))
        kept_seen += int(np.sum(rs & (retas > temperature)))
        np.testing.assert_array_equal(succ.numpy().astype(bool), rs)
        np.testing.assert_array_equal(probes.numpy(), rprobes)          # same bisection path
        np.testing.assert_allclose(last_eta.numpy(), retas, rtol=1e-5)
        if route == "diag":
            # (above D = 512 the inputs are scaled so that the sum keeps the size it has at 512, diag_highd_cases.update_scale)
            np.testing.assert_allclose(kl.numpy(), rkls, rtol=KL_RTOL[route], atol=1e-5 * min(d, 512))
            np.testing.assert_allclose(means.numpy(), m.means, rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(chols.numpy(), m.chol_cov, rtol=1e-4, atol=1e-6)
        else:
            np.testing.assert_allclose(kl.numpy(), rkls, rtol=KL_RTOL[route], atol=1e-5)
            np.testing.assert_allclose(means.numpy(), m.means, rtol=1e-3, atol=1e-3)
            np.testing.assert_allclose(chols.numpy(), m.chol_cov, rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(l2.numpy(), w.l2_regularizers, rtol=1e-6)
        np.testing.assert_allclose(nupd.numpy(), w.num_received_updates)
    assert kept_seen > 0 and (raised_seen > 0) == (temperature > 1)


@pytest.mark.parametrize("temperature", [0.5, 3.0])
@pytest.mark.parametrize("fused", [False, True], ids=["modular", "single_call"])
@pytest.mark.parametrize("kind,d,k,s", [("gmm", 4, 3, 32), ("stm", 20, 8, 64)])
def test_trajectory_at_temperature(kind, d, k, s, fused, temperature):
    run_pair(kind, d, k, s, seed=11, iters=8, cfg=samtron_config(s, temperature=temperature), fused=fused)


@pytest.mark.parametrize("temperature", [0.5, 3.0])
def test_diagonal_trajectory_at_temperature(temperature):
    o, g = run_diag_pair("diaggmm", 6, 4, 40, 8, samtron_config(40, diag=True, temperature=temperature))
    np.testing.assert_allclose(g.model.last_log_etas.numpy(), o.model.last_log_etas, rtol=5e-2, atol=1e-6)


@pytest.mark.parametrize("temperature", [0.5, 3.0])
def test_direct_weight_updater_trajectory_at_temperature(temperature):
    """bound / beta of the direct weight update (weight_updater.py:137)."""
    cfg = samtron_config(40, initial_stepsize=0.01, weight_updater="direct", wstep=0.05, temperature=temperature)
    run_pair("gmm", 4, 3, 40, seed=3, iters=6, cfg=cfg)
