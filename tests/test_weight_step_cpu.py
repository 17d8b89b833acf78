"""Host-side guard of tests/test_hip_weight_step.py and tests/test_hip_temperature.py (no GPU needed): the fp64 oracle alone
shows that the committed cases reach what the GPU tests are about and that fp32 and fp64 take the same bisection path."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import weights as oweights
import weight_step_cases as cases


@pytest.mark.parametrize("route,d,temperature", cases.kl_case_ids())
def test_kl_cases_take_both_sides_of_the_temperature_clamp(route, d, temperature):
    """eta = max(lo, temperature): in the warm round some successful component keeps the search's result (eta == lo >
    temperature) and, at temperature 30, another one is raised to the temperature (eta == temperature > lo), which makes a
    kernel evaluate the step at an eta its search never probed.  Below 1 the second branch cannot be reached
    (weight_step_cases.KL_SCALES), and the cold round never reaches it either."""
    rounds = cases.run_kl_case(route, d, temperature)
    for r in rounds:
        assert r["kl_margin"] >= cases.PROBE_MARGIN and r["width_margin"] >= cases.PROBE_MARGIN
        assert r["success"].all()
    cold, warm = rounds
    assert np.all(cold["etas"] == cold["lo"]) and np.all(cold["lo"] > temperature)
    s = warm["success"]
    kept = s & (warm["etas"] == warm["lo"]) & (warm["lo"] > temperature)
    raised = s & (warm["etas"] == temperature) & (warm["lo"] < temperature)
    assert kept.any() and np.all(kept | raised)
    if temperature > 1:
        assert raised.any()
    else:
        assert not raised.any() and np.all(warm["lo"] >= 1.0)
    assert cases.kl_case_holds(rounds, temperature)


def test_a_case_below_temperature_one_is_kept():
    assert min(cases.KL_TEMPERATURES) < 1 < max(cases.KL_TEMPERATURES)
    assert set(cases.KL_SEEDS) == set(cases.kl_case_ids())


@pytest.mark.parametrize("k", cases.WEIGHT_KS[1:])
def test_weight_cases_keep_clear_of_the_decision_thresholds(k):
    """Every probe of the categorical bisection, for every (beta, eps) of the GPU test: KL at least 1e-3 eps away from 0.9 eps,
    eps and 1.1 eps, bracket width at least 1e-3 away from 0.1; and the replay used for that IS the oracle's search."""
    lw, elr = cases.weight_inputs(k)
    assert abs(logsumexp(lw)) < 1e-6
    outcomes = set()
    for beta in cases.WEIGHT_BETAS:
        for eps in cases.WEIGHT_EPS:
            kl, eta, nl, klm, wm, _ = cases.replay_weight_search(lw, elr, eps, beta)
            rkl, reta, rnl = oweights.weights_bracketing_search(lw, elr, eps, beta)
            assert (kl, eta) == (rkl, reta) and np.array_equal(nl, rnl)
            assert klm >= cases.PROBE_MARGIN and wm >= cases.PROBE_MARGIN
            assert eta > 0
            outcomes.add(bool(abs(eps - kl) < 0.1 * eps))
    assert outcomes == {True, False}          # the search ends inside the acceptance band (small bounds) and at exp(ub) (1e4)
    assert cases.weight_case_holds(k)


def test_weight_floor_case_puts_some_but_not_all_weights_on_the_floor():
    """Before the final renormalisation at least one, but not all, new log weights sit on -69.07: trust region at eps 0.3 and
    1e4, and the direct update, at every beta."""
    k = cases.FLOOR_K
    lw, elr = cases.weight_inputs(k, floor=True)
    assert cases.weight_case_holds(k, floor=True)
    for beta in cases.WEIGHT_BETAS:
        for eps in cases.FLOOR_EPS:
            _, eta, nl, _, _, on_floor = cases.replay_weight_search(lw, elr, eps, beta)
            assert 0 < on_floor < k
            # the returned weights: floored, then renormalised once (a shift far below an fp64 ulp of 69.07 here)
            assert np.sum(nl == nl.min()) == on_floor and abs(nl.min() - cases.LOG_WEIGHT_FLOOR) < 1e-9
        assert 0 < cases.direct_floor_count(lw, elr, cases.DIRECT_STEPSIZE, beta) < k


def test_elr_formula_is_the_oracle_formula():
    """weight_step_cases.elr_formula in fp64 against the two forms of oracle/weights.py:10-29 (the plain importance weights go
    through log |rho| there), on the benign and the wide-range inputs."""
    rng = np.random.default_rng(1234)
    for ld, bg, tlp, logq, logw in (cases.elr_benign_inputs(rng, 3, 1025), cases.elr_wide_inputs(rng)):
        for beta in (0.4, 2.5):
            rho = tlp - beta * logq
            lw = ld - bg[None, :]
            e, reward, ess = cases.elr_formula(ld, bg, tlp, logq, beta, logw, True)
            w = np.exp(lw - logsumexp(lw, axis=1, keepdims=True))
            np.testing.assert_allclose(e, (w / w.sum(axis=1, keepdims=True)) @ rho, rtol=1e-12)
            np.testing.assert_allclose(ess, 1 / np.sum(w * w, axis=1), rtol=1e-12)
            np.testing.assert_allclose(reward, beta * logw + e, rtol=1e-15)
            e, _, _ = cases.elr_formula(ld, bg, tlp, logq, beta, logw, False)
            a = lw + np.log(np.abs(rho))[None, :]
            m = np.max(a, axis=1, keepdims=True)
            ref = np.sum(np.sign(rho)[None, :] * np.exp(a - m), axis=1) * np.exp(m[:, 0]) / ld.shape[1]
            np.testing.assert_allclose(e, ref, rtol=1e-11)


def test_elr_wide_case_is_wide():
    """ld - bg spans 150 nats, row 0 has its maximum at the last sample (third round of 4096, in its ragged tail), row 1 is
    carried by one sample (effective sample size 1), row 2 is not."""
    ld, bg, tlp, logq, logw = cases.elr_wide_inputs(np.random.default_rng(1234))
    a = ld - bg[None, :]
    n = cases.ELR_WIDE_N
    assert a.shape == (3, n) and 2 * 4096 < n < 3 * 4096 and n % 1024 != 0
    assert a.max() - a.min() >= 150.0
    assert np.argmax(a[0]) == n - 1 and n - 1 >= 8192
    _, _, ess = cases.elr_formula(ld, bg, tlp, logq, 1.0, logw, True)
    assert ess[1] < 1.0 + 1e-9 and np.argmax(a[1]) == 5000 and ess[2] > 50


def test_split_log_values_leaves_dead_rows():
    rng = np.random.default_rng(1234)
    logq = rng.normal(size=4097) * 3 - 12
    for r in (2, 9, 16):
        parts = cases.split_log_values(rng, logq, r)
        dead = np.isneginf(parts)
        assert dead.any(axis=1).sum() == 1 and 0.2 < dead.sum() / 4097 < 0.45
        assert np.all(np.isfinite(logsumexp(parts, axis=0)))
