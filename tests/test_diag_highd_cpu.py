"""Host-side checks of the diagonal path above D = 512 (no GPU needed): the limits agree between the header, the Python
mirror and the entry points' argument checks, and the oracle-only parts of tests/test_hip_diag_highd.py hold."""
import os
import re

import numpy as np
import pytest

from oracle import gmm as ogmm, updaters as oupd
import diag_highd_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry_point_bodies(source):
    """name -> body text of every `int gmmvi_*(...) {` definition of a .hip file (comments removed)."""
    code = re.sub(r"//[^\n]*", "", source)
    out = {}
    for m in re.finditer(r"\bint\s+(gmmvi_\w+)\s*\([^)]*\)\s*\{", code):
        end = code.find("\n}\n", m.end())
        out[m.group(1)] = code[m.end():end]
    return out


def test_diag_limit_agrees_between_header_mirror_and_checks():
    from gmmvi_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmmvi_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"#define\s+GMMVI_MAX_DIM_DIAG\s+(\d+)\b", code)
    assert m and int(m.group(1)) == _lib.MAX_DIM_DIAG == 131072
    m = re.search(r"#define\s+GMMVI_MAX_DIM_BLOCKED\s+(\d+)\b", code)
    assert m and int(m.group(1)) == _lib.MAX_DIM_BLOCKED == 512
    bodies = {}
    for name in ("diag.hip", "diag_sweep.hip"):
        bodies.update(_entry_point_bodies(open(os.path.join(ROOT, "gmmvi_amd", "csrc", name)).read()))
    for fn in ("gmmvi_diag_pack", "gmmvi_diag_mixture_eval", "gmmvi_diag_sample", "gmmvi_diag_stein",
               "gmmvi_update_components_diag_kl", "gmmvi_update_components_diag_iblr"):
        assert re.search(r"GMMVI_ARG_CHECK\(ctx,[^;]*D\s*<=\s*GMMVI_MAX_DIM_DIAG\b", bodies[fn]), fn
        assert not re.search(r"GMMVI_ARG_CHECK\(ctx,[^;]*D\s*<=\s*GMMVI_MAX_DIM_BLOCKED\b", bodies[fn]), fn
    for fn in ("gmmvi_diag_embed", "gmmvi_diag_extract"):                    # they build [K, D, D]
        assert re.search(r"GMMVI_ARG_CHECK\(ctx,[^;]*D\s*<=\s*GMMVI_MAX_DIM_BLOCKED\b", bodies[fn]), fn
    assert "MAX_DIM" not in bodies["gmmvi_reciprocal_f32"]                   # any length


def test_diag_model_refuses_dimensions_above_the_limit_without_a_device():
    """The range check comes before the first device call and names the limit."""
    from gmmvi_amd import _lib
    from gmmvi_amd.models.diagonal_gmm import DiagonalGMM

    class NoDevice:
        def asarray(self, a, dtype=None):
            return np.asarray(a)

    d = _lib.MAX_DIM_DIAG + 1
    with pytest.raises(ValueError, match=str(_lib.MAX_DIM_DIAG)):
        DiagonalGMM(np.ones(1), np.zeros((1, d), np.float32), np.ones((1, d), np.float32), ctx=NoDevice())


@pytest.mark.parametrize("k,d", cases.KL_CASES)
def test_committed_update_scaling_makes_every_fp64_step_succeed(k, d):
    """Item 4's inputs: with update_scale(d) every component's step is accepted in both rounds, with an accepted KL that is
    neither trivial nor beyond the reference's acceptance band."""
    m, hs, gs, steps = cases.diag_update_inputs(np.random.default_rng(1234), k, d)
    w = ogmm.GmmWrapper(m, 0.1, 1e-12, 4)
    for _ in range(2):
        succ, etas, kls, probes = oupd.apply_ng_update_kl(w, hs.astype(np.float64), gs.astype(np.float64), steps, 1.0, traces=[])
        assert succ.all()
        assert np.all(kls >= 0.04 * steps) and np.all(kls <= 1.1 * steps)
        assert np.all(probes >= 2) and np.all(etas > 1.0)


def test_eta_tolerance_figure():
    """The committed figure is the measured one (fp64 oracle against the oracle in fp32 mode at D = 512)."""
    worst = cases.eta_tolerance_cases()
    assert worst <= cases.ETA_RTOL_D512 and worst >= 0.5 * cases.ETA_RTOL_D512


def test_rounding_only_ess_figure():
    """Item 2: what rounding the fp64 ld and bg to fp32 alone does to the effective sample sizes at D = 20 000 -- a small
    but non-zero relative deviation (an fp32 ulp of a log density is 0.004 there), the device's allowance up to a factor 2."""
    _, _, ld, bg, e64, dev = cases.ess_case(np.random.default_rng(1234))
    k, d, n = cases.ESS_CASE
    assert ld.shape == (k, n) and np.all(e64 > 50) and np.all(e64 <= n / k + 1)
    assert 0.0 < dev < 1e-3
