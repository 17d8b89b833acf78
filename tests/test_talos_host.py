"""Talos target on the host (no GPU): the fixture, the URDF parser and the packed table against the independent fp64
reference walk, the reference's five terms, the names and defaults, the dataset directory."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest
from scipy.special import log_ndtr

from talos_ref import GOLDEN_DIR, URDF, TalosRef, rpy

from gmmvi_amd.experiments.target_distributions import talos_ik as ti

JOINTS = (["torso_1_joint", "torso_2_joint"] + [f"arm_right_{i}_joint" for i in range(1, 8)]
          + [f"arm_left_{i}_joint" for i in range(1, 8)] + [f"leg_right_{i}_joint" for i in range(1, 7)]
          + [f"leg_left_{i}_joint" for i in range(1, 7)])


@pytest.fixture(scope="module")
def model():
    return ti.TalosModel(URDF)


@pytest.fixture(scope="module")
def ref():
    return TalosRef([0.1, 0.5, 1.0])


def _draws(rng, n):
    """Near the standing pose, talos.yml's N(0, I), and entries up to 1e3."""
    stand = rng.normal(size=(n, 34)) * 0.1
    stand[:, 30] += 1.08
    return [stand, rng.normal(size=(n, 34)), rng.uniform(-1e3, 1e3, size=(n, 34))]


def test_fixture_is_small_and_holds_links_and_joints_only():
    assert os.path.getsize(URDF) < 64 << 10
    root = ET.parse(URDF).getroot()
    assert root.tag == "robot" and {c.tag for c in root} == {"link", "joint"}
    for link in root.iter("link"):
        assert {c.tag for c in link} <= {"inertial"}
        for inr in link.iter("inertial"):
            assert {c.tag for c in inr} <= {"origin", "mass"}
    for joint in root.iter("joint"):
        assert {c.tag for c in joint} <= {"parent", "child", "origin", "axis", "limit"}


def test_parser_finds_the_joints_limits_links_and_mass(model, ref):
    assert model.joint_names == JOINTS == ref.urdf.actuated
    np.testing.assert_array_equal(model.limits, ref.urdf.limits)
    assert model.limits.shape == (28, 2) and np.all(model.limits[:, 0] < model.limits[:, 1])
    assert len(model.path_links) == 37 and sorted(model.path_links) == sorted(ref.urdf.path_links)
    assert model.total_mass == pytest.approx(87.042342, abs=1e-9)
    assert model.table.dtype == np.float32 and model.table.shape == (ti.TABLE_SIZE,)


def test_reference_reproduces_the_anchor_values(ref):
    poses, com = ref.fk(np.zeros((1, 34)))
    np.testing.assert_allclose(poses[0, 2, :3], [-0.02, -0.085, -1.083], atol=1e-4)
    np.testing.assert_allclose(poses[0, 3, :3], [-0.02, 0.085, -1.083], atol=1e-4)
    np.testing.assert_allclose(poses[0, 0, :3], [0.0049, -0.294, -0.2788], atol=1e-4)
    np.testing.assert_allclose(poses[0, 1, :3], [0.0049, 0.294, -0.2788], atol=1e-4)
    np.testing.assert_allclose(poses[0, 0, 3:].reshape(3, 3), np.diag([-1., -1., 1.]), atol=1e-9)
    np.testing.assert_allclose(com[0], [-0.024861, 0.001271, -0.168302], atol=1e-4)


def _axis_angle(a, q):
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(q) * K + (1 - np.cos(q)) * (K @ K)


def table_fk(table, x):
    """The packed table evaluated in fp64 for one sample, the way the device walks it: (poses [4, 12], com [3])."""
    t = np.asarray(table, np.float64)
    nj, nt, M = int(t[0]), int(t[1]), t[2]
    J = t[ti.HEADER:ti.HEADER + nj * ti.JOINT_STRIDE].reshape(nj, ti.JOINT_STRIDE)
    T = t[ti.HEADER + nj * ti.JOINT_STRIDE:].reshape(nt, ti.TIP_STRIDE)
    Rb, pb = rpy(x[31], x[32], x[33]), x[28:31]
    frames, com = [], Rb @ t[5:8] + t[4] * pb
    for j in range(nj):
        p = int(J[j, 0])
        R, o = (Rb, pb) if p < 0 else frames[p]
        R0, p0, a = J[j, 8:17].reshape(3, 3), J[j, 17:20], J[j, 20:23]
        Rc, oc = R @ R0 @ _axis_angle(a, x[j]), o + R @ p0
        frames.append((Rc, oc))
        com = com + Rc @ J[j, 5:8] + J[j, 4] * oc
    poses = []
    for k in range(nt):
        R, o = frames[int(T[k, 0])]
        poses.append(np.concatenate([o + R @ T[k, 1:4], (R @ T[k, 4:13].reshape(3, 3)).reshape(-1)]))
    return np.array(poses), com / M


def test_packed_table_equals_the_reference_walk(model, ref):
    rng = np.random.default_rng(0)
    for x in _draws(rng, 8):
        P, c = ref.fk(x)
        for i in range(x.shape[0]):
            p, cc = table_fk(model.table, x[i])
            scale = 1.0 + np.abs(x[i, 28:31]).max()
            np.testing.assert_allclose(p, P[i], atol=2e-6 * scale)
            np.testing.assert_allclose(cc, c[i], atol=2e-6 * scale)


def test_table_fields(model):
    t = model.table
    assert t[0] == 28 and t[1] == 4 and t[3] == 1                   # one branch frame: torso_2
    J = t[ti.HEADER:ti.HEADER + 28 * ti.JOINT_STRIDE].reshape(28, ti.JOINT_STRIDE)
    assert list(J[:, 3][J[:, 3] >= 0]) == [0, 1, 2, 3]               # the tips on arm_right_7, arm_left_7, leg_*_6
    assert [int(v) for v in np.where(J[:, 3] >= 0)[0]] == [8, 15, 21, 27]
    np.testing.assert_allclose(t[4] + J[:, 4].sum(), 87.042342, rtol=1e-6)
    np.testing.assert_array_equal(J[:, 23:25], model.limits.astype(np.float32))


def test_reference_equals_the_five_terms_written_out(ref):
    rng = np.random.default_rng(1)
    for x in _draws(rng, 16):
        poses, com = ref.fk(x)
        q = x[:, :28]
        lo, hi = ref.urdf.limits[:, 0], ref.urdf.limits[:, 1]
        lit = np.zeros(x.shape[0])
        for j in range(28):
            lit += log_ndtr((q[:, j] - lo[j]) / 0.05) + log_ndtr((hi[j] - q[:, j]) / 0.05)
        for k in range(2):
            d = com[:, k] - poses[:, 3, k]
            lit += log_ndtr((d + 0.14) / 0.01) + log_ndtr((0.14 - d) / 0.01)
        for tip, mu in ((2, [-0.02, -0.09, 0.]), (3, [-0.02, 0.09, 0.])):
            for i in range(12):
                target = mu[i] if i < 3 else float(np.eye(3).reshape(-1)[i - 3])
                sd = 0.02 if i < 3 else 0.1
                lit += -0.5 * ((poses[:, tip, i] - target) / sd) ** 2 - np.log(sd) - 0.5 * np.log(2 * np.pi)
        for i in range(3):
            lit += -0.5 * ((poses[:, 1, i] - ref.context[i]) / 0.02) ** 2 - np.log(0.02) - 0.5 * np.log(2 * np.pi)
        np.testing.assert_allclose(ref.log_density(x), lit, rtol=1e-12, atol=1e-9)


def test_reference_gradient_agrees_with_a_coarser_difference(ref):
    x = _draws(np.random.default_rng(2), 4)[0]
    _, g = ref.log_density_and_grad(x)
    _, g2 = ref.log_density_and_grad(x, rel_step=1e-5)
    np.testing.assert_allclose(g, g2, rtol=1e-5, atol=1e-5 * np.abs(g).max())


def test_log_phi_terms_stay_finite_far_outside_the_limits(ref):
    x = np.zeros((3, 34))
    x[0, :28] = ref.urdf.limits[:, 0] - 0.05 * 1e4            # z = -1e4 below every lower limit
    x[1, :28] = ref.urdf.limits[:, 1] + 0.05 * 1e4
    x[2, :28] = 1e3
    t = ref.terms(x)
    assert np.all(np.isfinite(t))
    assert np.all(t[0, :2] < -28 * 0.5e8 * 0.99)               # log Phi(-1e4) ~ -5e7 per joint


def test_names_and_defaults_resolve():
    from gmmvi_amd.configs import get_default_experiment_config
    from gmmvi_amd.experiments import setup_experiment as se
    assert se._lookup_target("Talos") == ("talos_ik", "make_talos_target", True)
    c = get_default_experiment_config("talos")
    assert c["environment_name"] == "Talos" and c["environment_config"] == {"context": [0.1, 0.5, 1.]}
    assert c["start_seed"] == 10000
    assert c["model_initialization"] == {"use_diagonal_covs": False, "num_initial_components": 1, "prior_mean": 0.,
                                         "prior_scale": 1., "initial_cov": 1.}
    assert c["gmmvi_runner_config"]["log_metrics_interval"] == 500
    assert c["use_sample_database"] is True and c["max_database_size"] == 500000 and c["temperature"] == 1.


def test_unknown_names_are_still_refused():
    from gmmvi_amd.experiments import setup_experiment as se
    with pytest.raises(ValueError, match="unknown experiment name") as e:
        se.get_target_lnpdf("MNIST", {}, 0)
    assert "Talos" in str(e.value)


def test_missing_dataset_directory_says_what_to_set(monkeypatch, tmp_path):
    monkeypatch.delenv(ti.DATASET_DIR_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="GMMVI_DATASET_DIR") as e:
        ti.resolve_urdf()
    assert "dataset_dir" in str(e.value) and "talos_reduced.urdf" in str(e.value)
    with pytest.raises(FileNotFoundError, match="talos_reduced.urdf"):
        ti.resolve_urdf(str(tmp_path))


def test_dataset_directory_from_environment(monkeypatch):
    monkeypatch.setenv(ti.DATASET_DIR_ENV, GOLDEN_DIR)
    assert ti.resolve_urdf() == os.path.join(GOLDEN_DIR, "talos_reduced.urdf")
    assert ti.resolve_urdf(GOLDEN_DIR) == URDF


def test_table_sizes_agree_with_the_wrappers():
    from gmmvi_amd import hip_ops
    assert ti.TABLE_SIZE == hip_ops.TALOS_TABLE_SIZE and ti.NUM_DIMENSIONS == hip_ops.TALOS_DIM == 34
