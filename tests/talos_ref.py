"""fp64 NumPy restatement of the Talos target ("Talos (defined, not reproduced)") on the fixture
tests/golden/talos_reduced.urdf.  It parses the URDF with its own code and walks the tree link by link with 4x4 transforms,
sample-batched; log Phi is scipy's log_ndtr and the gradient is a central difference.  It shares nothing with the product's
packed table.  ``TalosRef`` has the oracle's target interface (oracle/targets.py), so ``oracle.train.OracleGMMVI`` runs on it.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np
from scipy.special import log_ndtr

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
URDF = os.path.join(GOLDEN_DIR, "talos_reduced.urdf")
TIP_LINKS = ("gripper_right_base_link", "gripper_left_base_link", "right_sole_link", "left_sole_link")
LOG_2PI = np.log(2 * np.pi)
R_FOOT = np.array([-0.02, -0.09, 0., 1., 0., 0., 0., 1., 0., 0., 0., 1.])
L_FOOT = np.array([-0.02, 0.09, 0., 1., 0., 0., 0., 1., 0., 0., 0., 1.])
FOOT_STD = np.array([0.02] * 3 + [0.1] * 9)


def _nums(s, default="0 0 0"):
    return np.array([float(v) for v in (s if s is not None else default).split()])


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    o, z = np.ones_like(a), np.zeros_like(a)
    return np.stack([np.stack([o, z, z], -1), np.stack([z, c, -s], -1), np.stack([z, s, c], -1)], -2)


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    o, z = np.ones_like(a), np.zeros_like(a)
    return np.stack([np.stack([c, z, s], -1), np.stack([z, o, z], -1), np.stack([-s, z, c], -1)], -2)


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    o, z = np.ones_like(a), np.zeros_like(a)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def rpy(r, p, y):
    """Rz(y) Ry(p) Rx(r), batched over the leading axes."""
    return _rot_z(np.asarray(y, float)) @ _rot_y(np.asarray(p, float)) @ _rot_x(np.asarray(r, float))


def axis_angle(axis, q):
    """Rotation by q [N] about the unit axis: I + sin q [a]x + (1 - cos q) [a]x^2."""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    q = np.asarray(q, float)[:, None, None]
    return np.eye(3) + np.sin(q) * K + (1 - np.cos(q)) * (K @ K)


def _homog(R, p):
    T = np.zeros(R.shape[:-2] + (4, 4))
    T[..., :3, :3] = R
    T[..., :3, 3] = p
    T[..., 3, 3] = 1.0
    return T


class Urdf:
    """Links (mass, inertial xyz), joints (type, parent, child, origin 4x4, axis, limits) of the fixture."""

    def __init__(self, path=URDF):
        root = ET.parse(path).getroot()
        self.links = {}
        for l in root.iter("link"):
            inr = l.find("inertial")
            if inr is None:
                self.links[l.get("name")] = (0.0, np.zeros(3))
                continue
            o = inr.find("origin")
            self.links[l.get("name")] = (float(inr.find("mass").get("value")), _nums(None if o is None else o.get("xyz")))
        self.joints = {}
        for j in root.iter("joint"):
            o, a, lim = j.find("origin"), j.find("axis"), j.find("limit")
            xyz = _nums(None if o is None else o.get("xyz"))
            r = _nums(None if o is None else o.get("rpy"))
            self.joints[j.get("name")] = dict(
                type=j.get("type"), parent=j.find("parent").get("link"), child=j.find("child").get("link"),
                origin=_homog(rpy(r[0], r[1], r[2]), xyz), axis=_nums(None if a is None else a.get("xyz"), "1 0 0"),
                limit=None if lim is None else (float(lim.get("lower")), float(lim.get("upper"))))
        self.joint_to = {j["child"]: name for name, j in self.joints.items()}
        # the four paths, in order; joints and links at their first appearance
        self.path_joints, self.actuated, self.path_links = [], [], ["base_link"]
        for tip in TIP_LINKS:
            chain, link = [], tip
            while link != "base_link":
                chain.append(self.joint_to[link])
                link = self.joints[chain[-1]]["parent"]
            for name in reversed(chain):
                if name in self.path_joints:
                    continue
                self.path_joints.append(name)
                self.path_links.append(self.joints[name]["child"])
                if self.joints[name]["type"] == "revolute":
                    self.actuated.append(name)
        self.limits = np.array([self.joints[n]["limit"] for n in self.actuated])

    @property
    def total_mass(self):
        return sum(self.links[l][0] for l in self.path_links)


class TalosRef:
    def __init__(self, context, urdf=None):
        self.urdf = urdf if urdf is not None else Urdf()
        self.context = np.asarray(context, float)
        self.nq = len(self.urdf.actuated)

    def get_num_dimensions(self):
        return self.nq + 6

    def link_transforms(self, x):
        """{link: [N, 4, 4] world transform} for the links on the four paths."""
        x = np.atleast_2d(np.asarray(x, np.float64))
        q = x[:, :self.nq]
        T = {"base_link": _homog(rpy(x[:, -3], x[:, -2], x[:, -1]), x[:, self.nq:self.nq + 3])}
        idx = {n: i for i, n in enumerate(self.urdf.actuated)}
        for name in self.urdf.path_joints:
            j = self.urdf.joints[name]
            M = T[j["parent"]] @ j["origin"]
            if j["type"] == "revolute":
                M = M @ _homog(axis_angle(j["axis"], q[:, idx[name]]), np.zeros(3))
            T[j["child"]] = M
        return T

    def fk(self, x):
        """-> (poses [N, 4, 12] = [p, R row-major] per tip, centre of mass [N, 3])."""
        T = self.link_transforms(x)
        poses = np.stack([np.concatenate([T[l][:, :3, 3], T[l][:, :3, :3].reshape(-1, 9)], 1) for l in TIP_LINKS], 1)
        com = sum(self.urdf.links[l][0] * (T[l][:, :3, :3] @ self.urdf.links[l][1] + T[l][:, :3, 3])
                  for l in self.urdf.path_links) / self.urdf.total_mass
        return poses, com

    def terms(self, x):
        """The five terms [5, N]: joint limits, centre of mass, right foot, left foot, left gripper."""
        x = np.atleast_2d(np.asarray(x, np.float64))
        poses, com = self.fk(x)
        q = x[:, :self.nq]
        lo, hi = self.urdf.limits[:, 0], self.urdf.limits[:, 1]
        t1 = (log_ndtr((q - lo) / 0.05) + log_ndtr((hi - q) / 0.05)).sum(1)
        d = com[:, :2] - poses[:, 3, :2]
        t2 = (log_ndtr((d + 0.14) / 0.01) + log_ndtr((0.14 - d) / 0.01)).sum(1)

        def normal(y, mu, sd):
            return (-0.5 * ((y - mu) / sd) ** 2 - np.log(sd) - 0.5 * LOG_2PI).sum(1)
        t3 = normal(poses[:, 2], R_FOOT, FOOT_STD)
        t4 = normal(poses[:, 3], L_FOOT, FOOT_STD)
        t5 = normal(poses[:, 1, :3], self.context, 0.02)
        return np.stack([t1, t2, t3, t4, t5])

    def log_density(self, x):
        return self.terms(x).sum(0)

    def log_density_and_grad(self, x, rel_step=1e-6):
        x = np.atleast_2d(np.asarray(x, np.float64))
        lp = self.log_density(x)
        g = np.empty_like(x)
        for d in range(x.shape[1]):
            h = rel_step * (1.0 + np.abs(x[:, d]))
            e = np.zeros_like(x)
            e[:, d] = h
            g[:, d] = (self.log_density(x + e) - self.log_density(x - e)) / (2 * h)
        return lp, g
