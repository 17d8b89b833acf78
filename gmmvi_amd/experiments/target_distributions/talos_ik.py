"""Talos humanoid inverse kinematics (reference: src/gmmvi/experiments/target_distributions/talos_ik.py:16-194).

Upstream builds this target on a fork of tf_robot_learning that is not vendored; this build defines the density instead
("Talos (defined, not reproduced)").  x in R^34 is 28 joint angles, the world position p_b of ``base_link``
and its roll, pitch, yaw (R_b = Rz Ry Rx).  Four chains leave ``base_link`` (r_gripper, l_gripper, r_foot, l_foot); the
actuated joints are the 28 revolute joints on them, in walk order.  The log density is the sum of
    joint limits    sum_j log Phi((q_j - lo_j) / 0.05) + log Phi((hi_j - q_j) / 0.05)
    centre of mass  sum_{k in x, y} log Phi((d_k + 0.14) / 0.01) + log Phi((0.14 - d_k) / 0.01),  d = c_xy - p_lfoot,xy
    right foot      log N(pose12(r_foot); [-0.02, -0.09, 0, I], diag([0.02]*3 + [0.1]*9)^2)
    left foot       the same around [-0.02, 0.09, 0, I]
    left gripper    log N(p(l_gripper); context, 0.02^2 I)
with c the mass-weighted mean of the <inertial> origins of the 37 links on the four paths.

The robot description is read from ``talos_reduced.urdf`` in ``dataset_dir`` (``environment_config["dataset_dir"]``), else
in the directory named by GMMVI_DATASET_DIR.  ``parse_urdf`` reads it with xml.etree only; ``TalosModel`` folds the fixed
joints into the revolute joints' origins and lumps every link's mass onto the frame that carries it, into the flat f32
table csrc/talos.hip walks (layout below).
"""
import os
import xml.etree.ElementTree as ET

import numpy as np

from ... import _lib, hip_ops
from ...device import get_context
from .lnpdf import LNPDF

URDF_FILE = "talos_reduced.urdf"
DATASET_DIR_ENV = "GMMVI_DATASET_DIR"
BASE_LINK = "base_link"
TIPS = (("r_gripper", "gripper_right_base_link"), ("l_gripper", "gripper_left_base_link"),
        ("r_foot", "right_sole_link"), ("l_foot", "left_sole_link"))       # talos_ik.py:57-62, walk order
NUM_JOINTS, NUM_TIPS = 28, len(TIPS)
NUM_DIMENSIONS = NUM_JOINTS + 6
JOINT_LIMIT_STD = 0.05                                                   # talos_ik.py:103-105
COM_LIMIT, COM_LIMIT_STD = 0.14, 0.01                                    # :129-131
FOOT_STD = np.array([0.02] * 3 + [0.1] * 9)                              # :119, :124
RIGHT_FOOT_TARGET = np.array([-0.02, -0.09, 0., 1., 0., 0., 0., 1., 0., 0., 0., 1.])   # :37-38
LEFT_FOOT_TARGET = np.array([-0.02, 0.09, 0., 1., 0., 0., 0., 1., 0., 0., 0., 1.])
GRIPPER_STD = 0.02                                                       # :114

# the packed table (f32): header, NUM_JOINTS joint records, NUM_TIPS tip records
#   header [8]:  NJ, NT, total mass, slots used, base mass m_0, base mass moment s_0 (3, in the base frame)
#   joint [28]:  parent joint (-1: base), parent source (-1: base, -2: the previous joint, k >= 0: saved slot k), slot this
#                frame is saved to (-1: none), tip attached (-1: none), lumped mass M_j, mass moment S_j (3, in the joint's
#                frame), origin rotation (9, row-major) and translation (3) from the parent frame with the fixed joints
#                between folded in, unit axis (3), lower and upper limit, 3 unused
#   tip [16]:    carrying joint, offset translation (3) and rotation (9, row-major), 3 unused
HEADER, JOINT_STRIDE, TIP_STRIDE = 8, 28, 16
TABLE_SIZE = HEADER + NUM_JOINTS * JOINT_STRIDE + NUM_TIPS * TIP_STRIDE
MAX_SLOTS = 2                                                            # saved branch frames the kernel keeps
assert TABLE_SIZE == hip_ops.TALOS_TABLE_SIZE and NUM_DIMENSIONS == hip_ops.TALOS_DIM


def _vec(text, n=3):
    if text is None:
        return np.zeros(n)
    v = np.array([float(t) for t in text.split()])
    if v.shape != (n,):
        raise ValueError(f"expected {n} numbers, got {text!r}")
    return v


def rpy_matrix(rpy):
    """URDF convention: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _transform(xyz, rpy):
    T = np.eye(4)
    T[:3, :3] = rpy_matrix(rpy)
    T[:3, 3] = xyz
    return T


def parse_urdf(path):
    """-> (links {name: (mass, inertial origin xyz)}, joints {name: dict(type, parent, child, xyz, rpy, axis, lower,
    upper)}).  Links without <inertial> have mass 0; a missing <origin> is the identity, a missing <axis> is x."""
    root = ET.parse(path).getroot()
    links = {}
    for link in root.findall("link"):
        inertial = link.find("inertial")
        mass, com = 0.0, np.zeros(3)
        if inertial is not None:
            m = inertial.find("mass")
            mass = float(m.get("value")) if m is not None else 0.0
            o = inertial.find("origin")
            com = _vec(o.get("xyz") if o is not None else None)
        links[link.get("name")] = (mass, com)
    joints = {}
    for joint in root.findall("joint"):
        o, a, lim = joint.find("origin"), joint.find("axis"), joint.find("limit")
        joints[joint.get("name")] = {
            "type": joint.get("type"), "parent": joint.find("parent").get("link"), "child": joint.find("child").get("link"),
            "xyz": _vec(o.get("xyz") if o is not None else None), "rpy": _vec(o.get("rpy") if o is not None else None),
            "axis": _vec(a.get("xyz")) if a is not None else np.array([1., 0., 0.]),
            "lower": float(lim.get("lower", 0.0)) if lim is not None else 0.0,
            "upper": float(lim.get("upper", 0.0)) if lim is not None else 0.0}
    return links, joints


class TalosModel:
    """The kinematic tree of the four chains: joint order, limits, path links and the packed device table."""

    def __init__(self, path):
        links, joints = parse_urdf(path)
        by_child = {j["child"]: name for name, j in joints.items()}
        chains = []
        for tip_name, tip_link in TIPS:
            path_j, link = [], tip_link
            while link != BASE_LINK:
                if link not in by_child:
                    raise ValueError(f"{path}: no joint path from {BASE_LINK} to {tip_link}")
                name = by_child[link]
                path_j.append(name)
                link = joints[name]["parent"]
            chains.append(path_j[::-1])
        # walk: every link's carrier (-1 base, else revolute joint index) and its transform from the carrier's frame
        carrier = {BASE_LINK: (-1, np.eye(4))}
        self.joint_names, self.path_links = [], [BASE_LINK]
        parent, origin, axis, lo, hi = [], [], [], [], []
        for path_j in chains:
            for name in path_j:
                j = joints[name]
                if j["child"] in carrier:
                    continue
                c, T = carrier[j["parent"]]
                T = T @ _transform(j["xyz"], j["rpy"])
                if j["type"] == "revolute":
                    n = np.linalg.norm(j["axis"])
                    if not n > 0:
                        raise ValueError(f"{path}: joint {name} has a zero axis")
                    parent.append(c)
                    origin.append(T)
                    axis.append(j["axis"] / n)
                    lo.append(j["lower"])
                    hi.append(j["upper"])
                    carrier[j["child"]] = (len(self.joint_names), np.eye(4))
                    self.joint_names.append(name)
                elif j["type"] == "fixed":
                    carrier[j["child"]] = (c, T)
                else:
                    raise ValueError(f"{path}: joint {name} of type {j['type']} is not supported")
                self.path_links.append(j["child"])
        if len(self.joint_names) != NUM_JOINTS:
            raise ValueError(f"{path}: {len(self.joint_names)} actuated joints on the four chains, expected {NUM_JOINTS}")
        self.parent = np.array(parent, np.int64)
        self.origins = np.array(origin)
        self.axes = np.array(axis)
        self.limits = np.stack([lo, hi], axis=1)
        self.link_masses = {name: links[name][0] for name in self.path_links}
        self.total_mass = float(sum(self.link_masses.values()))
        # masses lumped per frame: index 0 the base, j + 1 joint j
        mass = np.zeros(NUM_JOINTS + 1)
        moment = np.zeros((NUM_JOINTS + 1, 3))
        for name in self.path_links:
            m, com = links[name]
            c, T = carrier[name]
            mass[c + 1] += m
            moment[c + 1] += m * (T[:3, :3] @ com + T[:3, 3])
        self.frame_mass, self.frame_moment = mass, moment
        self.tip_carrier = np.array([carrier[link][0] for _, link in TIPS], np.int64)
        self.tip_offsets = np.array([carrier[link][1] for _, link in TIPS])
        self.table = self._pack()

    def _pack(self):
        """The flat f32 table of csrc/talos.hip.  The kernel walks the joints in order; a joint's parent frame is the base,
        the previous joint's frame or a saved branch frame, and walking back it steps from a joint's frame to its parent's
        or jumps to the frame stored for a tip, so every joint that is not followed by its child must carry a tip."""
        children = [[] for _ in range(NUM_JOINTS)]
        for j, p in enumerate(self.parent):
            if p >= 0:
                children[p].append(j)
        slot = -np.ones(NUM_JOINTS, np.int64)
        for j in range(NUM_JOINTS):
            if len(children[j]) > 1 or (len(children[j]) == 1 and children[j][0] != j + 1):
                slot[j] = slot.max() + 1
        if slot.max() + 1 > MAX_SLOTS:
            raise ValueError(f"the tree has {slot.max() + 1} branch frames; the kernel keeps {MAX_SLOTS}")
        tip_of = -np.ones(NUM_JOINTS, np.int64)
        for t, c in enumerate(self.tip_carrier):
            if c < 0 or tip_of[c] >= 0 or children[c]:
                raise ValueError("every tip must sit on a leaf joint of its own")
            tip_of[c] = t
        if list(np.sort(self.tip_carrier)) != list(self.tip_carrier):
            raise ValueError("the tips must come in walk order")
        if tip_of[NUM_JOINTS - 1] != NUM_TIPS - 1:
            raise ValueError("the last joint of the walk must carry the last tip")
        for j in range(NUM_JOINTS - 1):
            if self.parent[j + 1] != j and tip_of[j] < 0:
                raise ValueError(f"joint {self.joint_names[j]} is followed by a joint of another branch but carries no tip")
        t = np.zeros(TABLE_SIZE)
        t[0:8] = [NUM_JOINTS, NUM_TIPS, self.total_mass, slot.max() + 1, self.frame_mass[0], *self.frame_moment[0]]
        for j in range(NUM_JOINTS):
            r = t[HEADER + j * JOINT_STRIDE:HEADER + (j + 1) * JOINT_STRIDE]
            p = self.parent[j]
            src = -1 if p < 0 else (slot[p] if slot[p] >= 0 else -2)
            r[0:4] = [p, src, slot[j], tip_of[j]]
            r[4] = self.frame_mass[j + 1]
            r[5:8] = self.frame_moment[j + 1]
            r[8:17] = self.origins[j][:3, :3].reshape(-1)
            r[17:20] = self.origins[j][:3, 3]
            r[20:23] = self.axes[j]
            r[23:25] = self.limits[j]
        base = HEADER + NUM_JOINTS * JOINT_STRIDE
        for k in range(NUM_TIPS):
            r = t[base + k * TIP_STRIDE:base + (k + 1) * TIP_STRIDE]
            r[0] = self.tip_carrier[k]
            r[1:4] = self.tip_offsets[k][:3, 3]
            r[4:13] = self.tip_offsets[k][:3, :3].reshape(-1)
        return t.astype(np.float32)


def resolve_urdf(dataset_dir=None):
    d = dataset_dir if dataset_dir is not None else os.environ.get(DATASET_DIR_ENV)
    if not d:
        raise FileNotFoundError(
            f"no dataset directory for the Talos target: set environment_config['dataset_dir'] or the {DATASET_DIR_ENV} "
            f"environment variable to a directory holding {URDF_FILE}")
    path = os.path.join(d, URDF_FILE)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} does not exist: the dataset directory (environment_config['dataset_dir'] or "
                                f"{DATASET_DIR_ENV}) must hold {URDF_FILE}")
    return path


class Talos(LNPDF):
    """The Talos inverse-kinematics target, D = 34, with the left gripper's goal ``context`` (x, y, z)."""

    def __init__(self, context, dataset_dir=None):
        super().__init__(use_log_density_and_grad=True)
        context = np.asarray(context, np.float64)
        if context.shape != (3,) or not np.all(np.isfinite(context)):
            raise ValueError(f"context must be three finite numbers (the left gripper's goal), got {context!r}")
        self.context = context
        self.model = TalosModel(resolve_urdf(dataset_dir))
        self.ctx = get_context()
        self._table_dev = self.ctx.asarray(self.model.table)
        self._context_dev = self.ctx.asarray(context.astype(np.float32))

    @property
    def joint_names(self):
        return list(self.model.joint_names)

    @property
    def joint_limits(self):
        """[28, 2] (lower, upper) as the URDF gives them."""
        return self.model.limits.copy()

    def get_num_dimensions(self):
        return NUM_DIMENSIONS

    def _fast_path_target(self):
        """Descriptor for the single-call iteration (optimization/fused.py) and the phased sharded one (sharded.py)."""
        return _lib.TargetSpec(kind=4, talos_model=self._table_dev.ptr, talos_context=self._context_dev.ptr)

    def log_density(self, x):
        return hip_ops.target_talos(self.ctx, self._table_dev, self._context_dev, self.ctx.asarray(x), want_grad=False)[0]

    def log_density_and_grad(self, x):
        return hip_ops.target_talos(self.ctx, self._table_dev, self._context_dev, self.ctx.asarray(x), want_grad=True)

    def forward_kinematics(self, x):
        """-> (poses [N, 4, 12]: per tip [p (3), R row-major (9)] in the world frame, centre of mass [N, 3]), NumPy f32."""
        poses, com = hip_ops.talos_fk(self.ctx, self._table_dev, self.ctx.asarray(x))
        return poses.numpy(), com.numpy()

    def expensive_metrics(self, model, samples) -> dict:
        """Numbers in place of upstream's plot (talos_ik.py:151-156): over the given samples, the mean distance of the left
        gripper to ``context``, the mean distance of the feet to their targets and the fraction inside all joint limits."""
        x = np.asarray(samples.numpy() if hasattr(samples, "numpy") else samples, np.float32)
        if x.shape[0] == 0:
            return {}
        poses, _ = self.forward_kinematics(x)
        grip = np.linalg.norm(poses[:, 1, :3] - self.context[None], axis=1)
        feet = 0.5 * (np.linalg.norm(poses[:, 2, :3] - RIGHT_FOOT_TARGET[None, :3], axis=1)
                      + np.linalg.norm(poses[:, 3, :3] - LEFT_FOOT_TARGET[None, :3], axis=1))
        q = x[:, :NUM_JOINTS]
        inside = np.all((q >= self.model.limits[:, 0]) & (q <= self.model.limits[:, 1]), axis=1)
        return {"left_gripper_error": float(grip.mean()), "foot_position_error": float(feet.mean()),
                "fraction_within_joint_limits": float(inside.mean())}


def make_talos_target(context, dataset_dir=None):
    """talos_ik.py:200-211 (the unused TalosLeftGripperTargetPdf is left out)."""
    return Talos(context, dataset_dir=dataset_dir)
