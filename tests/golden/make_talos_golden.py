"""Generates tests/golden/talos_reduced.urdf: a trimmed copy of upstream's robot description
(src/gmmvi/experiments/target_distributions/datasets/talos_reduced.urdf) for the Talos target.  Data only.  Kept: every
<link> with its <inertial> origin and mass, every <joint> with its type, parent, child, origin, axis and limit.  Dropped:
gazebo, transmission, material, visual, collision and the inertia tensors (the target needs none of them).  Run:
    python tests/golden/make_talos_golden.py UPSTREAM_URDF
"""
import os
import sys
import xml.etree.ElementTree as ET

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "talos_reduced.urdf")
LIMIT_KEYS = ("lower", "upper")


def _copy(src, dst_parent, tag, keys):
    if src is None:
        return None
    return ET.SubElement(dst_parent, tag, {k: src.get(k) for k in keys if src.get(k) is not None})


def trim(root):
    out = ET.Element("robot", {"name": root.get("name", "talos")})
    for link in root.findall("link"):
        lo = ET.SubElement(out, "link", {"name": link.get("name")})
        inertial = link.find("inertial")
        if inertial is not None:
            io = ET.SubElement(lo, "inertial")
            _copy(inertial.find("origin"), io, "origin", ("xyz", "rpy"))
            _copy(inertial.find("mass"), io, "mass", ("value",))
    for joint in root.findall("joint"):
        jo = ET.SubElement(out, "joint", {"name": joint.get("name"), "type": joint.get("type")})
        _copy(joint.find("parent"), jo, "parent", ("link",))
        _copy(joint.find("child"), jo, "child", ("link",))
        _copy(joint.find("origin"), jo, "origin", ("xyz", "rpy"))
        _copy(joint.find("axis"), jo, "axis", ("xyz",))
        _copy(joint.find("limit"), jo, "limit", LIMIT_KEYS)
    return out


def main(src):
    out = trim(ET.parse(src).getroot())
    ET.indent(out, space="  ")
    ET.ElementTree(out).write(OUT, encoding="utf-8", xml_declaration=True)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(out.findall('link'))} links, {len(out.findall('joint'))} joints")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_talos_golden.py UPSTREAM_URDF")
    main(sys.argv[1])
