"""Synthetic scenes for the box - box contact tests (tests/test_contact_boxbox_cpu.py, tests/test_gpu_contact_boxbox.py), built on
contact_box_scenes: the same following box torso and chains of dynamic box plates, now meeting each other, and pairs of two boxes turned so
that one kind of contact decides. Every case the GPU tests run is listed in _CASES and checked for conditioning and for contact activity
on the CPU (test_contact_boxbox_cpu.py: test_cases_are_well_conditioned_and_touch)."""
import numpy as np

import contact_box_scenes as bs
import contact_scenes as cs
from contact_box_scenes import BOX, FORMS, FREE, PARAMS, SHORT, Builder, pose, run_reference, turn_to_x, write_pmx  # noqa: F401
from contact_scenes import G_COLLIDER
from physics_scenes import _quat

PI = float(np.pi)
DYN = [0.3, 0.6, 0.3]                  # the dynamic box of the pair scenes (contact_scenes.Builder.chain: radius, height, radius)


def pair(order="fd", lock=False, **kw):
    """contact_box_scenes.pair with two boxes: "fd" a following box first, "df" the dynamic box first, "dd" both dynamic. lock: the
    dynamic box's joint allows no rotation, so it keeps the rotation it hangs at against the carrier (a pair of faces that stays as
    parallel as it was built: left free, two faces in contact turn parallel, which is the tie of 1b between the face axes A_i and B_i)."""
    if not lock:
        return bs.pair(1, 1, order, **kw)
    assert order == "fd"
    b = Builder(kw.get("seed", 61))
    mu = kw.get("mu", (0.5, 0.5))
    b.collider([0.0, -0.5, 0.0], 1, list(kw.get("box", BOX)), rot=kw["box_rot"], friction=mu[0])
    b.chain(kw["at"], [1], mask=FREE, friction=mu[1], rot=kw["dyn_rot"], radius=kw.get("radius", DYN[0]), height=kw.get("height", DYN[1]))
    b.joints[-1].update(rotation_min=[0.0, 0.0, 0.0], rotation_max=[0.0, 0.0, 0.0])
    return b.scene(64)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


# rotations of the dynamic box (it hangs at +x of the following one and is pushed towards -x)
VERTEX = turn_to_x([-DYN[0], -DYN[1], -DYN[2]])                          # its (-, -, -) corner towards -x: a vertex on the other's +x face
EDGE_UP = _quat([0, 1, 0], PI / 4)                                       # a vertical edge towards -x, parallel to the other's +x face
EDGE_FLAT = qmul(_quat([1, 0, 0], 0.1), _quat([0, 0, 1], PI / 4))        # a horizontal edge (along z, tipped by 0.1) towards -x
NEAR = _quat([0, 1, 0], 5e-4)                                            # 5e-4 rad off parallel: 1 - C_00^2 = 2.5e-7 < 1e-6


def with_box_pair(apart=False):
    return bs.with_box_pair(apart=apart)


# the dynamic plate DYN against the following box BOX at the origin, unturned: (where the plate's centre is, its rotation's axis and angle)
# — found by a seeded search over 400 000 placements as those with one overlap of the fifteen below -0.03 and every other above 0.03
_SINGLE = {"A": ([0.973, -0.421, 0.495], [-0.47, 0.84, 0.27], 0.55),         # separated along A's axis 0
           "B": ([-0.716, 0.977, -0.513], [0.82, -0.55, -0.15], 1.20),       # along B's axis 0
           "edge": ([-0.94, -0.606, 0.108], [-0.02, -0.79, -0.61], -1.02)}   # along a_2 x b_1


def single_axis(kind, apart=False, seed=81):
    """a following box and a dynamic box plate on a joint that allows no rotation, overlapping along every axis but one, of the kind given
    — "A" a face axis of the lower index, "B" one of the higher, "edge" an edge pair: the search must find them separated. apart: the
    plate's mask names an empty group, so the pair does not exist. A sphere on a chain of its own rests against the following box, so
    that contacts are active. Run under single_axis_poses (the carrier stays where it is)."""
    at, axis, ang = _SINGLE[kind]
    b = Builder(seed)
    b.collider([0.0, -0.5, 0.0], 1, list(BOX))
    b.chain([0.62, 0, 0.3], [0], mask=FREE)
    b.chain(at, [1], mask=(1 << 9) if apart else (1 << G_COLLIDER), rot=_quat(axis, ang))
    b.joints[-1].update(rotation_min=[0.0, 0.0, 0.0], rotation_max=[0.0, 0.0, 0.0])
    return b.scene(64)


def single_axis_poses(sc):
    return [pose(sc, k, 0.0, 0.0) for k in range(len(SHORT))]


# name: (scene, pose amount, calls[, how far the carrier turns: contact_scenes.pose's `turn`, 0.05 unless given])
_CASES = {
    # the four instantiations: the plates of contact_box_scenes' strands and rings now meet the box torso
    "own 64": (lambda: bs.strands(6, 3, 71), 0.5, SHORT),
    "stride 64": (lambda: bs.strands(8, 4, 72, cross=True, tie=True), 0.5, SHORT),
    "own 256": (lambda: bs.strands(16, 4, 73, ring_radius=1.7, n_verts=160), 0.6, SHORT),
    "stride 256": (lambda: bs.rings(9, 29, 74), 0.5, SHORT),
    # the roles
    "box box fd": (lambda: pair("fd"), 0.3, SHORT),
    "box box df": (lambda: pair("df"), 0.3, SHORT),
    "box box dd": (lambda: pair("dd"), 0.3, SHORT),
    # the kinds of contact
    "vertex on a face of A": (lambda: pair("fd", box_rot=_quat([0, 1, 0], 0.05), dyn_rot=VERTEX, at=[1.16, 0, 0.05]), 0.3, SHORT),
    "vertex on a face of B": (lambda: pair("df", box_rot=_quat([0, 1, 0], 0.05), dyn_rot=VERTEX, at=[1.16, 0, 0.05]), 0.3, SHORT),
    "edge on a face": (lambda: pair("fd", box_rot=_quat([0, 1, 0], 0.05), dyn_rot=EDGE_UP, at=[0.9, 0, 0.05]), 0.3, SHORT),
    "edge on edge": (lambda: pair("fd", box_rot=bs.EDGE, dyn_rot=EDGE_FLAT, at=[1.25, 0, 0.02]), 0.3, SHORT),
    "face on face": (lambda: pair("fd", lock=True, box_rot=(0, 0, 0, 1), dyn_rot=_quat([0, 1, 0], 0.02), at=[0.78, 0, 0.05], box=[0.4, 0.9, 0.6]), 0.3, SHORT),
    "wide over narrow": (lambda: pair("fd", lock=True, box_rot=(0, 0, 0, 1), dyn_rot=_quat([0.13, 0.12, -0.98], -0.2), at=[1.08, 0.27, 0.68], box=[0.4, 0.2, 0.4], radius=0.5), 0.3, SHORT, 0.0),
    "near parallel": (lambda: pair("fd", lock=True, mu=(0.0, 0.5), box_rot=(0, 0, 0, 1), dyn_rot=NEAR, at=[0.78, 0, 0.05], box=[0.4, 0.9, 0.6]), 0.3, SHORT, 0.0),
    # friction: 0 on one box (the stage is skipped), and 1 against a following box (previous pose = current pose)
    "friction zero": (lambda: pair("fd", mu=(0.0, 0.8), box_rot=_quat([0, 1, 0], 0.05), dyn_rot=VERTEX, at=[1.16, 0, 0.05]), 0.3, SHORT),
    "friction follow": (lambda: pair("fd", mu=(1.0, 1.0), box_rot=_quat([0, 1, 0], 0.05), dyn_rot=VERTEX, at=[1.16, 0, 0.05]), 0.3, SHORT),
    "params": (lambda: bs.strands(6, 3, 76, **PARAMS), 0.5, SHORT),
}
# what a case is there for: a predicate over Sim.kinds' keys (which box's face or "edge", the axis, coordinates moved by the footprint clamp)
KINDS = {
    "vertex on a face of A": lambda k: k[0] == "A",
    "vertex on a face of B": lambda k: k[0] == "B",
    "edge on a face": lambda k: k[0] in "AB",
    "edge on edge": lambda k: k[0] == "edge",
    "face on face": lambda k: k[0] in "AB",
    "wide over narrow": lambda k: k[0] in "AB" and k[2] > 0,
    "near parallel": lambda k: k[0] in "AB",
}
CROWD = "own 64"
_cases = cs.Cases(_CASES, 3)
case, reference, conditioning, node_conditioning, sim_of = _cases.case, _cases.reference, _cases.conditioning, _cases.node_conditioning, _cases.sim_of
node_case = bs.node_case                    # (the same scene under either Cases: 'own 64' of the same builder)


def limit_table(n_follow):
    """256 dynamic boxes x n_follow following boxes, all in each other's masks: 256 n_follow follow entries, every one a pair of two boxes"""
    return cs.limit_table(n_follow, dyn_shape=1, fol_shape=1)
