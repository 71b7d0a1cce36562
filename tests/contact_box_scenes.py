"""Synthetic scenes for the box contact tests (tests/test_contact_box_cpu.py, tests/test_gpu_contact_boxes.py), built on
contact_scenes.Builder: following boxes on the colliders' bone, chains of dynamic box plates, capsules and spheres on the carrier the poses
move. Every case the GPU tests run is listed in _CASES and checked for conditioning and for contact activity on the CPU
(test_contact_box_cpu.py: test_cases_are_well_conditioned_and_touch)."""
import numpy as np

import contact_scenes as cs
from contact_scenes import ALL, FORMS, G_CHAIN, G_COLLIDER, PARAMS, SHORT, Builder, pose, ring, run_reference, write_pmx  # noqa: F401
from physics_scenes import _quat

PI = float(np.pi)
FREE = ALL & ~(1 << G_CHAIN)          # a chain that meets the colliders only
BOX = [0.4, 0.6, 0.4]                 # the following box of the pair scenes: half extents


def turn_to_x(v):
    """the rotation that turns direction v onto +x"""
    v = np.asarray(v, dtype=np.float64) / np.linalg.norm(v)
    axis = np.cross(v, [1.0, 0.0, 0.0])
    return _quat(axis, float(np.arccos(np.clip(v[0], -1, 1))))


def box_torso(b, half=(0.8, 2.05, 0.8)):
    """the colliders of the base scene: an upright following box under the carrier's height and a shoulder sphere beside it"""
    b.collider([0, -1.5, 0], 1, list(half), rot=_quat([0.1, 1, 0.05], 0.3))
    b.collider([0.9, -0.4, 0], 0, [0.5, 0, 0])


def plates(s, n_dyn):
    """a chain's shapes: every other body a box plate, capsules and spheres between them"""
    return [1 if (s + k) % 2 == 0 else (2, 0)[((s + k) // 2) % 2] for k in range(n_dyn)]


def strands(n_strands, n_dyn, seed, ring_radius=1.45, cross=False, tie=False, n_verts=96, **kw):
    """contact_scenes.strands around a following box: the chains meet the colliders only (follow entries: a round body against the box
    torso, a box plate against the shoulder sphere; a plate and the torso are a pair of two boxes, counted and left out)"""
    b = Builder(seed)
    box_torso(b)
    at = ring(n_strands, ring_radius)
    ch = [b.chain(at[s], plates(s, n_dyn), mask=FREE) for s in range(n_strands)]
    if cross:
        for s in range(n_strands):
            for k in range(n_dyn):
                b.loose_joint(ch[s][k], ch[(s + 1) % n_strands][k], (at[s] + at[(s + 1) % n_strands]) / 2 + [0, -k - 0.5, 0])
    if tie:
        b.loose_joint(ch[0][-1], ch[2][-1], (at[0] + at[2]) / 2 + [0, -n_dyn + 0.5, 0], play=0.8)
    return b.scene(n_verts, **kw)


def rings(n_rings, per_ring, seed, n_verts=600):
    """contact_scenes.rings around one tall following box and a tall capsule behind it: one dynamic body per chain, spheres and small box
    plates in turn (a sphere has the box and the capsule as partners, a plate the capsule)"""
    b = Builder(seed)
    b.collider([0, -0.5 * n_rings, 0], 1, [0.9, 0.5 * n_rings + 1, 0.9], rot=_quat([0, 1, 0], 0.2))
    b.collider([-0.2, -0.5 * n_rings, 0], 2, [1.0, 1.0 * n_rings + 2, 0])
    for r in range(n_rings):
        for k, at in enumerate(ring(per_ring, 1.5, phase=0.1 * r)):
            b.chain(at + [0, -0.8 * r, 0], [(k + r) % 2], mask=FREE, radius=0.12, height=0.1, spacing=0.6)
    return b.scene(n_verts)


def pair(first, second, order="fd", mu=(0.5, 0.5), seed=61, box_rot=None, dyn_rot=None, at=None, box=BOX, radius=0.3, height=0.6):
    """contact_scenes.shape_pair with a box among the two: `first` gets the lower index. "fd": a following `first` at the colliders' origin
    and a dynamic `second` beside it; "df": the dynamic body first; "dd": both dynamic side by side behind a following sphere that stops
    the first so the second runs into it. box_rot / dyn_rot / at: the following body's rotation, the dynamic body's, and where its chain
    hangs."""
    b = Builder(seed)
    if order == "dd":
        b.collider([0.0, -0.5, 0.0], 0, [0.4, 0, 0])
        b.chain([0.73, 0, 0], [first], friction=mu[0], radius=radius, height=height)
        b.chain([1.36, 0, 0.05], [second], friction=mu[1], radius=radius, height=height)
        return b.scene(64)
    dyn, fol = (second, first) if order == "fd" else (first, second)
    size = list(box) if fol == 1 else [0.4, 1.2, 0]
    rot = box_rot if box_rot is not None else _quat([0.2, 1, 0.1], 0.15)
    place = lambda: b.collider([0.0, -0.5, 0.0], fol, size, rot=rot, friction=mu[0 if order == "fd" else 1])
    if order == "fd":
        place()
    b.chain([0.74, 0, 0.1] if at is None else at, [dyn], mask=FREE, friction=mu[1 if order == "fd" else 0], rot=dyn_rot, radius=radius, height=height)
    if order == "df":
        place()
    return b.scene(64)


EDGE = _quat([0, 1, 0], PI / 4)                                        # the box's vertical edge towards +x, 0.4 sqrt(2) = 0.566 away
CORNER = turn_to_x(BOX)                                                 # its (+, +, +) corner towards +x, |BOX| = 0.825 away
EDGE_Z = _quat([0, 0.03, 1], PI / 4)                                    # [0.4, 0.4, 0.8]: a horizontal edge (along z) towards +x
LYING = _quat([0, 0.05, 1], PI / 2)                                     # a capsule along x
TILTED = _quat([0.05, 0, 1], 0.3)                                       # a capsule 0.3 rad off the box's +x face


def deep(seed=62):
    """a sphere whose centre the reset places inside a following box, 0.08 under its +x face (the other faces are 0.7 and more away: the
    smallest half extent is 0.8, so a tie is 0.6 and more away, 0.16 is asked for). Not a smaller sphere: with 0.4 m r^2 of inertia
    friction spins a sphere of radius 0.15 so fast after the push that the float32 probe's rotations stray 4e-5."""
    b = Builder(seed)
    b.collider([0.0, -0.5, 0.0], 1, [0.8, 0.9, 0.8])
    b.chain([0.72, 0, 0.1], [0], mask=FREE, radius=0.3, spacing=1.0)
    return b.scene(64)


def with_box_pair(apart=False, seed=63):
    """the 'box sphere fd' scene and one more dynamic box plate whose only partner by the masks is the following box: a pair of two
    boxes, counted and left out. apart: the plate's mask names an empty group instead, so the pair does not exist at all."""
    b = Builder(seed)
    b.collider([0.0, -0.5, 0.0], 1, list(BOX), rot=_quat([0.2, 1, 0.1], 0.15))
    b.chain([0.74, 0, 0.1], [0], mask=FREE)
    b.chain([0.5, 0, 0.3], [1], mask=(1 << 9) if apart else (1 << G_COLLIDER))
    return b.scene(64)


def no_boxes(seed=51):
    """a table without any box: contact_scenes' own chains"""
    return cs.strands(6, 3, seed)


def far_boxes(seed=64):
    """box candidates exist and never come within reach (the chains hang far from the box torso); the round bodies meet the shoulder
    sphere's group as well"""
    b = Builder(seed)
    box_torso(b)
    for s, at in enumerate(ring(4, 4.5)):
        b.chain(at, plates(s, 2), mask=FREE)
    return b.scene(64)


def masked_boxes(sc):
    """the same scene with the mask of every box 0"""
    t = dict(sc["table"])
    t["mask"] = np.where(np.asarray(t["shape"]) == 1, 0, t["mask"]).astype(t["mask"].dtype)
    return dict(sc, table=t)


# name: (scene, pose amount, calls)
_CASES = {
    # the four instantiations with boxes on
    "own 64": (lambda: strands(6, 3, 71), 0.5, SHORT),
    "stride 64": (lambda: strands(8, 4, 72, cross=True, tie=True), 0.5, SHORT),
    "own 256": (lambda: strands(16, 4, 73, ring_radius=1.7, n_verts=160), 0.6, SHORT),
    "stride 256": (lambda: rings(9, 29, 74), 0.5, SHORT),
    # shape pairs: following body first / dynamic body first / both dynamic
    "sphere box fd": (lambda: pair(0, 1), 0.3, SHORT),
    "sphere box df": (lambda: pair(0, 1, "df"), 0.3, SHORT),
    "sphere box dd": (lambda: pair(0, 1, "dd"), 0.3, SHORT),
    "box sphere fd": (lambda: pair(1, 0), 0.3, SHORT),
    "box sphere df": (lambda: pair(1, 0, "df"), 0.3, SHORT),
    "box sphere dd": (lambda: pair(1, 0, "dd"), 0.3, SHORT),
    "capsule box fd": (lambda: pair(2, 1), 0.3, SHORT),
    "capsule box df": (lambda: pair(2, 1, "df"), 0.3, SHORT),
    "capsule box dd": (lambda: pair(2, 1, "dd"), 0.3, SHORT),
    "box capsule fd": (lambda: pair(1, 2), 0.3, SHORT),
    "box capsule df": (lambda: pair(1, 2, "df"), 0.3, SHORT),
    "box capsule dd": (lambda: pair(1, 2, "dd"), 0.3, SHORT),
    # regions of the box
    "sphere face": (lambda: pair(1, 0, box_rot=_quat([0, 1, 0], 0.05)), 0.3, SHORT),
    "sphere edge": (lambda: pair(1, 0, box_rot=EDGE, at=[0.9, 0, 0.0]), 0.3, SHORT),
    "sphere corner": (lambda: pair(1, 0, box_rot=CORNER, at=[1.16, 0, 0.0]), 0.3, SHORT),
    "capsule end on": (lambda: pair(1, 2, dyn_rot=LYING, at=[1.04, 0, 0.05]), 0.3, SHORT),
    "capsule across edge": (lambda: pair(1, 2, box_rot=EDGE_Z, box=[0.4, 0.4, 0.8], dyn_rot=_quat([1, 0, 0.1], 0.1), at=[0.9, 0, 0.0]), 0.3, SHORT),
    "capsule tilted": (lambda: pair(1, 2, box_rot=_quat([0, 1, 0], 0.02), dyn_rot=TILTED, at=[0.84, 0, 0.05]), 0.3, SHORT),
    "deep": (lambda: deep(), 0.3, SHORT),
    # friction: 0 on the box (the stage is skipped), and 1 against a following box (previous pose = current pose)
    "friction zero": (lambda: pair(1, 2, mu=(0.0, 0.8)), 0.3, SHORT),
    "friction follow": (lambda: pair(1, 2, mu=(1.0, 1.0)), 0.3, SHORT),
    "box pair": (lambda: with_box_pair(), 0.3, SHORT),
    "params": (lambda: strands(6, 3, 76, **PARAMS), 0.5, SHORT),
}
# the region a case is there for: (clamped coordinates of the closest point, whether the bisection decides s)
REGIONS = {"sphere face": (1, False), "sphere edge": (2, False), "sphere corner": (3, False), "capsule end on": (1, False),
           "capsule across edge": (2, True), "capsule tilted": (1, False), "deep": (0, False)}
CROWD = "own 64"
_cases = cs.Cases(_CASES, 2)
case, reference, conditioning, node_case, node_conditioning, sim_of = _cases.case, _cases.reference, _cases.conditioning, _cases.node_case, _cases.node_conditioning, _cases.sim_of


def limit_table(n_follow):
    """256 dynamic spheres x n_follow following boxes, all in each other's masks: 256 n_follow follow entries against boxes"""
    return cs.limit_table(n_follow, fol_shape=1)
