"""Synthetic scenes for the contact tests (tests/test_contact_cpu.py, tests/test_gpu_contacts.py): chains of dynamic capsules and spheres
hanging from one following body on a carrier bone the poses move, around following collider bodies on a bone the poses leave alone, so
contacts arise from motion. Every case the GPU tests run is listed in CASES and checked for conditioning and for contact activity on the
CPU (test_contact_cpu.py: test_cases_are_well_conditioned_and_touch)."""
import os
import subprocess

import numpy as np

import contact_ref
import ik_ref
import physics_ref
import physics_scenes as ps
from physics_scenes import _quat, _scene, run_reference, write_pmx  # noqa: F401

PI = float(np.pi)
COLLIDER_BONE, CARRIER_BONE = 1, 2
HEIGHT = 10.0
G_COLLIDER, G_CHAIN = 1, 2            # collision groups
ALL = 0xffff


class Builder:
    """bone 0 the root, bone 1 the colliders' bone, bone 2 the carrier; body 0 the carrier's following body (mask 0: it touches nothing)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parents, self.bind = [-1, 0, 0], [[0.0, 0.0, 0.0], [0.0, HEIGHT, 0.0], [0.0, HEIGHT, 0.0]]
        self.bodies = [dict(bone=CARRIER_BONE, type=0, shape=0, size=[0.1, 0, 0], mass=0.0, group=0, mask=0)]
        self.joints = []

    def collider(self, at, shape, size, rot=None, group=G_COLLIDER, mask=ALL, friction=0.5, kind=0):
        """a following body on the colliders' bone at `at` (relative to that bone)"""
        self.bodies.append(dict(bone=COLLIDER_BONE, type=kind, shape=shape, size=size, mass=1.0 if kind == 2 else 0.0, offset_pos=list(at),
                                offset_rot=(0, 0, 0, 1) if rot is None else rot, group=group, mask=mask, friction=friction))
        return len(self.bodies) - 1

    def chain(self, at, shapes, group=G_CHAIN, mask=ALL, friction=0.5, radius=0.3, height=0.6, spacing=1.0, rot=None, mass=None, boned=True, free=False):
        """a chain hanging from the carrier's body at `at` (relative to the carrier): one dynamic body per entry of `shapes`, each on a bone
        of its own `spacing` below its parent, the body's centre half a spacing below its bone; limited, sprung joints. free: the first
        body has no joint (it falls)."""
        parent_bone, parent_body, step = CARRIER_BONE, 0, np.array(at, dtype=np.float64)
        here = np.array(self.bind[CARRIER_BONE]) + step
        out = []
        for k, shape in enumerate(shapes):
            bone = -1
            if boned:
                self.parents.append(parent_bone); self.bind.append(list(step))
                bone = len(self.parents) - 1
            size = [radius, 0, 0] if shape == 0 else [radius, height, radius] if shape == 1 else [radius, height, 0]
            q = _quat(self.rng.normal(size=3), self.rng.uniform(-0.2, 0.2)) if rot is None else rot
            self.bodies.append(dict(bone=bone, type=1, shape=shape, size=size, mass=float(self.rng.uniform(0.8, 1.5)) if mass is None else mass,
                                    linear_damping=0.99, angular_damping=0.99, offset_pos=[0, -spacing / 2, 0] if boned else list(here + [0, -spacing / 2, 0]),
                                    offset_rot=q, group=group, mask=mask, friction=friction))
            me = len(self.bodies) - 1
            if not (free and k == 0):
                lim = 0.6
                self.joints.append(dict(body_a=parent_body, body_b=me, position=list(here), rotation=[0.0, 0.0, 0.0], rotation_min=[-lim, -lim / 2, -lim],
                                        rotation_max=[lim, lim / 2, lim], spring_rotation=[100.0, 100.0, 100.0], spring_position=[0, 0, 0]))
            out.append(me)
            if boned:
                parent_bone = bone
            parent_body, step = me, np.array([0.0, -spacing, 0.0])
            here = here + step
        return out

    def loose_joint(self, a, b, at, play=0.4):
        self.joints.append(dict(body_a=a, body_b=b, position=list(np.array(self.bind[CARRIER_BONE]) + at), rotation=[0, 0, 0], position_min=[-play] * 3,
                                position_max=[play] * 3, rotation_min=ps.FREE_MIN, rotation_max=ps.FREE_MAX, spring_rotation=[0, 0, 0], spring_position=[0, 0, 0]))

    def scene(self, n_verts=96, **kw):
        return _scene(self.parents, self.bind, self.bodies, self.joints, self.rng, n_verts, **kw)


def ring(n, radius, phase=0.0):
    return [np.array([radius * np.cos(phase + 2 * PI * s / n), 0.0, radius * np.sin(phase + 2 * PI * s / n)]) for s in range(n)]


def torso(b, radius=0.8, height=2.5):
    """the colliders of the base scene: an upright capsule under the carrier's height and a shoulder sphere beside it"""
    b.collider([0, -1.5, 0], 2, [radius, height, 0])
    b.collider([0.9, -0.4, 0], 0, [0.5, 0, 0])


def strands(n_strands, n_dyn, seed, ring_radius=1.35, self_collide=False, cross=False, tie=False, n_verts=96, friction=0.5, **kw):
    """`n_strands` chains of alternating capsules and spheres on a ring around the torso. self_collide: the chains' group is in their own
    mask (dynamic pairs); otherwise they meet the colliders only (follow pairs). cross / tie: loose joints between neighbouring chains, as
    physics_scenes.strands adds them."""
    b = Builder(seed)
    torso(b)
    mask = ALL if self_collide else ALL & ~(1 << G_CHAIN)
    at = ring(n_strands, ring_radius)
    ch = [b.chain(at[s], [(2, 0)[(s + k) % 2] for k in range(n_dyn)], mask=mask, friction=friction) for s in range(n_strands)]
    if cross:
        for s in range(n_strands):
            for k in range(n_dyn):
                b.loose_joint(ch[s][k], ch[(s + 1) % n_strands][k], (at[s] + at[(s + 1) % n_strands]) / 2 + [0, -k - 0.5, 0])
    if tie:
        b.loose_joint(ch[0][-1], ch[2][-1], (at[0] + at[2]) / 2 + [0, -n_dyn + 0.5, 0], play=0.8)
    return b.scene(n_verts, **kw)


def rings(n_rings, per_ring, seed, n_verts=400):
    """one dynamic sphere per chain, `n_rings` rings of `per_ring` around one tall capsule: every dynamic body has one following partner"""
    b = Builder(seed)
    b.collider([0, -0.5 * n_rings, 0], 2, [1.0, 1.0 * n_rings + 2, 0])
    mask = ALL & ~(1 << G_CHAIN)
    for r in range(n_rings):
        for at in ring(per_ring, 1.45, phase=0.1 * r):
            b.chain(at + [0, -0.8 * r, 0], [0], mask=mask, radius=0.12, spacing=0.6)
    return b


def many_partners(seed=41):
    """body 1 .. 70: following spheres packed on a small patch (a list longer than a wave); one chain of two dynamic bodies over it, the
    lower one reaching the patch; one more dynamic body aside with an empty list (its mask names nothing)"""
    b = Builder(seed)
    rng = np.random.default_rng(seed)
    for k in range(70):
        b.collider([0.5 + 0.02 * (k % 10), -1.4 - 0.02 * (k // 10), 0.01 * rng.uniform(-1, 1)], 0, [0.45, 0, 0])
    b.chain([1.47, 0, 0], [0, 2], mask=ALL & ~(1 << G_CHAIN))
    b.chain([0, 0, 3.0], [0], mask=0)
    return b.scene(64, iterations=2)


def pair_field(seed=42):
    """514 dynamic spheres in eight group classes (33 + 33 bodies once, 32 + 32 seven times): within a class every body of the first half
    meets every body of the second (complete bipartite, greedy colour = i xor j), so colour 0 holds the 257 disjoint pairs (i, i); only
    those are close enough to touch: the second of a pair hangs 0.57 beside the first (radii 0.3), the reset places them in contact. No
    follow entries."""
    b = Builder(seed)
    sizes = [33] + [32] * 7
    slot = lambda k: np.array([1.5 * (k % 17) - 12.0, 0.0, 1.2 * (k // 17) - 9.0])
    k0 = 0
    for half in (0, 1):
        k0 = 0
        for c, n in enumerate(sizes):
            ga, gb = (2 * c, 2 * c + 1) if half == 0 else (2 * c + 1, 2 * c)
            for i in range(n):
                b.chain(slot(k0 + i) + [0.57 * half, 0, 0], [0], group=ga, mask=1 << gb, radius=0.3, spacing=1.0)
            k0 += n
    return b.scene(600, iterations=2)


def three_colours(seed=43):
    """three chains in a row beside the torso, their group in its own mask: a body of the middle chain sits in dynamic pairs with both
    neighbours and with its own chain's other body (three colours and more), and all of them may meet the torso (follow entries on the
    same bodies); the carrier's slide stacks them against it"""
    b = Builder(seed)
    torso(b)
    for x in (1.15, 1.77, 2.39):
        b.chain([x, 0, 0.03 * x], [0, 0], radius=0.3)
    return b.scene(64)


def shape_pair(first, second, order="fd", skew=False, ends=False, mu=(0.5, 0.5), seed=44):
    """Two bodies that meet when the carrier slides towards -x; `first` gets the lower index. order "fd": a following `first` at the
    colliders' origin and a dynamic `second` beside it; "df": the dynamic body first, the following one behind it in the table; "dd": both
    dynamic, side by side, behind a following sphere that stops the first so the second runs into it. ends: capsules lying along x, end
    against end (both clamps act)."""
    b = Builder(seed)
    lying = _quat([0, 0.05, 1], PI / 2)                               # a capsule along x (nearly: the pair is not exactly collinear)
    tilt_a, tilt_b = _quat([1, 0.2, 0], 0.5), _quat([0.3, 0, 1], -0.6)
    free = ALL & ~(1 << G_CHAIN)
    if order == "dd":
        b.collider([0.0, -0.5, 0.0], 0, [0.4, 0, 0])
        if ends:
            b.chain([1.05, 0, 0], [first], friction=mu[0], rot=lying)
            b.chain([2.28, 0, 0.04], [second], friction=mu[1], rot=lying)
        else:
            b.chain([0.73, 0, 0], [first], friction=mu[0], rot=tilt_a if skew else None)
            b.chain([1.36, 0, 0.05], [second], friction=mu[1], rot=tilt_b if skew else None)
    else:
        dyn, fol = (second, first) if order == "fd" else (first, second)
        place = lambda: b.collider([0.0, -0.5, 0.0], fol, [0.4, 1.2, 0], rot=tilt_a if skew else None, friction=mu[0 if order == "fd" else 1])
        if order == "fd":
            place()
        b.chain([0.74, 0, 0.1], [dyn], mask=free, friction=mu[1 if order == "fd" else 0], rot=tilt_b if skew else None)
        if order == "df":
            place()
    return b.scene(64)


def reset_into_contact(seed=45):
    """the chains start inside the torso by a third of their radius: the reset places them in penetration. (Spheres on top: an upright
    capsule pressed into the upright torso is the parallel, ill-conditioned closest-point case, which the float32 probe shows at once.)"""
    b = Builder(seed)
    torso(b)
    for at in ring(4, 1.0):
        b.chain(at, [0, 2], mask=ALL & ~(1 << G_CHAIN))
    return b.scene(64)


def apart(seed=46):
    """pairs exist, and never come within reach: the chains hang far from the torso"""
    b = Builder(seed)
    torso(b)
    for at in ring(4, 4.0):
        b.chain(at, [2, 0])
    return b.scene(64)


def masked(sc):
    """the same scene with every mask 0: no candidate pair"""
    t = dict(sc["table"])
    t["mask"] = np.zeros_like(t["mask"])
    return dict(sc, table=t)


def pose(scene, k, amount=0.5, turn=0.05):
    """call k's local pose: the colliders' bone stays, the carrier slides towards -x, sweeping round, and tips a little (k = 0: the bind
    pose, every pair apart)"""
    B = scene["B"]
    q = np.zeros((B, 4), dtype=np.float32); q[:, 3] = 1
    t = np.zeros((B, 3), dtype=np.float32)
    if k:
        ang = 0.5 * (k - 1)
        t[CARRIER_BONE] = [-amount * np.cos(ang), 0.1 * amount * np.sin(2 * ang), amount * np.sin(ang)]
        q[CARRIER_BONE] = _quat([np.sin(ang), 0.2, np.cos(ang)], turn * np.sin(1.3 * k)).astype(np.float32)
    return q, t


CALLS = (1, 10, 10, 10, 10)
SHORT = (1, 10, 10)
PARAMS = dict(h=1 / 120, iterations=6, gravity=(3.0, -40.0, 25.0))

# name: (scene, pose amount, calls)
_CASES = {
    # the four instantiations with contacts on
    "own 64": (lambda: strands(6, 3, 51), 0.5, CALLS),
    "stride 64": (lambda: strands(8, 4, 52, cross=True, tie=True, ring_radius=1.4), 0.5, SHORT),
    "own 256": (lambda: strands(16, 4, 53, ring_radius=1.6, n_verts=160), 0.6, SHORT),
    "stride 256": (lambda: rings(9, 29, 54).scene(600), 0.5, SHORT),                 # 261 joints; 261 dynamic bodies, one partner each
    # pass F: a list longer than a wave, an empty list beside it
    "70 partners": (lambda: many_partners(), 0.4, (1, 6, 6)),
    # pass D
    "257 pairs": (lambda: pair_field(), 0.0, (1, 5)),
    "three colours": (lambda: three_colours(), 0.5, SHORT),
    # shape pairs: following body first / dynamic body first / both dynamic
    "sphere sphere fd": (lambda: shape_pair(0, 0), 0.3, SHORT),
    "sphere sphere dd": (lambda: shape_pair(0, 0, "dd"), 0.3, SHORT),
    "sphere capsule fd": (lambda: shape_pair(0, 2), 0.3, SHORT),
    "sphere capsule df": (lambda: shape_pair(0, 2, "df"), 0.3, SHORT),
    "sphere capsule dd": (lambda: shape_pair(0, 2, "dd"), 0.3, SHORT),
    "capsule sphere fd": (lambda: shape_pair(2, 0), 0.3, SHORT),
    "capsule sphere df": (lambda: shape_pair(2, 0, "df"), 0.3, SHORT),
    "capsule sphere dd": (lambda: shape_pair(2, 0, "dd"), 0.3, SHORT),
    "capsule capsule skew fd": (lambda: shape_pair(2, 2, skew=True), 0.3, SHORT),
    "capsule capsule skew dd": (lambda: shape_pair(2, 2, "dd", skew=True), 0.3, SHORT),
    "capsule capsule ends": (lambda: shape_pair(2, 2, "dd", ends=True), 0.3, SHORT),
    # friction: 0 on one side (the stage is skipped), and against a following body (previous pose = current pose)
    "friction zero": (lambda: shape_pair(2, 0, mu=(0.0, 0.8)), 0.3, SHORT),
    "friction follow": (lambda: shape_pair(2, 0, mu=(1.0, 1.0)), 0.3, SHORT),
    "reset into contact": (lambda: reset_into_contact(), 0.3, SHORT),
    "params": (lambda: strands(6, 3, 56, **PARAMS), 0.5, SHORT),
}
# name: (lanes per workgroup, joints in registers?) — the form the launch must take
FORMS = {"own 64": (64, 1), "stride 64": (64, 0), "own 256": (256, 1), "stride 256": (256, 0)}
CROWD = "own 64"


def limit_table(n_follow, dyn_shape=0, fol_shape=0):
    """256 dynamic x n_follow following bodies (spheres, or boxes where the shape is 1), all in each other's masks: 256 n_follow follow
    entries (65 536 with 256, the limit) under the modes that pair the two shapes"""
    size = lambda shape: [0.1, 0.1, 0.1] if shape == 1 else [0.1, 0, 0]
    dyn = dict(bone=-1, type=1, mass=1.0, shape=dyn_shape, size=size(dyn_shape), group=1, mask=1 << 2)
    fol = dict(bone=1, type=0, mass=0.0, shape=fol_shape, size=size(fol_shape), group=2, mask=1 << 1)
    return physics_ref.make_table([dict(dyn, offset_pos=[3.0 * k, 0, 0]) for k in range(256)] + [dict(fol, offset_pos=[3.0 * k, 50.0, 0]) for k in range(n_follow)], [])


# ---- the host half's stand-alone program (tests/contact_table_main.cpp around reze-engine_amd/csrc/contact_table.h) ----

def build_table_tool(folder):
    """the table program under ASan and UBSan"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(folder / "contact_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(root, "tests", "contact_table_main.cpp")])
    return exe


def run_table_tool(tool, t, mode=1):
    """the program's lines for table t under the mode, as {first word: the rest, split}, and its whole output"""
    rows = ["%d" % t["n_bodies"]]
    for b in range(t["n_bodies"]):
        rows.append("%d %d %d %d %r %r %r %r %r" % (t["type"][b], t["shape"][b], t["group"][b], t["mask"][b], float(t["size"][b][0]), float(t["size"][b][1]), float(t["size"][b][2]),
                                                    float(t["mass"][b]), float(t["friction"][b])))
    out = subprocess.run([tool, "%d" % mode], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True).stdout
    return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1].split() if " " in ln else [] for ln in out.strip().split("\n")}, out


def assert_host_lists(rows, L):
    """the program's lines against the definition's lists of the same mode, entry for entry: counts, shape records with the box bit, c_box,
    the follow CSR, the dynamic pairs in solve order and the colour offsets"""
    assert [int(v) for v in rows["counts"]] == [L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"]] and rows["refused"][0] == "0"
    assert int(rows["box_pairs"][0]) == L["box_pairs"] and int(rows["box_box"][0]) == L["n_box_box"]
    shape = np.array([float(v) for v in rows["shape"]], dtype=np.float32).reshape(-1, 4)          # (%.9g round-trips a float32)
    assert np.array_equal(shape[:, 0], L["radius"]) and np.array_equal(shape[:, 1], L["half"]) and np.array_equal(shape[:, 2], L["friction"])
    assert np.array_equal(shape[:, 3], L["takes"].astype(int) + 4 * L["box"].astype(int))
    box = np.array([float(v) for v in rows["box"]], dtype=np.float32).reshape(-1, 4)
    if len(box):
        assert np.array_equal(box[:, :3], L["ext"]) and not box[:, 3].any()
    else:                                                                                         # (mode 1 uploads no c_box)
        assert not L["box"].any() and not L["ext"].any()
    assert [int(v) for v in rows["follow_off"]] == list(L["follow_off"]) and [int(v) for v in rows["follow_idx"]] == list(L["follow_idx"])
    assert [int(v) for v in rows["pair"]] == list(L["pairs"].reshape(-1)) and [int(v) for v in rows["colour_off"]] == list(L["colour_off"])


class Cases:
    """What the tests ask of a table of cases — name: (scene, pose amount, calls[, how far the carrier turns: pose's `turn`, 0.05 unless
    given]) — under the contact mode they are there for. Scenes and float64 references are built once."""

    def __init__(self, cases, mode):
        self.cases, self.mode, self.memo = cases, mode, {}

    def sim_of(self, sc, dtype=np.float64, mode=None):
        return contact_ref.Sim(sc["table"], sc["parents"], sc["bind"], dtype=dtype, mode=self.mode if mode is None else mode)

    def case(self, name):
        """(scene, poses, calls)"""
        if name not in self.memo:
            make, amount, calls = self.cases[name][:3]
            sc = make()
            self.memo[name] = (sc, [pose(sc, k, amount, *self.cases[name][3:]) for k in range(len(calls))], calls)
        return self.memo[name]

    def reference(self, name, dtype=np.float64, mode=None):
        """the case's run_reference under the mode (memoised): per call (world [B,16], state [nb,13]); also the Sim"""
        key = (name, np.dtype(dtype).name, self.mode if mode is None else mode)
        if key not in self.memo:
            sc, poses, calls = self.case(name)
            sim = self.sim_of(sc, dtype, mode)
            self.memo[key] = (run_reference(sc, poses, calls, dtype=dtype, sim=sim), sim)
        return self.memo[key]

    def conditioning(self, name):
        """(largest float32-probe deviation from the float64 run in units of extent, the fraction of substeps with an active contact, the
        probe's largest quaternion deviation up to sign)"""
        sc, _, _ = self.case(name)
        a, sim = self.reference(name)
        b, _ = self.reference(name, dtype=np.float32)
        worst = turn = 0.0
        for (wa, sa), (wb, sb) in zip(a, b):
            worst = max(worst, float(np.abs(wa - wb).max()), float(np.abs(sa[:, :3] - sb[:, :3]).max()))
            turn = max(turn, float(np.minimum(np.abs(sa[:, 3:7] - sb[:, 3:7]).max(axis=1), np.abs(sa[:, 3:7] + sb[:, 3:7]).max(axis=1)).max()))
        act = np.array(sim.active)
        return worst / sc["extent"], float((act > 0).mean()), turn

    def node_case(self):
        """The Node end-to-end test's scene: the 'own 64' chains as a PMX file, run with the table its loader derives from the file, under
        one fixed local pose of the carrier. Returns (scene, pmx bytes, q [B,4])."""
        if "node" not in self.memo:
            sc, _, _ = self.case("own 64")
            data, want = write_pmx(sc)
            q, _ = pose(sc, 3, turn=0.5)
            self.memo["node"] = (dict(sc, table=want), data, q)
        return self.memo["node"]

    def node_conditioning(self):
        """the Node case under the engine's substeps: (largest float32-probe deviation from the float64 run in units of extent, the
        fraction of substeps with an active contact, the float64 Sim)"""
        sc, _, q = self.node_case()
        calls = ps.node_substeps()
        poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * len(calls)
        sims = [self.sim_of(sc, dt) for dt in (np.float64, np.float32)]
        a, b = (run_reference(sc, poses, calls, dtype=dt, sim=sim) for dt, sim in zip((np.float64, np.float32), sims))
        c = max(max(float(np.abs(x[0] - y[0]).max()), float(np.abs(x[1][:, :3] - y[1][:, :3]).max())) for x, y in zip(a, b)) / sc["extent"]
        return c, float((np.array(sims[0].active) > 0).mean()), sims[0]


_cases = Cases(_CASES, 1)
case, reference, conditioning, node_case, node_conditioning, sim_of = _cases.case, _cases.reference, _cases.conditioning, _cases.node_case, _cases.node_conditioning, _cases.sim_of
