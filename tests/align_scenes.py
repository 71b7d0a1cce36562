"""Scenes for the PMX type-2 bodies (rz_physics_aligned; tests/align_ref.py; tests/test_align_cpu.py, tests/test_gpu_align.py): tables of
physics_scenes, spring_scenes, the contact scenes, follow_scenes and after_scenes with the FIRST LINK of every strand — the dynamic body a
joint hangs from a following one — made type 2 on a copy, as PMX authors rig the first link of a hair strand, a tie or a skirt's top row.
Every case the GPU tests run is listed in CASES, with the launch form it is there for, and is checked for conditioning on the CPU. The
calls are short — a handful of calls of 1 - 3 substeps, the pose moving between them — so that the re-pin, which happens once per call,
happens often."""
import numpy as np

import after_ref
import align_ref
import contact_boxbox_scenes as bbs
import contact_scenes as cs
import follow_ref
import ik_ref
import physics_ref
import physics_scenes as ps
import spring_scenes as ss
from physics_scenes import _quat

CALLS = (1, 3, 2, 3, 1)             # substeps per call; the first is the implicit reset
CROWD = "own 64"


def retyped(sc, types, mass=None):
    """the scene with the type (and the mass) of the given bodies replaced on a copy of its table: {body: type}, {body: mass}"""
    t = dict(sc["table"])
    t["type"] = np.array(t["type"], copy=True)
    t["mass"] = np.array(t["mass"], copy=True)
    for b, ty in types.items():
        t["type"][b] = ty
    for b, m in (mass or {}).items():
        t["mass"][b] = m
    return dict(sc, table=t)


def first_links(t):
    """the dynamic bodies that a joint hangs from a body that is not dynamic, ascending"""
    dyn = physics_ref.is_dynamic(t)
    out = set()
    for a, b in zip(t["body_a"], t["body_b"]):
        if dyn[b] and not dyn[a]:
            out.add(int(b))
        if dyn[a] and not dyn[b]:
            out.add(int(a))
    return sorted(out)


def with_first_links(sc, every=1, also=()):
    """every `every`-th first link and the bodies `also` become type 2; a type-2 body the scene already had (physics_scenes.strands gives
    every third base one, with a mass: aligned and hung from nothing it would fall through every call) becomes type 0"""
    t = sc["table"]
    types = {int(b): 0 for b in np.nonzero(t["type"] == 2)[0]}
    types.update({b: 2 for b in first_links(t)[::every]})
    types.update({int(b): 2 for b in also})
    return retyped(sc, types)


def _own64():
    """the "crowd" strands with the fourth strand's bodies off the skeleton (bone = -1): 25 bodies, 20 joints. Type 2: the first link of
    every strand — three aligned, the fourth a plain dynamic body then (no bone) —, the free body (aligned and held by no joint: it falls
    during a call and is back on its bone at the next), and the first base with mass 0 (it keeps following)"""
    sc = ps.strands(4, 5, base=True, seed=7, n_verts=96, free_body=True, boned=3)
    t = sc["table"]
    free = t["n_bodies"] - 1
    sc = with_first_links(sc, also=[free])
    return retyped(sc, {0: 2}, {0: 0.0})


def _follow():
    """3 strands of 3 sprung dynamic bodies, the first links type 2; per strand a tip bone WITHOUT a body directly below the aligned bone,
    beside the strand's next dynamic bone: with rz_override_follow it rides the aligned bone — its rotation, and the animated position"""
    base = ps.strands(3, 3, base=True, seed=44, n_verts=64, sprung=True)
    parents, bind = [int(p) for p in base["parents"]], [list(map(float, b)) for b in base["bind"]]
    ride = {}
    for b in first_links(base["table"]):
        bone = int(base["table"]["bone"][b])
        parents.append(bone); bind.append([0.4, -0.6, 0.2])
        ride[len(parents) - 1] = bone
    sc = ps._scene(parents, bind, base["bodies"], base["joints"], np.random.default_rng(45), 3 * len(parents))
    sc.update(ride=ride)
    return with_first_links(sc)


def _after():
    """after_scenes.physics' skeleton with every helper appending from the strand's FIRST dynamic bone, whose body is type 2: the helper
    takes the rotation the aligned body gave its bone (the second: -0.7 of it and, with move, of its translation away from the bind pose —
    which for an aligned bone is the animation's)"""
    base = ps.strands(3, 4, base=True, seed=46, n_verts=64, sprung=True)
    parents, bind = [int(p) for p in base["parents"]], [list(map(float, b)) for b in base["bind"]]
    B0 = len(parents)
    ap, ratio, move, order = [-1] * B0, [1.0] * B0, [0] * B0, []
    for s, b in enumerate(first_links(base["table"])):
        src = int(base["table"]["bone"][b])
        parents.append(parents[src]); bind.append([0.5, -0.3, 0.2 * s]); ap.append(src); ratio.append(1.0 if s != 1 else -0.7); move.append(int(s == 1))
        order.append(len(parents) - 1)
    for h in list(order):
        parents.append(h); bind.append([0.0, -4.0, 0.0]); ap.append(-1); ratio.append(1.0); move.append(0)
        order.append(len(parents) - 1)
    sc = ps._scene(parents, bind, base["bodies"], base["joints"], np.random.default_rng(47), 3 * len(parents), gravity=(60.0, -98.0, 40.0), h=1.0 / 30.0)
    sc.update(ap=np.array(ap, dtype=np.int32), ratio=np.array(ratio, dtype=np.float32), move=np.array(move, dtype=np.uint8), order=np.array(order, dtype=np.uint32))
    return with_first_links(sc)


def _strand_poses(make, amount=1.0):
    def build():
        sc = make()
        return sc, [ps.pose(sc, 500 + k, amount) for k in range(len(CALLS))], CALLS
    return build


def _carrier_poses(make, amount):
    def build():
        sc = make()
        return sc, [cs.pose(sc, k, amount) for k in range(len(CALLS))], CALLS
    return build


# name: (builder of (scene, poses, calls), contact mode, linear springs?, (lanes per workgroup, joints in registers?) the launch must take,
#        what the frame does behind the overrides: None, "follow" or "after")
CASES = {
    # the launch forms: a few bodies in one wave; 65 bodies; 257 joints, every second strand's body aligned
    "own 64": (_strand_poses(_own64), 0, False, (64, 1), None),
    "own 256": (_strand_poses(lambda: with_first_links(ps.scene("65 bodies"))), 0, False, (256, 1), None),
    "stride 256": (_strand_poses(lambda: with_first_links(ps.scene("257 joints"), every=2)), 0, False, (256, 0), None),
    # the stages it composes with
    "contacts 1": (_carrier_poses(lambda: with_first_links(cs.strands(6, 3, 51)), 0.5), 1, False, (64, 1), None),
    # an aligned box against a following box, a vertical edge on a face (contact_boxbox_scenes' "edge on a face": the plain "box box fd" pair
    # starts in deep contact, where the float32 probe leaves the float64 run by 5e-2 x extent once the re-pin moves the box)
    "contacts 3 box on box": (_carrier_poses(lambda: with_first_links(bbs.pair("fd", box_rot=_quat([0, 1, 0], 0.05), dyn_rot=bbs.EDGE_UP, at=[0.9, 0, 0.05])), 0.3),
                              3, False, (64, 1), None),
    "springs": (_strand_poses(lambda: with_first_links(ss.sprung(ps.scene("crowd"), 1))), 0, True, (64, 1), None),
    "follow": (_strand_poses(_follow), 0, False, (64, 1), "follow"),
    "after": (_strand_poses(_after), 0, False, (64, 1), "after"),
}
ORDER = list(CASES)
_memo = {}


def case(name):
    """(scene, poses, calls)"""
    if name not in _memo:
        _memo[name] = CASES[name][0]()
    return _memo[name]


def sim_of(sc, mode=0, springs=False, dtype=np.float64, aligned=True):
    return align_ref.Sim(sc["table"], sc["parents"], sc["bind"], dtype=dtype, mode=mode, springs=springs, aligned=aligned)


def solved(sc, q, t, dtype=np.float64):
    """the un-overridden hierarchy solve of one local pose: [B,16]"""
    return ik_ref.solve(sc["parents"], sc["bind"], q, t, (), sc.get("ap"), sc.get("ratio"), sc.get("move"), dtype=dtype)[0]


def frame(sc, q, t, S, ovr, behind=None, dtype=np.float64):
    """the world matrices the frame uses: the solve S with the overrides in place, and behind them the followers or the after-physics bones"""
    bones = sorted(ovr)
    F = np.asarray(physics_ref.apply_overrides(S, ovr), dtype=dtype)
    if behind == "follow":
        return np.asarray(follow_ref.follow(sc["parents"], S, bones, np.stack([ovr[b] for b in bones]), dtype=dtype), dtype=np.float64)
    if behind == "after":
        return np.asarray(after_ref.solve(sc["parents"], sc["bind"], q, t, sc["ap"], sc["ratio"], sc["move"], F, bones, sc["order"], dtype=dtype), dtype=np.float64)
    return F.astype(np.float64)


def run(sc, poses, calls, mode=0, springs=False, behind=None, dtype=np.float64, aligned=True, sim=None):
    """one instance through the calls under the definition: per call (world [B,16] as the frame uses it, state [nb,13], the un-overridden
    solve [B,16]); also the Sim. A call "reset" is rz_physics_reset under that call's pose: a step of no substep that places every body"""
    sim = sim or sim_of(sc, mode, springs, dtype, aligned)
    out = []
    for (q, t), n in zip(poses, calls):
        S = solved(sc, q, t, dtype=dtype)
        if n == "reset":
            sim.pending_reset, n = True, 0
        ovr = sim.step(S, n)
        out.append((frame(sc, q, t, S, ovr, behind, dtype), sim.state13().astype(np.float64), np.asarray(S, dtype=np.float64)))
    return out, sim


def reference(name, dtype=np.float64, aligned=True):
    """the case's run under the definition (memoised, not to be written to)"""
    key = (name, np.dtype(dtype).name, aligned)
    if key not in _memo:
        sc, poses, calls = case(name)
        _, mode, springs, _, behind = CASES[name]
        _memo[key] = run(sc, poses, calls, mode, springs, behind, dtype, aligned)[0]
    return _memo[key]


def deviation(a, b):
    """largest difference of two runs over their calls: world-matrix entries and body positions"""
    return max(max(float(np.abs(x[0] - y[0]).max()), float(np.abs(x[1][:, :3] - y[1][:, :3]).max())) for x, y in zip(a, b))


def conditioning(name):
    """largest float32-probe deviation from the float64 run over the case's calls, in units of extent"""
    return deviation(reference(name), reference(name, dtype=np.float32)) / case(name)[0]["extent"]


# the other sequences of calls tests/test_gpu_align.py makes on the CROWD case: a call without substeps, a reset between calls, and the calls
# whose split into calls of one substep must not add up
ZERO_CALLS = (1, 3, 0, 2)
RESET_CALLS = (2, 3, "reset", 2)
SPLIT_CALLS = (1, 2, 2, 2)


def split(poses, calls):
    """every call of n substeps as n calls of one under the same pose: (poses, calls)"""
    return [p for p, n in zip(poses, calls) for _ in range(n)], tuple(1 for n in calls for _ in range(n))


def plain_scene():
    """the "crowd" strands without any type-2 body, and its poses for SPLIT_CALLS"""
    sc = ps.scene("crowd")
    sc = retyped(sc, {int(b): 0 for b in np.nonzero(sc["table"]["type"] == 2)[0]})
    return sc, [ps.pose(sc, 500 + k) for k in range(len(SPLIT_CALLS))]


def two_on_one_bone(sc):
    """the scene with one more type-2 body on the bone its first aligned body drives, that body itself made type 1: valid as uploaded (one
    dynamic body on the bone), refused once both are dynamic. Returns (scene, the two bodies)"""
    t = sc["table"]
    first = int(np.nonzero(align_ref.aligned_bodies(t))[0][0])
    bodies = [dict(b, type=int(t["type"][k]), mass=float(t["mass"][k])) for k, b in enumerate(sc["bodies"])]
    bodies[first]["type"] = 1
    bodies.append(dict(bodies[first], type=2))
    return dict(sc, table=physics_ref.make_table(bodies, sc["joints"])), first, len(bodies) - 1


def aligned_bones(sc):
    t = sc["table"]
    return [int(t["bone"][b]) for b in np.nonzero(align_ref.aligned_bodies(t))[0]]


def crowd_poses(sc, instance):
    return [ps.pose(sc, 600 + 10 * k + instance) for k in range(len(CALLS))]


def cost_scene():
    """tools/align_cost.py: the "crowd" strands with the first link of every strand type 2"""
    return with_first_links(ps.scene("crowd"))


def node_case():
    """The Node end-to-end test's scene: cost_scene as a PMX file, run with the table its loader derives from the file, under one fixed
    local pose. Returns (scene, pmx bytes, q [B,4])."""
    if "node" not in _memo:
        sc = cost_scene()
        data, want = ps.write_pmx(sc)
        q, _ = ps.pose(sc, 70, amount=2.0)
        _memo["node"] = (dict(sc, table=want), data, q)
    return _memo["node"]
