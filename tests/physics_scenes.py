"""Synthetic skeletons with rigid-body tables for the physics tests (tests/test_physics_cpu.py, tests/test_gpu_physics.py): strands of
dynamic bodies hanging from bodies that follow their bones, as hair, ribbons and skirts are rigged in PMX models. Every scene the GPU tests
use is listed in SCENES and checked for conditioning on the CPU (test_physics_cpu.py: test_scenes_are_well_conditioned)."""
import os
import subprocess

import numpy as np

import ik_ref
import physics_ref

PI = float(np.pi)
FREE_MIN, FREE_MAX = (-PI, -PI / 2, -PI), (PI, PI / 2, PI)


def _quat(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]])


def strands(n_strands, n_dyn, base=True, seed=1, n_verts=96, free_body=False, sprung=False, cross=False, tie=False, boned=None, gravity=None, h=0.0, iterations=0):
    """A root bone carrying `n_strands` chains of `n_dyn` dynamic bones. base=True: every strand hangs from a bone of its own whose body
    follows it; base=False: every strand hangs from ONE following body on the root (joints of one colour then share it). free_body: one more
    dynamic body without joints on a bone of its own. sprung: every joint is limited and has a spring on every axis (a body on a free joint
    without a spring about its own axis keeps whatever twist rounding gives it: its quaternion wanders at 1e-4 while its position holds).
    cross: every dynamic body is also joined to the body at its height on the next strand, as the panels of a skirt are: a loose joint
    (0.3 units of play per axis, rotation free), so a dynamic body sits in up to four joints and the joints outnumber the bodies. tie: one
    more such joint, between the last bodies of the first and the third strand (an odd joint count). boned: only the dynamic bodies of the
    first `boned` strands drive bones of their own; those of the other strands have bone = -1 and are placed by their offsets in model
    space (a table may hold more bodies than the hierarchy solve takes bones). gravity, h, iterations: the table's parameters (None / 0 =
    the defaults)."""
    rng = np.random.default_rng(seed)
    parents, bind, bodies, joints = [-1, 0], [[0.0, 0.0, 0.0], [0.0, 16.0, 0.0]], [], []        # a centre bone at the origin, a head at MMD height
    level = []                      # [strand][k] = (body, model-space position of its bone)
    root_body = None
    if not base:
        bodies.append(dict(bone=1, type=0, shape=1, size=[0.5, 0.2, 0.5], mass=0.0, offset_pos=[0, -0.1, 0]))
        root_body = 0
    pos = [np.array(bind[0]), np.array(bind[1])]
    for s in range(n_strands):
        ang = 2 * PI * s / max(n_strands, 1)
        rad = 1.0 + 0.01 * s
        at = np.array([rad * np.cos(ang), 0.0, rad * np.sin(ang)])
        parent_bone, parent_body = 1, root_body
        level.append([])
        if base:
            parents.append(1); bind.append(list(at)); pos.append(pos[1] + at)
            parent_bone = len(parents) - 1
            bodies.append(dict(bone=parent_bone, type=0 if s % 3 else 2, shape=0, size=[0.2, 0, 0], mass=1.0 if s % 3 == 0 else 0.0,
                               offset_pos=[0, 0, 0], offset_rot=_quat(rng.normal(size=3), rng.uniform(-0.3, 0.3))))
            parent_body = len(bodies) - 1
            at = np.zeros(3)
        has_bone = boned is None or s < boned
        parent_pos = pos[parent_bone]
        for k in range(n_dyn):
            step = at + (np.array([0.0, -1.0, 0.0]) if (k or base) else np.zeros(3))
            here = parent_pos + step
            b = -1
            if has_bone:
                parents.append(parent_bone); bind.append(list(step))
                b = len(parents) - 1
                pos.append(here)
            shape = (s + k) % 3
            size = [[0.5, 0, 0], [0.3, 0.5, 0.3], [0.3, 0.6, 0]][shape]
            bodies.append(dict(bone=b, type=1, shape=shape, size=size, mass=float(rng.uniform(0.5, 2.0)),
                               linear_damping=float(rng.uniform(0.98, 0.9995)), angular_damping=float(rng.uniform(0.98, 0.9995)),
                               offset_pos=[0, -0.5, 0] if has_bone else list(here + [0, -0.5, 0]), offset_rot=_quat(rng.normal(size=3), rng.uniform(-0.4, 0.4))))
            kind = 2 + s % 2 if sprung else (s + 2 * k) % 4
            lim = float(rng.uniform(0.3, 0.8))
            joints.append(dict(body_a=parent_body, body_b=len(bodies) - 1, position=list(here), rotation=list(rng.uniform(-0.5, 0.5, size=3)),
                               rotation_min=FREE_MIN if kind == 0 else [-lim, -lim / 2, -lim], rotation_max=FREE_MAX if kind == 0 else [lim, lim / 2, lim],
                               spring_rotation=[0, 0, 0] if kind == 1 else [float(rng.choice([50, 200] if sprung else [0, 50, 200])) for _ in range(3)],
                               spring_position=[0, 0, 0]))
            level[s].append((len(bodies) - 1, here))
            parent_bone, parent_body, at, parent_pos = (b if has_bone else parent_bone), len(bodies) - 1, np.zeros(3), here
    if cross:
        for s in range(n_strands):
            for k in range(n_dyn):
                (a, pa), (b, pb) = level[s][k], level[(s + 1) % n_strands][k]
                joints.append(dict(body_a=a, body_b=b, position=list((pa + pb) / 2), rotation=[0, 0, 0], position_min=[-0.3] * 3, position_max=[0.3] * 3,
                                   rotation_min=FREE_MIN, rotation_max=FREE_MAX, spring_rotation=[0, 0, 0], spring_position=[0, 0, 0]))
    if tie:
        (a, pa), (b, pb) = level[0][-1], level[2][-1]
        joints.append(dict(body_a=a, body_b=b, position=list((pa + pb) / 2), rotation=[0, 0, 0], position_min=[-0.6] * 3, position_max=[0.6] * 3,
                           rotation_min=FREE_MIN, rotation_max=FREE_MAX, spring_rotation=[0, 0, 0], spring_position=[0, 0, 0]))
    if free_body:
        parents.append(1); bind.append([0.0, -3.0, 0.0]); pos.append(pos[1] + [0, -3.0, 0])
        bodies.append(dict(bone=len(parents) - 1, type=1, shape=0, size=[0.5, 0, 0], mass=1.0, linear_damping=0.9, angular_damping=0.9))
    return _scene(parents, bind, bodies, joints, rng, n_verts, gravity=gravity, h=h, iterations=iterations)


def single_body(n_verts=64):
    """one dynamic body on a bone of its own, no joints: it falls"""
    rng = np.random.default_rng(5)
    parents, bind = [-1, 0, 1], [[0.0, 0.0, 0.0], [0.0, 16.0, 0.0], [0.0, -1.0, 0.0]]
    bodies = [dict(bone=2, type=1, shape=1, size=[0.3, 0.4, 0.5], mass=2.0, linear_damping=0.9, angular_damping=0.9, offset_pos=[0.1, -0.2, 0.0],
                   offset_rot=_quat([1, 2, 3], 0.3))]
    return _scene(parents, bind, bodies, [], rng, n_verts)


def falling_bodies(n_bodies, n_boned=100, seed=11, n_verts=300):
    """`n_bodies` dynamic bodies and no joint: the first `n_boned` on bones of their own under the head (their bones fall with them), the
    rest with bone = -1, placed by their offsets in model space. The largest table the LDS takes when no joint needs a multiplier."""
    rng = np.random.default_rng(seed)
    parents, bind, bodies = [-1, 0], [[0.0, 0.0, 0.0], [0.0, 16.0, 0.0]], []
    for k in range(n_bodies):
        at = [float(x) for x in rng.uniform(-4.0, 4.0, size=3)]
        bone = -1
        if k < n_boned:
            parents.append(1); bind.append(at)
            bone, at = len(parents) - 1, [0.0, -0.2, 0.0]
        shape = k % 3
        bodies.append(dict(bone=bone, type=1, shape=shape, size=[[0.4, 0, 0], [0.3, 0.4, 0.2], [0.2, 0.5, 0]][shape], mass=float(rng.uniform(0.5, 2.0)),
                           linear_damping=float(rng.uniform(0.5, 0.99)), angular_damping=float(rng.uniform(0.5, 0.99)), offset_pos=at,
                           offset_rot=_quat(rng.normal(size=3), rng.uniform(-0.5, 0.5))))
    return _scene(parents, bind, bodies, [], rng, n_verts)


def contents(n_verts=64, seed=12):
    """What a table may hold beside strands, in 8 bodies and 6 joints:
      body 0  follows nothing (bone = -1): an anchor fixed in model space            joint 0  0 - 1   the hanging body; sprung, limited
      body 1  dynamic, bone = -1: hangs from the anchor, overrides no bone            joint 1  2 - 3   rotation limits given max first
      body 2  follows bone 2                                                         joint 2  3 - 4   position play + rotation limits + springs
      body 3  dynamic on bone 3, linear and angular damping 1.0                       joint 3  2 - 5   between two followers: nothing to move
      body 4  dynamic on bone 4, damping 0.0                                          joint 4  5 - 6   the zero-inertia sphere under a follower, limits
      body 5  type 2 on bone 5 (dynamic + bone: follows)                                       of 0.02 rad and springs: K = 0, det K = 0, skipped
      body 6  dynamic on bone 6, a sphere of size 0 (no inertia: nothing turns it)    joint 5  6 - 7   a body under the sphere: K = its own inertia
      body 7  dynamic on bone 7"""
    rng = np.random.default_rng(seed)
    parents = [-1, 0, 1, 2, 3, 1, 5, 6]
    bind = [[0, 0, 0], [0, 16, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [-1, 0, 0], [0, -1, 0], [0, -1, 0]]
    bp = ik_ref.bind_positions(parents, bind)
    dyn = dict(type=1, shape=1, size=[0.3, 0.5, 0.3], mass=1.0, linear_damping=0.99, angular_damping=0.99, offset_pos=[0, -0.5, 0])
    bodies = [dict(bone=-1, type=0, shape=0, size=[0.2, 0, 0], mass=0.0, offset_pos=[0.0, 17.0, 1.0], offset_rot=_quat([0, 1, 0], 0.3)),
              dict(dyn, bone=-1, offset_pos=[0.0, 16.0, 1.0], offset_rot=_quat([1, 0, 1], 0.2), mass=1.5),
              dict(bone=2, type=0, shape=1, size=[0.2, 0.2, 0.2], mass=0.0, offset_rot=_quat([0, 0, 1], 0.2)),
              dict(dyn, bone=3, linear_damping=1.0, angular_damping=1.0, offset_rot=_quat([1, 2, 0], 0.3)),
              dict(dyn, bone=4, linear_damping=0.0, angular_damping=0.0, shape=2, size=[0.25, 0.6, 0], offset_rot=_quat([0, 1, 1], -0.2)),
              dict(bone=5, type=2, shape=0, size=[0.3, 0, 0], mass=1.0, offset_rot=_quat([1, 0, 0], 0.25)),
              dict(dyn, bone=6, shape=0, size=[0.0, 0, 0], mass=0.7, offset_pos=[0, -0.3, 0]),
              dict(dyn, bone=7, mass=2.0, shape=0, size=[0.4, 0, 0])]
    lim = dict(rotation_min=[-0.5, -0.25, -0.5], rotation_max=[0.5, 0.25, 0.5])
    joints = [dict(lim, body_a=0, body_b=1, position=[0.0, 16.6, 1.0], rotation=[0.1, 0.0, -0.2], spring_rotation=[100, 100, 100]),
              dict(body_a=2, body_b=3, position=list(bp[3]), rotation=[0.2, -0.1, 0.1], rotation_min=[0.6, 0.3, 0.6], rotation_max=[-0.6, -0.3, -0.6], spring_rotation=[50, 50, 50]),
              dict(lim, body_a=3, body_b=4, position=list(bp[4]), rotation=[-0.1, 0.2, 0.3], position_min=[-0.1, -0.05, -0.1], position_max=[0.1, 0.05, 0.1],
                   spring_rotation=[200, 50, 200]),
              dict(lim, body_a=2, body_b=5, position=list((bp[2] + bp[5]) / 2), rotation=[0.3, 0.1, 0.0], spring_rotation=[50, 50, 50]),
              dict(body_a=5, body_b=6, position=list(bp[6]), rotation=[0.0, 0.3, 0.1], rotation_min=[-0.02] * 3, rotation_max=[0.02] * 3, spring_rotation=[100, 50, 100]),
              dict(lim, body_a=6, body_b=7, position=list(bp[7]), rotation=[0.1, 0.1, 0.1], spring_rotation=[50, 200, 50])]
    return _scene(parents, bind, bodies, joints, rng, n_verts)


def gimbal(n_verts=64, seed=13):
    """two dynamic bodies under a following one; the first joint is locked at the gimbal angle (rotation_min.y = rotation_max.y = pi / 2),
    where the Euler angles' x and z fall together and the branch euler_xyz takes turns on the last bit of one matrix entry"""
    rng = np.random.default_rng(seed)
    parents, bind = [-1, 0, 1, 2, 3], [[0, 0, 0], [0, 16, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0]]
    bp = ik_ref.bind_positions(parents, bind)
    dyn = dict(type=1, shape=1, size=[0.3, 0.5, 0.3], mass=1.0, linear_damping=0.99, angular_damping=0.99, offset_pos=[0, -0.5, 0])
    bodies = [dict(bone=2, type=0, shape=0, size=[0.2, 0, 0], mass=0.0), dict(dyn, bone=3, offset_rot=_quat([1, 1, 0], 0.2)), dict(dyn, bone=4, shape=2, size=[0.25, 0.6, 0])]
    joints = [dict(body_a=0, body_b=1, position=list(bp[3]), rotation=[0.1, 0.2, 0.0], rotation_min=[-0.5, PI / 2, -0.5], rotation_max=[0.5, PI / 2, 0.5], spring_rotation=[50, 50, 50]),
              dict(body_a=1, body_b=2, position=list(bp[4]), rotation=[0.0, 0.0, 0.1], rotation_min=[-0.5, -0.25, -0.5], rotation_max=[0.5, 0.25, 0.5], spring_rotation=[50, 0, 50])]
    return _scene(parents, bind, bodies, joints, rng, n_verts)


def _scene(parents, bind, bodies, joints, rng, n_verts, gravity=None, h=0.0, iterations=0):
    parents = np.array(parents, dtype=np.int32)
    bind = np.array(bind, dtype=np.float32)
    B = len(parents)
    bp = ik_ref.bind_positions(parents, bind)
    # a small mesh: every vertex near a bone, BDEF1 / BDEF2 on it and its parent
    vb = (np.arange(n_verts) * B // n_verts) if n_verts >= B else rng.integers(0, B, size=n_verts)
    vb = np.maximum(vb, 0)
    pos = (bp[vb] + rng.uniform(-0.3, 0.3, size=(n_verts, 3)) + [0, -0.5, 0]).astype(np.float32)
    nrm = rng.normal(size=(n_verts, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    jn = np.zeros((n_verts, 4), dtype=np.uint16)
    wt = np.zeros((n_verts, 4), dtype=np.uint8)
    jn[:, 0] = vb
    jn[:, 1] = np.maximum(parents[vb], 0)
    w0 = rng.integers(128, 256, size=n_verts)
    w0[::3] = 255
    wt[:, 0], wt[:, 1] = w0, 255 - w0
    inv_bind = np.zeros((B, 16), dtype=np.float32)
    inv_bind[:, 0] = inv_bind[:, 5] = inv_bind[:, 10] = inv_bind[:, 15] = 1
    inv_bind[:, 12:15] = -bp.astype(np.float32)
    mesh = dict(pos=pos, nrm=nrm, joints=jn, weights=wt, parents=parents, bind=bind, inv_bind=inv_bind)
    table = physics_ref.make_table(bodies, joints, gravity=gravity, h=h, iterations=iterations)
    return dict(mesh=mesh, table=table, parents=parents, bind=bind, B=B, extent=ik_ref.extent(bp), bodies=bodies, joints=joints)


def pose(scene, seed, amount=1.0):
    """A local pose (q [B,4], t [B,3]) that moves the centre, turns the head and bends every bone a little; the dynamic bones' own rotations are overridden
    by physics but still steer the un-overridden matrices their children keep."""
    rng = np.random.default_rng(1000 + seed)
    B = scene["B"]
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-0.1, 0.1, size=B) * amount
    a[0], a[1] = rng.uniform(-0.02, 0.02) * amount, rng.uniform(-0.08, 0.08) * amount     # (the head is 16 units above the centre)
    q = np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1).astype(np.float32)
    t = np.zeros((B, 3), dtype=np.float32)
    t[0] = rng.uniform(-0.15, 0.15, size=3) * amount
    return q, t


def ik_scene(n_verts=96):
    """An arm (upper, lower, effector) solved by IK towards a goal bone, a following body on the lower arm and a strand of three dynamic
    bodies hanging from it: physics must read the pose AFTER IK."""
    rng = np.random.default_rng(9)
    parents = [-1, 0, 1, 2, 3, 0, 3, 6, 7]
    bind = [[0, 0, 0], [0, 16, 0], [1, 0, 0], [2, 0, 0], [2, 0, 0], [4.2, 15.2, 0.8], [1, -0.2, 0], [0, -1, 0], [0, -1, 0]]
    pos = ik_ref.bind_positions(parents, bind)
    bodies = [dict(bone=3, type=0, shape=1, size=[1.0, 0.2, 0.2], mass=0.0, offset_pos=[1, 0, 0])]
    joints = []
    for k, b in enumerate((6, 7, 8)):
        bodies.append(dict(bone=b, type=1, shape=2, size=[0.25, 0.5, 0], mass=1.0, linear_damping=0.99, angular_damping=0.99, offset_pos=[0, -0.5, 0],
                           offset_rot=_quat([0, 0, 1], 0.1 * k)))
        joints.append(dict(body_a=k, body_b=k + 1, position=list(pos[b]), rotation=[0.1, 0.2, -0.1], rotation_min=[-0.6, -0.3, -0.6], rotation_max=[0.6, 0.3, 0.6],
                           spring_rotation=[50, 0, 50], spring_position=[0, 0, 0]))
    sc = _scene(parents, bind, bodies, joints, rng, n_verts)
    sc["chains"] = [dict(goal=5, effector=4, loops=8, limit_angle=1.0, links=[dict(bone=3, min=None, max=None), dict(bone=2, min=None, max=None)])]
    return sc


def ik_pose(scene, seed):
    """the goal bone moves (so the arm does), everything else as pose()"""
    q, t = pose(scene, seed)
    t[5] = np.random.default_rng(50 + seed).uniform(-0.4, 0.4, size=3)
    return q, t


def motion(scene, seed, n_keys=6):
    """A gentle motion (rz_animation fields): the centre drifts, the head and every bone without a dynamic body turn a little, a key every
    3 frames."""
    rng = np.random.default_rng(300 + seed)
    t = scene["table"]
    driven = set(int(b) for b in t["bone"][physics_ref.is_dynamic(t)] if b >= 0)
    bones = np.array([b for b in range(scene["B"]) if b not in driven][:24], dtype=np.int32)
    n = len(bones)
    ax = rng.normal(size=(n, n_keys, 3))
    ax /= np.linalg.norm(ax, axis=2, keepdims=True)
    a = rng.uniform(-0.08, 0.08, size=(n, n_keys))
    a[0] *= 0.25                    # (the head is 16 units above the centre)
    kq = np.concatenate([ax * np.sin(a / 2)[..., None], np.cos(a / 2)[..., None]], axis=2).astype(np.float32)
    kp = np.zeros((n, n_keys, 3), dtype=np.float32)
    kp[0] = rng.uniform(-0.15, 0.15, size=(n_keys, 3))
    return dict(track_bone=bones, key_off=(np.arange(n + 1) * n_keys).astype(np.uint32), key_frame=np.tile(np.arange(n_keys, dtype=np.float32) * 3, n),
                key_rot=kq.reshape(-1, 4), key_pos=kp.reshape(-1, 3), key_interp=rng.integers(20, 107, size=(n * n_keys, 16)).astype(np.uint8))


def write_pmx(scene, seed=0):
    """A PMX 2.0 byte stream of the scene with its rigid-body and joint sections (tests/pmx_synth.py writes none): shapePosition = the bone's
    bind position + the body's offset, shapeRotation = random Euler angles. Returns (bytes, the table a loader must derive from it:
    offsets = inverseBind x T(shapePosition) R(Quat.fromEuler(shapeRotation)))."""
    import struct
    rng = np.random.default_rng(700 + seed)

    def text(x):
        b = x.encode("utf-16le")
        return struct.pack("<i", len(b)) + b
    m, t = scene["mesh"], scene["table"]
    B, V = scene["B"], len(scene["mesh"]["pos"])
    out = bytearray(b"PMX ") + struct.pack("<f", 2.0) + bytes([8, 0, 0, 4, 1, 1, 2, 2, 1])
    out += text("physics scene") + text("") + text("") + text("")
    out += struct.pack("<i", V)
    for v in range(V):
        out += m["pos"][v].tobytes() + m["nrm"][v].tobytes() + struct.pack("<2f", 0.5, 0.5)
        out += bytes([1]) + struct.pack("<hhf", int(m["joints"][v, 0]), int(m["joints"][v, 1]), float(m["weights"][v, 0]) / 255.0) + struct.pack("<f", 1.0)
    tri = (np.arange(3 * (V // 3)) % V).astype(np.int32)
    out += struct.pack("<i", len(tri)) + tri.tobytes()
    out += struct.pack("<i", 0)
    out += struct.pack("<i", 1) + text("body") + text("") + struct.pack("<11f", *([0.5] * 11)) + bytes([0x10])
    out += struct.pack("<5f", 0, 0, 0, 1, 1.25) + struct.pack("<bb", -1, -1) + bytes([0, 1, 0]) + text("") + struct.pack("<i", len(tri))
    bp = ik_ref.bind_positions(scene["parents"], scene["bind"]).astype(np.float32)
    out += struct.pack("<i", B)
    for b in range(B):
        out += text("bone%d" % b) + text("") + bp[b].tobytes() + struct.pack("<h", int(scene["parents"][b])) + struct.pack("<i", 0)
        out += struct.pack("<H", 0) + struct.pack("<3f", 0, 1, 0)
    out += struct.pack("<i", 0) + struct.pack("<i", 0)                   # morphs, display frames
    nb, nj = t["n_bodies"], t["n_joints"]
    want = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in t.items()}
    out += struct.pack("<i", nb)
    for b in range(nb):
        bone = int(t["bone"][b])
        sp = (t["offset_pos"][b] + (bp[bone] if bone >= 0 else 0)).astype(np.float32)
        sr = rng.uniform(-0.6, 0.6, size=3).astype(np.float32)
        out += text("body%d" % b) + text("") + struct.pack("<h", bone) + bytes([int(t["group"][b])]) + struct.pack("<H", int(t["mask"][b])) + bytes([int(t["shape"][b])])
        out += t["size"][b].tobytes() + sp.tobytes() + sr.tobytes()
        out += struct.pack("<5f", t["mass"][b], t["linear_damping"][b], t["angular_damping"][b], t["restitution"][b], t["friction"][b]) + bytes([int(t["type"][b])])
        want["offset_pos"][b] = sp - (bp[bone] if bone >= 0 else np.float32(0))
        want["offset_rot"][b] = physics_ref.quat_from_pmx_euler(sr).astype(np.float32)
    out += struct.pack("<i", nj)
    for j in range(nj):
        out += text("joint%d" % j) + text("") + bytes([0]) + struct.pack("<bb", int(t["body_a"][j]), int(t["body_b"][j]))
        for k in physics_ref.JOINT_F:
            out += np.asarray(t[k][j], dtype=np.float32).tobytes()
    return bytes(out), want


CROWD = dict(n_strands=4, n_dyn=5, base=True, seed=7, n_verts=96, free_body=True)
PARAMS = dict(h=1 / 120, iterations=7, gravity=(3.0, -40.0, 25.0))        # every parameter of a table away from its default
LDS_LIMIT, LDS_PER_BODY, LDS_PER_JOINT = 160 * 1024, 96, 12


def lds_bytes(n_bodies, n_joints):
    """include/reze_deform.h: 96 B per body, + 12 B per joint once the joints outnumber the lanes (64 when the table fits a wave, else 256);
    with more than 64 bodies the block is 256"""
    return n_bodies * LDS_PER_BODY + (n_joints * LDS_PER_JOINT if n_joints > (64 if n_bodies <= 64 else 256) else 0)


MOST_STRANDS = (LDS_LIMIT - LDS_PER_BODY) // (LDS_PER_BODY + LDS_PER_JOINT)      # strands of one body under one shared base: 1516
MOST_BODIES = LDS_LIMIT // LDS_PER_BODY                                           # 1706

SCENES = {
    "one body": lambda: single_body(),
    "63 bodies": lambda: strands(9, 6, base=True, seed=2, n_verts=128),
    "65 bodies": lambda: strands(13, 4, base=True, seed=3, n_verts=130),
    "wide colour": lambda: strands(260, 1, base=False, seed=4, n_verts=300, sprung=True),
    "skirt": lambda: strands(8, 5, base=True, seed=8, n_verts=100, sprung=True, cross=True),     # 48 bodies, 80 joints: one wave, lanes stride
    "one joint": lambda: strands(1, 1, base=True, seed=6, n_verts=64),
    "crowd": lambda: strands(**CROWD),
    "ik": lambda: ik_scene(),
    # the table's parameters: all three set, and one at a time (the rest of the table is the "crowd" scene's)
    "params": lambda: strands(**CROWD, **PARAMS),
    "params h": lambda: strands(**CROWD, h=PARAMS["h"]),
    "params iterations": lambda: strands(**CROWD, iterations=1),       # (1, not 7: 7 passes move these strands by 32 x the bar against 4, 1 pass by 208 x)
    "params gravity": lambda: strands(**CROWD, gravity=PARAMS["gravity"]),
    # the counts at which rz_launch_physics changes its form (FORMS below)
    "64 bodies": lambda: strands(8, 7, base=True, seed=21, n_verts=128),
    "64 bodies 63 joints": lambda: strands(9, 7, base=False, seed=22, n_verts=128, sprung=True),
    "64 joints": lambda: strands(8, 4, base=True, seed=23, n_verts=96, sprung=True, cross=True),
    "65 joints": lambda: strands(8, 4, base=True, seed=24, n_verts=96, sprung=True, cross=True, tie=True),
    "65 bodies 64 joints": lambda: strands(16, 4, base=False, seed=25, n_verts=130, sprung=True),
    "256 joints": lambda: strands(128, 2, base=True, seed=26, n_verts=400, sprung=True),
    "257 joints": lambda: strands(257, 1, base=True, seed=27, n_verts=520, sprung=True),
    # the largest tables the LDS takes
    # (the hierarchy solve takes 1 517 bones, 108 B of LDS each: 1 000 strands drive bones, the bodies of the other 516 have none)
    "most strands": lambda: strands(MOST_STRANDS, 1, base=False, seed=28, n_verts=600, sprung=True, boned=1000),
    "most bodies": lambda: falling_bodies(MOST_BODIES),
    "contents": lambda: contents(),
    "gimbal": lambda: gimbal(),
}
# name: (bodies, joints, lanes per workgroup, joints in registers?) — what the upload must choose for the scene
FORMS = {
    "64 bodies": (64, 56, 64, 1), "64 bodies 63 joints": (64, 63, 64, 1), "64 joints": (40, 64, 64, 1), "65 joints": (40, 65, 64, 0),
    "65 bodies 64 joints": (65, 64, 256, 1), "256 joints": (384, 256, 256, 1), "257 joints": (514, 257, 256, 0),
    "most strands": (MOST_STRANDS + 1, MOST_STRANDS, 256, 0), "most bodies": (MOST_BODIES, 0, 256, 1),
}
EDGE_CALLS = (1, 10, 10)            # the largest tables run the crowd's shorter sequence
_memo = {}

NODE_H, NODE_MAX_SUBSTEPS = 1 / 75, 10
NODE_TIMES = tuple(16.7 * k for k in range(13))         # the engine clock (ms) of the Node end-to-end frames: step(0), step(16.7), ...


def node_substeps(times=NODE_TIMES):
    """what Engine { devicePhysics } owes per frame: the clock's advance joins the accumulator, min(10, floor(acc / h)) substeps leave it
    (the same double arithmetic as host/src/engine.ts: physicsSubsteps())"""
    import math
    acc, last, out = 0.0, 0.0, []
    for now in times:
        if now > last:
            acc += (now - last) / 1000
        last = now
        owed = math.floor(acc / NODE_H)
        acc -= owed * NODE_H
        out.append(min(NODE_MAX_SUBSTEPS, owed))
    return tuple(out)


def node_case():
    """The Node end-to-end test's scene: the 'crowd' strands as a PMX file, run with the table its loader derives from the file, under one
    fixed local pose (no translations: the engine sends none without a motion). Returns (scene, pmx bytes, q [B,4])."""
    if "node" not in _memo:
        sc = scene("crowd")
        data, want = write_pmx(sc)
        q, _ = pose(sc, 70, amount=2.0)
        _memo["node"] = (dict(sc, table=want), data, q)
    return _memo["node"]


def bone_morph_case():
    """The bone-morph GPU test's inputs: (scene, the morph, its weight, the un-morphed local poses); the morph moves body 0's bone, the
    base of the first strand, whose body follows it."""
    sc = scene("crowd")
    base_bone = int(sc["table"]["bone"][0])
    bm = dict(morph=np.array([0], dtype=np.uint32), bone=np.array([base_bone], dtype=np.uint32), t=np.array([[0.3, 0.1, -0.2]], dtype=np.float32),
              q=np.array([[0.0, 0.0, np.sin(0.2), np.cos(0.2)]], dtype=np.float32))
    return sc, bm, np.array([0.7], dtype=np.float32), [pose(sc, 20 + k) for k in range(3)]


def scene(name):
    if name not in _memo:
        _memo[name] = SCENES[name]()
    return _memo[name]


CALLS = (1, 10, 10, 10, 10)        # substeps per call of the standard sequence: 1, 10, then 3 x 10, the pose changing between calls
CROWD_CALLS = (1, 10, 10)


def crowd_frames(instance, call):
    """every instance at its own frame, one frame on per call"""
    return 1.3 + 2.1 * instance + 1.0 * call


def local_crowd_pose(scene, instance, call):
    """the crowds fed through rz_set_pose_local: every instance at a pose of its own, a new one per call"""
    return pose(scene, 200 + 10 * call + instance)


def world_of(scene, q, t, chains=(), dtype=np.float64):
    return ik_ref.solve(scene["parents"], scene["bind"], q, t, chains, dtype=dtype)[0]


def run_reference(scene, poses, calls=CALLS, chains=(), dtype=np.float64, sim=None):
    """The standard sequence on one instance: per call (float64 world with overrides applied [B,16], state [nb,13]). `poses` has one local
    pose per call."""
    sim = sim or physics_ref.Sim(scene["table"], scene["parents"], scene["bind"], dtype=dtype)
    out = []
    for (q, t), n in zip(poses, calls):
        w = world_of(scene, q, t, chains, dtype=dtype)
        ovr = sim.step(w, n)
        out.append((physics_ref.apply_overrides(w, ovr), sim.state13().astype(np.float64)))
    return out


def conditioning(scene, poses, calls=CALLS, chains=()):
    """largest float32-probe deviation from the float64 run over the whole horizon (positions and world-matrix entries), in units of extent"""
    a = run_reference(scene, poses, calls, chains)
    b = run_reference(scene, poses, calls, chains, dtype=np.float32)
    worst = 0.0
    for (wa, sa), (wb, sb) in zip(a, b):
        worst = max(worst, float(np.abs(wa - wb).max()), float(np.abs(sa[:, :3] - sb[:, :3]).max()))
    return worst / scene["extent"]


# ---- the host half's stand-alone program (tests/physics_table_main.cpp around reze-engine_amd/csrc/physics_table.h) ----

def build_table_tool(folder):
    """the table program under ASan and UBSan"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(folder / "physics_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(root, "tests", "physics_table_main.cpp")])
    return exe


def dump_table(t, parents, bind, column=True):
    """the program's input for table t; column=False: spring_position is written, and handed on as NULL"""
    rows = ["%d %d %d %.9g %d %d %d" % (len(parents), t["n_bodies"], t["n_joints"], float(t["h"]), t["iterations"], 0 if t["gravity"] is None else 1, 1 if column else 0)]
    if t["gravity"] is not None:
        rows.append(" ".join("%.9g" % x for x in t["gravity"]))
    rows.append(" ".join(str(int(p)) for p in parents))
    rows.append(" ".join("%.9g" % x for x in np.asarray(bind, dtype=np.float32).reshape(-1)))
    for b in range(t["n_bodies"]):
        rows.append(" ".join([str(int(t["bone"][b])), str(int(t["type"][b])), str(int(t["shape"][b]))] + ["%.9g" % x for x in
                    list(t["size"][b]) + list(t["offset_pos"][b]) + list(t["offset_rot"][b]) + [t["mass"][b], t["linear_damping"][b], t["angular_damping"][b]]]))
    for j in range(t["n_joints"]):
        rows.append(" ".join([str(int(t["body_a"][j])), str(int(t["body_b"][j]))] + ["%.9g" % x for k in
                    ("position", "rotation", "position_min", "position_max", "rotation_min", "rotation_max", "spring_rotation", "spring_position") for x in t[k][j]]))
    return "\n".join(rows) + "\n"
