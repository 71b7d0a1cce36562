"""Hand-laid scenes for the after-physics stage (rz_upload_after_physics; tests/after_ref.py): skeletons small enough that every GPU case
runs in a few seconds, each laid out so that one edge of the stage is the only thing it can get wrong. STATIC lists the scenes fed through
rz_set_pose_local + rz_override_world — per scene the skeleton, a small mesh with vertices on every bone (follow_scenes' helpers), the
ordered list `order`, and per instance a local pose and an override set; SOURCES are the three cases of (h), whose pose comes from a bone
morph, rz_set_pose_sampled and rz_set_pose_blended; physics() is (j), whose overrides the physics step writes.
tests/test_after_cpu.py checks the conditioning of every one of them and that every one moves.

  (a)  a helper beside the chain: bone 5 under bone 1 appends rotation at ratio 0.5 from the overridden bone 3 and is not below it
  (b)  ratios -1, 0.3 and 1.7 (rotation clamped, move unclamped) from one overridden bone, append move on, t_b != 0
  (c)  listed bones 2 and 3 below the overridden bone 1, no append, own keyed rotation and translation; run with rz_override_follow on
       and off against the same reference
  (d)  three levels against index order: b1 = 4 appends from the overridden bone 3, b2 = 5 is a child of b1, b3 = 1 appends from b1 and
       has the lower index but transform level 1, bone 6 below b3; order [4, 5, 1, 6]
  (e)  a crowd of 3 with three override sets: one empty, one that overrides a listed bone (skipped, keeps O), one plain
  (f1) 257 entries in level 0 and 65 in level 1      (f2) 256 and 64
  (f3) 300 + 300 + 42 entries in three levels: more than 512 entries (beyond the two register slots per thread), bones beyond 512
  (f4) a chain of 20 listed bones, 20 levels          (f5) a 600-bone skeleton with the listed bones at indices >= 590
  (g)  a listed root that appends from an overridden ROOT, and a listed child of it
  (h)  pose sources: a bone morph on the listed bone; the listed bone keyed under rz_set_pose_sampled; rz_set_pose_blended
  (i)  an IK table resident, the helper appends from an IK link: its final rotation is the solved one
  (j)  physics strands (physics_scenes.strands) with a helper per strand appending from a dynamic body's bone
"""
import numpy as np

import after_ref as ar
import follow_ref as fr
import follow_scenes as fs
import ik_ref
import physics_scenes as ps


def _scene(name, parents, bind, sets, seed, order, ap=None, ratio=None, move=None, chains=(), per_bone=3):
    B = len(parents)
    ap = [-1] * B if ap is None else ap
    ratio = [1.0] * B if ratio is None else ratio
    move = [0] * B if move is None else move
    sc = fs._scene(name, parents, bind, sets, seed, ap=ap, ratio=ratio, move=move, chains=chains, per_bone=per_bone)
    sc["order"] = np.array(order, dtype=np.uint32)
    return sc


def frame_without(sc, inst, follow=False, dtype=np.float64):
    """F of one instance: the frame as it leaves the overrides today"""
    S = fs.solved(sc, inst["q"], inst["t"], dtype=dtype)
    if follow:
        return fr.follow(sc["parents"], S, inst["bones"], inst["mats"], dtype=dtype)
    return fr.replaced(S, inst["bones"], inst["mats"]).astype(dtype)


def reference(sc, inst, follow=False, dtype=np.float64):
    """the definition's world matrices [B,16] of one instance of a context that holds override entries"""
    F = frame_without(sc, inst, follow, dtype)
    return ar.solve(sc["parents"], sc["bind"], inst["q"], inst["t"], sc["ap"], sc["ratio"], sc["move"], F, inst["bones"], sc["order"], dtype=dtype)


def _helpers(parents, ap, ratio, move, n, under, source, rng, with_move=True):
    """n helper bones under `under` that append from `source`; returns their indices"""
    first = len(parents)
    for k in range(n):
        parents.append(under)
        ap.append(source)
        ratio.append(float(rng.choice([0.5, -0.5, 1.0, 0.3, 1.7, -1.0])))
        move.append(int(with_move and k % 2))
    return list(range(first, first + n))


def _plain(parents, ap, ratio, move, under):
    """one bone per entry of `under`, below it, without append; returns their indices"""
    first = len(parents)
    for u in under:
        parents.append(u); ap.append(-1); ratio.append(1.0); move.append(0)
    return list(range(first, first + len(under)))


def scene_a():
    return _scene("a", [-1, 0, 1, 2, 3, 1], fs._bind(np.random.default_rng(11), 6), [[3]], 207, [5],
                  ap=[-1, -1, -1, -1, -1, 3], ratio=[1, 1, 1, 1, 1, 0.5])


def scene_b():
    return _scene("b", [-1, 0, 1, 0, 0, 0], fs._bind(np.random.default_rng(12), 6), [[2]], 202, [3, 4, 5],
                  ap=[-1, -1, -1, 2, 2, 2], ratio=[1, 1, 1, -1.0, 0.3, 1.7], move=[0, 0, 0, 1, 1, 1])


def scene_c():
    return _scene("c", [-1, 0, 1, 2, 0], fs._bind(np.random.default_rng(13), 5), [[1]], 203, [2, 3])


def scene_d():
    #          0   1  2  3  4  5  6
    parents = [-1, 0, 0, 2, 0, 4, 1]
    return _scene("d", parents, fs._bind(np.random.default_rng(14), 7), [[3]], 204, [4, 5, 1, 6],
                  ap=[-1, 4, -1, -1, 3, -1, -1], ratio=[1, 0.7, 1, 1, 0.5, 1, 1], move=[0, 1, 0, 0, 0, 0, 0])


def scene_e():
    # bone 5 appends from 3, bone 6 (below 5) appends from 5; instance 1 overrides the listed bone 5 itself
    parents = [-1, 0, 1, 2, 3, 1, 5, 0]
    return _scene("e", parents, fs._bind(np.random.default_rng(15), 8), [[], [3, 5], [3, 7]], 205, [5, 6],
                  ap=[-1, -1, -1, -1, -1, 3, 5, -1], ratio=[1, 1, 1, 1, 1, 0.5, -0.8, 1], move=[0, 0, 0, 0, 0, 0, 1, 0])


def _wide(name, sizes, seed):
    """root 0, the overridden bone 1 below it; level 0: sizes[0] helpers under the root appending from bone 1; level l > 0: sizes[l] plain
    bones below the first bones of the level before"""
    rng = np.random.default_rng(seed)
    parents, ap, ratio, move = [-1, 0], [-1, -1], [1.0, 1.0], [0, 0]
    level = _helpers(parents, ap, ratio, move, sizes[0], 0, 1, rng)
    order = list(level)
    for n in sizes[1:]:
        level = _plain(parents, ap, ratio, move, level[:n])
        order += level
    return _scene(name, parents, fs._bind(rng, len(parents)), [[1]], seed + 1000, order, ap=ap, ratio=ratio, move=move, per_bone=1)


def scene_f1():
    return _wide("f1", (257, 65), 21)


def scene_f2():
    return _wide("f2", (256, 64), 22)


def scene_f3():
    return _wide("f3", (300, 300, 42), 23)


def scene_f4():
    parents = [-1, 0] + list(range(1, 21))
    return _scene("f4", parents, fs._bind(np.random.default_rng(24), 22) * 0.5, [[1]], 224, list(range(2, 22)))


def scene_f5():
    rng = np.random.default_rng(25)
    parents, depth = [-1], [0]
    for i in range(1, 590):
        p = int(rng.integers(0, i))
        while depth[p] >= 7:
            p = parents[p]
        parents.append(p); depth.append(depth[p] + 1)
    ap, ratio, move = [-1] * 590, [1.0] * 590, [0] * 590
    hs = _helpers(parents, ap, ratio, move, 6, 7, 3, rng)                  # 590..595 under bone 7, from the overridden bone 3
    below = _plain(parents, ap, ratio, move, hs[:4])                       # 596..599
    return _scene("f5", parents, fs._bind(rng, 600), [[3]], 225, hs + below, ap=ap, ratio=ratio, move=move, per_bone=1)


def scene_g():
    # roots 0 (overridden) and 1 (listed, appends rotation and move from the root 0), bone 2 below 1 (listed), bone 3 below 0
    return _scene("g", [-1, -1, 1, 0], fs._bind(np.random.default_rng(16), 4), [[0]], 206, [1, 2],
                  ap=[-1, 0, -1, -1], ratio=[1, 0.6, 1, 1], move=[0, 1, 0, 0])


def scene_i():
    # follow_scenes' arm (links 2 and 3, effector 4, goal 5; bone 6 off the lower arm, overridden); helper 9 under the root appends from link
    # 3 — the first solve read the solved rotation too, so it must come out where it was — and helper 10 from bone 6, whose final local
    # rotation is taken against the SOLVED link 3
    parents = [-1, 0, 1, 2, 3, 0, 3, 6, 7, 0, 0]
    bind = [[0, 0, 0], [0, 16, 0], [1, 0, 0], [2, 0, 0], [2, 0, 0], [4.2, 15.2, 0.8], [1, -0.2, 0], [0, -1, 0], [0, -1, 0], [-1, 14, 0.5], [-2, 13, 0.5]]
    chains = [dict(goal=5, effector=4, loops=8, limit_angle=1.0, links=[dict(bone=3, min=None, max=None), dict(bone=2, min=None, max=None)])]
    rng = np.random.default_rng(209)
    B = len(parents)
    sc = dict(name="i", parents=np.asarray(parents, dtype=np.int32), bind=np.asarray(bind, dtype=np.float32), B=B,
              ap=np.array([-1] * 9 + [3, 6], dtype=np.int32), ratio=np.array([1.0] * 9 + [0.8, 1.0], dtype=np.float32), move=np.array([0] * 10 + [1], dtype=np.uint8),
              chains=chains, expect=None, order=np.array([9, 10], dtype=np.uint32))
    sc["mesh"] = fs._mesh(parents, bind, rng)
    q = fs._quats(rng, B, 0.1)
    t = np.zeros((B, 3), dtype=np.float32)
    t[0] = rng.uniform(-0.15, 0.15, size=3)
    t[5] = rng.uniform(-0.4, 0.4, size=3)
    t[9:11] = rng.uniform(-0.2, 0.2, size=(2, 3))
    sc["instances"] = [dict(q=q, t=t, **_override(sc, q, t, [6], rng))]
    return sc


def _override(sc, q, t, bones, rng, swing=0.8, shift=0.6):
    """an override set on the solved pose of (q, t): follow_scenes._instance's recipe"""
    S = fs.solved(sc, q, t)
    mats = np.zeros((len(bones), 16), dtype=np.float32)
    for k, b in enumerate(bones):
        M = S[b].reshape(4, 4).T.copy()
        M[:3, :3] = ik_ref._qmat(fs._quats(rng, 1, swing)[0].astype(np.float64), np.float64) @ M[:3, :3]
        M[:3, 3] += rng.uniform(-shift, shift, size=3)
        mats[k] = M.T.reshape(16)
    return dict(bones=np.array(bones, dtype=np.uint32), mats=mats)


STATIC = dict(a=scene_a, b=scene_b, c=scene_c, d=scene_d, e=scene_e, f1=scene_f1, f2=scene_f2, f3=scene_f3, f4=scene_f4, f5=scene_f5, g=scene_g, i=scene_i)
_memo = {}


def scene(name):
    if name not in _memo:
        _memo[name] = physics() if name == "j" else physics(node=True) if name == "j node" else STATIC[name]()
    return _memo[name]


# ---- (h): the three other pose sources, on the skeleton of (a) ----

SOURCES = ("bone morph", "sampled", "blended")
H_FRAME = 4.3
H_STATE = (0, 4.3, 1, 7.9, 0.35)          # clip a, frame a, clip b, frame b, blend


def _clip(sc, seed, n_keys=5):
    """a motion that keys every bone of (a) — rotations of up to 0.5 rad, translations — a key every 3 frames, its own Bezier curves"""
    rng = np.random.default_rng(seed)
    B = sc["B"]
    kq = np.stack([fs._quats(rng, n_keys, 0.5) for _ in range(B)])
    kp = rng.uniform(-0.2, 0.2, size=(B, n_keys, 3)).astype(np.float32)
    return dict(track_bone=np.arange(B, dtype=np.int32), key_off=(np.arange(B + 1) * n_keys).astype(np.uint32), key_frame=np.tile(np.arange(n_keys, dtype=np.float32) * 3, B),
                key_rot=kq.reshape(-1, 4), key_pos=kp.reshape(-1, 3), key_interp=rng.integers(20, 107, size=(B * n_keys, 16)).astype(np.uint8))


def source_case(kind):
    """(scene, extras, instance) of one pose source: the instance's q / t are the float64 local pose after bone morphs the source yields;
    extras carries what the GPU test uploads"""
    key = "h " + kind
    if key in _memo:
        return _memo[key]
    import motion_ref
    from helpers import bone_morph_reference, sample_reference
    sc = dict(scene("a"))
    rng = np.random.default_rng((300, 301, 341)[SOURCES.index(kind)])
    extras = {}
    if kind == "bone morph":
        base = sc["instances"][0]
        bm = dict(morph=np.array([0, 1], dtype=np.uint32), bone=np.array([5, 5], dtype=np.uint32), t=np.array([[0.3, 0.1, -0.2], [-0.1, 0.2, 0.1]], dtype=np.float32),
                  q=np.array([[0.0, 0.0, np.sin(0.2), np.cos(0.2)], [np.sin(0.15), 0.0, 0.0, np.cos(0.15)]], dtype=np.float32))
        mw = np.array([0.7, 0.4], dtype=np.float32)
        q, t = bone_morph_reference(base["q"], base["t"], bm["morph"], bm["bone"], bm["t"], bm["q"], mw)
        extras = dict(bm=bm, mw=mw, q0=base["q"], t0=base["t"])
    elif kind == "sampled":
        clip = _clip(sc, 31)
        q, t = sample_reference(clip, float(np.float32(H_FRAME)), sc["B"], 0)[:2]
        extras = dict(clips=[clip])
    else:
        clips = [_clip(sc, 32), _clip(sc, 33)]
        st = (H_STATE[0], float(np.float32(H_STATE[1])), H_STATE[2], float(np.float32(H_STATE[3])), float(np.float32(H_STATE[4])))
        q, t = motion_ref.blend_reference(clips, st, sc["B"], 0)[:2]
        extras = dict(clips=clips)
    inst = dict(q=np.asarray(q, dtype=np.float64), t=np.asarray(t, dtype=np.float64), **_override(sc, q, t, [3], rng))
    sc["name"] = key
    _memo[key] = (sc, extras, inst)
    return _memo[key]


# ---- (j): the physics step writes the overrides ----

SUBSTEPS = 3


def physics(node=False):
    """3 strands of 6 dynamic bodies under 3 following ones (follow_scenes' table, under a strong side wind and steps of 1/30 s so that
    three substeps swing the strands visibly); per strand a helper bone under the strand's base bone that appends the rotation (the
    second: -0.7 of it, with move) of the strand's last dynamic bone, and a plain listed bone four units below every helper. node: the table's parameters at their defaults, which
    is all a PMX file can say (the Node end-to-end run)"""
    base = ps.strands(3, 6, base=True, seed=41, n_verts=64, sprung=True)
    parents, bind = [int(p) for p in base["parents"]], [list(map(float, b)) for b in base["bind"]]
    dyn = [int(b["bone"]) for b in base["bodies"] if b["type"] == 1]
    B0 = len(parents)
    ap, ratio, move, order = [-1] * B0, [1.0] * B0, [0] * B0, []
    for s in range(3):
        src = dyn[6 * s + 5]
        top = parents[dyn[6 * s]]
        parents.append(top); bind.append([0.5, -0.3, 0.2 * s]); ap.append(src); ratio.append(1.0 if s != 1 else -0.7); move.append(int(s == 1))
        order.append(len(parents) - 1)
    for h in list(order):
        parents.append(h); bind.append([0.0, -4.0, 0.0]); ap.append(-1); ratio.append(1.0); move.append(0)
        order.append(len(parents) - 1)
    sc = ps._scene(parents, bind, base["bodies"], base["joints"], np.random.default_rng(43), 3 * len(parents), gravity=None if node else (60.0, -98.0, 40.0), h=0.0 if node else 1.0 / 30.0)
    sc.update(name="j node" if node else "j", ap=np.array(ap, dtype=np.int32), ratio=np.array(ratio, dtype=np.float32), move=np.array(move, dtype=np.uint8), chains=[],
              order=np.array(order, dtype=np.uint32))
    return sc


def physics_pose(sc, instance):
    return ps.pose(sc, 400 + instance)


def physics_reference(sc, pose, dtype=np.float64):
    """(F without the stage, F with it, the dynamic bones) of one instance after rz_physics_step(SUBSTEPS) from a reset state and a frame"""
    import physics_ref
    q, t = pose
    sim = physics_ref.Sim(sc["table"], sc["parents"], sc["bind"], dtype=dtype)
    S = fs.solved(sc, q, t, dtype=dtype)
    ovr = sim.step(S, SUBSTEPS)
    bones = sorted(ovr)
    F = np.asarray(physics_ref.apply_overrides(S, ovr), dtype=dtype)
    W = ar.solve(sc["parents"], sc["bind"], q, t, sc["ap"], sc["ratio"], sc["move"], F, bones, sc["order"], dtype=dtype)
    return F, W, bones


# ---- a small synthetic PMX of a scene: bones with flag 0x1000 and transform levels, optionally IK blocks and the physics sections ----

def transform_levels(sc):
    """a transform level per listed bone under which (level, index) sorts to the scene's `order`: the running count of index descents"""
    lv, cur, prev = {}, 0, -1
    for b in sc["order"]:
        b = int(b)
        if b < prev:
            cur += 1
        lv[b], prev = cur, b
    return lv


def write_pmx(sc, levels=None, chains=True):
    """A PMX 2.0 byte stream of the scene: its mesh, its bones with append rotate / move, flag 0x1000 and transform level `levels[b]` on
    the listed bones, an IK block per chain on the chain's goal bone, and — for a scene with a table — physics_scenes.write_pmx's
    rigid-body and joint sections. Returns (bytes, the table a loader must derive from it or None)."""
    import struct
    import physics_ref
    rng = np.random.default_rng(701)
    levels = transform_levels(sc) if levels is None else levels

    def text(x):
        b = x.encode("utf-16le")
        return struct.pack("<i", len(b)) + b
    m = sc["mesh"]
    B, V = sc["B"], len(m["pos"])
    out = bytearray(b"PMX ") + struct.pack("<f", 2.0) + bytes([8, 0, 0, 4, 1, 1, 2, 2, 1])
    out += text("after-physics scene") + text("") + text("") + text("")
    out += struct.pack("<i", V)
    for v in range(V):
        out += m["pos"][v].tobytes() + m["nrm"][v].tobytes() + struct.pack("<2f", 0.5, 0.5)
        out += bytes([1]) + struct.pack("<hhf", int(m["joints"][v, 0]), int(m["joints"][v, 1]), float(m["weights"][v, 0]) / 255.0) + struct.pack("<f", 1.0)
    tri = (np.arange(3 * (V // 3)) % V).astype(np.int32)
    out += struct.pack("<i", len(tri)) + tri.tobytes()
    out += struct.pack("<i", 0)
    out += struct.pack("<i", 1) + text("body") + text("") + struct.pack("<11f", *([0.5] * 11)) + bytes([0x10])
    out += struct.pack("<5f", 0, 0, 0, 1, 1.25) + struct.pack("<bb", -1, -1) + bytes([0, 1, 0]) + text("") + struct.pack("<i", len(tri))
    bp = ik_ref.bind_positions(sc["parents"], sc["bind"]).astype(np.float32)
    listed = set(int(b) for b in sc["order"])
    goals = {int(ch["goal"]): ch for ch in (sc["chains"] if chains else [])}
    out += struct.pack("<i", B)
    for b in range(B):
        a = int(sc["ap"][b])
        flags = (0x1000 if b in listed else 0) | (0x0100 if a >= 0 else 0) | (0x0200 if a >= 0 and sc["move"][b] else 0) | (0x0020 if b in goals else 0)
        out += text("bone%d" % b) + text("") + bp[b].tobytes() + struct.pack("<h", int(sc["parents"][b])) + struct.pack("<i", int(levels.get(b, 0)))
        out += struct.pack("<H", flags) + struct.pack("<3f", 0, 1, 0)
        if a >= 0:
            out += struct.pack("<hf", a, float(sc["ratio"][b]))
        if b in goals:
            ch = goals[b]
            out += struct.pack("<hif", int(ch["effector"]), int(ch["loops"]), float(ch["limit_angle"])) + struct.pack("<i", len(ch["links"]))
            for l in ch["links"]:
                out += struct.pack("<h", int(l["bone"])) + bytes([0])
    out += struct.pack("<i", 0) + struct.pack("<i", 0)                   # morphs, display frames
    t = sc.get("table")
    if t is None:
        out += struct.pack("<i", 0) + struct.pack("<i", 0)
        return bytes(out), None
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
