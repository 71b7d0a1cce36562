"""Hand-laid scenes for the follow stage (rz_override_follow; tests/follow_ref.py): skeletons small enough that every GPU case runs in a
few seconds, each laid out so that one edge of the stage is the only thing it can get wrong. STATIC lists the scenes fed through
rz_override_world — per scene the skeleton, a small mesh with vertices on every bone, and per instance a local pose and an override set —
physics() is scene (j), whose overrides the physics step writes. tests/test_follow_cpu.py checks the conditioning of every one of them.

  (a) 8 bones: override at bone 2, followers 3..5, a sibling branch (6, 7) that must not move
  (b) nested: overrides at depth 1 and 3 of a 6-chain; bone 2 follows the upper, 4..5 the lower
  (c) override on a root bone; a second root with a child that must not move
  (d) a follower whose append parent is overridden: the definition's result, not re-appended
  (e) a chain of 18 bones under one override, 20 levels in all: ancestors beyond the bone record's 16 levels (anc_more)
  (f) 257 followers under one override and 300 under another: the lane stride wraps at the block of 256
  (g) a 520-bone skeleton with followers at indices >= 512: rows beyond the two register slots per thread
  (h) a crowd of 3 with a different override set per instance and one instance with none
  (i) an IK chain above the overridden bone: the IK instantiation
  (j) 21-body strands (physics_scenes.strands) extended by a body-less tip bone per strand and one ornament branch
"""
import numpy as np

import ik_ref
import physics_scenes as ps


def _quats(rng, n, amount):
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-amount, amount, size=n)
    return np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1).astype(np.float32)


def _mesh(parents, bind, rng, per_bone=3):
    """`per_bone` vertices near every bone, BDEF1 / BDEF2 on it and its parent (physics_scenes._scene's recipe, every bone covered)"""
    parents = np.asarray(parents, dtype=np.int32)
    bind = np.asarray(bind, dtype=np.float32)
    B = len(parents)
    bp = ik_ref.bind_positions(parents, bind)
    vb = np.repeat(np.arange(B), per_bone)
    V = len(vb)
    pos = (bp[vb] + rng.uniform(-0.3, 0.3, size=(V, 3))).astype(np.float32)
    nrm = rng.normal(size=(V, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    jn = np.zeros((V, 4), dtype=np.uint16)
    wt = np.zeros((V, 4), dtype=np.uint8)
    jn[:, 0], jn[:, 1] = vb, np.maximum(parents[vb], 0)
    w0 = rng.integers(128, 256, size=V)
    w0[::3] = 255
    wt[:, 0], wt[:, 1] = w0, 255 - w0
    inv_bind = np.zeros((B, 16), dtype=np.float32)
    inv_bind[:, 0] = inv_bind[:, 5] = inv_bind[:, 10] = inv_bind[:, 15] = 1
    inv_bind[:, 12:15] = -bp.astype(np.float32)
    return dict(pos=pos, nrm=nrm, joints=jn, weights=wt, parents=parents, bind=bind, inv_bind=inv_bind)


def solved(sc, q, t, dtype=np.float64):
    """S of one local pose: [B,16]"""
    return ik_ref.solve(sc["parents"], sc["bind"], q, t, sc["chains"], sc["ap"], sc["ratio"], sc["move"], dtype=dtype)[0]


def _instance(sc, rng, bones, amount=0.5, swing=0.8, shift=0.6):
    """a local pose and an override set: every overridden bone's solved matrix turned by up to `swing` rad about a random axis through
    its own origin and moved by up to `shift` — what a physics body does to its bone — rounded to the float32 that is uploaded"""
    B = len(sc["parents"])
    q = _quats(rng, B, amount)
    t = rng.uniform(-0.2, 0.2, size=(B, 3)).astype(np.float32)
    S = solved(sc, q, t)
    mats = np.zeros((len(bones), 16), dtype=np.float32)
    for k, b in enumerate(bones):
        M = S[b].reshape(4, 4).T.copy()
        R = ik_ref._qmat(_quats(rng, 1, swing)[0].astype(np.float64), np.float64)
        M[:3, :3] = R @ M[:3, :3]
        M[:3, 3] += rng.uniform(-shift, shift, size=3)
        mats[k] = M.T.reshape(16)
    return dict(q=q, t=t, bones=np.array(bones, dtype=np.uint32), mats=mats)


def _scene(name, parents, bind, sets, seed, ap=None, ratio=None, move=None, chains=(), expect=None, per_bone=3):
    """sets: per instance the overridden bones; expect: per instance {follower bone: the bone it must follow} for the CPU test"""
    rng = np.random.default_rng(seed)
    sc = dict(name=name, parents=np.asarray(parents, dtype=np.int32), bind=np.asarray(bind, dtype=np.float32), B=len(parents),
              ap=None if ap is None else np.asarray(ap, dtype=np.int32), ratio=None if ratio is None else np.asarray(ratio, dtype=np.float32),
              move=None if move is None else np.asarray(move, dtype=np.uint8), chains=list(chains), expect=expect)
    sc["mesh"] = _mesh(parents, bind, rng, per_bone)
    sc["instances"] = [_instance(sc, rng, bones) for bones in sets]
    return sc


def _bind(rng, n):
    b = rng.uniform(-1.0, 1.0, size=(n, 3))
    b[0] = [0.0, 10.0, 0.0]
    return b


def scene_a():
    return _scene("a", [-1, 0, 1, 2, 3, 4, 1, 6], _bind(np.random.default_rng(1), 8), [[2]], 101, expect=[{3: 2, 4: 2, 5: 2}])


def scene_b():
    return _scene("b", [-1, 0, 1, 2, 3, 4], _bind(np.random.default_rng(2), 6), [[1, 3]], 102, expect=[{2: 1, 4: 3, 5: 3}])


def scene_c():
    return _scene("c", [-1, 0, 0, 1, -1, 4], _bind(np.random.default_rng(3), 6), [[0]], 103, expect=[{1: 0, 2: 0, 3: 0}])


def scene_d():
    # bone 3 takes half of bone 1's rotation and translation (append rotation + move); bone 1 is overridden, bone 3 follows it
    return _scene("d", [-1, 0, 1, 2, 0], _bind(np.random.default_rng(4), 5), [[1]], 104, ap=[-1, -1, -1, 1, -1], ratio=[1, 1, 1, 0.5, 1], move=[0, 0, 0, 1, 0],
                  expect=[{2: 1, 3: 1}])


def scene_e():
    return _scene("e", [-1] + list(range(19)), _bind(np.random.default_rng(5), 20) * 0.5, [[1]], 105, expect=[{b: 1 for b in range(2, 20)}])


def scene_f():
    # bones 1 and 2 under the root; 257 bones below bone 1 and 300 below bone 2, in chains of three
    parents = [-1, 0, 0]
    expect = {}
    for top, n in ((1, 257), (2, 300)):
        first = len(parents)
        for k in range(n):
            parents.append(top if k % 3 == 0 else first + k - 1)
            expect[first + k] = top
    return _scene("f", parents, _bind(np.random.default_rng(6), len(parents)), [[1, 2]], 106, expect=[expect], per_bone=1)


def scene_g():
    # 510 bones of a random tree at most 8 deep, bone 510 under bone 7 overridden, bones 511..519 below it; bone 3 overridden too
    rng = np.random.default_rng(7)
    parents, depth = [-1], [0]
    for i in range(1, 510):
        p = int(rng.integers(0, i))
        while depth[p] >= 7:
            p = parents[p]
        parents.append(p); depth.append(depth[p] + 1)
    parents += [7, 510, 511, 512, 510, 514, 515, 516, 517, 518]
    expect = {b: 510 for b in range(511, 520)}
    for b in range(510):            # whatever the random tree hung below bone 3
        p = parents[b]
        while p >= 0 and p != 3:
            p = parents[p]
        if p == 3:
            expect[b] = 3
    return _scene("g", parents, _bind(rng, 520), [[3, 510]], 107, expect=[expect], per_bone=1)


def scene_h():
    parents = [-1, 0, 1, 2, 3, 4, 1, 6, 7, 0, 9, 10]
    return _scene("h", parents, _bind(np.random.default_rng(8), 12), [[2], [6, 3, 10], []], 108,
                  expect=[{3: 2, 4: 2, 5: 2}, {4: 3, 5: 3, 7: 6, 8: 6, 11: 10}, {}])


def scene_i():
    # physics_scenes.ik_scene's arm: links 2 and 3, effector 4, goal 5; bone 6 hangs off the lower arm with 7, 8 below it
    parents = [-1, 0, 1, 2, 3, 0, 3, 6, 7]
    bind = [[0, 0, 0], [0, 16, 0], [1, 0, 0], [2, 0, 0], [2, 0, 0], [4.2, 15.2, 0.8], [1, -0.2, 0], [0, -1, 0], [0, -1, 0]]
    chains = [dict(goal=5, effector=4, loops=8, limit_angle=1.0, links=[dict(bone=3, min=None, max=None), dict(bone=2, min=None, max=None)])]
    rng = np.random.default_rng(109)
    sc = dict(name="i", parents=np.asarray(parents, dtype=np.int32), bind=np.asarray(bind, dtype=np.float32), B=9, ap=None, ratio=None, move=None, chains=chains,
              expect=[{7: 6, 8: 6}])
    sc["mesh"] = _mesh(parents, bind, rng)
    # a gentle pose (physics_scenes.pose's amounts) with the goal moved: the chain has to work, and stays well conditioned
    q = _quats(rng, 9, 0.1)
    t = np.zeros((9, 3), dtype=np.float32)
    t[0] = rng.uniform(-0.15, 0.15, size=3)
    t[5] = rng.uniform(-0.4, 0.4, size=3)
    S = solved(sc, q, t)
    M = S[6].reshape(4, 4).T.copy()
    M[:3, :3] = ik_ref._qmat(_quats(rng, 1, 0.8)[0].astype(np.float64), np.float64) @ M[:3, :3]
    M[:3, 3] += rng.uniform(-0.6, 0.6, size=3)
    sc["instances"] = [dict(q=q, t=t, bones=np.array([6], dtype=np.uint32), mats=M.T.reshape(1, 16).astype(np.float32))]
    return sc


STATIC = dict(a=scene_a, b=scene_b, c=scene_c, d=scene_d, e=scene_e, f=scene_f, g=scene_g, h=scene_h, i=scene_i)
_memo = {}


def scene(name):
    if name not in _memo:
        _memo[name] = physics() if name == "j" else STATIC[name]()
    return _memo[name]


# ---- (j): the physics step writes the overrides ----

SUBSTEPS = (10, 10)         # 20 substeps in two calls, the pose changing between them


def physics():
    """3 strands of 6 dynamic bodies under 3 following ones (21 bodies), every joint limited and sprung; per strand a tip bone WITHOUT a
    body below its last dynamic bone, and an ornament of two bones hanging off the third dynamic bone of the first strand. tips / ornament:
    {follower bone: the dynamic bone it must ride on}."""
    base = ps.strands(3, 6, base=True, seed=41, n_verts=64, sprung=True)
    assert base["table"]["n_bodies"] == 21
    parents, bind = [int(p) for p in base["parents"]], [list(map(float, b)) for b in base["bind"]]
    dyn = [int(b["bone"]) for b in base["bodies"] if b["type"] == 1]
    ride = {}
    for s in range(3):
        last = dyn[6 * s + 5]
        parents.append(last); bind.append([0.0, -1.0, 0.0])
        ride[len(parents) - 1] = last
    mid = dyn[2]
    parents.append(mid); bind.append([0.4, -0.2, 0.1])
    ride[len(parents) - 1] = mid
    parents.append(len(parents) - 1); bind.append([0.0, -0.5, 0.0])
    ride[len(parents) - 1] = mid
    sc = ps._scene(parents, bind, base["bodies"], base["joints"], np.random.default_rng(42), 3 * len(parents))
    sc.update(name="j", ride=ride, ap=None, ratio=None, move=None, chains=[])
    return sc


def physics_poses(sc, instance):
    return [ps.pose(sc, 300 + 10 * k + instance) for k in range(len(SUBSTEPS))]


def physics_reference(sc, poses, dtype=np.float64):
    """per call (S [B,16], bones [nd], O [nd,16]) of one instance through SUBSTEPS: the un-followed solve and the overrides the step emits"""
    import physics_ref
    sim = physics_ref.Sim(sc["table"], sc["parents"], sc["bind"], dtype=dtype)
    out = []
    for (q, t), n in zip(poses, SUBSTEPS):
        S = ps.world_of(sc, q, t, dtype=dtype)
        ovr = sim.step(S, n)
        bones = sorted(ovr)
        out.append((S, bones, np.stack([ovr[b] for b in bones])))
    return out
