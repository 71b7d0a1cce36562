"""The scenes of the motion-library tests, shared by tests/test_gpu_motion.py (which runs them on the device) and
tests/test_motion_cpu.py (which holds their inputs to the rule the GPU bars rest on). Test infrastructure.

The rule: every key of a bone, across all clips of a scene, lies within a 45 degree rotation of a per-bone base rotation, so any two
samples of that bone — a sample is a slerp between two keys, which stays inside that ball — have |dot| >= cos(45 deg) > 0.7 as
quaternions. A bone that some clip leaves at rest is sampled as identity there, so its base is identity."""
import numpy as np

V, B, M = 2048, 300, 8          # more than 256 bones: a second chunk of bones per instance
M_SPARSE = 260                  # more than 256 vertex morphs: a second chunk of morphs
SPARSE_STATE = (0, 5.5, 1, 12.25, 0.4)      # the state of sparse_scene() that the GPU test holds to float64
NO_CLIP = 0xffffffff
_memo = {}


def deep_skeleton(n_bones, rng, chain=20):
    """parents with a chain of `chain` bones at the front (a hierarchy deeper than 16: a third doubling round) and random parents behind"""
    parents = np.full(n_bones, -1, dtype=np.int32)
    for i in range(1, n_bones):
        parents[i] = i - 1 if i < chain else int(rng.integers(0, i))
    return parents


def depth_of(parents):
    d = np.zeros(len(parents), dtype=np.int64)
    for i in range(len(parents)):
        d[i] = 0 if parents[i] < 0 else d[parents[i]] + 1
    return int(d.max()) + 1


def _mesh(n_verts, n_bones, seed):
    from reze_engine_amd import synth
    mesh = synth.make_mesh(n_verts, n_bones, seed=seed)
    mesh["parents"] = deep_skeleton(n_bones, np.random.default_rng(seed + 1))
    mesh["bind"] = (mesh["bind"] * np.float32(0.5)).astype(np.float32)
    mesh["inv_bind"] = synth.inverse_bind_translation_only(mesh["parents"], mesh["bind"])
    return mesh


def _clips(n_bones, n_morphs, seed, group_feed=(2, 0.5)):
    """three clips: bones keyed by all of them (random base), by clip 0 only, by clip 1 only, by none (identity base)"""
    from reze_engine_amd import synth
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, size=n_bones)                  # 0 all clips, 1 clip 0 only, 2 clip 1 only, 3 none
    base = synth.make_motion_base(n_bones, seed=seed + 1)
    base[kind != 0] = (0.0, 0.0, 0.0, 1.0)
    gf = group_feed if n_morphs else None
    clips = [synth.make_motion(n_bones, n_morphs, seed=seed + 2, keyed=(kind == 0) | (kind == 1), base=base, group_feed=gf),
             synth.make_motion(n_bones, n_morphs, seed=seed + 3, keyed=(kind == 0) | (kind == 2), base=base, flip=0.5, n_keys=7, group_feed=gf),
             synth.make_motion(n_bones, n_morphs, seed=seed + 4, keyed=(kind == 0), base=base, flip=0.2, n_keys=5, interp=False)]
    return clips, kind


def main_scene():
    """V = 2048, B = 300 (hierarchy 20 deep), M = 8 dense morphs (morph 2 also fed by a group track), three clips, five states: before the
    first key, past the last key, fractional frames; blend 0 / 0.25 / 0.5 / 1 and no second clip; one state blends two times of one clip."""
    if "main" not in _memo:
        from reze_engine_amd import synth
        mesh = _mesh(V, B, 41)
        dense, _ = synth.make_morphs_dense(V, M, seed=43)
        clips, kind = _clips(B, M, 50)
        states = [(0, -3.0, None, 0.0, 0.0),
                  (0, 4.37, 1, 1000.0, 0.25),
                  (1, 7.5, 1, 2.25, 0.5),
                  (2, 11.1, 0, 6.6, 1.0),
                  (2, 3.3, 1, 9.9, 0.0)]
        extra = [(1, 5.125, 2, 8.75, 0.5), (0, 9.5, 2, -1.0, 0.25)]       # blended pairs the five do not cover: the CPU tests only, no GPU test runs them
        _memo["main"] = dict(mesh=mesh, dense=dense, clips=clips, kind=kind, states=states, extra=extra)
    return _memo["main"]


def clips_for_morphs(scene, n_morphs):
    """the main scene's clips rebuilt for a morph set of another size"""
    return _clips(B, n_morphs, 50)[0]


def ring_scene():
    """V = 1024, B = 300, no morphs: with I = 32 the local pose is 268 800 bytes"""
    if "ring" not in _memo:
        mesh = _mesh(1024, B, 61)
        clips, _ = _clips(B, 0, 70)
        _memo["ring"] = dict(mesh=mesh, clips=clips)
    return _memo["ring"]


def sparse_scene():
    """V = 1024, B = 300, M = 260 sparse morphs, two clips"""
    if "sparse" not in _memo:
        from reze_engine_amd import synth
        mesh = _mesh(1024, B, 81)
        sparse = synth.make_morphs_sparse(1024, M_SPARSE, density=0.02, seed=83)
        clips, _ = _clips(B, M_SPARSE, 90, group_feed=(258, 0.5))
        _memo["sparse"] = dict(mesh=mesh, sparse=sparse, clips=clips[:2])
    return _memo["sparse"]


def leg_motion(rng, nk=8):
    """keys for the centre and the four IK goals of synth.make_leg_rig only, as a dance has them: the centre squats, the goals move"""
    bones = np.array([1, 10, 11, 12, 13], dtype=np.int32)
    n = len(bones)
    kq = np.zeros((n, nk, 4), dtype=np.float32)
    kq[..., 3] = 1
    ax = rng.normal(size=(nk, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-0.4, 0.4, size=nk)
    kq[0] = np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1)
    kp = np.zeros((n, nk, 3), dtype=np.float32)
    kp[0] = rng.uniform(-1.0, 1.0, size=(nk, 3))
    kp[0, :, 1] = rng.uniform(-3.0, -0.5, size=nk)
    for r in (1, 3):
        kp[r] = rng.uniform(-1.5, 1.5, size=(nk, 3))
        kp[r, :, 1] = rng.uniform(0.0, 2.5, size=nk)
        kp[r + 1] = rng.uniform(-0.3, 0.3, size=(nk, 3))
    return dict(track_bone=bones, key_off=(np.arange(n + 1) * nk).astype(np.uint32),
                key_frame=np.tile(np.cumsum(rng.integers(2, 9, size=nk)).astype(np.float32), n),
                key_rot=kq.reshape(-1, 4), key_pos=kp.reshape(-1, 3), key_interp=rng.integers(1, 127, size=(n * nk, 16)).astype(np.uint8))


def leg_scene():
    """synth.make_leg_rig (14 bones, four IK chains) with two motions of the centre and the goals"""
    if "leg" not in _memo:
        from reze_engine_amd import synth
        mesh = synth.make_leg_rig(n_verts=2000)
        clips = [leg_motion(np.random.default_rng(3)), leg_motion(np.random.default_rng(4), nk=6)]
        states = [(0, 11.3, 1, 7.7, 0.5), (1, 3.25, 0, 20.5, 0.25), (0, 15.5, 1, 9.0, 0.75), (1, 12.5, None, 0.0, 0.0)]
        _memo["leg"] = dict(mesh=mesh, clips=clips, states=states)
    return _memo["leg"]


def all_blended_states():
    """every (clips, state, bones) the GPU tests blend two clips in and hold to a float64 reference (the Node scene's states are held to the
    same rule by the host test of tests/test_motion_cpu.py, which has their flattened motions), and the main scene's two CPU-only states"""
    m, leg, sp = main_scene(), leg_scene(), sparse_scene()
    return ([(m["clips"], st, B) for st in m["states"] + m["extra"]] + [(leg["clips"], st, 14) for st in leg["states"]]
            + [(sp["clips"], SPARSE_STATE, B)])


# ---- the Node scene: a synthetic PMX and two VMDs over its bones and morphs ----
NODE_STATES = [dict(a="walk", frameA=0), dict(a="walk", frameA=7.5, b="run", frameB=3.25, blend=0.25), dict(a="run", frameA=12.5, b="walk", frameB=40, blend=0.5),
               dict(a="walk", frameA=21.75, b="run", frameB=9.5, blend=1), dict(a="run", frameA=5.5, b="run", frameB=17.25, blend=0.75),
               dict(a="run", frameA=-1, b="walk", frameB=11, blend=0)]


def node_vmd_keys(seed, bones, flip, n_keys=5):
    """(bone keys, morph keys) of one synthetic VMD: rotations within 45 degrees of identity, uneven integer frames with one duplicate,
    random interpolation bytes 1 .. 126, `flip` of the keys stored with the opposite sign"""
    rng = np.random.default_rng(seed)
    bone_keys = []
    for b in bones:
        f = np.cumsum(rng.integers(1, 9, size=n_keys))
        f[3:] -= f[3] - f[2]
        for k in range(n_keys):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            a = rng.uniform(-np.pi / 4, np.pi / 4)
            q = np.concatenate([ax * np.sin(a / 2), [np.cos(a / 2)]]) * (-1.0 if rng.random() < flip else 1.0)
            interp = bytes(rng.integers(1, 127, size=16).astype(np.uint8)) + bytes(48)
            bone_keys.append(("bone%d" % b, int(f[k]), tuple(float(x) for x in q.astype(np.float32)), tuple(float(x) for x in rng.uniform(-0.3, 0.3, size=3).astype(np.float32)), interp))
    return bone_keys


def write_node_scene(pmx_synth, out_dir):
    """m.pmx, walk.vmd, run.vmd under out_dir; returns their paths. 'walk' keys bones 0 1 3 5 20, 'run' keys 1 3 8 20 25; both key morphs,
    'run' through the group morph 'grp' too."""
    import os
    paths = dict(pmx=os.path.join(out_dir, "m.pmx"), vmd_a=os.path.join(out_dir, "walk.vmd"), vmd_b=os.path.join(out_dir, "run.vmd"))
    with open(paths["pmx"], "wb") as f:
        f.write(pmx_synth.write_pmx(V=3000, B=40, seed=5))
    with open(paths["vmd_a"], "wb") as f:
        f.write(pmx_synth.write_vmd(node_vmd_keys(1, (0, 1, 3, 5, 20), 0.0), [("v1", 0, 0.8), ("v1", 20, 0.1), ("v2", 6, 0.4), ("blink", 10, 0.5), ("blink", 30, 0.0)]))
    with open(paths["vmd_b"], "wb") as f:
        f.write(pmx_synth.write_vmd(node_vmd_keys(2, (1, 3, 8, 20, 25), 0.5), [("v1", 5, 0.3), ("grp", 0, 0.0), ("grp", 30, 1.0), ("v3", 0, 0.6), ("v3", 12, 0.2)]))
    return paths
