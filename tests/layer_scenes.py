"""The scenes of the layered-pose tests, shared by tests/test_gpu_layers.py (which runs them on the device) and tests/test_layer_cpu.py
(which holds their inputs to the rule the GPU bars rest on). Built on tests/motion_scenes.py. Test infrastructure.

The rule: override clips keep motion_scenes' rule — every key of a bone, across all override clips of a scene, lies within 45 degrees of a
per-bone base rotation (identity for a bone some clip leaves at rest) — additive clips have keys within 15 degrees of identity, and no held
state has more than two additive layers below an override layer. A pose in front of an override layer is then at most 45 + 2 x 15 = 75
degrees from the bone's base and the layer's sample at most 45, so any slerp the definition performs spans at most 120 degrees:
|dot| >= cos(60 deg) = 0.5 as quaternions. tests/test_layer_cpu.py computes the smallest |dot| over every slerp of every held state."""
import numpy as np

import motion_scenes as ms
from layer_ref import ADDITIVE as ADD, NO_CLIP, NO_MASK, OVERRIDE as OVR

B, M, M_SPARSE = ms.B, ms.M, ms.M_SPARSE
NAN = float("nan")
_memo = {}


def bone_masks(n_bones=B):
    """four masks that flip at bone indices 31|32, 63|64, 255|256 and 298|299: [0, 32) + [64, 256) + {299}; its complement; nothing; a
    random half"""
    a = np.zeros(n_bones, dtype=np.uint8)
    a[0:32] = 1; a[64:256] = 1; a[299:] = 1
    r = (np.random.default_rng(7).random(n_bones) < 0.5).astype(np.uint8)
    return np.stack([a, 1 - a, np.zeros(n_bones, dtype=np.uint8), r])


def morph_masks(n_morphs):
    """the morph side of the four masks: the first half (of 8) or [0, 256) (of 260, a flip at 255|256); the complement; nothing; all"""
    a = np.zeros(n_morphs, dtype=np.uint8)
    a[:256 if n_morphs > 256 else n_morphs // 2] = 1
    return np.stack([a, 1 - a, np.zeros(n_morphs, dtype=np.uint8), np.ones(n_morphs, dtype=np.uint8)])


def _layer_clips(n_bones, n_morphs, seed, kind, group_feed):
    """two more clips for a library built by motion_scenes._clips(n_bones, n_morphs, seed): clip 3, an override clip on the same per-bone
    bases that keys a random half of the bones ('upper body'), and clip 4, an additive clip within 15 degrees of identity that keys 60 %"""
    from reze_engine_amd import synth
    rng = np.random.default_rng(seed + 10)
    base = synth.make_motion_base(n_bones, seed=seed + 1)
    base[kind != 0] = (0.0, 0.0, 0.0, 1.0)
    gf = group_feed if n_morphs else None
    upper = synth.make_motion(n_bones, n_morphs, seed=seed + 11, keyed=rng.random(n_bones) < 0.5, base=base, flip=0.3, n_keys=5, group_feed=gf, morph_keyed=0.5)
    add = synth.make_motion(n_bones, n_morphs, seed=seed + 12, keyed=rng.random(n_bones) < 0.6, max_angle=np.pi / 12, flip=0.3, n_keys=6, trans=0.05,
                            group_feed=gf, morph_keyed=0.6)
    return [upper, add]


def main_scene():
    """motion_scenes.main_scene() (V = 2048, B = 300, M = 8 dense) with five clips — its three, the upper-body clip 3, the additive clip 4
    — four masks, and six states carrying 0, 1, 2, 4, 4 and 3 layers: override and additive, weights 0, 0.35 and 1, NO_MASK and masks, a
    layer clip that keys only some bones (all of them do), a skipped layer between live ones (with a NaN frame), cross-fading bases."""
    if "main" not in _memo:
        s = ms.main_scene()
        clips = list(s["clips"]) + _layer_clips(B, M, 50, s["kind"], (2, 0.5))
        states = [((0, 4.37, 1, 1000.0, 0.25), []),
                  ((1, 7.5, None, 0.0, 0.0), [(3, 5.5, 0.35, None, OVR)]),
                  ((0, -3.0, None, 0.0, 0.0), [(2, 6.25, 1.0, 0, OVR), (4, 3.75, 0.35, None, ADD)]),
                  ((1, 7.5, 1, 2.25, 0.5), [(4, 9.5, 1.0, 1, ADD), (NO_CLIP, NAN, 0.5, 0, OVR), (3, 12.0, 0.35, 0, OVR), (4, 2.0, 0.35, None, ADD)]),
                  ((0, 9.5, 2, -1.0, 0.25), [(4, 1.5, 0.35, 3, ADD), (4, 6.0, 1.0, 0, ADD), (1, 3.0, 0.35, 1, OVR), (3, NAN, 0.0, None, OVR)]),
                  ((2, 3.3, None, 0.0, 0.0), [(0, 4.0, 1.0, None, OVR), (2, 5.0, 0.35, 2, OVR), (4, 7.0, 1.0, None, ADD)])]
        _memo["main"] = dict(mesh=s["mesh"], dense=s["dense"], clips=clips, kind=s["kind"], states=states, bone_masks=bone_masks(), morph_masks=morph_masks(M))
    return _memo["main"]


def sparse_scene():
    """motion_scenes.sparse_scene() (M = 260 sparse morphs: a second chunk of morphs) with the two extra clips and morph masks that flip
    at 255|256"""
    if "sparse" not in _memo:
        s = ms.sparse_scene()
        kind = ms._clips(B, M_SPARSE, 90, group_feed=(258, 0.5))[1]
        clips = list(s["clips"]) + _layer_clips(B, M_SPARSE, 90, kind, (258, 0.5))        # clips 2 (upper body) and 3 (additive)
        states = [((0, 5.5, 1, 12.25, 0.4), [(2, 7.5, 0.35, 0, OVR), (3, 4.25, 1.0, 1, ADD)]),
                  ((1, 3.0, None, 0.0, 0.0), [(3, 8.0, 0.35, 0, ADD), (2, 2.5, 1.0, 1, OVR)])]
        _memo["sparse"] = dict(mesh=s["mesh"], sparse=s["sparse"], clips=clips, states=states, bone_masks=bone_masks(), morph_masks=morph_masks(M_SPARSE))
    return _memo["sparse"]


def ring_scene():
    """motion_scenes.ring_scene() (B = 300, no morphs; with I = 32 the local pose is 268 800 bytes) with the two extra clips and the masks"""
    if "ring" not in _memo:
        s = ms.ring_scene()
        kind = ms._clips(B, 0, 70)[1]
        _memo["ring"] = dict(mesh=s["mesh"], clips=list(s["clips"]) + _layer_clips(B, 0, 70, kind, None), bone_masks=bone_masks())
    return _memo["ring"]


def random_layers(rng, n, n_clips=5, n_masks=4):
    """n layers for the bit-for-bit tests (no float64 bar rests on them): any clip, weight, mask and mode, some of them skipped"""
    out = []
    for _ in range(n):
        clip = NO_CLIP if rng.random() < 0.15 else int(rng.integers(0, n_clips))
        out.append((clip, float(rng.uniform(-2, 40)), float(rng.choice([0.0, 0.35, 0.6, 1.0])), None if rng.random() < 0.4 else int(rng.integers(0, n_masks)),
                    int(rng.integers(0, 2))))
    return out


def leg_additive(rng, nk=6):
    """motion_scenes.leg_motion() made additive: the centre's rotations within 15 degrees of identity, a fifth of the translations"""
    c = ms.leg_motion(rng, nk=nk)
    ax = rng.normal(size=(nk, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-np.pi / 12, np.pi / 12, size=nk)
    c["key_rot"] = c["key_rot"].copy()
    c["key_rot"][:nk] = np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1).astype(np.float32)
    c["key_pos"] = (c["key_pos"] * np.float32(0.2)).astype(np.float32)
    return c


def leg_scene():
    """motion_scenes.leg_scene() (14 bones, four IK chains) with an additive third clip and two masks: centre + left goals, right goals"""
    if "leg" not in _memo:
        s = ms.leg_scene()
        masks = np.zeros((2, 14), dtype=np.uint8)
        masks[0, [1, 10, 11]] = 1
        masks[1, [12, 13]] = 1
        states = [((0, 11.3, 1, 7.7, 0.5), [(1, 4.5, 0.35, 1, OVR), (2, 6.5, 1.0, None, ADD)]),
                  ((1, 3.25, None, 0.0, 0.0), [(2, 9.0, 0.35, 0, ADD), (0, 15.5, 1.0, 1, OVR)]),
                  ((0, 15.5, 1, 9.0, 0.75), [(0, 2.5, 0.35, None, OVR)])]
        _memo["leg"] = dict(mesh=s["mesh"], clips=list(s["clips"]) + [leg_additive(np.random.default_rng(5))], states=states, bone_masks=masks)
    return _memo["leg"]


def additive_clips(scene_name):
    """the indices of a scene's additive clips (everything else is an override clip)"""
    return {"main": [4], "sparse": [3], "leg": [2]}[scene_name]


def all_held_states():
    """every (scene name, clips, base, layers, bones, morphs, bone masks, morph masks) the GPU tests hold to the float64 reference"""
    out = []
    for name, s, nb, nm in (("main", main_scene(), B, M), ("sparse", sparse_scene(), B, M_SPARSE), ("leg", leg_scene(), 14, 0)):
        for base, layers in s["states"]:
            out.append((name, s["clips"], base, layers, nb, nm, s["bone_masks"], s.get("morph_masks")))
    return out


def concat_clips(body, face):
    """one clip holding the bone tracks of both (they drive disjoint bones) and, per vertex morph, the feeds of whichever of the two
    holds a key for it (disjoint vertex morphs): the morph tracks of `face` are renumbered behind those of `body`"""
    nb = len(body["track_bone"])
    out = dict(track_bone=np.concatenate([body["track_bone"], face["track_bone"]]).astype(np.int32),
               key_off=np.concatenate([body["key_off"], face["key_off"][1:] + body["key_off"][nb]]).astype(np.uint32))
    for k in ("key_frame", "key_rot", "key_pos", "key_interp"):
        out[k] = np.concatenate([body[k], face[k]])
    mt = len(body["mkey_off"]) - 1
    out["mkey_off"] = np.concatenate([body["mkey_off"], face["mkey_off"][1:] + body["mkey_off"][mt]]).astype(np.uint32)
    out["mkey_frame"] = np.concatenate([body["mkey_frame"], face["mkey_frame"]])
    out["mkey_weight"] = np.concatenate([body["mkey_weight"], face["mkey_weight"]])
    n_morphs = len(body["feed_off"]) - 1
    from layer_ref import keyed_morphs
    in_face = keyed_morphs(face, n_morphs)
    off, tr, ra = [0], [], []
    for m in range(n_morphs):
        src, shift = (face, mt) if in_face[m] else (body, 0)
        for f in range(int(src["feed_off"][m]), int(src["feed_off"][m + 1])):
            tr.append(int(src["feed_track"][f]) + shift); ra.append(float(src["feed_ratio"][f]))
        off.append(len(tr))
    out.update(feed_off=np.array(off, dtype=np.uint32), feed_track=np.array(tr, dtype=np.int32), feed_ratio=np.array(ra, dtype=np.float32))
    return out


def body_and_face(n_bones=B, n_morphs=M, seed=120):
    """a body clip and a face clip that drive disjoint bones and disjoint vertex morphs (body: even bones, morphs 0 .. M/2; face: every
    third odd bone, the other morphs), and their concatenation"""
    from reze_engine_amd import synth
    idx = np.arange(n_bones)
    body = synth.make_motion(n_bones, n_morphs, seed=seed, keyed=idx % 2 == 0, flip=0.3)
    face = synth.make_motion(n_bones, n_morphs, seed=seed + 1, keyed=idx % 6 == 1, flip=0.3, n_keys=5)

    def keep_morphs(clip, keep):
        """empty the own tracks of the morphs outside `keep` (a track without keys contributes nothing)"""
        c = dict(clip)
        moff = c["mkey_off"].astype(np.int64)
        sel = np.concatenate([np.arange(moff[t], moff[t + 1]) for t in range(n_morphs) if keep[t]] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        cnt = np.array([(moff[t + 1] - moff[t]) if keep[t] else 0 for t in range(n_morphs)])
        c["mkey_off"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        c["mkey_frame"], c["mkey_weight"] = c["mkey_frame"][sel], c["mkey_weight"][sel]
        return c
    half = np.arange(n_morphs) < n_morphs // 2
    body, face = keep_morphs(body, half), keep_morphs(face, ~half)
    return body, face, concat_clips(body, face)


# ---- the Node scene: motion_scenes' synthetic PMX and two body VMDs, and a morph-only face file ----
NODE_MASKS = {"upper": dict(bones=["bone3"], withDescendants=True, morphs="none"), "face": dict(bones=[], morphs=["v0", "blink", "v4"])}
NODE_STATES = [dict(a="walk", frameA=7.5, layers=[dict(motion="face", frame=7.5)]),
               dict(a="walk", frameA=7.5, b="run", frameB=3.25, blend=0.25, layers=[dict(motion="run", frame=12.5, weight=0.35, mask="upper")]),
               dict(a="run", frameA=12.5, b="walk", frameB=40, blend=0.5,
                    layers=[dict(motion="walk", frame=21.75, weight=1, mask="upper"), dict(motion="face", frame=10, weight=0.5, mask="face", additive=True)]),
               dict(a="walk", frameA=21.75, layers=[dict(motion="run", frame=9.5, weight=0.35), dict(motion="face", frame=0, weight=0),
                                                     dict(motion="face", frame=15, weight=0.35, mask="face"), dict(motion="face", frame=22, weight=1, additive=True)]),
               dict(a="run", frameA=5.5, b="run", frameB=17.25, blend=0.75),
               dict(a="run", frameA=-1, layers=[dict(motion="walk", frame=11, weight=1)])]


def write_node_scene(pmx_synth, out_dir):
    """motion_scenes.write_node_scene()'s m.pmx, walk.vmd and run.vmd, and face.vmd: no bone keys, morph keys for v0, v4, v5, blink and the
    group morph 'grp' (which feeds v0, blink and the bone morph 'twist')"""
    import os
    paths = ms.write_node_scene(pmx_synth, out_dir)
    paths["vmd_c"] = os.path.join(out_dir, "face.vmd")
    with open(paths["vmd_c"], "wb") as f:
        f.write(pmx_synth.write_vmd([], [("v0", 0, 0.2), ("v0", 18, 0.9), ("v4", 4, 0.7), ("v4", 25, 0.1), ("v5", 9, 0.5), ("blink", 0, 1.0), ("blink", 14, 0.0),
                                         ("blink", 28, 0.6), ("grp", 2, 0.1), ("grp", 20, 0.8)]))
    return paths
