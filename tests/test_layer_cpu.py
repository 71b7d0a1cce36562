"""CPU checks of layered poses: the float64 definition tests/layer_ref.py, the inputs the GPU tests rest on (tests/layer_scenes.py), the
bindings, and the host twin Model.applyLayeredFrame / Engine.setMotionMask against a recording addon."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import layer_ref
import layer_scenes as ls
import motion_ref
import motion_scenes as ms
from helpers import sample_reference
from layer_ref import ADDITIVE as ADD, NO_CLIP, OVERRIDE as OVR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
JS = os.path.join(ROOT, "tests", "js")


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def test_the_inputs_of_the_gpu_tests_keep_every_slerp_within_120_degrees():
    """Every state the GPU tests hold to float64 (main, sparse-morph and leg scenes; no state is left out): the smallest |dot| over every
    slerp the definition performs — the base's cross-fade and every override layer — is >= 0.5, every additive sample has |qL.w| >= 0.9,
    and no state has more than two additive layers below an override layer."""
    worst, worst_add, n_slerp, n_add = 1.0, 1.0, 0, 0
    held = ls.all_held_states()
    assert len(held) == 6 + 2 + 3
    for name, clips, base, layers, nb, nm, bm, mm in held:
        worst = min(worst, motion_ref.min_abs_dot(clips, base, nb))
        dots = []
        layer_ref.layered_reference(clips, base, layers, nb, nm, bm, mm, dots=dots)
        for kind, d in dots:
            if kind == "add":
                worst_add, n_add = min(worst_add, d), n_add + 1
            else:
                worst, n_slerp = min(worst, d), n_slerp + 1
        adds = 0
        for ly in layers:
            if layer_ref.skipped(ly):
                continue
            assert (int(ly[0]) in ls.additive_clips(name)) == (ly[4] == ADD), (name, ly)       # additive clips are used additively, only they
            if ly[4] == ADD:
                adds += 1
            else:
                assert adds <= 2, (name, base, layers)
    print("smallest |dot| over %d override slerps: %.3f; smallest |qL.w| over %d additive samples: %.4f" % (n_slerp, worst, n_add, worst_add))
    assert n_slerp > 300 and n_add > 300
    assert worst >= 0.5 and worst_add >= 0.9


def test_the_clips_follow_their_rules():
    from reze_engine_amd import synth
    s = ls.main_scene()
    base = synth.make_motion_base(ls.B, seed=51)
    base[s["kind"] != 0] = (0.0, 0.0, 0.0, 1.0)
    for k, clip in enumerate(s["clips"]):
        rot = clip["key_rot"].astype(np.float64).reshape(len(clip["track_bone"]), -1, 4)
        if k == 4:          # additive: within 15 degrees of identity
            assert np.abs(rot[..., 3]).min() >= np.cos(np.pi / 24) - 1e-6
        else:               # override: within 45 degrees of the bone's base
            d = np.abs(np.sum(rot * base[clip["track_bone"]][:, None, :], axis=2))
            assert d.min() >= np.cos(np.pi / 8) - 1e-6, k
    # the states: 0, 1, 2, 4, 4 and 3 layers; weights 0, 0.35 and 1; both modes; masks and none; a skipped layer between live ones
    assert [len(l) for _b, l in s["states"]] == [0, 1, 2, 4, 4, 3]
    flat = [ly for _b, l in s["states"] for ly in l]
    assert {ly[2] for ly in flat} == {0.0, 0.35, 0.5, 1.0} and {ly[4] for ly in flat} == {OVR, ADD}
    assert any(ly[3] is None for ly in flat) and {ly[3] for ly in flat if ly[3] is not None} == {0, 1, 2, 3}
    mid = s["states"][3][1]
    assert layer_ref.skipped(mid[1]) and not layer_ref.skipped(mid[0]) and not layer_ref.skipped(mid[2]) and np.isnan(mid[1][1])
    assert any(b[2] is not None and 0 < b[4] < 1 and l for b, l in s["states"])           # a base that itself cross-fades, with layers
    keyed = [layer_ref.keyed_bones(c, ls.B) for c in s["clips"]]
    assert all(0.2 < k.mean() < 0.9 for k in keyed)                                       # every clip keys only some of the bones
    bm = s["bone_masks"]
    for lo in (31, 63, 255, 298):
        assert bm[0][lo] != bm[0][lo + 1] and bm[1][lo] != bm[1][lo + 1]
    assert not bm[2].any() and 0.3 < bm[3].mean() < 0.7
    sp = ls.sparse_scene()
    assert sp["morph_masks"][0][255] != sp["morph_masks"][0][256]
    for k in (2, 3):
        km = layer_ref.keyed_morphs(sp["clips"][k], ls.M_SPARSE)
        assert km[:256].any() and km[256:].any() and not km.all()


def test_no_layers_is_the_blend():
    s = ls.main_scene()
    for base, _ in s["states"]:
        want = motion_ref.blend_reference(s["clips"], base, ls.B, ls.M)
        assert same(layer_ref.layered_reference(s["clips"], base, [], ls.B, ls.M), want)
        # weight 0 and no clip are skipped as a whole (a NaN frame there is legal); a mask of zeros acts on nothing
        for layers in ([(3, 5.0, 0.0, None, OVR)], [(NO_CLIP, float("nan"), 1.0, 0, ADD)], [(None, 1.0, 1.0, None, OVR), (4, float("nan"), 0.0, 1, ADD)],
                       [(3, 5.0, 0.35, 2, OVR), (4, 6.0, 1.0, 2, ADD)]):
            assert same(layer_ref.layered_reference(s["clips"], base, layers, ls.B, ls.M, s["bone_masks"], s["morph_masks"]), want), layers


def test_override_at_weight_one_of_a_clip_that_keys_everything_is_that_clips_sample():
    from reze_engine_amd import synth
    s = ls.main_scene()
    full = synth.make_motion(ls.B, ls.M, seed=77, keyed=np.ones(ls.B, dtype=bool), morph_keyed=1.0)
    assert layer_ref.keyed_bones(full, ls.B).all() and layer_ref.keyed_morphs(full, ls.M).all()
    clips = list(s["clips"]) + [full]
    want = sample_reference(full, 6.5, ls.B, ls.M)
    for base, _ in s["states"][:3]:
        assert same(layer_ref.layered_reference(clips, base, [(5, 6.5, 1.0, None, OVR)], ls.B, ls.M), want)
    # ... and under a mask, that clip's sample inside the mask and the base outside it
    base = s["states"][1][0]
    q0, t0, w0 = motion_ref.blend_reference(clips, base, ls.B, ls.M)
    q, t, w = layer_ref.layered_reference(clips, base, [(5, 6.5, 1.0, 0, OVR)], ls.B, ls.M, s["bone_masks"], s["morph_masks"])
    inb, inm = s["bone_masks"][0] != 0, s["morph_masks"][0] != 0
    assert np.array_equal(q[inb], want[0][inb]) and np.array_equal(q[~inb], q0[~inb]) and np.array_equal(t[inb], want[1][inb]) and np.array_equal(t[~inb], t0[~inb])
    assert np.array_equal(w[inm], want[2][inm]) and np.array_equal(w[~inm], w0[~inm]) and not np.array_equal(w, w0)
    # without morph masks every mask includes every morph
    w_all = layer_ref.layered_reference(clips, base, [(5, 6.5, 1.0, 0, OVR)], ls.B, ls.M, s["bone_masks"], None)[2]
    assert np.array_equal(w_all, want[2])


def test_an_additive_identity_clip_changes_nothing_and_additive_layers_add():
    from reze_engine_amd import synth
    s = ls.main_scene()
    ident = synth.make_motion(ls.B, ls.M, seed=78, keyed=np.ones(ls.B, dtype=bool), max_angle=0.0, trans=0.0, morph_keyed=1.0)
    ident["mkey_weight"] = np.zeros_like(ident["mkey_weight"])
    clips = list(s["clips"]) + [ident]
    for base, _ in s["states"][:3]:
        want = motion_ref.blend_reference(clips, base, ls.B, ls.M)
        for wt in (0.35, 1.0):
            got = layer_ref.layered_reference(clips, base, [(5, 3.0, wt, None, ADD)], ls.B, ls.M)
            assert np.abs(got[0] - want[0]).max() < 1e-7 and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])    # (f32-stored identity keys are unit to 1e-7)
    # an additive layer at weight 1: q * qL, t + tL, w + wL where the clip keys; order matters for what follows it
    base = s["states"][1][0]
    q0, t0, w0 = motion_ref.blend_reference(clips, base, ls.B, ls.M)
    ql, tl, wl = sample_reference(clips[4], 7.0, ls.B, ls.M)
    q, t, w = layer_ref.layered_reference(clips, base, [(4, 7.0, 1.0, None, ADD)], ls.B, ls.M)
    kb, km = layer_ref.keyed_bones(clips[4], ls.B), layer_ref.keyed_morphs(clips[4], ls.M)
    for b in np.flatnonzero(kb)[:8]:
        assert np.allclose(q[b], layer_ref.multiply(q0[b], ql[b] if ql[b][3] >= 0 else -ql[b]), atol=1e-12) and np.allclose(t[b], t0[b] + tl[b], atol=0)
    assert np.array_equal(q[~kb], q0[~kb]) and np.array_equal(w[km], (w0 + wl)[km]) and np.array_equal(w[~km], w0[~km])
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-6
    a = layer_ref.layered_reference(clips, base, [(4, 7.0, 1.0, None, ADD), (3, 5.5, 0.35, None, OVR)], ls.B, ls.M)
    b = layer_ref.layered_reference(clips, base, [(3, 5.5, 0.35, None, OVR), (4, 7.0, 1.0, None, ADD)], ls.B, ls.M)
    assert np.abs(a[0] - b[0]).max() > 1e-3


def test_body_and_face_concatenated_is_body_with_face_on_top():
    """the construction of the GPU bit test, in float64: the concatenation of two clips that drive disjoint bones and vertex morphs, sampled
    alone, is the body with the face as one override layer at weight 1 and the same frame"""
    body, face, cat = ls.body_and_face()
    kb, kf = layer_ref.keyed_bones(body, ls.B), layer_ref.keyed_bones(face, ls.B)
    mb, mf = layer_ref.keyed_morphs(body, ls.M), layer_ref.keyed_morphs(face, ls.M)
    assert kb.any() and kf.any() and not (kb & kf).any() and mb.any() and mf.any() and not (mb & mf).any()
    clips = [body, face, cat]
    for f in (-1.0, 6.25, 13.5, 400.0):
        assert same(layer_ref.layered_reference(clips, (0, f, None, 0.0, 0.0), [(1, f, 1.0, None, OVR)], ls.B, ls.M), sample_reference(cat, f, ls.B, ls.M))


def test_bindings_know_the_new_symbols(rz):
    capi = rz.capi
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "reze_deform.h")).read()
    for name in ("rz_upload_motion_masks", "rz_set_pose_layered"):
        assert hasattr(L, name) and name in capi.SYMBOLS and name in capi.OPTIONAL_SYMBOLS and ("int %s(rz_ctx *ctx" % name) in header
    assert "#define RZ_ABI_VERSION 8" in header and "#define RZ_MAX_MOTION_LAYERS 4" in header and "#define RZ_NO_MASK 0xffffffffu" in header
    assert "enum { RZ_LAYER_OVERRIDE = 0, RZ_LAYER_ADDITIVE = 1 };" in header
    assert capi.MOTION_LAYER_DTYPE.itemsize == 20 == ctypes.sizeof(capi.RzMotionLayer)
    assert capi.MOTION_LAYER_DTYPE.names == tuple(f[0] for f in capi.RzMotionLayer._fields_) == ("clip", "frame", "weight", "mask", "mode")
    assert (capi.MAX_MOTION_LAYERS, capi.NO_MASK, capi.LAYER_OVERRIDE, capi.LAYER_ADDITIVE) == (4, 0xffffffff, 0, 1)
    ly = rz.DeformContext.pack_motion_layers(2, [[dict(clip=1, frame=2.5, weight=0.5, mask=3, additive=True)], []])
    assert ly.shape == (2, 1) and ly.dtype == capi.MOTION_LAYER_DTYPE
    assert list(np.frombuffer(ly.tobytes(), dtype=np.uint32).reshape(2, 5)[:, 0]) == [1, capi.NO_CLIP]
    assert tuple(ly[0, 0]) == (1, 2.5, 0.5, 3, 1) and ly[1, 0]["clip"] == capi.NO_CLIP
    assert rz.DeformContext.pack_motion_layers(3, ly.reshape(-1)[:0].reshape(3, 0)).shape == (3, 0)
    assert L.rz_upload_motion_masks(None, 0, None, None) == -1 and L.rz_set_pose_layered(None, None, 0, None) == -1      # a null context is refused, not followed


def _node_flat_to_clip(f):
    names = dict(trackBone="track_bone", keyOff="key_off", keyFrame="key_frame", keyRot="key_rot", keyPos="key_pos", keyInterp="key_interp",
                 mkeyOff="mkey_off", mkeyFrame="mkey_frame", mkeyWeight="mkey_weight", feedOff="feed_off", feedTrack="feed_track", feedRatio="feed_ratio")
    c = {names[k]: np.asarray(v) for k, v in f.items()}
    c["key_interp"] = c["key_interp"].astype(np.uint8)
    return c


@needs_node
def test_apply_layered_frame_against_the_float64_definition(tmp_path):
    """Model.applyLayeredFrame on the synthetic PMX with three synthetic VMDs (walk, run and a morph-only face file) at the Node GPU
    test's states: rotations, translations and effective morph weights within 1e-6 absolute of layer_ref on the flattened motions — f64
    arithmetic on f32-stored keys, the bar of applyBlendedFrame's own check (tests/test_motion_cpu.py)."""
    import pmx_synth
    files = ls.write_node_scene(pmx_synth, str(tmp_path))
    (tmp_path / "states.json").write_text(json.dumps(dict(masks=ls.NODE_MASKS, states=ls.NODE_STATES)))
    out = subprocess.check_output(["node", os.path.join(JS, "motion_layers.js"), files["pmx"], files["vmd_a"], files["vmd_b"], files["vmd_c"],
                                   str(tmp_path / "states.json")], timeout=120)
    r = json.loads(out.decode().strip().splitlines()[-1])
    B, M = r["bones"], r["morphs"]
    clips = [_node_flat_to_clip(f) for f in r["flats"]]
    order = {"walk": 0, "run": 1, "face": 2}
    assert B == 40 and M == 9 and len(clips[2]["track_bone"]) == 0 and layer_ref.keyed_morphs(clips[2], M).any()
    names = list(ls.NODE_MASKS)
    bm = np.array([r["masks"][n]["bones"] for n in names], dtype=np.uint8)
    mm = np.array([r["masks"][n]["morphs"] for n in names], dtype=np.uint8)
    assert bm.shape == (len(names), B) and mm.shape == (len(names), M)
    assert bm[names.index("upper")].sum() > 5 and r["descendantsAdded"] > 0           # withDescendants grew the mask over the parent table
    worst, changed = 0.0, 0
    for st, res in zip(ls.NODE_STATES, r["results"]):
        base = (order[st["a"]], st["frameA"], order[st["b"]] if st.get("b") else None, st.get("frameB", 0), st.get("blend", 0))
        layers = [(order[l["motion"]], l["frame"], l.get("weight", 1), None if l.get("mask") is None else names.index(l["mask"]), ADD if l.get("additive") else OVR)
                  for l in st.get("layers", [])]
        dots = []
        q, t, w = layer_ref.layered_reference(clips, base, layers, B, M, bm, mm, dots=dots)
        assert all(d >= (0.9 if k == "add" else 0.5) for k, d in dots) and motion_ref.min_abs_dot(clips, base, B) >= 0.5, st       # the rule the Node GPU test's bar rests on
        e = max(np.abs(np.array(res["rot"]).reshape(B, 4) - q).max(), np.abs(np.array(res["tra"]).reshape(B, 3) - t).max(), np.abs(np.array(res["mw"]) - w).max())
        worst = max(worst, e)
        assert e <= 1e-6, (st, e)
        q0, _t0, w0 = motion_ref.blend_reference(clips, base, B, M)
        changed += bool(layers) and (np.abs(q - q0).max() > 1e-3 or np.abs(w - w0).max() > 1e-3)
    assert changed >= 4 and r["badLayerThrows"] == 4
    print("applyLayeredFrame vs float64: worst %.3e over %d states" % (worst, len(ls.NODE_STATES)))


@needs_node
def test_engine_uploads_masks_once_and_sends_one_layered_pose_per_frame(tmp_path):
    import pmx_synth
    files = ls.write_node_scene(pmx_synth, str(tmp_path))
    out = subprocess.check_output(["node", os.path.join(JS, "motion_layers_mock.js"), files["pmx"], files["vmd_a"], files["vmd_b"], files["vmd_c"]], timeout=60)
    r = json.loads(out.decode().strip().splitlines()[-1])
    calls = r["calls"]
    kinds = [next(iter(c)) for c in calls]
    # without layers: what seekMotions sent before
    assert r["plain"] == ["setPoseBlended", "deform"]
    ups = [c for c in calls if "uploadMotionMasks" in c]
    assert len(ups) == 2 and ups[0]["n"] == 1 and ups[1]["n"] == 2 and ups[0]["morphs"] is True          # once per mask set: again after a second mask was set
    poses = [c for c in calls if "setPoseLayered" in c]
    NO, NOM = motion_ref.NO_CLIP, layer_ref.NO_MASK
    assert [(p["nLayers"], len(p["states"])) for p in poses] == [(1, 1), (1, 1), (2, 1), (2, 3)]
    assert poses[0]["states"] == [[0, 3.5, NO, 0, 0]] and poses[0]["layers"] == [[2, 3.5, 1, NOM, 0]]
    assert poses[2]["layers"] == [[1, 2, 0.5, 0, 0], [2, 7, 0.25, 1, 1]]
    assert poses[3]["layers"] == [[2, 1, 1, NOM, 0], [NO, 0, 0, NOM, 0], [1, 4, 0.5, 0, 0], [2, 4, 1, 1, 1], [NO, 0, 0, NOM, 0], [NO, 0, 0, NOM, 0]]       # shorter lists are padded with skipped layers
    for i, c in enumerate(calls):
        if "setPoseLayered" in c:
            assert calls[i + 1] == {"deform": c["setPoseLayered"]}
    assert kinds.count("uploadMotions") == 1
    assert "unknown mask" in r["unknownMask"] and "unknown motion" in r["unknownMotion"] and "at most 4" in r["tooMany"] and "unknown bone" in r["unknownBone"]
    # the host path: no masks on the device — applyLayeredFrame, then a plain frame
    assert [next(iter(c)) for c in r["hostCalls"]] == ["setPose", "deform"] and "one character" in r["hostCrowd"]
