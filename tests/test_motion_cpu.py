"""CPU checks of the motion library: the float64 definition tests/motion_ref.py, the inputs the GPU tests rest on, the host twin
Model.applyBlendedFrame, Engine.loadMotion / seekMotions against a recording addon, the bindings."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref
import motion_scenes as ms
from helpers import sample_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
JS = os.path.join(ROOT, "tests", "js")


def test_blend_endpoints_are_the_clips_bit_for_bit():
    s = ms.main_scene()
    clips = s["clips"]
    a = sample_reference(clips[0], 4.37, ms.B, ms.M)
    b = sample_reference(clips[1], 8.5, ms.B, ms.M)
    for st, want in (((0, 4.37, 1, 8.5, 0.0), a), ((0, 4.37, None, 0.0, 0.0), a), ((0, 4.37, motion_ref.NO_CLIP, 0.0, 0.7), a), ((0, 4.37, 1, 8.5, 1.0), b),
                     ((0, float("nan"), 1, 8.5, 1.0), b)):
        got = motion_ref.blend_reference(clips, st, ms.B, ms.M)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), st
    assert not np.array_equal(a[0], b[0])


def test_blend_gives_unit_quaternions_on_the_shortest_path():
    s = ms.main_scene()
    for st in s["states"] + s["extra"]:
        q = motion_ref.blend_reference(s["clips"], st, ms.B, ms.M)[0]
        assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() < 1e-6, st          # (f32-stored keys are unit to 1e-7; the slerp keeps that)
    # a second quaternion stored on the far side (dot -0.9): the blend goes the short way, through the negated one
    a = np.array([0.0, 0.0, 0.0, 1.0])
    half = np.arccos(0.9)
    b = -np.array([np.sin(half), 0.0, 0.0, np.cos(half)])
    assert abs(float(a @ b) + 0.9) < 1e-12
    for t in (0.25, 0.5, 0.75):
        q = motion_ref.slerp(a, b, t)
        assert abs(np.linalg.norm(q) - 1.0) < 1e-12
        assert np.allclose(q, [np.sin(half * t), 0.0, 0.0, np.cos(half * t)], atol=1e-12), (t, q)     # angle t x the short arc, not t x the long one
    # nearly parallel: the normalised lerp
    c = np.array([1e-3, 0.0, 0.0, 1.0]); c /= np.linalg.norm(c)
    assert abs(np.linalg.norm(motion_ref.slerp(a, c, 0.3)) - 1.0) < 1e-12


def test_a_clip_that_does_not_key_a_bone_or_morph_counts_as_rest():
    s = ms.main_scene()
    kind, clips = s["kind"], s["clips"]
    only0, only1, none = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2), np.flatnonzero(kind == 3)
    assert len(only0) > 10 and len(only1) > 10 and len(none) > 10 and (kind == 0).sum() > 10
    qa, ta, wa = sample_reference(clips[0], 4.37, ms.B, ms.M)
    qb, tb, wb = sample_reference(clips[1], 8.5, ms.B, ms.M)
    ident = np.array([0.0, 0.0, 0.0, 1.0])
    assert (qb[only0] == ident).all() and (tb[only0] == 0).all() and (qa[only1] == ident).all() and (qa[none] == ident).all()
    q, t, w = motion_ref.blend_reference(clips, (0, 4.37, 1, 8.5, 0.5), ms.B, ms.M)
    assert (q[none] == ident).all() and (t[none] == 0).all()
    for b in only0[:5]:
        assert np.allclose(q[b], motion_ref.slerp(qa[b], ident, 0.5), atol=0) and np.allclose(t[b], ta[b] * 0.5)
    for b in only1[:5]:
        assert np.allclose(q[b], motion_ref.slerp(ident, qb[b], 0.5), atol=0) and np.allclose(t[b], tb[b] * 0.5)
    # morphs: a morph a clip leaves without keys weighs 0 there; the blend is linear on the effective weights (own track + group feed)
    unkeyed_a = [m for m in range(ms.M) if wa[m] == 0.0]
    assert unkeyed_a and np.allclose(w, wa + (wb - wa) * 0.5, atol=0)
    for m in unkeyed_a:
        assert w[m] == wb[m] * 0.5
    own = dict(clips[0]); own["feed_off"] = np.array([0] * 3 + [1] * (ms.M - 2), dtype=np.uint32); own["feed_track"] = np.array([2], dtype=np.int32)
    own["feed_ratio"] = np.array([1.0], dtype=np.float32)
    w_own = sample_reference(own, 4.37, ms.B, ms.M)[2][2]
    assert wa[2] != w_own and wa[2] > w_own                     # morph 2 is also fed by the group track (ratio 0.5)


def test_the_inputs_of_the_gpu_tests_keep_the_blends_sign_choice_safe():
    """every state the GPU tests blend two clips in and hold to float64 (main scene, leg rig, the sparse-morph scene): |qa . qb| >= 0.7 on
    every bone, in float64"""
    worst = 1.0
    n = 0
    for clips, st, bones in ms.all_blended_states():
        d = motion_ref.min_abs_dot(clips, st, bones)
        worst = min(worst, d)
        n += d < 1.0
        assert d >= 0.7, (st, d)
    assert n >= 8                   # main: 2 of the five + 2 extra; leg rig: 3; sparse-morph scene: 1
    print("smallest |dot| over %d blended states: %.3f" % (n, worst))
    s = ms.main_scene()
    assert ms.depth_of(s["mesh"]["parents"]) > 16 and ms.B > 256
    # the keys themselves: uneven frames with a duplicate, flipped signs in clip 1, interpolation bytes 1 .. 126
    c1 = s["clips"][1]
    kf = c1["key_frame"][:7]
    assert (np.diff(kf) >= 0).all() and (np.diff(kf) == 0).sum() == 1 and len(set(np.diff(kf))) > 2
    assert c1["key_interp"].min() >= 1 and c1["key_interp"].max() <= 126
    rot = c1["key_rot"].reshape(-1, 7, 4)
    flips = (np.sum(rot[:, 1:] * rot[:, :-1], axis=2) < 0).mean()
    assert 0.3 < flips < 0.7, flips


def test_make_motion_builds_a_valid_clip():
    from reze_engine_amd import synth
    c = synth.make_motion(20, 6, seed=3, group_feed=(1, 0.25))
    n = len(c["track_bone"])
    assert c["key_off"][-1] == len(c["key_frame"]) == len(c["key_rot"]) == len(c["key_pos"]) == len(c["key_interp"]) == n * 6
    assert np.abs(np.linalg.norm(c["key_rot"], axis=1) - 1).max() < 1e-6
    assert len(c["feed_off"]) == 7 and c["feed_off"][-1] == len(c["feed_track"]) == len(c["feed_ratio"])
    assert c["feed_track"].max() == 6 and len(c["mkey_off"]) == 8 and c["mkey_off"][-1] == len(c["mkey_frame"]) == len(c["mkey_weight"])
    lo, hi = c["feed_off"][1], c["feed_off"][2]
    assert list(c["feed_track"][lo:hi])[-1] == 6 and c["feed_ratio"][hi - 1] == 0.25
    d = synth.make_motion(20, 0, seed=3, uneven=False, interp=False, keyed=np.arange(20) < 5)
    assert list(d["track_bone"]) == [0, 1, 2, 3, 4] and d["key_interp"] is None and "mkey_off" not in d
    assert (np.diff(d["key_frame"][:6]) == 8).all()


def test_bindings_know_the_new_symbols(rz):
    capi = rz.capi
    L = capi.load()
    assert hasattr(L, "rz_upload_motions") and hasattr(L, "rz_set_pose_blended")
    assert "rz_upload_motions" in capi.SYMBOLS and "rz_set_pose_blended" in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "reze_deform.h")).read()
    assert "#define RZ_ABI_VERSION 8" in header and "#define RZ_NO_CLIP 0xffffffffu" in header
    assert capi.MOTION_STATE_DTYPE.itemsize == 20 == __import__("ctypes").sizeof(capi.RzMotionState)
    st = rz.DeformContext.pack_motion_states(3, [0, 1, 2], 1.5, [-1, 0, capi.NO_CLIP], [0.0, 2.0, 3.0], [0.0, 0.5, 1.0])
    raw = np.frombuffer(st.tobytes(), dtype=np.uint32).reshape(3, 5)
    assert list(raw[:, 0]) == [0, 1, 2] and list(raw[:, 2]) == [capi.NO_CLIP, 0, capi.NO_CLIP]
    assert list(np.frombuffer(st.tobytes(), dtype=np.float32).reshape(3, 5)[:, 4]) == [0.0, 0.5, 1.0]
    assert L.rz_upload_motions(None, 0, None) == -1 and L.rz_set_pose_blended(None, None) == -1          # a null context is refused, not followed


def _node_flat_to_clip(f):
    names = dict(trackBone="track_bone", keyOff="key_off", keyFrame="key_frame", keyRot="key_rot", keyPos="key_pos", keyInterp="key_interp",
                 mkeyOff="mkey_off", mkeyFrame="mkey_frame", mkeyWeight="mkey_weight", feedOff="feed_off", feedTrack="feed_track", feedRatio="feed_ratio")
    c = {names[k]: np.asarray(v) for k, v in f.items()}
    c["key_interp"] = c["key_interp"].astype(np.uint8)
    return c


@needs_node
def test_apply_blended_frame_against_the_float64_definition(tmp_path):
    """Model.applyBlendedFrame on the synthetic PMX (40 bones, an append bone, vertex / bone / group morphs: 'grp' feeds v0, blink and the
    bone morph 'twist') with the two synthetic VMDs the Node GPU test uses, at that test's states and two more: rotations, translations
    and effective morph weights within 1e-6 absolute of motion_ref on the flattened motions — f64 arithmetic on f32-stored keys, the bar
    of the host sampler's own checks (tests/test_host_js.py)."""
    import pmx_synth
    files = ms.write_node_scene(pmx_synth, str(tmp_path))
    order = {"walk": 0, "run": 1}
    states = [[order[s["a"]], s["frameA"], order[s["b"]] if s.get("b") else None, s.get("frameB", 0), s.get("blend", 0)] for s in ms.NODE_STATES]
    states += [[0, 1000, 1, -5, 0.5], [1, 6, 0, 6, 0.125]]
    (tmp_path / "states.json").write_text(json.dumps(states))
    out = subprocess.check_output(["node", os.path.join(JS, "motion_blend.js"), files["pmx"], files["vmd_a"], files["vmd_b"], str(tmp_path / "states.json")], timeout=120)
    r = json.loads(out.decode().strip().splitlines()[-1])
    B, M = r["bones"], r["morphs"]
    clips = [_node_flat_to_clip(f) for f in r["flats"]]
    assert B == 40 and M == 9 and r["badBlendThrows"] == 3
    assert sorted(clips[0]["track_bone"]) == [0, 1, 3, 5, 20] and sorted(clips[1]["track_bone"]) == [1, 3, 8, 20, 25]
    grp_fed = [m for m in range(M) if clips[1]["feed_off"][m + 1] - clips[1]["feed_off"][m] >= 1]
    assert len(grp_fed) >= 3                                     # 'grp' feeds v0, blink and twist in the second motion
    worst = 0.0
    for st, res in zip(states, r["results"]):
        q, t, w = motion_ref.blend_reference(clips, tuple(st), B, M)
        assert motion_ref.min_abs_dot(clips, tuple(st), B) >= 0.7, st          # the rule the Node GPU test's bar rests on
        e = max(np.abs(np.array(res["rot"]).reshape(B, 4) - q).max(), np.abs(np.array(res["tra"]).reshape(B, 3) - t).max(), np.abs(np.array(res["mw"]) - w).max())
        worst = max(worst, e)
        assert e <= 1e-6, (st, e)
        assert np.abs(w).max() > 0.05 or st[1] <= 0
    print("applyBlendedFrame vs float64: worst %.3e" % worst)


@needs_node
def test_engine_uploads_the_library_once_and_sends_one_state_per_instance(tmp_path):
    import pmx_synth
    files = ms.write_node_scene(pmx_synth, str(tmp_path))
    out = subprocess.check_output(["node", os.path.join(JS, "motion_mock.js"), files["vmd_a"], files["vmd_b"]], timeout=60)
    r = json.loads(out.decode().strip().splitlines()[-1])
    calls = r["calls"]
    ups = [i for i, c in enumerate(calls) if "uploadMotions" in c]
    assert len(ups) == 2 and all(calls[i]["uploadMotions"] == "ctx0" and calls[i]["clips"] == 2 for i in ups)      # once, and again after the replaced clip
    assert calls[ups[0]]["tracks"] == [3, 2] and calls[ups[1]]["tracks"] == [3, 3]                                 # 'run' became the first motion's file, in place
    assert r["forkMade"] and {"destroy": "fork1"} in calls and calls.index({"destroy": "fork1"}) < ups[1]           # forks go before the static upload
    poses = [c for c in calls if "setPoseBlended" in c]
    NO = motion_ref.NO_CLIP
    assert [len(p["states"]) for p in poses] == [1, 1, 1, 3, 3]
    assert poses[0]["states"] == [[0, 3.5, NO, 0, 0]] and poses[1]["states"] == [[0, 4.5, 1, 2, 0.25]] and poses[2]["states"] == [[1, 1, NO, 0, 0]]
    assert poses[3]["states"] == [[0, 1, NO, 0, 0], [1, 2, 0, 3, 1], [0, 5, 0, 6, 0.5]] and poses[4]["states"] == [[1, 9, NO, 0, 0]] * 3
    assert poses[0]["setPoseBlended"] != poses[1]["setPoseBlended"]                                                  # two frames in flight alternate contexts
    for i, c in enumerate(calls):
        if "setPoseBlended" in c:
            assert calls[i + 1] == {"deform": c["setPoseBlended"]}
    assert "unknown motion" in r["unknown"] and "jump" in r["unknownB"] and "2 states for 3 instances" in r["wrongCount"]
    # the host path: no library upload, no blended pose on the device — applyBlendedFrame, then a plain frame
    kinds = [next(iter(c)) for c in r["hostCalls"]]
    assert kinds == ["setPose", "deform"] and "one character" in r["hostCrowd"]
    assert abs(np.linalg.norm(r["hostRot1"]) - 1) < 1e-6 and abs(r["hostRot1"][3]) < 0.99999
