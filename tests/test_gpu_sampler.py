"""The device motion sampler (kernels/fk.hip.h: span_guess / span_bisect / bone_issue / bone_finish / morph_issue / morph_finish / bezier_y)
held to the float64 sampler on long, uneven key tracks: the scenes of tests/sampler_scenes.py — tracks of 1 to 70 000 keys, bursts, gaps of
hundreds of frames, runs of equal frames, key indices beyond 65 536, frames beyond 100 000, curves whose x(t) is flat at an end — through
every kernel that samples: rz_fk_kernel's generic solve, the fused frame's specialised sampled solve, the tail loop of skeletons beyond
512 bones, the one-launch crowd front, and rz_motion_kernel on a library whose second clip lies behind 80 000 keys of the first.

Bars, none of them new: world matrices within 5e-5 x max(1, |ref|.max()) of fk_reference(sample_reference(...)) (the bar of
test_device_motion_sampling_matches_the_float64_sampler), positions and normals within helpers.POS_TOL / NRM_TOL of the oracle fed the
device's world matrices and the reference's morph weights; blended poses: the bars of tests/test_gpu_motion.py. Consecutive keys of every
track differ by 100 x the world bar or more, so a neighbouring span cannot pass; tests/test_sampler_cpu.py holds the float32 arithmetic on
exactly these samples to a quarter of the bar. Every test prints its worst errors before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref
import sampler_scenes as ss
from helpers import NRM_TOL, POS_TOL, fk_reference, parity_errors, sample_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_BAR = 5e-5                        # x max(1, |ref|.max())
BLEND_W_BAR, BLEND_P_BAR = 5e-5, 2e-4      # tests/test_gpu_motion.py: W_BAR, P_BAR
MORPH_KEYS = ("mkey_off", "mkey_frame", "mkey_weight", "feed_off", "feed_track", "feed_ratio")
_refs = {}


def without_morphs(clip):
    c = dict(clip)
    for k in MORPH_KEYS:
        c[k] = None
    return c


def world_of(sc, q, t):
    m = sc["mesh"]
    return fk_reference(m["parents"], m["bind"], q, t, sc["ap"], sc["ratio"], sc["move"])


def ref_a(sc, k):
    """(world [B,16], morph weights [M]) in float64 of clip A at the scene's frame k, computed once per scene"""
    key = (sc["name"], "a", k)
    if key not in _refs:
        q, t, w = sample_reference(sc["clip_a"], float(sc["frames"][k]), sc["B"], sc["M"])
        _refs[key] = (world_of(sc, q, t), w)
    return _refs[key]


def ref_state(sc, state):
    """the same of a library state (clip_a, frame_a, clip_b, frame_b, blend) over [clip A, clip B]"""
    key = (sc["name"], "state") + tuple(state)
    if key not in _refs:
        q, t, w = motion_ref.blend_reference([sc["clip_a"], sc["clip_b"]], state, sc["B"], sc["M"])
        _refs[key] = (world_of(sc, q, t), w)
    return _refs[key]


def make_ctx(lib, sc, morphs="dense", instances=1, animation=True, library=False):
    m = sc["mesh"]
    c = lib.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    if morphs == "dense":
        c.upload_morphs_dense(sc["dense"])
    elif morphs == "sparse":
        c.upload_morphs_sparse(*sc["sparse"])
    if instances > 1:
        c.set_instances(instances)
    c.upload_skeleton_topology(m["parents"], m["bind"], sc["ap"], sc["ratio"], sc["move"])
    strip = without_morphs if morphs == "none" else dict
    if animation:
        c.upload_animation(**strip(sc["clip_a"]))
    if library:
        c.upload_motions([strip(sc["clip_a"]), strip(sc["clip_b"])])
    return c


def snapshot(c, inst=0):
    p, n = c.read(inst)
    return c.read_world(inst), p, n


def same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def errors(sc, oracle, snap, ref, morphs):
    """(world error / max(1, |ref|), worst position error, worst normal error) of one snapshot against its float64 reference"""
    wg, pg, ng = snap
    world, w = ref
    assert np.isfinite(wg).all() and np.isfinite(pg).all() and np.isfinite(ng).all()
    ew = float(np.abs(wg - world).max()) / max(1.0, float(np.abs(world).max()))
    m = sc["mesh"]
    pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], wg, m["inv_bind"],
                           sc["dense"] if morphs != "none" else None, w.astype(np.float32) if morphs != "none" else None)
    ep, en = parity_errors(pg, ng, pr, nr)
    return np.array([ew, float(ep.max()), float(en.max())])


def report(path, worst, bars=(W_BAR, POS_TOL, NRM_TOL)):
    print("sampler parity | %s | world %.3e x max(1, |ref|) (bar %.0e) | positions %.3e (bar %.0e) | normals %.3e (bar %.0e)"
          % (path, worst[0], bars[0], worst[1], bars[1], worst[2], bars[2]))
    assert worst[0] <= bars[0] and worst[1] <= bars[1] and worst[2] <= bars[2], (path, worst)


def run_frames(c, sc, oracle, morphs, what):
    """one call per scene frame on a single character: every frame against its reference; returns the snapshots"""
    worst, shots = np.zeros(3), []
    for k, f in enumerate(sc["frames"]):
        c.set_pose_sampled([f])
        c.deform()
        shots.append(snapshot(c))
        e = errors(sc, oracle, shots[-1], ref_a(sc, k), morphs)
        if (e > 0.5 * np.array([W_BAR, POS_TOL, NRM_TOL])).any():
            print("  %s frame %r (%s): %s" % (what, float(f), sc["frame_notes"][k], e))
        worst = np.maximum(worst, e)
    return worst, shots


def test_one_character_behind_the_generic_sampler_of_rz_fk_kernel(rz, oracle):
    sc = ss.scene("b48")
    with make_ctx(rz, sc) as c:
        c.set_tuning(fuse_fk=0)
        c.set_pose_sampled([sc["frames"][0]])
        assert c.get_tuning("effective_fuse_fk") == 0
        worst, _ = run_frames(c, sc, oracle, "dense", "rz_fk_kernel")
    report("one character, rz_fk_kernel (B = 48, 8 dense morphs)", worst)


@pytest.mark.parametrize("zero_copy", [1, 0])
@pytest.mark.parametrize("morphs", ["dense", "sparse", "none"])
def test_one_character_in_the_fused_frame(rz, oracle, morphs, zero_copy):
    """The fused frame: the specialised sampled solve (KIND 2, unpredicated key loads) with 8 dense morphs and with none; 260 sparse morphs
    are beyond the 256 it covers and take the generic solve inside the fused frame, the second chunk of morphs included. zero_copy = 1: the
    frame number rides in the kernel arguments; 0: it travels through the frames buffer."""
    sc = ss.scene("b48_sparse" if morphs == "sparse" else "b48")
    with make_ctx(rz, sc, morphs) as c:
        c.set_tuning(fuse_fk=1, zero_copy=zero_copy)
        c.set_pose_sampled([sc["frames"][0]])
        assert c.get_tuning("effective_fuse_fk") == 1
        assert c.get_tuning("effective_fk_kind") == (0 if morphs == "sparse" else 2)
        worst, _ = run_frames(c, sc, oracle, morphs, "fused frame")
    if morphs == "sparse":
        assert max(float(np.abs(ref_a(sc, k)[1][256:]).max()) for k in range(len(sc["frames"]))) > 0.3      # the second chunk's weights matter
    report("one character, fused frame (B = 48, %s morphs, zero_copy = %d)" % (morphs, zero_copy), worst)


@pytest.mark.parametrize("fuse", [0, 1])
def test_a_skeleton_beyond_512_bones_samples_its_tail_bones(rz, oracle, fuse):
    """B = 520: bones 512 .. 519 — the 70 000-key track among them — are sampled by the `i + 2 * kBlock` loop of the generic solve"""
    sc = ss.scene("b520")
    with make_ctx(rz, sc) as c:
        c.set_tuning(fuse_fk=fuse)
        c.set_pose_sampled([sc["frames"][0]])
        assert c.get_tuning("effective_fuse_fk") == fuse
        if fuse:
            assert c.get_tuning("effective_fk_kind") == 0
        worst, _ = run_frames(c, sc, oracle, "dense", "B = 520 fuse_fk = %d" % fuse)
    report("one character, B = 520, %s" % ("fused frame" if fuse else "rz_fk_kernel"), worst)


def test_a_crowd_of_48_behind_rz_fk_kernel_and_in_the_one_launch_front(rz, oracle):
    """I = 48, one scene frame per instance, no morphs (the crowd kernel's forms). The front of rz_skin_instances_fk_kernel samples the
    closure of its vertex run's bones — the append bones pull in their append parents' long tracks. Both forms: bit for bit."""
    sc = ss.scene("b48")
    idx, frames = ss.crowd_frames(sc, 48)
    outs = {}
    with make_ctx(rz, sc, "none", instances=48) as c:
        for fuse in (-1, 0):
            c.set_tuning(fuse_fk=fuse)
            c.set_pose_sampled(frames)
            assert c.get_tuning("effective_fuse_fk") == (1 if fuse else 0)
            c.deform()
            if fuse:
                assert "rz_skin_instances_fk_kernel" in c.kernel_name() and c.get_tuning("effective_closure_bones") > 0
            outs[fuse] = [c.read(i) for i in range(48)]
            worlds = [c.read_world(i) for i in range(48)]
            worst = np.zeros(3)
            for i in range(48):
                worst = np.maximum(worst, errors(sc, oracle, (worlds[i],) + tuple(outs[fuse][i]), ref_a(sc, int(idx[i])), "none"))
            report("crowd of 48, %s" % ("one-launch front" if fuse else "rz_fk_kernel + skin kernel"), worst)
    for i in range(48):
        assert same_bits(outs[-1][i], outs[0][i]), "instance %d (frame %r): the one-launch front differs from rz_fk_kernel" % (i, float(frames[i]))


def test_the_library_with_clip_b_behind_clip_a(rz, oracle):
    """upload_motions([A, B]): every key index of B's records is shifted by A's 80 000 keys. blend 0 on A has the bits of
    rz_set_pose_sampled on A; blend 1 into B at B's frames and blend 0.5 of both against the float64 definition, for one character and
    for a crowd."""
    sc = ss.scene("b48")
    assert len(sc["clip_a"]["key_frame"]) > 65536
    pick = [0, 1, 2, 9, 12, 15, 17, 19, 29, 32, 41, 45, 46, 49, 50, 54]          # a key run, bursts, gaps, deep in the long track, one float32 step off a key
    fb = sc["frames_b"]
    with make_ctx(rz, sc, library=True) as c, make_ctx(rz, sc) as d:
        assert c.get_tuning("motion_clips") == 2
        for k in pick:
            f = float(sc["frames"][k])
            d.set_pose_sampled([f]); d.deform()
            c.set_pose_blended(0, f, None, 0.0, 0.0); c.deform()
            assert same_bits(snapshot(c), snapshot(d)), "blend 0 on clip A at frame %r (%s) is not rz_set_pose_sampled's frame" % (f, sc["frame_notes"][k])
        worst1, worst5 = np.zeros(3), np.zeros(3)
        alone = []
        states = [(0, float(sc["frames"][k]), 1, float(fb[n % len(fb)]), 0.5) for n, k in enumerate(pick)]
        for n, st in enumerate(states):
            one = (0, st[1], 1, float(fb[n % len(fb)]), 1.0)
            c.set_pose_blended(*one); c.deform()
            worst1 = np.maximum(worst1, errors(sc, oracle, snapshot(c), ref_state(sc, one), "dense"))
            c.set_pose_blended(*st); c.deform()
            alone.append(snapshot(c))
            worst5 = np.maximum(worst5, errors(sc, oracle, alone[-1], ref_state(sc, st), "dense"))
    report("library, blend 1 into clip B (records shifted by %d keys)" % len(sc["clip_a"]["key_frame"]), worst1, (BLEND_W_BAR, BLEND_P_BAR, BLEND_P_BAR))
    report("library, blend 0.5 of A and B, one character", worst5, (BLEND_W_BAR, BLEND_P_BAR, BLEND_P_BAR))
    worst = np.zeros(3)
    with make_ctx(rz, sc, instances=len(states), animation=False, library=True) as c:
        c.set_pose_blended(*zip(*states)); c.deform()
        for i, st in enumerate(states):
            worst = np.maximum(worst, errors(sc, oracle, snapshot(c, i), ref_state(sc, st), "dense"))
    report("library, blend 0.5 of A and B, crowd of %d" % len(states), worst, (BLEND_W_BAR, BLEND_P_BAR, BLEND_P_BAR))


def test_variants_build_equals_the_product(rz, rzv):
    sc = ss.scene("b48")
    out = []
    for lib in (rz, rzv):
        got = []
        with make_ctx(lib, sc) as c:
            for fuse in (0, 1):
                c.set_tuning(fuse_fk=fuse)
                for f in sc["frames"]:
                    c.set_pose_sampled([f]); c.deform()
                    got.append(snapshot(c))
        out.append(got)
    for k in range(len(out[0])):
        assert same_bits(out[0][k], out[1][k]), "fuse_fk %d frame %r" % (k // len(sc["frames"]), float(sc["frames"][k % len(sc["frames"])]))


# ---- refusals: non-finite frames and keys ----
def _bad_clips(sc):
    """(what the message must name, clip): clip A with one non-finite value in a track that drives a bone / feeds a morph of the model"""
    a = sc["clip_a"]
    t_long = int(np.flatnonzero(a["track_bone"] == ss.bone_of(sc, "long"))[0])
    k0 = int(a["key_off"][t_long])
    out = []
    for field, at, value, msg in (("key_frame", k0, -np.inf, "track %d key 0: the frame is not finite" % t_long),
                                  ("key_frame", k0 + 69999, np.inf, "track %d key 69999: the frame is not finite" % t_long),
                                  ("key_rot", (k0 + 65600, 2), np.nan, "track %d key 65600: the rotation is not finite" % t_long),
                                  ("key_pos", (k0 + 7, 0), np.inf, "track %d key 7: the position is not finite" % t_long),
                                  ("mkey_weight", int(a["mkey_off"][3]) + 4000, np.nan, "morph track 3 key 4000: the weight is not finite"),
                                  ("mkey_frame", int(a["mkey_off"][0]), np.nan, "morph track 0 key 0: the frame is not finite")):
        c = dict(a)
        c[field] = np.array(a[field], copy=True)
        c[field][at] = value
        out.append((msg, c))
    return out


def test_non_finite_frames_and_keys_are_refused_and_leave_the_resident_motion_alone(rz):
    sc = ss.scene("b48")
    f = float(sc["frames"][20])
    with make_ctx(rz, sc) as c:
        c.set_pose_sampled([f]); c.deform()
        before = snapshot(c)
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(rz.RzError) as e:
                c.set_pose_sampled([bad])
            assert e.value.code == -1 and "instance 0: a frame that would be sampled is not finite" in str(e.value)
            c.deform()
            assert same_bits(before, snapshot(c)), "a refused frame changed the resident pose"
        for msg, clip in _bad_clips(sc):
            with pytest.raises(rz.RzError) as e:
                c.upload_animation(**clip)
            assert e.value.code == -1 and msg in str(e.value), (msg, str(e.value))
        c.set_pose_sampled([f]); c.deform()
        assert same_bits(before, snapshot(c)), "a refused upload changed the resident motion"
        # keys that drive nothing of this model are not looked at: a bone the model lacks, a morph track no feed names
        ok = dict(sc["clip_a"])
        t_lost = int(np.flatnonzero(ok["track_bone"] >= sc["B"])[0])
        ok["key_rot"] = ok["key_rot"].copy(); ok["key_rot"][int(ok["key_off"][t_lost])] = np.nan
        c.upload_animation(**ok)
        c.set_pose_sampled([f]); c.deform()
        assert same_bits(before, snapshot(c))
    with make_ctx(rz, sc, instances=3) as c:
        with pytest.raises(rz.RzError) as e:
            c.set_pose_sampled([1.0, 2.0, np.nan])
        assert "instance 2: a frame that would be sampled is not finite" in str(e.value)
    with make_ctx(rz, sc, animation=False, library=True) as c:
        st = (0, f, 1, 7.0, 0.5)
        c.set_pose_blended(*st); c.deform()
        before = snapshot(c)
        for msg, clip in _bad_clips(sc)[:3]:
            with pytest.raises(rz.RzError) as e:
                c.upload_motions([sc["clip_b"], clip])
            assert "rz_upload_motions: clip 1: " + msg in str(e.value), (msg, str(e.value))
            assert c.get_tuning("motion_clips") == 2
        c.set_pose_blended(*st); c.deform()
        assert same_bits(before, snapshot(c)), "a refused library changed the resident one"


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_addon_surfaces_the_refusals_unchanged(rz):
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "sampler_refusals.js")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.loads(p.stdout.decode().strip().splitlines()[-1])
    want = ["instance 0: a frame that would be sampled is not finite"] * 2 + ["track 0 key 1: the rotation is not finite",
                                                                              "track 1 key 1: the position is not finite", "track 0 key 0: the frame is not finite"]
    assert [m is not None and m.endswith(w) for m, w in zip(out["messages"], want)] == [True] * 5, out["messages"]
    assert out["sameBits"] is True
