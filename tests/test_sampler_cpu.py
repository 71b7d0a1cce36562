"""What the GPU bars of tests/test_gpu_sampler.py rest on, checked without a device on exactly the scenes and frames those tests use
(tests/sampler_scenes.py): the float32 restatement of the device sampler (helpers.sample_device_f32: bezier_y's 24 iterations and 1e-7
threshold, span_guess + span_bisect, the slerp and the lerps in float32) stays within a quarter of the GPU bar of the float64 sampler on
every sample, its span search returns the float64 sampler's spans, the scene really sends that search down its repair path, one-off errors
in the search leave the bar, and the host sampler (host/vmd-sampler.js) agrees with the float64 reference on the same long tracks."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sampler_scenes as ss
from helpers import SPAN_MUTANTS, bezier_reference, fk_reference, sample_reference, span_device_f32, span_guess_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_BAR = 5e-5                    # the GPU bar on world matrices: 5e-5 x max(1, |ref|.max())
SCENES = ("b48", "b48_sparse", "b520")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
_memo = {}


def world_of(sc, pose):
    q, t, _ = pose
    m = sc["mesh"]
    return fk_reference(m["parents"], m["bind"], q, t, sc["ap"], sc["ratio"], sc["move"])


def samples(name):
    """every (frame, float64 pose, float64 world matrices) of a scene: clip A at the scene's frames, clip B at its own"""
    if name not in _memo:
        sc = ss.scene(name)
        out = []
        for clip, frames in ((sc["clip_a"], sc["frames"]), (sc["clip_b"], sc["frames_b"])):
            for f in frames:
                pose = sample_reference(clip, float(f), sc["B"], sc["M"])
                out.append((clip, f, pose, world_of(sc, pose)))
        _memo[name] = out
    return _memo[name]


def world_error(sc, clip, f, ref_world, **kw):
    w = world_of(sc, sample_reference(clip, float(f), sc["B"], sc["M"], dtype=np.float32, **kw))
    return float(np.abs(w - ref_world).max()) / max(1.0, float(np.abs(ref_world).max()))


def tracks_of(clip):
    """(key frames f32, first key, one past the last key) of every bone and morph track that holds keys"""
    out = []
    for kf, off in ((clip["key_frame"], clip["key_off"]), (clip["mkey_frame"], clip["mkey_off"])):
        kf = np.asarray(kf, dtype=np.float32)
        out += [(kf, int(off[t]), int(off[t + 1])) for t in range(len(off) - 1) if off[t + 1] > off[t]]
    return out


def reference_span(kf, b, e, f):
    """sample_reference's span(): bisection in float64"""
    lo, hi = b, e - 1
    if f <= kf[lo]:
        return lo, lo
    if f >= kf[hi]:
        return hi, hi
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if kf[mid] <= f:
            lo = mid
        else:
            hi = mid
    return lo, hi


@pytest.mark.parametrize("name", SCENES)
def test_float32_restatement_stays_within_a_quarter_of_the_gpu_bar(name):
    """Conditioning: on every (scene, frame) the GPU tests sample, the device's arithmetic restated in float32 gives world matrices within
    a quarter of the GPU bar of the float64 run, and morph weights within 1e-6. None is left out."""
    sc = ss.scene(name)
    worst, worst_w, at = 0.0, 0.0, None
    for clip, f, pose, world in samples(name):
        e = world_error(sc, clip, f, world)
        w32 = sample_reference(clip, float(f), sc["B"], sc["M"], dtype=np.float32)[2]
        worst_w = max(worst_w, float(np.abs(w32 - pose[2]).max()))
        if e > worst:
            worst, at = e, float(f)
    print("%s: float32 restatement vs float64 over %d samples: world %.3e x max(1, |ref|) at frame %r (a quarter of the bar: %.3e), morph weights %.3e"
          % (name, len(samples(name)), worst, at, W_BAR / 4, worst_w))
    assert worst <= W_BAR / 4 and worst_w <= 1e-6


def test_float32_bezier_on_the_extreme_curves():
    """bezier_y in float32 against the float64 solve on the curves whose x(t) is flat at an end and 60 random ones. The solve stops at
    |x(t) - x| < 1e-7, which leaves y off by up to 1e-7 x dy/dx. On the flattest curves x(t) = t^3 and y(t) = 1 - (1 - t)^3 (or their mirror
    images), so dy/dx = ((1 - t) / t)^2 with t = x^(1/3): 13 at x = 1/100, 81 at x = 1/1000. Bars: 1.5e-6 at x = k / 100, 1e-5 at
    x = k / 1000 near both ends — a property of the curve, not of the solver: the float64 solve fed x +- 1e-7 moves as far."""
    rng = np.random.default_rng(1)
    curves = [tuple(v / 127.0 for v in c) for c in ss.EXTREME] + [tuple(rng.integers(0, 128, size=4) / 127.0) for _ in range(60)]
    mid = [k / 100 for k in range(1, 100)]
    ends = [k / 1000 for k in range(1, 10)] + [1 - k / 1000 for k in range(1, 10)]
    worst = {}
    for xs, key in ((mid, "k/100"), (ends, "k/1000")):
        worst[key] = max(abs(float(bezier_reference(np.float32(x), *c, dtype=np.float32)) - bezier_reference(float(np.float32(x)), *(float(np.float32(v)) for v in c)))
                         for c in curves for x in xs)
    print("float32 bezier_y vs float64: %.2e at k/100, %.2e at k/1000 near the ends" % (worst["k/100"], worst["k/1000"]))
    assert worst["k/100"] <= 1.5e-6 and worst["k/1000"] <= 1e-5


def test_default_float64_sampler_is_unchanged():
    """dtype is float64 unless asked: the same objects come back as before the argument existed (bit for bit on a motion with curves)"""
    sc = ss.scene("b48")
    a = sample_reference(sc["clip_b"], 11.5, sc["B"], sc["M"])
    b = sample_reference(sc["clip_b"], 11.5, sc["B"], sc["M"], dtype=np.float64)
    assert all(x.dtype == np.float64 and np.array_equal(x, y) for x, y in zip(a, b))
    assert bezier_reference(0.3, 0.2, 0.8, 0.6, 0.1) == bezier_reference(0.3, 0.2, 0.8, 0.6, 0.1, dtype=np.float64)
    assert isinstance(bezier_reference(0.3, 0.2, 0.8, 0.6, 0.1), float)


@pytest.mark.parametrize("name", ("b48", "b520"))
def test_guess_and_repair_returns_the_reference_spans(name):
    """span_guess + span_bisect in float32 return sample_reference's (i0, i1) for every (track, frame) of the scene, and for 2 000 random
    frames over every track of 700 keys or more (a tenth of them exactly on keys)."""
    sc = ss.scene(name)
    rng = np.random.default_rng(5)
    n = 0
    for clip, frames in ((sc["clip_a"], sc["frames"]), (sc["clip_b"], sc["frames_b"])):
        for kf, b, e in tracks_of(clip):
            fs = list(frames)
            if e - b >= 700:
                lo, hi = float(kf[b]), float(kf[e - 1])
                extra = rng.uniform(lo - 5.0, hi + 5.0, size=2000).astype(np.float32)
                extra[::10] = kf[rng.integers(b, e, size=200)]
                fs += list(extra)
            kf64 = kf.astype(np.float64)
            for f in fs:
                assert span_device_f32(kf, b, e, f) == reference_span(kf64, b, e, float(f)), (b, e, float(f))
                n += 1
    print("%s: %d spans equal" % (name, n))


def scene_stats(sc):
    """span statistics of clip A's tracks 1-8 (sampler_scenes.KINDS) over the scene's frames: {kind: [stats of every sample]}"""
    clip = sc["clip_a"]
    kf = np.asarray(clip["key_frame"], dtype=np.float32)
    out = {}
    for kind in ss.KINDS:
        bone = ss.bone_of(sc, kind)
        t = int(np.flatnonzero(clip["track_bone"] == bone)[0])
        b, e = int(clip["key_off"][t]), int(clip["key_off"][t + 1])
        rows = []
        for f in sc["frames"]:
            st = {}
            i0, _ = span_device_f32(kf, b, e, f, stats=st)
            st.update(i0=i0, b=b, e=e, frame=float(f), unclamped=span_guess_f32(kf, b, e, np.float32(f), clamp=1)[1])
            rows.append(st)
        out[kind] = rows
    return out


@pytest.mark.parametrize("name", ("b48", "b520"))
def test_the_scene_sends_the_search_down_its_repair_path(name):
    sc = ss.scene(name)
    st = scene_stats(sc)
    line = []
    for kind in ("bursts", "runs", "long"):
        inner = [s for s in st[kind] if s["interior"]]
        wrong = [s for s in inner if not s["right"]]
        line.append("%s: %d of %d interior guesses wrong, longest repair %d probes, furthest guess %d keys off"
                    % (kind, len(wrong), len(inner), max(s["steps"] for s in inner), max(abs(s["guess"] - s["i0"]) for s in inner)))
        assert len(inner) >= 8 and 3 * len(wrong) >= len(inner), line[-1]
    print("%s: %s" % (name, "; ".join(line)))
    every = [s for kind in ("bursts", "runs", "long") for s in st[kind] if s["interior"]]
    assert max(s["steps"] for s in every) >= 12                                     # what the guess left holds 4 096 keys or more
    assert max(abs(s["guess"] - s["i0"]) for s in st["long"]) >= 2000               # a guess thousands of keys away
    assert any(s["guess"] < s["i0"] for s in every) and any(s["guess"] > s["i0"] for s in every)       # on each side of the true span
    even = [s for s in st["even"] if s["interior"]]
    assert len(even) >= 10 and all(s["right"] for s in even)                        # evenly spaced keys: the guess is right, nothing is repaired
    # one sample's guess is the last key itself before the clamp pulls it back (frame - first rounds up to last - first)
    assert any(s["interior"] and s["unclamped"] == s["e"] - 1 for s in st["frac"])
    # key indices beyond 65 536 are reached, in clip A itself and — shifted by clip A's keys — in every record of clip B in the library
    assert max(s["i0"] for s in st["long"]) > 65536 or len(sc["clip_a"]["key_frame"]) > 65536
    assert len(sc["clip_a"]["key_frame"]) > 65536 and float(sc["clip_a"]["key_frame"].max()) > 100000.0


def test_the_keys_of_a_track_are_far_apart_and_both_slerp_branches_are_taken():
    """Consecutive keys differ by at least 100 x the world bar in rotation and in position (a neighbouring span cannot pass), stay within
    45 degrees of the bone's base, and the small-step tracks take the slerp's lerp branch (c > 0.9995) while the others take the sine form."""
    for name in ("b48", "b520"):
        sc = ss.scene(name)
        for bone, t in sc["tracks"].items():
            q, p = t["rot"].astype(np.float64), t["pos"].astype(np.float64)
            if len(q) < 2:
                continue
            c = np.abs(np.sum(q[1:] * q[:-1], axis=1))
            step = 2 * np.arccos(np.minimum(c, 1.0))
            assert step.min() >= 100 * W_BAR * 4 and np.linalg.norm(p[1:] - p[:-1], axis=1).min() >= 100 * W_BAR * 4, (name, bone)
            assert (c > 0.9995).all() if t["kind"] in ss.SMALL_STEPS else (c < 0.9995).all(), (name, bone, t["kind"])
            assert np.abs(q @ sc["base"][bone]).min() >= np.cos(np.pi / 8) - 1e-6, (name, bone)
            assert (np.sum(q * sc["base"][bone], axis=1) < 0).any() or len(q) < 8       # some keys are stored negated


@pytest.mark.parametrize("mutant", SPAN_MUTANTS)
def test_a_one_off_error_in_the_span_search_leaves_the_bar(mutant):
    """Each mutant of the restated search puts the float32 restatement outside the GPU bar on at least one scene sample — the GPU comparison
    would catch it. One exception, which no comparison of outputs can catch: `n - 1` for `n - 2` in the clamp of the guess. The guess then
    names the last key; the check that follows compares that key's frame with the sampled frame, which is below it (a frame on or past the
    last key never gets this far), so the repair always runs and returns the right span. What the mutant does is read key `e`, one past its
    track — the next track's, or beyond the clip. The restatement reports that read, and this test asserts it on the sample that makes the
    clamp engage."""
    worst, beyond = 0.0, 0
    for name in ("b48", "b520"):
        sc = ss.scene(name)

        def search(kf, b, e, f):
            st = {}
            out = span_device_f32(kf, b, e, f, stats=st, mutant=mutant)
            search.beyond += bool(st["beyond"])
            return out
        search.beyond = 0
        for clip, f, _pose, world in samples(name):
            e = world_error(sc, clip, f, world, span_fn=search)
            worst = max(worst, e if e == e else np.inf)
        beyond += search.beyond
    print("%s: worst world error %.3e x max(1, |ref|) (bar %.0e), reads beyond a track %d" % (mutant, worst, W_BAR, beyond))
    if mutant == "clamp_n_minus_1":
        assert beyond >= 1 and worst <= W_BAR / 4
    else:
        assert worst > W_BAR and beyond == 0


@needs_node
def test_host_sampler_agrees_with_the_float64_reference_on_the_long_tracks(tmp_path):
    """host/vmd-sampler.js on clip A written as a VMD (its fractional-frame tracks left out: a VMD stores integer frames), sampled at the
    scene's frames: every bone's rotation and position and every morph track's weight within 1e-9 of the float64 reference."""
    import pmx_synth
    sc = ss.scene("b48")
    clip = sc["clip_a_vmd"]
    (tmp_path / "a.vmd").write_bytes(pmx_synth.write_vmd(*ss.to_vmd_keys(sc)))
    frames = [float(f) for f in sc["frames"]]
    (tmp_path / "frames.json").write_text(json.dumps(frames))
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "sampler_long.js"), str(tmp_path / "a.vmd"), str(tmp_path / "frames.json")], timeout=300)
    got = json.loads(out.decode().strip().splitlines()[-1])
    bones = [int(b) for b in clip["track_bone"]]
    n_tracks = len(clip["mkey_off"]) - 1
    assert sorted(got["bones"]) == sorted("b%d" % b for b in bones) and got["keys"] == len(clip["key_frame"]) > 65536
    # the reference samples a model with one bone per track and one vertex morph per morph track, each fed by its own track alone
    flat = dict(clip, feed_off=np.arange(n_tracks + 1, dtype=np.uint32), feed_track=np.arange(n_tracks, dtype=np.int32), feed_ratio=np.ones(n_tracks, dtype=np.float32))
    nb = max(bones) + 1
    worst = 0.0
    for k, f in enumerate(frames):
        q, t, w = sample_reference(flat, f, nb, n_tracks)
        for b in bones:
            s = got["samples"][k]["b%d" % b]
            worst = max(worst, float(np.abs(np.array(s["rotation"]) - q[b]).max()), float(np.abs(np.array(s["position"]) - t[b]).max()))
        for m in range(n_tracks):
            v = got["samples"][k].get("m%d" % m)
            assert (v is None) == (clip["mkey_off"][m + 1] == clip["mkey_off"][m])
            if v is not None:
                worst = max(worst, abs(v - w[m]))
    print("host sampler vs float64 on %d keys at %d frames: %.3e" % (got["keys"], len(frames), worst))
    assert worst <= 1e-9
