"""The motion stores' host half without a GPU: reze-engine_amd/csrc/motion_table.h — what rz_upload_animation and rz_upload_motions check of a
motion and the arrays they upload — through tests/motion_table_main.cpp, built with -fsanitize=address,undefined and run as a program of
its own. What it prints is held to the concatenation restated here in numpy (restate): per clip the [B] track records with absolute key
indices, [M + 1] absolute feed offsets, the concatenated feeds, keys and morph keys, the interpolation bytes with the 20 / 107 default
curve for a clip that has none beside one that has them. Floats are compared as bits. Every refusal is compared as text, once bare (the
single motion) and once as clip 1 of 2 of a library, with rz_upload_motions' prefix."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bone_rec", "feed_off", "feed_range", "feed_ratio", "key_frame", "key_rot", "key_pos", "key_interp", "mkey_frame", "mkey_weight")
NULL = dict(track_bone=1, key_off=2, key_frame=4, key_rot=8, key_pos=16, mkey_off=64, mkey_frame=128, mkey_weight=256, feed_off=512, feed_track=1024,
            feed_ratio=2048)
LINEAR = [20] * 8 + [107] * 8
NAN, INF = float("nan"), float("inf")


def bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


def clip(tracks=(), interp=False, morph_tracks=(), feeds=None, seed=0, null=0):
    """tracks: (bone, key frames); morph_tracks: key frames; feeds: per vertex morph a list of (morph track, ratio), or None = no feed arrays.
    Rotations, positions, weights and interpolation bytes are drawn from `seed`."""
    rng = np.random.default_rng(seed)
    K = sum(len(f) for _, f in tracks)
    Km = sum(len(f) for f in morph_tracks)
    c = dict(track_bone=[b for b, _ in tracks], key_off=np.cumsum([0] + [len(f) for _, f in tracks]).tolist(),
             key_frame=np.array([x for _, f in tracks for x in f], dtype=np.float32), key_rot=rng.normal(size=(K, 4)).astype(np.float32),
             key_pos=rng.normal(size=(K, 3)).astype(np.float32), interp=rng.integers(0, 128, size=(K, 16)).astype(np.uint8) if interp else None,
             mkey_off=np.cumsum([0] + [len(f) for f in morph_tracks]).tolist(), mkey_frame=np.array([x for f in morph_tracks for x in f], dtype=np.float32),
             mkey_weight=rng.random(Km).astype(np.float32), feed_off=None, feed_track=[], feed_ratio=np.zeros(0, dtype=np.float32), null=null)
    if feeds is not None:
        c["feed_off"] = np.cumsum([0] + [len(f) for f in feeds]).tolist()
        c["feed_track"] = [t for f in feeds for t, _ in f]
        c["feed_ratio"] = np.array([r for f in feeds for _, r in f], dtype=np.float32)
    return c


def restate(B, M, clips):
    """the arrays of the clips behind each other, as lists of integers (floats as bits)"""
    any_interp = any(c["interp"] is not None and len(c["track_bone"]) for c in clips)
    out = {k: [] for k in NAMES}
    key_base = mkey_base = feed_base = 0

    def record(off, frames, t, base):
        if t is None or off[t + 1] == off[t]:
            return [0, 0, 0, 0]
        return [base + off[t], base + off[t + 1], int(bits(frames[off[t]])[0]), int(bits(frames[off[t + 1] - 1])[0])]
    for c in clips:
        K, Km = c["key_off"][-1], c["mkey_off"][-1]
        track = {b: t for t, b in enumerate(c["track_bone"]) if 0 <= b < B}
        for b in range(B):
            out["bone_rec"] += record(c["key_off"], c["key_frame"], track.get(b), key_base)
        fed = M and len(c["mkey_off"]) > 1
        off = c["feed_off"] if fed else [0] * (M + 1)
        out["feed_off"] += [feed_base + o for o in off[:M + 1]]
        for f in range(off[M]):
            out["feed_range"] += record(c["mkey_off"], c["mkey_frame"], c["feed_track"][f], mkey_base)
        out["feed_ratio"] += bits(c["feed_ratio"][:off[M]]).tolist()
        out["key_frame"] += bits(c["key_frame"]).tolist()
        out["key_rot"] += bits(c["key_rot"]).tolist()
        out["key_pos"] += bits(c["key_pos"]).tolist()
        if any_interp:
            out["key_interp"] += c["interp"].reshape(-1).tolist() if c["interp"] is not None else LINEAR * K
        out["mkey_frame"] += bits(c["mkey_frame"]).tolist()
        out["mkey_weight"] += bits(c["mkey_weight"]).tolist()
        key_base, mkey_base, feed_base = key_base + K, mkey_base + Km, feed_base + off[M]
    return out


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("motion_table") / "motion_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "motion_table_main.cpp")])
    return exe


def run(tool, B, M, clips, library, limit=0):
    rows = ["%d %d %d %d %d" % (library, B, M, len(clips), limit)]
    ints = lambda v: " ".join("%d" % x for x in v)
    for c in clips:
        rows += ["%d %d %d" % (c["null"], c["interp"] is not None, len(c["track_bone"])), ints(c["track_bone"]), ints(c["key_off"]), ints(bits(c["key_frame"])),
                 ints(bits(c["key_rot"])), ints(bits(c["key_pos"]))]
        if c["interp"] is not None:
            rows.append(ints(c["interp"].reshape(-1)))
        fo = c["feed_off"] or []
        rows += ["%d" % (len(c["mkey_off"]) - 1), ints(c["mkey_off"]), ints(bits(c["mkey_frame"])), ints(bits(c["mkey_weight"])), "%d" % len(fo), ints(fo),
                 "%d" % len(c["feed_track"]), ints(c["feed_track"]), ints(bits(c["feed_ratio"]))]
    p = subprocess.run([tool], input="\n".join(rows) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for ln in p.stdout.strip().split("\n"):
        name, _, rest = ln.partition(" ")
        out[name] = rest if name == "error" else [int(v) for v in rest.split()]
    return out


def agrees(got, want):
    assert "error" not in got, got
    for k in NAMES:
        assert got[k] == want[k], k


def test_one_clip_is_its_own_arrays_from_base_zero(tool):
    """the single motion, and a library of one clip: the same arrays, the clip's own"""
    B, M = 4, 2
    c = clip(tracks=[(2, [0, 5, 9]), (0, [1.5])], interp=True, morph_tracks=[[0, 10], [3]], feeds=[[(0, 1.0), (1, 0.25)], [(1, 1.0)]], seed=1)
    one, lib = run(tool, B, M, [c], 0), run(tool, B, M, [c], 1)
    assert one == lib
    agrees(one, restate(B, M, [c]))
    assert one["key_frame"] == bits(c["key_frame"]).tolist() and one["key_rot"] == bits(c["key_rot"]).tolist() and one["key_pos"] == bits(c["key_pos"]).tolist()
    assert one["key_interp"] == c["interp"].reshape(-1).tolist()
    assert one["mkey_frame"] == bits(c["mkey_frame"]).tolist() and one["mkey_weight"] == bits(c["mkey_weight"]).tolist()
    assert one["feed_off"] == c["feed_off"] and one["feed_ratio"] == bits(c["feed_ratio"]).tolist()
    z = [0, 0, 0, 0]
    f = lambda x: int(bits(x)[0])
    assert one["bone_rec"] == [3, 4, f(1.5), f(1.5)] + z + [0, 3, f(0), f(9)] + z
    assert one["feed_range"] == [0, 2, f(0), f(10)] + [2, 3, f(3), f(3)] * 2


def three_clips():
    """B = 5, M = 3. Clip 0, no interpolation bytes: bone 0 with duplicate key frames, a track for bone 7 (>= B) and one for bone -1 whose keys
    are not finite, bone 2 with a track of no keys, bones 1 3 4 undriven; morph 0 fed by its own track and a group track, morph 1 by nothing,
    morph 2 by its own; a morph track no feed names, with a key that is not finite. Clip 1, with bytes: two tracks, no morph tracks at all.
    Clip 2, no bytes: one key, one morph track feeding morph 1."""
    c0 = clip(tracks=[(0, [0, 4, 4, 4, 11]), (7, [NAN, 1]), (2, []), (-1, [INF])], morph_tracks=[[0, 2, 2], [1], [5, 6], [INF]],
              feeds=[[(0, 1.0), (1, 0.5)], [], [(2, 1.0)]], seed=2)
    c0["key_rot"][5] = NAN
    c0["key_pos"][7] = INF
    c0["mkey_weight"][6] = NAN
    c1 = clip(tracks=[(4, [2, 3, 5, 8]), (1, [0, 30])], interp=True, seed=3)
    c2 = clip(tracks=[(3, [7])], morph_tracks=[[0, 1, 2, 3]], feeds=[[], [(0, 0.75)], []], seed=4)
    return [c0, c1, c2]


@pytest.mark.parametrize("M", [3, 0])
def test_three_clips_are_concatenated_with_absolute_indices(tool, M):
    B, clips = 5, three_clips()
    got, want = run(tool, B, M, clips, 1), restate(B, M, clips)
    agrees(got, want)
    rec = np.array(got["bone_rec"]).reshape(3, B, 4)
    assert not rec[0, [1, 2, 3, 4]].any() and not rec[1, [0, 2, 3]].any() and not rec[2, [0, 1, 2, 4]].any()       # undriven, and the track of no keys
    assert rec[0, 0, :2].tolist() == [0, 5] and rec[1, 4, :2].tolist() == [8, 12] and rec[1, 1, :2].tolist() == [12, 14] and rec[2, 3, :2].tolist() == [14, 15]
    it = np.array(got["key_interp"]).reshape(-1, 16)
    assert it.shape[0] == 15 and (it[:8] == LINEAR).all() and (it[14:] == LINEAR).all() and (it[8:14] == clips[1]["interp"]).all()
    if M:
        assert got["feed_off"] == [0, 2, 2, 3, 3, 3, 3, 3, 3, 3, 4, 4]
        fr = np.array(got["feed_range"]).reshape(-1, 4)
        assert fr[:, :2].tolist() == [[0, 3], [3, 4], [4, 6], [7, 11]]         # own track, group track; clip 2's keys behind clip 0's seven
    else:
        assert got["feed_off"] == [0, 0, 0] and got["feed_range"] == [] and got["feed_ratio"] == []


def test_no_clip_with_interpolation_bytes_gives_none(tool):
    B, M = 5, 3
    clips = three_clips()
    clips[1]["interp"] = None
    got = run(tool, B, M, clips, 1)
    agrees(got, restate(B, M, clips))
    assert got["key_interp"] == []
    # bytes on a clip without bone tracks do not count either
    empty = clip(interp=True)
    assert run(tool, B, M, [clips[0], empty], 1)["key_interp"] == []


def refusals():
    """(what, B, M, clip, the refusal)"""
    ok = dict(tracks=[(0, [0, 1]), (1, [2, 3, 4])], morph_tracks=[[0, 1], [2]], feeds=[[(0, 1.0)], [(1, 1.0), (0, 0.5)]])
    out = []
    out.append(("null bone-track arrays", clip(**ok, null=NULL["key_rot"]), "null bone-track arrays"))
    out.append(("null morph-track arrays", clip(**ok, null=NULL["mkey_weight"]), "null morph-track arrays"))
    out.append(("null feed offsets", clip(**ok, null=NULL["feed_off"]), "null morph feeds"))
    out.append(("null feed tracks", clip(**ok, null=NULL["feed_track"]), "null morph feeds"))
    c = clip(**ok)
    c["key_off"] = [2, 1, 5]
    out.append(("descending key offsets", c, "key offsets must be non-decreasing"))
    c = clip(**ok)
    c["mkey_off"] = [1, 0, 3]
    out.append(("descending morph key offsets", c, "morph key offsets must be non-decreasing"))
    out.append(("two tracks on one bone", clip(**dict(ok, tracks=[(1, [0]), (0, [1]), (1, [2])])), "bone 1 is driven by two tracks"))
    out.append(("descending key frames", clip(**dict(ok, tracks=[(0, [0, 1]), (1, [2, 4, 3])])), "track 1: key frames must not descend"))
    out.append(("descending morph key frames", clip(**dict(ok, morph_tracks=[[1, 0], [2]])), "morph track 0: key frames must not descend"))
    out.append(("a frame that is not a number", clip(**dict(ok, tracks=[(0, [0, 1]), (1, [NAN])])), "track 1 key 0: the frame is not finite"))
    out.append(("an infinite frame", clip(**dict(ok, tracks=[(0, [0, INF]), (1, [2])])), "track 0 key 1: the frame is not finite"))
    c = clip(**ok)
    c["key_rot"][3, 2] = INF
    out.append(("rotation", c, "track 1 key 1: the rotation is not finite"))
    c = clip(**ok)
    c["key_pos"][4, 0] = NAN
    out.append(("position", c, "track 1 key 2: the position is not finite"))
    out.append(("morph frame", clip(**dict(ok, morph_tracks=[[0, 1], [NAN]])), "morph track 1 key 0: the frame is not finite"))
    c = clip(**ok)
    c["mkey_weight"][1] = -INF
    out.append(("morph weight", c, "morph track 0 key 1: the weight is not finite"))
    out.append(("a feed past the last track", clip(**dict(ok, feeds=[[(0, 1.0)], [(2, 1.0)]])), "feed 1 names morph track 2 of 2"))
    out.append(("a negative feed track", clip(**dict(ok, feeds=[[(-1, 1.0)], []])), "feed 0 names morph track -1 of 2"))
    c = clip(**ok)
    c["feed_off"] = [0, 3, 2]
    c["feed_track"], c["feed_ratio"] = c["feed_track"][:2], c["feed_ratio"][:2]
    out.append(("descending feed offsets", c, "feed offsets must be non-decreasing"))
    return out


@pytest.mark.parametrize("what,bad,text", refusals(), ids=[r[0].replace(" ", "_") for r in refusals()])
def test_refusal_bare_and_as_a_clip_of_a_library(tool, what, bad, text):
    B, M = 2, 2
    good = clip(tracks=[(1, [0, 9])], seed=9)
    assert run(tool, B, M, [bad], 0) == {"error": text}
    assert run(tool, B, M, [good, bad], 1) == {"error": "rz_upload_motions: clip 1: " + text}


def test_a_skeleton_of_no_bones_is_refused(tool):
    assert run(tool, 0, 0, [clip()], 0) == {"error": "upload the skeleton before a motion"}
    assert run(tool, 0, 0, [clip()], 1) == {"error": "rz_upload_motions: clip 0: upload the skeleton before a motion"}


def test_indices_past_the_limit_are_refused(tool):
    """the 32-bit index guard, reached with a small limit: keys, morph keys and feeds each, and the limit itself still fits"""
    B, M = 2, 1
    a = clip(tracks=[(0, [0, 1, 2])], morph_tracks=[[0, 1]], feeds=[[(0, 1.0)]], seed=5)
    text = {"error": "rz_upload_motions: the library's keys do not fit 32-bit indices"}
    agrees(run(tool, B, M, [a, a], 1, limit=6), restate(B, M, [a, a]))
    assert run(tool, B, M, [a, a], 1, limit=5) == text                                     # 6 keys
    few = clip(tracks=[(0, [0])], morph_tracks=[[0, 1]], feeds=[[(0, 1.0)]], seed=6)
    agrees(run(tool, B, M, [few, few], 1, limit=4), restate(B, M, [few, few]))
    assert run(tool, B, M, [few, few], 1, limit=3) == text                                 # 4 morph keys
    fed = clip(tracks=[(0, [0])], morph_tracks=[[0]], feeds=[[(0, 1.0), (0, 0.5), (0, 0.25)]], seed=7)
    agrees(run(tool, B, M, [fed, fed], 1, limit=6), restate(B, M, [fed, fed]))
    assert run(tool, B, M, [fed, fed], 1, limit=5) == text                                 # 6 feeds
    assert run(tool, B, M, [a], 0, limit=2) == {"error": "the library's keys do not fit 32-bit indices"}
