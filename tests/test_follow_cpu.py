"""The follow stage without a GPU: known answers of the definition (tests/follow_ref.py), the conditioning of every scene the GPU tests
use (tests/follow_scenes.py), the host twin Model.followOverrides under Node, the Engine option and the Python binding.

The GPU bar for world matrices is 5e-5 x max(1, |ref|) (tests/test_gpu_follow.py). A scene belongs in the GPU tests only when the float32
run of the definition — float32 solve, float32 stage — stays within a QUARTER of that bar of the float64 run: then a device result off the
bar is a wrong result, not an ill-conditioned scene. No scene is left out."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import follow_ref as fr
import follow_scenes as fs
import ik_ref
import physics_scenes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_BAR = 5e-5
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def solved_exact(sc, x):
    """S of the instance's pose with its quaternions made unit in float64: the scenes carry float32 quaternions, unit to 2^-24, whose
    rotations are orthogonal only to that — the known answers below are exact statements about rigid matrices"""
    q = x["q"].astype(np.float64)
    return fs.solved(sc, q / np.linalg.norm(q, axis=1, keepdims=True), x["t"])


# ---- known answers ----

def test_translation_override_moves_followers_by_that_translation():
    sc = fs.scene("a")
    x = sc["instances"][0]
    S = solved_exact(sc, x)
    d = np.array([0.5, -2.0, 3.0])
    O = S[2].copy()
    O[12:15] += d
    W = fr.follow(sc["parents"], S, [2], O[None])
    moved = np.zeros_like(S)
    moved[[2, 3, 4, 5], 12:15] = d            # the overridden bone and its three followers; the root, its child and the sibling branch stay
    assert np.abs(W - (S + moved)).max() < 1e-12


def test_identity_override_changes_nothing():
    """O_a = S_a: W = S on every bone, in float64 to rounding"""
    for name in ("a", "e", "g"):
        sc = fs.scene(name)
        x = sc["instances"][0]
        S = solved_exact(sc, x)
        W = fr.follow(sc["parents"], S, x["bones"], S[x["bones"]])
        assert np.abs(W - S).max() < 1e-12, name


def test_followers_keep_their_pose_relative_to_the_overridden_bone():
    """O_a^-1 W_b = S_a^-1 S_b: rigidly attached, whatever the override"""
    sc = fs.scene("f")
    x = sc["instances"][0]
    S = solved_exact(sc, x)
    W = fr.follow(sc["parents"], S, x["bones"], x["mats"])
    M = lambda w: np.asarray(w, dtype=np.float64).reshape(4, 4).T
    for b, k in fr.followers(sc["parents"], x["bones"]):
        a = int(x["bones"][k])
        assert np.abs(np.linalg.inv(M(W[a])) @ M(W[b]) - np.linalg.inv(M(S[a])) @ M(S[b])).max() < 1e-9


def test_nesting_rule():
    """an override below another override is absolute; bones between the two follow the upper one, bones below the lower one the lower one"""
    sc = fs.scene("b")
    x = sc["instances"][0]
    assert list(x["bones"]) == [1, 3]
    S = fs.solved(sc, x["q"], x["t"])
    W = fr.follow(sc["parents"], S, x["bones"], x["mats"])
    assert fr.followers(sc["parents"], x["bones"]) == [(2, 0), (4, 1), (5, 1)]
    assert np.array_equal(W[0], S[0])
    assert np.abs(W[1] - x["mats"][0]).max() == 0 and np.abs(W[3] - x["mats"][1]).max() == 0
    only_upper = fr.follow(sc["parents"], S, [1], x["mats"][:1])
    only_lower = fr.follow(sc["parents"], S, [3], x["mats"][1:])
    assert np.array_equal(W[2], only_upper[2]) and np.array_equal(W[4:], only_lower[4:])
    assert np.abs(only_upper[4:] - W[4:]).max() > 0.1           # (and the lower override is not the followed pose of the upper one)
    # of two entries for one bone the last wins, as rz_override_world keeps them
    twice = fr.follow(sc["parents"], S, [1, 3, 1], np.concatenate([x["mats"][1:], x["mats"][1:], x["mats"][:1]]))
    assert np.array_equal(twice, W)


def test_every_scene_lays_out_what_it_says():
    """the follower lists are the ones the scenes were laid out for, entry by entry"""
    for name in fs.STATIC:
        sc = fs.scene(name)
        for x, want in zip(sc["instances"], sc["expect"]):
            got = {b: int(x["bones"][k]) for b, k in fr.followers(sc["parents"], x["bones"])}
            assert got == want, name
    counts = {n: [len(e) for e in fs.scene(n)["expect"]] for n in fs.STATIC}
    assert counts["f"] == [557] and counts["e"] == [18] and counts["h"] == [3, 5, 0]
    f = fs.scene("f")["expect"][0]
    assert sorted(f.values()).count(1) == 257 and sorted(f.values()).count(2) == 300          # past one block of 256 lanes, and past two
    g = fs.scene("g")
    assert g["B"] == 520 and sum(b >= 512 for b in g["expect"][0]) == 8
    e = fs.scene("e")
    assert max(ik_ref.Hierarchy(e["parents"], e["bind"], e["instances"][0]["q"]).depth) == 19  # 20 levels: a third doubling round (anc_more)
    d = fs.scene("d")
    assert d["ap"][3] == 1 and 3 in d["expect"][0] and 1 in d["instances"][0]["bones"]
    assert fs.scene("i")["chains"] and fs.scene("i")["chains"][0]["links"][0]["bone"] == 3     # the chain ends above bone 6
    j = fs.scene("j")
    assert j["table"]["n_bodies"] == 21 and len(j["ride"]) == 5
    driven = set(int(b) for b in j["table"]["bone"])
    assert not driven & set(j["ride"])                          # body-less bones


def test_append_follower_is_not_re_appended():
    """(d): bone 3 takes half of bone 1's rotation in S; under the override of bone 1 it keeps that share of the SOLVED rotation"""
    sc = fs.scene("d")
    x = sc["instances"][0]
    S = solved_exact(sc, x)
    W = fr.follow(sc["parents"], S, x["bones"], x["mats"])
    plain = ik_ref.solve(sc["parents"], sc["bind"], x["q"], x["t"])[0]
    assert np.abs(plain[3] - S[3]).max() > 0.01                 # the append transform is at work in S
    M = lambda w: np.asarray(w, dtype=np.float64).reshape(4, 4).T
    assert np.abs(np.linalg.inv(M(W[1])) @ M(W[3]) - np.linalg.inv(M(S[1])) @ M(S[3])).max() < 1e-12


# ---- conditioning ----

def _worst(pairs):
    return max(float(np.abs(a.astype(np.float64) - b).max()) / max(1.0, float(np.abs(b).max())) for a, b in pairs)


@pytest.mark.parametrize("name", list(fs.STATIC))
def test_static_scene_is_well_conditioned(name):
    sc = fs.scene(name)
    pairs = []
    for x in sc["instances"]:
        w64 = fr.follow(sc["parents"], fs.solved(sc, x["q"], x["t"]), x["bones"], x["mats"])
        w32 = fr.follow(sc["parents"], fs.solved(sc, x["q"], x["t"], np.float32), x["bones"], x["mats"], np.float32)
        assert w32.dtype == np.float32
        pairs.append((w32, w64))
    e = _worst(pairs)
    print("(%s) float32 against float64: %.2e x max(1, |ref|) (a quarter of the bar: %.2e)" % (name, e, W_BAR / 4))
    assert e <= W_BAR / 4


@pytest.mark.parametrize("instance", [0, 1, 2])
def test_physics_scene_is_well_conditioned_and_shows_the_defect(instance):
    """(j), every instance of the crowd of 3 (instance 0 is the single character): float32 physics + float32 stage within a quarter of the
    bar of the float64 run after both calls, and the riding bones more than 100 x the bar from where the un-followed seam leaves them"""
    sc = fs.scene("j")
    poses = fs.physics_poses(sc, instance)
    a, b = fs.physics_reference(sc, poses), fs.physics_reference(sc, poses, np.float32)
    pairs, off = [], 0.0
    for (S, bones, O), (S2, bones2, O2) in zip(a, b):
        assert bones == bones2
        w64 = fr.follow(sc["parents"], S, bones, O)
        pairs.append((fr.follow(sc["parents"], S2, bones2, O2, np.float32), w64))
        seam = fr.replaced(S, bones, O)
        off = min(np.abs(w64[r] - seam[r]).max() for r in sc["ride"])
    e = _worst(pairs)
    print("(j) instance %d: float32 against float64 %.2e x max(1, |ref|) (a quarter of the bar: %.2e); riding bones move by at least %.3f" % (instance, e, W_BAR / 4, off))
    assert e <= W_BAR / 4
    assert off > 100 * W_BAR * max(1.0, float(np.abs(pairs[-1][1]).max()))


# ---- the host twin and the bindings ----

@needs_node
def test_host_twin_equals_the_definition(tmp_path):
    """Model.followOverrides (doubles, f32 stores) on every static scene and on (j)'s last call: the definition at float32 rounding"""
    cases, refs = [], []
    for name in fs.STATIC:
        sc = fs.scene(name)
        for x in sc["instances"]:
            S = fs.solved(sc, x["q"], x["t"]).astype(np.float32)
            cases.append(dict(parents=[int(p) for p in sc["parents"]], world=S.reshape(-1).tolist(), bones=[int(b) for b in x["bones"]],
                              mats=x["mats"].reshape(-1).astype(np.float64).tolist()))
            refs.append(fr.follow(sc["parents"], S, x["bones"], x["mats"]))
    sc = fs.scene("j")
    S, bones, O = fs.physics_reference(sc, fs.physics_poses(sc, 0))[-1]
    S, O = S.astype(np.float32), O.astype(np.float32)
    cases.append(dict(parents=[int(p) for p in sc["parents"]], world=S.reshape(-1).tolist(), bones=bones, mats=O.reshape(-1).astype(np.float64).tolist()))
    refs.append(fr.follow(sc["parents"], S, bones, O))
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    out = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "follow_host.js"), str(tmp_path / "cases.json")], timeout=120).decode().strip().splitlines()[-1])
    worst = 0.0
    for got, ref in zip(out, refs):
        got = np.array(got).reshape(-1, 16)
        assert np.array_equal(got, got.astype(np.float32))      # f32 stores
        # one rounding of the stored result: half an ulp of float32, relative to the matrix's largest entry
        worst = max(worst, float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())))
    print("Model.followOverrides against the definition: %.2e x max(1, |ref|)" % worst)
    assert worst <= 2.0 ** -24


@needs_node
def test_engine_option_with_a_recording_addon(tmp_path):
    """Engine { followOverrides } against a stand-in for the addon: overrideFollow(1) right behind the topology upload on every shard, with
    and without devicePhysics, and on a fork before its overrides; no call without the option; it throws without deviceFK"""
    sc = fs.scene("j")
    data, _ = ps.write_pmx(sc)
    (tmp_path / "j.pmx").write_bytes(data)
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "follow_engine_mock.js"), str(tmp_path / "j.pmx"), "follow", "physics", "fork", "off"],
                                           timeout=60).decode().strip().splitlines()[-1])
    assert r["needsDeviceFK"] and r["needsDeviceFKWithPhysicsHook"]
    assert r["shards"] >= 2
    for tag in ("follow", "physics", "fork"):
        assert len(r[tag]) == r["shards"]
        for calls in r[tag]:
            at = calls.index("topology")
            assert calls[at + 1] == "overrideFollow:1" and calls.count("overrideFollow:1") == 1, (tag, calls)
            assert ("uploadPhysics" in calls) == (tag == "physics")
    for calls in r["physics"]:
        assert calls.index("uploadPhysics") > calls.index("overrideFollow:1")
    for calls in r["fork"]:
        at = calls.index("fork")
        assert calls[at + 1:at + 3] == ["overrideFollow:1:fork", "overrideWorld:fork"], calls
    assert all("overrideFollow" not in " ".join(calls) for calls in r["off"]) and all("uploadPhysics" in calls for calls in r["off"])


def test_python_binding_lists_the_symbol(rz):
    capi = rz.capi
    assert hasattr(capi.load(), "rz_override_follow")
    assert "rz_override_follow" in capi.SYMBOLS and "rz_override_follow" in capi.OPTIONAL_SYMBOLS
    assert hasattr(capi.DeformContext, "override_follow")
