"""The after-physics stage without a GPU: known answers of the definition (tests/after_ref.py), the conditioning of every scene the GPU
tests use (tests/after_scenes.py) and that every one of them moves, the host half of rz_upload_after_physics
(reze-engine_amd/csrc/after_table.h, through tests/after_table_main.cpp built with -fsanitize=address,undefined) against the level
arithmetic restated in Python, the loader on a small synthetic PMX, the host twin Model.solveAfterPhysics under Node, the Engine option
and the Python binding.

The GPU bar for world matrices is 5e-5 x max(1, |ref|) (tests/test_gpu_after.py). A scene belongs in the GPU tests only when the float32
run of the definition — float32 solve, float32 stage — stays within a QUARTER of that bar of the float64 run: then a device result off the
bar is a wrong result, not an ill-conditioned scene. No scene is left out."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import after_ref as ar
import after_scenes as asc
import ik_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_BAR = 5e-5
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def _err(a, b):
    return float(np.abs(a.astype(np.float64) - b).max()) / max(1.0, float(np.abs(b).max()))


# ---- known answers ----

def test_quat_of_takes_every_branch_and_inverts_the_matrix():
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        R = ik_ref._qmat(q, np.float64)
        d = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]
        seen.add(int(np.argmax(d)))
        p = ar.quat_of(R, np.float64)
        assert abs(abs(p.dot(q)) - 1.0) < 1e-12
    assert seen == {0, 1, 2, 3}


def test_an_unmoved_override_changes_nothing_unless_the_append_parent_appends():
    """overrides that repeat the solved matrices: the stage re-derives what the first solve had (float64: to rounding) — except on (e)'s bone
    6 and (d)'s bone 1 (with bone 6 below it), whose append parents take append themselves: the stage sees their FULL local rotation,
    the first solve only their pose quaternions"""
    for name, differs in (("a", []), ("b", []), ("d", [1, 6]), ("g", []), ("e", [6])):
        sc = asc.scene(name)
        x = sc["instances"][-1]
        q = x["q"].astype(np.float64)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        S = ik_ref.solve(sc["parents"], sc["bind"], q, x["t"], (), sc["ap"], sc["ratio"], sc["move"])[0]
        keep = [b for b in x["bones"] if b not in sc["order"]]
        W = ar.solve(sc["parents"], sc["bind"], q, x["t"], sc["ap"], sc["ratio"], sc["move"], S, keep, sc["order"])
        for b in range(sc["B"]):
            d = float(np.abs(W[b] - S[b]).max())
            assert (d > 1e-3) if b in differs else (d < 1e-12), (name, b, d)


def test_an_overridden_listed_bone_keeps_its_override():
    sc = asc.scene("e")
    x = sc["instances"][1]
    assert 5 in x["bones"] and 5 in sc["order"]
    W = asc.reference(sc, x)
    assert np.array_equal(W[5], x["mats"][list(x["bones"]).index(5)].astype(np.float64))
    assert np.abs(W[6] - asc.frame_without(sc, x)[6]).max() > 0.01          # the bone below it is evaluated on the override


def test_a_listed_bone_below_an_override_is_the_override_times_its_local():
    sc = asc.scene("c")
    x = sc["instances"][0]
    W = asc.reference(sc, x)
    M = lambda w: np.asarray(w, dtype=np.float64).reshape(4, 4).T
    L = np.eye(4)
    L[:3, :3] = ik_ref._qmat(x["q"][2].astype(np.float64), np.float64)
    L[:3, 3] = sc["bind"][2].astype(np.float64) + x["t"][2]
    assert np.abs(M(W[2]) - M(x["mats"][0]) @ L).max() < 1e-12
    assert np.array_equal(W[4], asc.frame_without(sc, x)[4])               # a bone elsewhere keeps its matrix


def test_scenes_are_what_their_names_say():
    assert [len(asc.scene(n)["order"]) for n in ("f1", "f2", "f3")] == [322, 320, 642]
    for n, sizes in (("f1", [257, 65]), ("f2", [256, 64]), ("f3", [300, 300, 42])):
        sc = asc.scene(n)
        off = ar.sorted_entries(sc["parents"], sc["ap"], sc["ratio"], sc["order"])[1]
        assert list(np.diff(off)) == sizes
    f4 = asc.scene("f4")
    assert max(ar.levels(f4["parents"], f4["ap"], f4["ratio"], f4["order"])) == 19
    f5 = asc.scene("f5")
    assert f5["B"] == 600 and min(f5["order"]) >= 590
    d = asc.scene("d")
    assert list(d["order"]) == [4, 5, 1, 6] and ar.levels(d["parents"], d["ap"], d["ratio"], d["order"]) == [0, 1, 1, 2]
    b = asc.scene("b")
    assert [float(b["ratio"][k]) for k in b["order"]] == pytest.approx([-1.0, 0.3, 1.7]) and all(b["move"][k] for k in b["order"])
    g = asc.scene("g")
    assert g["parents"][1] < 0 and g["parents"][g["ap"][1]] < 0
    e = asc.scene("e")
    assert [len(x["bones"]) for x in e["instances"]] == [0, 2, 2]
    i = asc.scene("i")
    assert i["ap"][9] == i["chains"][0]["links"][0]["bone"] and i["parents"][i["ap"][10]] == 3
    j = asc.scene("j")
    driven = set(int(b) for b in j["table"]["bone"])
    assert not driven & set(int(b) for b in j["order"]) and all(int(j["ap"][b]) in driven for b in j["order"][:3])


# ---- conditioning, and every scene moves ----

def _final_append_angles(sc, x, W):
    """the rotation angle of every append parent's final local rotation, in degrees"""
    out = []
    M = lambda w: np.asarray(w, dtype=np.float64).reshape(4, 4).T[:3, :3]
    for b in sc["order"]:
        a = ar.effective_append(sc["ap"], sc["ratio"], int(b))
        if a < 0:
            continue
        R = M(W[a]) if sc["parents"][a] < 0 else M(W[sc["parents"][a]]).T @ M(W[a])
        out.append(float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))))
    return out


@pytest.mark.parametrize("name", list(asc.STATIC))
def test_static_scene_is_well_conditioned_and_moves(name):
    sc = asc.scene(name)
    worst, moved, angle = 0.0, 0.0, 0.0
    for x in sc["instances"]:
        w64 = asc.reference(sc, x)
        w32 = asc.reference(sc, x, dtype=np.float32)
        assert w32.dtype == np.float32
        worst = max(worst, _err(w32, w64))
        moved = max(moved, float(np.abs(w64 - asc.frame_without(sc, x))[sc["order"]].max()))
        angle = max([angle] + _final_append_angles(sc, x, w64))
    print("(%s) float32 against float64: %.2e x max(1, |ref|) (a quarter of the bar: %.2e); listed bones move by %.3f; append parents turn by at most %.0f degrees"
          % (name, worst, W_BAR / 4, moved, angle))
    assert worst <= W_BAR / 4
    assert moved > 0.1
    assert angle <= 165.0


@pytest.mark.parametrize("kind", asc.SOURCES)
def test_pose_source_case_is_well_conditioned_and_moves(kind):
    sc, _, x = asc.source_case(kind)
    w64, w32 = asc.reference(sc, x), asc.reference(sc, x, dtype=np.float32)
    moved = float(np.abs(w64 - asc.frame_without(sc, x))[sc["order"]].max())
    print("(h %s) float32 against float64: %.2e (a quarter of the bar: %.2e); listed bones move by %.3f" % (kind, _err(w32, w64), W_BAR / 4, moved))
    assert _err(w32, w64) <= W_BAR / 4 and moved > 0.1
    assert max(_final_append_angles(sc, x, w64)) <= 165.0


@pytest.mark.parametrize("instance", [0, 1, 2])
def test_physics_scene_is_well_conditioned_and_moves(instance):
    sc = asc.scene("j")
    pose = asc.physics_pose(sc, instance)
    F, W, bones = asc.physics_reference(sc, pose)
    _, W32, bones32 = asc.physics_reference(sc, pose, np.float32)
    assert bones == bones32
    moved = float(np.abs(W - F)[sc["order"]].max())
    print("(j) instance %d: float32 against float64 %.2e (a quarter of the bar: %.2e); listed bones move by %.3f" % (instance, _err(W32, W), W_BAR / 4, moved))
    assert _err(W32, W) <= W_BAR / 4 and moved > 0.1
    assert max(_final_append_angles(sc, dict(), W)) <= 165.0


# ---- the host half (tests/after_table_main.cpp around reze-engine_amd/csrc/after_table.h) ----

@pytest.fixture(scope="module")
def table_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("after_table") / "after_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "after_table_main.cpp")])
    return exe


def run_table_tool(tool, sc, order):
    B = sc["B"]
    rows = ["%d" % B]
    for b in range(B):
        rows.append("%d %d %r %d %r %r %r" % (sc["parents"][b], sc["ap"][b], float(sc["ratio"][b]), int(sc["move"][b]), float(sc["bind"][b][0]), float(sc["bind"][b][1]),
                                              float(sc["bind"][b][2])))
    rows.append("%d" % len(order))
    rows.append(" ".join("%d" % b for b in order))
    out = subprocess.run([tool], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True).stdout
    return {ln.split(" ", 1)[0]: (ln.split(" ", 1)[1] if " " in ln else "") for ln in out.strip().split("\n")}


@pytest.mark.parametrize("name", list(asc.STATIC) + ["j"])
def test_host_table_equals_the_restated_levels(table_tool, name):
    sc = asc.scene(name)
    rows = run_table_tool(table_tool, sc, sc["order"])
    assert "error" not in rows, rows
    lv = ar.levels(sc["parents"], sc["ap"], sc["ratio"], sc["order"])
    bones, off = ar.sorted_entries(sc["parents"], sc["ap"], sc["ratio"], sc["order"])
    assert [int(v) for v in rows["level"].split()] == lv
    assert [int(v) for v in rows["level_off"].split()] == off
    assert [int(v) for v in rows["sorted"].split()] == bones
    index = [int(v) for v in rows["index"].split()]
    assert index == [bones.index(b) if b in bones else -1 for b in range(sc["B"])]
    rec = np.array([int(v) for v in rows["rec"].split()], dtype=np.uint32).reshape(-1, 12)
    for k, b in enumerate(bones):
        a = ar.effective_append(sc["ap"], sc["ratio"], b)
        assert rec[k, 0].view(np.int32) == sc["parents"][b] and rec[k, 1].view(np.int32) == a and rec[k, 7] == b
        assert rec[k, 2:3].view(np.float32)[0] == np.float32(sc["ratio"][b]) and (rec[k, 3] & 1) == int(sc["move"][b])
        assert np.array_equal(rec[k, 4:7].view(np.float32), sc["bind"][b].astype(np.float32))
        if a >= 0:
            assert np.array_equal(rec[k, 8:11].view(np.float32), sc["bind"][a].astype(np.float32)) and rec[k, 11].view(np.int32) == sc["parents"][a]
        else:
            assert rec[k, 11].view(np.int32) == -1
    assert int(rows["lds"]) == 48 * sc["B"] + (len(bones) + 15) // 16 * 16


def test_host_table_refusals(table_tool):
    d = asc.scene("d")
    cases = [([4, 7], "bone 7 of 7"), ([4, 5, 4], "bone 4 is listed twice"), ([5, 4], "bone 5 (entry 0) is evaluated before its parent, bone 4"),
             ([1, 4], "bone 1 (entry 0) is evaluated before its append parent, bone 4")]
    for order, words in cases:
        rows = run_table_tool(table_tool, d, order)
        assert words in rows["error"], rows
        with pytest.raises(ValueError):
            ar.levels(d["parents"], d["ap"], d["ratio"], order)
    a = asc.scene("a")
    rows = run_table_tool(table_tool, a, [5, 2])
    assert "bone 5 (entry 0) is evaluated before its append parent's parent, bone 2" in rows["error"]
    with pytest.raises(ValueError):
        ar.levels(a["parents"], a["ap"], a["ratio"], [5, 2])
    # an append ratio of 0 leaves no append in effect: the append parent may come later
    z = dict(a, ratio=np.array([1, 1, 1, 1, 1, 0.0], dtype=np.float32))
    rows = run_table_tool(table_tool, z, [5, 3])
    assert "error" not in rows and [int(v) for v in rows["level"].split()] == [0, 0] == ar.levels(z["parents"], z["ap"], z["ratio"], [5, 3])


def test_python_binding_lists_the_symbol(rz):
    capi = rz.capi
    assert hasattr(capi.load(), "rz_upload_after_physics")
    assert "rz_upload_after_physics" in capi.SYMBOLS and "rz_upload_after_physics" in capi.OPTIONAL_SYMBOLS
    assert hasattr(capi.DeformContext, "upload_after_physics")


# ---- the loader, the host twin and the Engine option ----

def _node(script, *args, timeout=120):
    return json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", script)] + [str(a) for a in args], timeout=timeout).decode().strip().splitlines()[-1])


def _case(sc, x=None, order=None, levels=None):
    c = dict(parents=[int(p) for p in sc["parents"]], bind=sc["bind"].astype(np.float64).reshape(-1).tolist(), ap=[int(a) for a in sc["ap"]],
             ratio=[float(r) for r in sc["ratio"]], move=[int(m) for m in sc["move"]], flagged=[int(b) for b in (sc["order"] if order is None else order)],
             levels={str(k): v for k, v in (asc.transform_levels(sc) if levels is None else levels).items()})
    if x is not None:
        F = asc.frame_without(sc, x).astype(np.float32)
        c.update(q=np.asarray(x["q"], dtype=np.float32).reshape(-1).tolist(), t=np.asarray(x["t"], dtype=np.float32).reshape(-1).tolist(), world=F.reshape(-1).tolist(),
                 overridden=[int(b) for b in x["bones"]])
    return c


@needs_node
def test_host_twin_equals_the_definition(tmp_path):
    """Model.solveAfterPhysics (doubles, f32 stores) on every static scene: the definition on the float32 frame, within the roundings of the
    stores — every listed bone is stored once in float32 (half an ulp, 2^-24 relative to the matrix's largest entry) and later levels read
    the stored matrices, so an entry `levels` deep carries at most `levels` such roundings, each taken through products of rotations
    (entries <= 1: three terms per entry of the product, a factor of 4 covers them)"""
    cases, refs, bars = [], [], []
    for name in asc.STATIC:
        sc = asc.scene(name)
        lv = max(ar.levels(sc["parents"], sc["ap"], sc["ratio"], sc["order"])) + 1
        for x in sc["instances"]:
            c = _case(sc, x)
            cases.append(c)
            F = np.array(c["world"], dtype=np.float32).reshape(-1, 16)
            refs.append(ar.solve(sc["parents"], sc["bind"], np.asarray(x["q"], dtype=np.float32), np.asarray(x["t"], dtype=np.float32), sc["ap"], sc["ratio"], sc["move"], F,
                                 x["bones"], sc["order"]))
            bars.append(4 * lv * 2.0 ** -24)
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    out = _node("after_host.js", tmp_path / "cases.json")
    worst = 0.0
    for got, ref, bar, c in zip(out, refs, bars, cases):
        assert "error" not in got, got
        assert got["order"] == c["flagged"]
        w = np.array(got["world"]).reshape(-1, 16)
        assert np.array_equal(w, w.astype(np.float32))          # f32 stores
        e = float(np.abs(w - ref).max()) / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, e / bar)
        assert e <= bar, (e, bar)
    print("Model.solveAfterPhysics against the definition: at most %.2f of the rounding bar" % worst)


@needs_node
def test_host_order_and_its_refusal(tmp_path):
    d = asc.scene("d")
    ok = _case(d)                                               # levels 0 0 1 1 by transform level: [4, 5, 1, 6]
    flat = _case(d, levels={})                                  # every level 0: index order [1, 4, 5, 6] lists bone 1 before its append parent 4
    (tmp_path / "cases.json").write_text(json.dumps([ok, flat]))
    out = _node("after_host.js", tmp_path / "cases.json")
    assert out[0] == {"order": [4, 5, 1, 6]}
    assert "bone 1 (b1)" in out[1]["error"] and "append parent, bone 4 (b4)" in out[1]["error"]


@needs_node
def test_loader_and_engine_option_with_a_recording_addon(tmp_path):
    """the loader on a synthetic PMX with flag 0x1000 and transform levels 0 / 1 / 2: the two fields only where set; afterPhysicsOrder();
    Engine { afterPhysics } uploads the order behind the topology on every shard, behind uploadIK when both are on, never without the
    option; a fork gets no call of its own; the option throws without deviceFK, pointing at Model.solveAfterPhysics"""
    sc = asc.scene("i")
    levels = {9: 1, 10: 0, 5: 2}                                 # bone 5 (the IK goal) carries a level without the flag
    data, _ = asc.write_pmx(sc, levels=levels)
    (tmp_path / "i.pmx").write_bytes(data)
    r = _node("after_engine_mock.js", tmp_path / "i.pmx", "after", "ik", "fork", "off", timeout=60)
    want = [dict(after=True if b in (9, 10) else None, level=levels.get(b) or None) for b in range(sc["B"])]        # (a level of 0 is not kept)
    assert r["fields"] == want
    assert r["order"] == [10, 9]
    assert r["needsDeviceFK"]
    for tag in ("after", "ik", "fork"):
        assert len(r[tag]) == r["shards"] >= 2
        for calls in r[tag]:
            ups = [c for c in calls if c.startswith("uploadAfterPhysics")]
            assert ups == ["uploadAfterPhysics:10,9"], (tag, calls)
            at = calls.index("topology")
            if tag == "ik":
                assert calls[at + 1:at + 3] == ["uploadIK", "uploadAfterPhysics:10,9"], calls
            else:
                assert calls[at + 1] == "uploadAfterPhysics:10,9" and "uploadIK" not in calls, calls
    assert all("fork" in calls for calls in r["fork"])
    assert all("uploadAfterPhysics" not in " ".join(calls) for calls in r["off"])
    # a parent listed later throws out of loadModel with the bone's name
    c = asc.scene("c")
    data, _ = asc.write_pmx(c, levels={2: 1})                   # bone 3 (level 0) is now ahead of its parent 2
    (tmp_path / "c.pmx").write_bytes(data)
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "after_engine_mock.js"), str(tmp_path / "c.pmx")], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "bone 3 (bone3) is evaluated before its parent, bone 2 (bone2)" in p.stderr
