"""CPU checks of the per-chain IK switches (VMD IK on / off keys): the definition tests/ik_switch_ref.py on the scenes and key tracks of
tests/ik_switch_scenes.py — not vacuous, well conditioned, flatten / state_at / choose at their edges —, the VMD loader's show / IK block,
the host twins (Model.solveIK with switches, VMDSampler.ikStateAt, applyBlendedFrame's choice), the engine's { ikKeys } option over a
recording stand-in for the addon, and the ABI. Every test prints its figures before it asserts."""
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ik_ref
import ik_switch_ref as sw
import ik_switch_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
BAR, ILL = 1e-4, 2.5e-5


def test_restatement_is_not_vacuous(rz):
    """for every scene, every chain some instance has switched off: with the switch off its effector ends more than 100 x the bar from
    where the full solve puts it (in at least one of the scene's poses), and a chain that stays on is still solved"""
    for name in sc.SCENES:
        s = sc.scene(name)
        sk, ext = s["sk"], s["sk"]["extent"]
        least = np.inf
        full_of = [ik_ref.solve(sk["parents"], sk["bind"], q, t, s["chains"])[0] for q, t in s["poses"]]
        for i in sorted({s["masks"][i].tobytes(): i for i in range(s["I"])}.values()):          # every distinct mask once
            mask = s["masks"][i]
            if mask.all():
                continue
            moved = np.zeros(len(s["chains"]))
            for p in range(len(s["poses"])):
                full = full_of[p]
                part = sc.reference(name, p, i)
                for k, ch in enumerate(s["chains"]):
                    if not mask[k]:
                        moved[k] = max(moved[k], float(np.abs(full[ch["effector"]] - part[ch["effector"]]).max()) / ext)
            least = min(least, float(moved[mask == 0].min()))
        print("%s: every switched-off chain's effector moves by at least %.3f x extent (bar %.0e)" % (name, least, BAR))
        assert least > 100 * BAR, name
    # all off = the plain hierarchy, bit for bit in the definition; a chain that is off leaves its links' rotations alone
    s = sc.scene("leg rig, crowd of 3")
    q, t = s["poses"][0]
    from helpers import fk_reference
    w, qs = sw.solve(s["sk"]["parents"], s["sk"]["bind"], q, t, s["chains"], [0, 0, 0, 0])
    assert np.array_equal(qs, q.astype(np.float64)) and np.abs(w - fk_reference(s["sk"]["parents"], s["sk"]["bind"], q, t).reshape(-1, 16)).max() < 1e-12
    w, qs = sw.solve(s["sk"]["parents"], s["sk"]["bind"], q, t, s["chains"], [1, 0, 0, 1])
    for k, on in enumerate([1, 0, 0, 1]):
        for ln in s["chains"][k]["links"]:
            # (the left ankle is the toe chain's link and below the leg chain: only its own chain turns it)
            assert np.array_equal(qs[ln["bone"]], q[ln["bone"]].astype(np.float64)) == (not on), (k, ln["bone"])


def test_device_test_poses_are_well_conditioned(rz):
    """every (scene, instance mask, pose) tests/test_gpu_ik_switch.py holds the kernel to: the definition's float32 run stays within
    2.5e-5 x extent of its float64 run, so the device tests leave out none"""
    for name in sc.SCENES:
        s = sc.scene(name)
        worst, out, n = 0.0, 0, 0
        for batch in sc.batches(s):
            for i, p in enumerate(batch):
                e = float(np.abs(sc.reference(name, p, i, np.float32).astype(np.float64) - sc.reference(name, p, i)).max()) / s["sk"]["extent"]
                worst, out, n = max(worst, e), out + (e > ILL), n + 1
        print("%s: float32 vs float64 definition over %d poses: worst %.2e x extent, %d beyond %.1e" % (name, n, worst, out, ILL))
        assert out <= 0.02 * n, name


def _flat(track):
    return sw.flatten(sc.tracks()[track][0], sc.rig_chain_names())


def test_flatten_and_state_at_on_the_track_cases(rz):
    L, TL, R, TR = range(4)
    kf, ke = _flat("eight keys")
    assert kf.dtype == np.float32 and list(kf) == [5, 10, 20, 20, 20, 30, 100001, 100003] and ke.shape == (8, 4)
    # sorted stably; a chain a key does not name keeps its state; on before any key names it; the unknown name is ignored
    assert ke.tolist() == [[0, 1, 1, 1], [1, 1, 0, 1], [1, 0, 0, 1], [1, 1, 0, 0], [0, 1, 1, 1], [0, 1, 0, 1], [0, 0, 0, 0], [1, 1, 1, 1]]
    at = lambda f: sw.state_at(kf, ke, f).tolist()
    assert at(-3.0) == [0, 1, 1, 1] and at(np.nextafter(np.float32(5), np.float32(-np.inf))) == [0, 1, 1, 1]       # before the first key: its row
    assert at(5.0) == [0, 1, 1, 1] and at(7.5) == [0, 1, 1, 1] and at(10.0) == [1, 1, 0, 1] and at(15.0) == [1, 1, 0, 1]
    assert at(np.nextafter(np.float32(20), np.float32(-np.inf))) == [1, 1, 0, 1]
    assert at(20.0) == [0, 1, 1, 1] and at(np.nextafter(np.float32(20), np.float32(np.inf))) == [0, 1, 1, 1]         # three keys on one frame: the last wins
    assert at(25.0) == [0, 1, 1, 1] and at(30.0) == [0, 1, 0, 1] and at(50000.0) == [0, 1, 0, 1]
    assert at(np.nextafter(np.float32(100001), np.float32(-np.inf))) == [0, 1, 0, 1] and at(100001.0) == [0, 0, 0, 0]
    assert at(100002.0) == [0, 0, 0, 0] and at(100003.0) == [1, 1, 1, 1] and at(1e6) == [1, 1, 1, 1]
    # compared as float32 values: a float64 frame a hair below the key rounds onto it
    assert at(20.0 - 1e-9) == [0, 1, 1, 1]
    kf1, ke1 = _flat("one key")
    assert list(kf1) == [12] and all(sw.state_at(kf1, ke1, f).tolist() == [1, 0, 0, 0] for f in sc.tracks()["one key"][1])
    kf0, ke0 = _flat("no keys")
    assert kf0.size == 0 and ke0.shape == (0, 4) and sw.state_at(kf0, ke0, 3.0).tolist() == [1, 1, 1, 1]
    kf3, ke3 = _flat("300 keys")
    assert kf3.size == 300 and (np.diff(kf3) >= 0).all() and (np.diff(kf3) == 0).any()
    # against a slow restatement of the rule on the file-order keys: replay every key with frame <= f in (frame, file order)
    keys = sc.tracks()["300 keys"][0]
    names = sc.rig_chain_names()
    srt = sorted(keys, key=lambda k: k[0])
    for f in sc.tracks()["300 keys"][1]:
        upto = [k for k, (fr, _) in enumerate(srt) if np.float32(fr) <= np.float32(f)]
        st = [1, 1, 1, 1]
        for fr, lst in srt[:(upto[-1] if upto else 0) + 1]:
            for n, e in lst:
                st[names.index(n)] = int(e)
        assert sw.state_at(kf3, ke3, f).tolist() == st, f
    rows = {tuple(sw.state_at(kf3, ke3, f)) for f in sc.tracks()["300 keys"][1]}
    print("300 keys: %d distinct rows over %d frames asked" % (len(rows), len(sc.tracks()["300 keys"][1])))
    assert len(rows) >= 4


def test_choose(rz):
    a, b = _flat("eight keys"), _flat("one key")
    sets = {0: a, 1: b, 2: None}
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    ch = lambda st: sw.choose(st, sets, 4).tolist()
    assert ch((0, 10.0, 1, 12.0, 0.0)) == [1, 1, 0, 1] and ch((0, 10.0, 1, 12.0, below)) == [1, 1, 0, 1]
    assert ch((0, 10.0, 1, 12.0, 0.5)) == [1, 0, 0, 0] and ch((0, 10.0, 1, 12.0, 1.0)) == [1, 0, 0, 0]          # it flips at 0.5
    assert ch((0, 10.0, sw.NO_CLIP, 12.0, 1.0)) == [1, 1, 0, 1]                                                   # no second clip: A whatever the blend
    assert ch((0, 10.0, 2, 3.0, 0.75)) == [1, 1, 1, 1] and ch((2, 10.0, 0, 30.0, 0.25)) == [1, 1, 1, 1]           # a chosen clip without keys: all on
    assert ch((2, 10.0, 0, 30.0, 0.5)) == [0, 1, 0, 1]


def test_abi_8_still_and_the_three_symbols_are_exported(rz):
    header = open(os.path.join(ROOT, "include", "reze_deform.h")).read()
    assert int(re.search(r"#define RZ_ABI_VERSION (\d+)", header).group(1)) == 8
    for decl in (r"int rz_set_ik_enabled\(rz_ctx \*ctx, const uint8_t \*enabled\);", r"int rz_upload_ik_keys\(rz_ctx \*ctx, uint32_t clip, const rz_ik_keys \*keys\);",
                 r"int rz_read_ik_enabled\(rz_ctx \*ctx, uint8_t \*out\);"):
        assert re.search(decl, header), decl
    L = rz.capi.load()
    assert L.rz_abi_version() == 8
    for name in ("rz_set_ik_enabled", "rz_upload_ik_keys", "rz_read_ik_enabled"):
        assert hasattr(L, name) and name in rz.capi.SYMBOLS and name in rz.capi.OPTIONAL_SYMBOLS, name
    for name in ("upload_ik_keys", "set_ik_enabled", "read_ik_enabled"):
        assert hasattr(rz.DeformContext, name), name
    assert L.rz_set_ik_enabled(None, None) < 0 and L.rz_last_error()
    assert L.rz_upload_ik_keys(None, 0, None) < 0 and L.rz_read_ik_enabled(None, None) < 0


# ---- the VMD loader ----

def write_vmd_with_ik(bone_keys, morph_keys, ik_keys, cameras=2, lights=1, shadows=1, stop=None):
    """pmx_synth.write_vmd's bone and morph blocks, then `cameras` camera records of 61 bytes, `lights` of 28, `shadows` of 9 and the show /
    IK block: per key u32 frame, u8 show, u32 n, n x (20-byte Shift-JIS name, u8 enabled). Returns (bytes, offsets of every block
    boundary, offsets inside a record of every block)."""
    from pmx_synth import write_vmd
    out = bytearray(write_vmd(bone_keys, morph_keys))
    bounds, inside = [len(out)], []
    rng = np.random.default_rng(5)
    for n, size in ((cameras, 61), (lights, 28), (shadows, 9)):
        out += struct.pack("<I", n)
        inside.append(len(out) + size // 2)
        out += bytes(rng.integers(0, 256, size=n * size).astype(np.uint8))
        bounds.append(len(out))
    out += struct.pack("<I", len(ik_keys))
    for frame, show, lst in ik_keys:
        out += struct.pack("<IBI", frame, 1 if show else 0, len(lst))
        if lst:
            inside.append(len(out) + 7)
        for name, en in lst:
            b = name.encode("shift-jis")
            out += b + b"\0" * (20 - len(b)) + bytes([1 if en else 0])
    bounds.append(len(out))
    return bytes(out), bounds, inside


def node_host(tmp_path, inp, tag):
    fi, fo = tmp_path / (tag + "_in.json"), tmp_path / (tag + "_out.json")
    fi.write_text(json.dumps(inp))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "js", "ik_switch_host.js"), str(fi), str(fo)], timeout=300)
    return json.loads(fo.read_text())


BONE_KEYS = [("センター", 0, (0.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0)), ("左足ＩＫ", 0, (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.5)),
             ("センター", 12, (0.0, 0.38268343, 0.0, 0.92387953), (0.5, 0.0, 0.0)), ("左足ＩＫ", 30, (0.0, 0.0, 0.0, 1.0), (0.0, 2.0, 0.0))]
MORPH_KEYS = [("あ", 0, 0.0), ("あ", 10, 1.0), ("まばたき", 5, 0.5)]
IK_KEYS = [(30, True, [("右足ＩＫ", False), ("右つま先ＩＫ", False)]), (0, True, [("左足ＩＫ", True), ("右足ＩＫ", True), ("左つま先ＩＫ", False), ("右つま先ＩＫ", True)]),
           (30, False, [("右足ＩＫ", True)]), (45, True, [])]


@needs_node
def test_loader_returns_the_ik_block_and_everything_else_as_before(rz, tmp_path):
    """fails without the feature (ikFrames undefined). The IK block comes back as written, sorted stably by frame; bone and morph results
    equal those of the same file cut after the morph block; files truncated at every block boundary and inside a record of every block
    do not throw, keep what was parsed completely and have ikFrames == []"""
    data, bounds, inside = write_vmd_with_ik(BONE_KEYS, MORPH_KEYS, IK_KEYS)
    files = {"full": data, "cut": data[:bounds[0]], "no ik keys": write_vmd_with_ik(BONE_KEYS, MORPH_KEYS, [], 0, 0, 0)[0]}
    for k, b in enumerate(bounds[:-1]):
        files["boundary %d" % k] = data[:b]
        files["count %d" % k] = data[:b + 2]                 # inside the next block's count
    for k, b in enumerate(inside):
        files["inside %d" % k] = data[:b]
    files["inside the morph block"] = data[:bounds[0] - 10]
    for name, b in files.items():
        (tmp_path / (name.replace(" ", "_") + ".vmd")).write_bytes(b)
    names = list(files)
    out = dict(zip(names, node_host(tmp_path, dict(mode="parse", vmds=[str(tmp_path / (n.replace(" ", "_") + ".vmd")) for n in names]), "parse")))
    assert not any("error" in r for r in out.values()), {n: r.get("error") for n, r in out.items()}
    full, cut = out["full"], out["cut"]
    want = [dict(frame=f, time=f / 30.0, show=s, ik=[dict(name=n, enabled=e) for n, e in lst]) for f, s, lst in sorted(IK_KEYS, key=lambda k: k[0])]
    assert full["ik"] == want, full["ik"]
    assert cut["ik"] == [] and out["no ik keys"]["ik"] == []
    assert full["bone"] == cut["bone"] and full["morph"] == cut["morph"] and len(full["morph"]) == 3 and sum(len(g["frames"]) for g in full["bone"]) == 4
    for name, r in out.items():
        if name in ("full", "no ik keys"):
            continue
        assert r["ik"] == [], name
        assert r["bone"] == full["bone"], name
        assert r["morph"] == (full["morph"] if name != "inside the morph block" else r["morph"]), name
    assert len(out["inside the morph block"]["morph"]) == 2
    print("loader: %d files, %d IK keys back as written, %d truncations tolerated" % (len(files), len(want), len(files) - 2))


# ---- the host twins ----

@needs_node
def test_host_solver_with_switches_against_the_definition(rz, tmp_path):
    worst_all = 0.0
    for name in ("leg rig, crowd of 3", "leg rig, descending goals", "three stages, middle stage off", "nine legs, crowd of 5"):
        s = sc.scene(name)
        sk = s["sk"]
        masks = [m for m in {s["masks"][i].tobytes(): s["masks"][i].tolist() for i in range(s["I"])}.values()]
        poses = s["poses"][:4]
        inp = dict(mode="solve", parents=[int(p) for p in sk["parents"]], bind=np.asarray(sk["bind"], dtype=np.float64).tolist(), masks=masks,
                   chains=[dict(goal=c["goal"], effector=c["effector"], loops=c["loops"], limitAngle=c["limit_angle"],
                                links=[dict(bone=ln["bone"], min=ln["min"], max=ln["max"]) for ln in c["links"]]) for c in s["chains"]],
                   poses=[dict(q=np.asarray(q, dtype=np.float64).reshape(-1).tolist(), t=np.asarray(t, dtype=np.float64).reshape(-1).tolist()) for q, t in poses])
        out = node_host(tmp_path, inp, "solve_" + name.replace(" ", "_").replace(",", ""))
        worst = 0.0
        by_goal = sorted(range(len(s["chains"])), key=lambda k: s["chains"][k]["goal"])
        for mask, r in zip(masks, out):
            assert r["enabled"] == [bool(mask[k]) for k in by_goal], name
            for (q, t), w in zip(poses, r["worlds"]):
                w64 = sw.solve(sk["parents"], sk["bind"], q, t, s["chains"], mask)[0]
                worst = max(worst, float(np.abs(np.array(w, dtype=np.float32).reshape(-1, 16).astype(np.float64) - w64).max()) / sk["extent"])
        print("Model.solveIK with switches, %s: %.2e x extent (bar %.0e)" % (name, worst, BAR))
        assert worst <= BAR, name
        worst_all = max(worst_all, worst)


@needs_node
def test_sampler_ik_state_and_blended_choice(rz, tmp_path):
    """VMDSampler.ikStateAt equals state_at on every track case, flatten().ikKeys equals flatten, and applyBlendedFrame / applyLayeredFrame
    pick by choose — only with setIKKeys(true): without it they leave the switches alone"""
    from pmx_synth import write_vmd
    names = sc.rig_chain_names()
    for track, (keys, ask) in sc.tracks().items():
        vmd = tmp_path / (track.replace(" ", "_") + ".vmd")
        vmd.write_bytes(write_vmd_with_ik([("centre", 0, (0, 0, 0, 1))], [], [(int(f), True, lst) for f, lst in keys])[0])
        other = tmp_path / "other.vmd"
        okeys = sc.tracks()["one key"][0]
        other.write_bytes(write_vmd_with_ik([("centre", 0, (0, 0, 0, 1))], [], [(int(f), True, lst) for f, lst in okeys])[0])
        plain = tmp_path / "plain.vmd"
        plain.write_bytes(write_vmd([("centre", 0, (0, 0, 0, 1))]))
        below = float(np.nextafter(np.float32(0.5), np.float32(0)))
        states = [[10.0, None, 0.0, 0.0], [10.0, str(other), 12.0, below], [10.0, str(other), 12.0, 0.5], [25.0, str(other), 3.0, 1.0], [25.0, str(plain), 3.0, 0.75]]
        out = node_host(tmp_path, dict(mode="state", vmd=str(vmd), frames=ask, names=names, states=states), "state_" + track.replace(" ", "_"))
        kf, ke = sw.flatten(keys, names)
        named = sorted({n for _, lst in keys for n, _ in lst})
        for f, got in zip(ask, out["states"]):
            got = dict(got)
            assert sorted(got) == named, (track, f)
            row = sw.state_at(kf, ke, f, 4)
            assert all(got.get(n, True) == bool(row[k]) for k, n in enumerate(names)), (track, f, got, row)
        if len(keys):
            assert out["keys"]["frames"] == kf.tolist() and out["keys"]["enabled"] == ke.reshape(-1).tolist(), track
        else:
            assert out["keys"] is None
        assert out["noNames"]
        sets = {0: (kf, ke) if len(keys) else None, 1: sw.flatten(okeys, names), 2: None}
        want = [sw.choose((0, st[0], sw.NO_CLIP if st[1] is None else (1 if st[1] == str(other) else 2), st[2], st[3]), sets, 4).astype(bool).tolist() for st in states]
        assert out["chosen"] == want and out["layered"] == want, (track, out["chosen"], want)
        assert all(all(r) for r in out["before"]), track


@needs_node
def test_engine_uploads_the_keys_behind_the_motion_and_nothing_without_the_option(rz):
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "ik_switch_engine_mock.js")], timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    fns = lambda k: [(c["fn"], c["ctx"]) for c in r[k]["calls"]]
    # device sampling: uploadIKKeys right behind uploadAnimation / uploadMotions on every shard with instances (the third shard has none)
    assert fns("seek") == [("animation", "ctx0"), ("ikKeys", "ctx0"), ("animation", "ctx1"), ("ikKeys", "ctx1")] + [("sampled", "ctx0"), ("sampled", "ctx1")] * 2
    k = r["seek"]["calls"][1]
    assert k["clip"] is None and k["frames"] == [0, 20] and k["enabled"] == [0, 1, 1, 0]          # chains legIK, toeIK; the name the model lacks is ignored
    assert fns("motions") == [("motions", "ctx0"), ("ikKeys", "ctx0"), ("ikKeys", "ctx0"), ("motions", "ctx1"), ("ikKeys", "ctx1"), ("ikKeys", "ctx1"), ("blended", "ctx0"), ("blended", "ctx1")]
    assert [(c["clip"], c["frames"]) for c in r["motions"]["calls"] if c["fn"] == "ikKeys"][:2] == [(0, [0, 20]), (1, [])]      # the clip without keys: a set of no keys
    # a motion without keys behind one with keys: a set of no keys ("all on") goes up behind it, so the old switches do not stay
    assert fns("seekThenPlain") == ([("animation", "ctx0"), ("ikKeys", "ctx0"), ("animation", "ctx1"), ("ikKeys", "ctx1"), ("sampled", "ctx0"), ("sampled", "ctx1")]) * 2
    assert [(c["frames"], c["enabled"]) for c in r["seekThenPlain"]["calls"] if c["fn"] == "ikKeys"] == [([0, 20], [0, 1, 1, 0])] * 2 + [([], [])] * 2
    assert [(c["fn"], c.get("clip"), c.get("frames")) for c in r["motionsPlain"]["calls"] if c["ctx"] == "ctx0"] == [("motions", None, None), ("ikKeys", 0, []), ("blended", None, None)]
    # without the option: no new addon call, on any path, and the host model's switches stay on
    new = {"ikKeys", "setIK"}
    for k in ("seekOff", "motionsOff", "hostSampledOff", "hostOff"):
        assert not new & {c["fn"] for c in r[k]["calls"]} and r[k]["enabled"] == [True, True], k
    assert fns("seekOff") == [x for x in fns("seek") if x[0] != "ikKeys"] and fns("motionsOff") == [x for x in fns("motions") if x[0] != "ikKeys"]
    # host-sampled deviceFK frames: setIKEnabled behind every setPoseLocal, with the switches at the frame (10: legIK off; 25: toeIK off)
    assert fns("hostSampled") == [("local", "ctx0"), ("setIK", "ctx0"), ("local", "ctx1"), ("setIK", "ctx1")] * 2
    assert [c["mask"] for c in r["hostSampled"]["calls"] if c["fn"] == "setIK"] == [[0, 1], [0, 1], [1, 0], [1, 0]]
    # host path: the model's switches, no addon call
    assert not new & {c["fn"] for c in r["host"]["calls"]} and r["host"]["enabled"] == [True, False]
    # switches held by hand: laid over all on (no ikKeys) or over what the keys gave (read back behind the pose call), only the named one
    # changes; handed back, the context gets all on once (no ikKeys) or nothing (the next pose call writes the keys' state)
    m0 = [(c["fn"], c.get("mask", "-")) for c in r["manual"]["calls"] if c["ctx"] == "ctx0"]
    assert m0 == [("animation", "-"), ("sampled", "-"), ("setIK", [1, 0]), ("sampled", "-"), ("setIK", None), ("sampled", "-")], m0
    m1 = [(c["fn"], c.get("mask", "-")) for c in r["manualKeys"]["calls"] if c["ctx"] == "ctx1"]
    assert m1 == [("animation", "-"), ("ikKeys", "-"), ("sampled", "-"), ("readIK", "-"), ("setIK", [0, 0]), ("sampled", "-"), ("sampled", "-")], m1
    # playAnimation starts from "every chain on": the frame-0 key switches legIK off, the toe switch an earlier playback left is gone
    assert r["play"]["enabled"] == [False, True]
    assert r["threw"] and "ik: true" in r["threw"]
