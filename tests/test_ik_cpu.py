"""CPU checks of opt-in PMX inverse kinematics: the float64 restatement (tests/ik_ref.py) is not vacuous, the PMX loader keeps the IK
blocks without changing anything else it returns, Model.solveIK() against the restatement, the engine's { ik } option over a recording
stand-in for the addon, the ABI, and the conditioning of every pose the device tests use (tests/test_gpu_ik.py leaves a pose out only
when the restatement's own float32 run strays; with the seeds chosen none does, and that is asserted here)."""
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ik_ref
from pmx_synth import write_vmd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
BAR, ILL = 1e-4, 2.5e-5


def test_restatement_is_not_vacuous(rz):
    from reze_engine_amd import synth
    rig = synth.make_leg_rig()
    l1, l2 = rig["l1"], rig["l2"]
    knees = (3, 7)
    lo, hi = -np.pi, -0.5 * np.pi / 180
    n, closer, ten = 0, 0, 0
    for seed in range(300):
        q, t = synth.leg_rig_pose(rig, 10_000 + seed, reach=(0.15, 1.2))
        info = []
        h0 = ik_ref.Hierarchy(rig["parents"], rig["bind"], q, t)
        world, qs = ik_ref.solve(rig["parents"], rig["bind"], q, t, rig["chains"], info=info)
        for ch in info:
            if ch["goal"] not in rig["hips"]:
                continue
            d = np.linalg.norm(h0.P[ch["goal"]] - h0.P[rig["hips"][ch["goal"]]])
            if not (1.05 * abs(l1 - l2) <= d <= 0.95 * (l1 + l2)):
                continue
            n += 1
            assert ch["end"] < ch["start"], (seed, ch)
            closer += 1
            ten += ch["end"] * 10 <= ch["start"]
        for k in knees:
            x, y, z, w = qs[k]
            assert abs(y) < 1e-9 and abs(z) < 1e-9, (seed, qs[k])
            ang = 2 * np.arctan2(x, w)
            assert lo - 1e-6 <= ang <= hi + 1e-6, (seed, ang)
    print("leg chains in reach: %d, all closer, %.1f %% at least 10x closer" % (n, 100.0 * ten / n))
    assert n >= 300 and ten >= 0.95 * n
    # loops = 0: the plain hierarchy solve
    from helpers import fk_reference
    q, t = synth.leg_rig_pose(rig, 5)
    w0, q0 = ik_ref.solve(rig["parents"], rig["bind"], q, t, [dict(ch, loops=0) for ch in rig["chains"]])
    assert np.array_equal(q0, q.astype(np.float64))
    assert np.abs(w0 - fk_reference(rig["parents"], rig["bind"], q, t).reshape(-1, 16)).max() < 1e-12


def test_device_test_poses_are_well_conditioned(rz):
    """every pose tests/test_gpu_ik.py holds the kernel to: the float32 run of the restatement stays within 2.5e-5 x extent of the float64
    run, so the device tests leave out none and their exclusion cannot hide a kernel fault"""
    import test_gpu_ik as g
    worst = 0.0
    for name, make in g.CASES.items():
        sk, chains, poses = make()
        assert ik_ref.validate(len(sk["parents"]), sk["parents"], chains) is None, name
        for k, (q, t) in enumerate(poses):
            w64, _ = ik_ref.solve(sk["parents"], sk["bind"], q, t, chains, sk["ap"], sk["ratio"])
            w32, _ = ik_ref.solve(sk["parents"], sk["bind"], q, t, chains, sk["ap"], sk["ratio"], dtype=np.float32)
            e = float(np.abs(w32.astype(np.float64) - w64).max()) / sk["extent"]
            worst = max(worst, e)
            assert e <= ILL, "%s pose %d: float32 restatement strays by %.2e x extent" % (name, k, e)
    print("float32 vs float64 restatement over the device tests' poses: worst %.2e x extent" % worst)


# ---- the PMX loader ----

def _text(s):
    b = s.encode("utf-16le")
    return struct.pack("<i", len(b)) + b


def write_ik_pmx(rig, bone_size=1, with_ik=True, limits=True):
    """A PMX 2.0 stream of a rig dict (synth.make_leg_rig with vertices): BDEF1 / BDEF2 vertices, the rig's bones, and — with_ik — its
    chains as IK blocks on the goal bones. with_ik=False writes the same file without the flag and the blocks."""
    fmt = {1: "<b", 2: "<h", 4: "<i"}[bone_size]
    out = bytearray(b"PMX ") + struct.pack("<f", 2.0) + bytes([8, 0, 0, 4, 1, 1, bone_size, 1, 1])
    out += _text("ik") + _text("") + _text("") + _text("")
    V = len(rig["pos"])
    out += struct.pack("<i", V)
    for v in range(V):
        out += rig["pos"][v].tobytes() + rig["nrm"][v].tobytes() + struct.pack("<2f", 0.5, 0.5)
        j, w = rig["joints"][v], rig["weights"][v]
        if w[1] == 0 or w[2] > 0:
            out += bytes([0]) + struct.pack(fmt, int(j[0]))
        else:
            out += bytes([1]) + struct.pack(fmt, int(j[0])) + struct.pack(fmt, int(j[1])) + struct.pack("<f", float(w[0]) / 255.0)
        out += struct.pack("<f", 1.0)
    tri = (np.arange(30) % V).astype(np.int32)
    out += struct.pack("<i", len(tri)) + tri.tobytes()
    out += struct.pack("<i", 0) + struct.pack("<i", 0)                    # textures, materials
    B = len(rig["parents"])
    bpos = ik_ref.bind_positions(rig["parents"], rig["bind"]).astype(np.float32)
    by_goal = {ch["goal"]: ch for ch in rig["chains"]}
    out += struct.pack("<i", B)
    for b in range(B):
        ch = by_goal.get(b) if with_ik else None
        out += _text(rig["names"][b]) + _text("") + bpos[b].tobytes() + struct.pack(fmt, int(rig["parents"][b])) + struct.pack("<i", 0)
        out += struct.pack("<H", 0x0020 if ch else 0) + struct.pack("<3f", 0, 1, 0)
        if ch:
            out += struct.pack(fmt, ch["effector"]) + struct.pack("<if", ch["loops"], ch["limit_angle"]) + struct.pack("<i", len(ch["links"]))
            for ln in ch["links"]:
                has = limits and ln.get("min") is not None
                out += struct.pack(fmt, ln["bone"]) + bytes([1 if has else 0])
                if has:
                    out += struct.pack("<3f", *ln["min"]) + struct.pack("<3f", *ln["max"])
    out += struct.pack("<i", 0) * 4                                       # morphs, frames, bodies, joints
    return bytes(out)


def write_leg_pmx_vmd(tmp_path):
    """the leg rig as a PMX and a VMD that keys only the centre and the four IK goals; returns the two paths"""
    from reze_engine_amd import synth
    rig = synth.make_leg_rig(n_verts=1500)
    rng = np.random.default_rng(17)
    keys = []
    for f in (0, 10, 20, 30):
        a = rng.uniform(-0.3, 0.3)
        keys.append(("centre", f, (0.0, float(np.sin(a / 2)), 0.0, float(np.cos(a / 2))), (float(rng.uniform(-1, 1)), float(rng.uniform(-3, 0)), float(rng.uniform(-1, 1)))))
        for g in ("leg_ik_L", "leg_ik_R"):
            keys.append((g, f, (0, 0, 0, 1), (float(rng.uniform(-1.5, 1.5)), float(rng.uniform(0, 2.5)), float(rng.uniform(-1.5, 1.5)))))
        for g in ("toe_ik_L", "toe_ik_R"):
            keys.append((g, f, (0, 0, 0, 1), tuple(float(x) for x in rng.uniform(-0.3, 0.3, 3))))
    pmx, vmd = tmp_path / "legs.pmx", tmp_path / "legs.vmd"
    pmx.write_bytes(write_ik_pmx(rig))
    vmd.write_bytes(write_vmd(keys))
    return str(pmx), str(vmd)


def node_json(script, *args):
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", script)] + list(args), timeout=300)
    return json.loads(out.decode().strip().splitlines()[-1])


@needs_node
@pytest.mark.parametrize("bone_size", [1, 2, 4])
def test_loader_returns_ik_blocks_and_everything_else_as_before(rz, tmp_path, bone_size):
    from reze_engine_amd import synth
    rig = synth.make_leg_rig(n_verts=400)
    (tmp_path / "ik.pmx").write_bytes(write_ik_pmx(rig, bone_size))
    (tmp_path / "plain.pmx").write_bytes(write_ik_pmx(rig, bone_size, with_ik=False))
    r, p = node_json("ik_parse.js", str(tmp_path / "ik.pmx")), node_json("ik_parse.js", str(tmp_path / "plain.pmx"))
    by_goal = {ch["goal"]: ch for ch in rig["chains"]}
    for b in range(14):
        got = r["ik"][b]
        if b not in by_goal:
            assert got is None and "ik" not in r["keys"][b].split(",")
            continue
        ch = by_goal[b]
        assert got["effector"] == ch["effector"] and got["loops"] == ch["loops"] and np.float32(got["limitAngle"]) == np.float32(ch["limit_angle"])
        assert [ln["bone"] for ln in got["links"]] == [ln["bone"] for ln in ch["links"]]
        for g, ln in zip(got["links"], ch["links"]):
            if ln["min"] is None:                      # links with and without limits
                assert "min" not in g and "max" not in g
            else:
                assert np.array_equal(np.float32(g["min"]), np.float32(ln["min"])) and np.array_equal(np.float32(g["max"]), np.float32(ln["max"]))
    assert [c["goal"] for c in r["chains"]] == sorted(by_goal) and p["chains"] == [] and all(x is None for x in p["ik"])
    # everything else: what the same model without IK blocks parses to — the parent's field set, byte for byte
    for k in ("rest", "vertices", "indices", "joints", "weights", "invBind", "morphs", "materials"):
        assert r[k] == p[k], k
    assert p["keys"][10] == "name,parentIndex,bindTranslation,children,appendParentIndex,appendRatio,appendRotate,appendMove"
    assert r["keys"][10] == p["keys"][10] + ",ik" and r["keys"][0] == p["keys"][0]


# ---- the host solver ----

def run_host(tmp_path, sk, chains, poses, tag):
    inp = dict(parents=[int(p) for p in sk["parents"]], bind=np.asarray(sk["bind"], dtype=np.float64).tolist(),
               appendParent=None if sk["ap"] is None else [int(a) for a in sk["ap"]],
               appendRatio=None if sk["ratio"] is None else [float(x) for x in sk["ratio"]],
               chains=[dict(goal=c["goal"], effector=c["effector"], loops=c["loops"], limitAngle=c["limit_angle"],
                            links=[dict(bone=ln["bone"], min=ln["min"], max=ln["max"]) for ln in c["links"]]) for c in chains],
               poses=[dict(q=np.asarray(q, dtype=np.float64).reshape(-1).tolist(), t=np.asarray(t, dtype=np.float64).reshape(-1).tolist()) for q, t in poses])
    fi, fo = tmp_path / (tag + "_in.json"), tmp_path / (tag + "_out.json")
    fi.write_text(json.dumps(inp))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "js", "ik_solve.js"), str(fi), str(fo)], timeout=300)
    return json.loads(fo.read_text())


@needs_node
def test_host_solver_against_the_restatement(rz, tmp_path):
    import test_gpu_ik as g
    for name in ("leg rig, local poses", "random tree", "random tree, rigid", "append children, 600 bones"):
        sk, chains, poses = g.CASES[name]()
        poses = poses[:6]
        out = run_host(tmp_path, sk, chains, poses, name.replace(" ", "_").replace(",", ""))
        worst, moved = 0.0, 0.0
        for (q, t), r in zip(poses, out):
            w64, _ = ik_ref.solve(sk["parents"], sk["bind"], q, t, chains, sk["ap"], sk["ratio"])
            on, off, plain = (np.array(r[k], dtype=np.float32).reshape(-1, 16) for k in ("on", "off", "plain"))
            worst = max(worst, float(np.abs(on.astype(np.float64) - w64).max()) / sk["extent"])
            assert np.array_equal(off, plain)          # { ik: false }: today's world matrices, bit for bit
            assert r["kept"]
            moved = max(moved, float(np.abs(on - off).max()))
        print("Model.solveIK, %s: %.2e x extent" % (name, worst))
        assert worst <= BAR and moved > 0.05, (name, worst, moved)


@needs_node
def test_engine_uploads_the_table_once_per_context_after_the_topology():
    r = node_json("ik_engine_mock.js")
    calls = r["device"]["calls"]
    assert [(c["fn"], c["ctx"]) for c in calls] == [("topology", "ctx0"), ("ik", "ctx0"), ("topology", "ctx1"), ("ik", "ctx1")]
    ik = calls[1]
    assert ik["goal"] == [4] and ik["effector"] == [3] and ik["loops"] == [40] and ik["off"] == [0, 2] and ik["bone"] == [2, 1] and ik["limited"] == [1, 0]
    assert ik["min"][3:] == [0, 0, 0] and abs(ik["min"][0] + np.pi) < 1e-6 and calls[3]["min"] == ik["min"]
    assert not r["device"]["hostIK"]
    assert r["host"]["calls"] == [] and r["host"]["hostIK"]                        # without deviceFK: the host solver, no upload
    for k in ("off", "none"):                                                      # not asked / no IK bones: the topology alone
        assert [c["fn"] for c in r[k]["calls"]] == ["topology", "topology"] and not r[k]["hostIK"]
    assert r["hostNone"]["calls"] == [] and not r["hostNone"]["hostIK"]


def test_abi_8_still_and_rz_upload_ik_is_exported(rz):
    header = open(os.path.join(ROOT, "include", "reze_deform.h")).read()
    assert int(re.search(r"#define RZ_ABI_VERSION (\d+)", header).group(1)) == 8
    assert re.search(r"int rz_upload_ik\(rz_ctx \*ctx, uint32_t n_chains, const uint32_t \*goal, const uint32_t \*effector,", header)
    assert "detects the feature by the symbol" in header
    L = rz.capi.load()
    assert L.rz_abi_version() == 8 and hasattr(L, "rz_upload_ik") and "rz_upload_ik" in rz.capi.SYMBOLS
    assert hasattr(rz.DeformContext, "upload_ik")
    assert L.rz_upload_ik(None, 1, None, None, None, None, None, None, None, None, None) < 0 and L.rz_last_error()


def test_make_ik_builds_valid_tables(rz):
    from reze_engine_amd import synth
    mesh = synth.make_mesh(100, 120, seed=31)
    for rigid in (False, True):
        chains = synth.make_ik(mesh, n_chains=6, seed=3, links=2, rigid=rigid)
        assert len(chains) >= 4 and ik_ref.validate(120, mesh["parents"], chains) is None
        assert [c["goal"] for c in chains] == sorted(set(c["goal"] for c in chains))
    rig = synth.make_leg_rig()
    assert len(rig["parents"]) == 14 and len(rig["chains"]) == 4 and ik_ref.validate(14, rig["parents"], rig["chains"]) is None
    assert ik_ref.validate(14, rig["parents"], [dict(rig["chains"][0], links=list(reversed(rig["chains"][0]["links"])))]) is not None
