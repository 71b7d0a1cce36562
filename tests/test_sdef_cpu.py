"""CPU checks of opt-in SDEF skinning (PMX weight type 3): the float64 reference (tests/sdef_ref.py) and its identities, the PMX loader
collecting C / R0 / R1 (Geometry.sdef) without changing how it folds the vertex into BDEF2, the engine's { sdef } option over a
recording stand-in for the addon, and the ABI bump. The device pass is tests/test_gpu_sdef.py."""
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sdef_ref
from oracle import rz_oracle_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def rot(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    x, y, z = axis
    c, s = np.cos(ang), np.sin(ang)
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def palette16(R, t):
    """[B,3,3] rotations + [B,3] translations -> [B,16] column-major palette."""
    m = np.zeros((len(R), 4, 4))
    m[:, :3, :3] = R
    m[:, :3, 3] = t
    m[:, 3, 3] = 1
    return np.transpose(m, (0, 2, 1)).reshape(-1, 16).astype(np.float32)


def random_case(rng, n=200, B=6):
    pos = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    j = np.zeros((n, 4), np.uint16)
    j[:, 0] = rng.integers(0, B, n)
    j[:, 1] = rng.integers(0, B, n)
    w = np.zeros((n, 4), np.uint8)
    w[:, 0] = rng.integers(1, 255, n)
    w[:, 1] = 255 - w[:, 0]
    c = rng.uniform(-1, 1, size=(n, 3))
    r0 = c + rng.uniform(-0.1, 0.1, size=(n, 3))
    r1 = c + rng.uniform(-0.1, 0.1, size=(n, 3))
    return pos, nrm, j, w, c, r0, r1


def test_reference_identities():
    rng = np.random.default_rng(11)
    B = 6
    pos, nrm, j, w, c, r0, r1 = random_case(rng, B=B)
    idx = np.arange(len(pos))
    # identity pose: P' = p~, N' = n
    ident = palette16(np.repeat(np.eye(3)[None], B, 0), np.zeros((B, 3)))
    P, N = sdef_ref.sdef(pos, nrm, j, w, ident, idx, c, r0, r1)
    assert np.abs(P - pos).max() < 1e-6 and np.abs(N - nrm).max() < 1e-6
    # every bone the same rotation (different translations): P' = the BDEF2 result
    Rs = rot([1, 2, 3], 1.1)
    pal = palette16(np.repeat(Rs[None], B, 0), rng.uniform(-2, 2, size=(B, 3)))
    P, N = sdef_ref.sdef(pos, nrm, j, w, pal, idx, c, r0, r1)
    Pl, Nl = onp.skin(pos, nrm, j, w, pal)
    assert np.abs(P - Pl).max() < 1e-4 and np.abs(N - Nl).max() < 1e-4
    # w0 = 1: P' = S0 p~ (BDEF1)
    w1 = w.copy()
    w1[:, 0] = 255
    w1[:, 1] = 0
    pal = palette16(np.stack([rot(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(B)]), rng.uniform(-2, 2, size=(B, 3)))
    P, N = sdef_ref.sdef(pos, nrm, j, w1, pal, idx, c, r0, r1)
    S = sdef_ref.rows(pal)[j[:, 0].astype(np.int64)]
    P1 = np.einsum("nij,nj->ni", S[:, :, :3], pos.astype(np.float64)) + S[:, :, 3]
    assert np.abs(P - P1).max() < 1e-5


def test_reference_twist_differs_from_bdef2():
    """A 90 degree twist between two bones: SDEF keeps the vertex off the candy-wrapper collapse that linear blending produces."""
    B = 2
    pal = palette16(np.stack([np.eye(3), rot([1, 0, 0], np.pi / 2)]), np.zeros((B, 3)))
    pos = np.array([[0.5, 1.0, 0.0], [0.5, 0.0, 1.0]], np.float32)
    nrm = np.array([[0, 1, 0], [0, 0, 1]], np.float32)
    j = np.array([[0, 1, 0, 0]] * 2, np.uint16)
    w = np.array([[128, 127, 0, 0]] * 2, np.uint8)
    c = np.array([[0.5, 0.0, 0.0]] * 2)
    P, N = sdef_ref.sdef(pos, nrm, j, w, pal, [0, 1], c, c, c)
    Pl, _ = onp.skin(pos, nrm, j, w, pal)
    # SDEF rotates about the joint: the distance to the twist axis is kept; LBS shrinks it by ~cos(45 deg)
    assert np.allclose(np.linalg.norm(P[:, 1:], axis=1), 1.0, atol=1e-6)
    assert np.linalg.norm(Pl[:, 1:], axis=1).max() < 0.75
    assert np.abs(P - Pl).max() > 0.2


# ---- the PMX loader ----

def _text(s):
    b = s.encode("utf-16le")
    return struct.pack("<i", len(b)) + b


def write_sdef_pmx(V=300, B=40, bone_size=2, seed=3, fold=False):
    """A PMX 2.0 stream with a mix of BDEF1 / BDEF2 / BDEF4 / SDEF vertices and `bone_size`-byte bone indices. fold = True writes every
    SDEF vertex as the BDEF2 vertex the loader folds it into (same joints, same weight, no C / R0 / R1). Returns (bytes, sdef dict)."""
    rng = np.random.default_rng(seed)
    fmt = {1: "<b", 2: "<h", 4: "<i"}[bone_size]
    out = bytearray(b"PMX ") + struct.pack("<f", 2.0) + bytes([8, 0, 0, 4, 1, 1, bone_size, 1, 1])
    out += _text("sdef") + _text("") + _text("") + _text("")
    kinds = rng.choice([0, 1, 2, 3], size=V, p=[0.2, 0.3, 0.1, 0.4])
    out += struct.pack("<i", V)
    sd = dict(idx=[], c=[], r0=[], r1=[])
    for v in range(V):
        p = rng.uniform(-5, 5, 3).astype(np.float32)
        n = rng.normal(size=3).astype(np.float32)
        out += p.tobytes() + n.tobytes() + struct.pack("<2f", 0.25, 0.75)
        js = [int(x) for x in rng.integers(0, B, 4)]
        k = int(kinds[v])
        if k == 0:
            out += bytes([0]) + struct.pack(fmt, js[0])
        elif k == 1 or k == 3:
            wt = float(rng.random())
            out += bytes([1 if (k == 1 or fold) else 3]) + struct.pack(fmt, js[0]) + struct.pack(fmt, js[1]) + struct.pack("<f", wt)
            if k == 3:
                cr = rng.uniform(-2, 2, size=(3, 3)).astype(np.float32)
                if not fold:
                    out += cr.tobytes()
                sd["idx"].append(v); sd["c"].append(cr[0]); sd["r0"].append(cr[1]); sd["r1"].append(cr[2])
        else:
            out += bytes([2]) + b"".join(struct.pack(fmt, x) for x in js) + rng.random(4).astype(np.float32).tobytes()
        out += struct.pack("<f", 1.0)
    tri = rng.integers(0, V, size=30).astype(np.int32)
    out += struct.pack("<i", len(tri)) + tri.tobytes()
    out += struct.pack("<i", 0)                                           # textures
    out += struct.pack("<i", 0)                                           # materials
    out += struct.pack("<i", B)
    bpos = np.cumsum(rng.uniform(-1, 1, size=(B, 3)), axis=0).astype(np.float32)
    for b in range(B):
        out += _text("bone%d" % b) + _text("") + bpos[b].tobytes() + struct.pack(fmt, b - 1) + struct.pack("<i", 0)
        out += struct.pack("<H", 0) + struct.pack("<3f", 0, 1, 0)
    out += struct.pack("<i", 0) + struct.pack("<i", 0) + struct.pack("<i", 0) + struct.pack("<i", 0)   # morphs, frames, bodies, joints
    sdef = {k: np.array(v, dtype=np.uint32 if k == "idx" else np.float32).reshape((-1,) if k == "idx" else (-1, 3)) for k, v in sd.items()}
    return bytes(out), sdef


def parse(path):
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "sdef_parse.js"), path], timeout=120)
    return json.loads(out.decode().strip().splitlines()[-1])


@needs_node
@pytest.mark.parametrize("bone_size", [1, 2, 4])
def test_loader_collects_sdef_and_folds_the_skinning_as_before(tmp_path, bone_size):
    data, sd = write_sdef_pmx(bone_size=bone_size, seed=bone_size)
    folded, _ = write_sdef_pmx(bone_size=bone_size, seed=bone_size, fold=True)
    (tmp_path / "s.pmx").write_bytes(data)
    (tmp_path / "f.pmx").write_bytes(folded)
    r, f = parse(str(tmp_path / "s.pmx")), parse(str(tmp_path / "f.pmx"))
    assert len(sd["idx"]) > 50
    assert r["index"] == sd["idx"].tolist()
    for k in ("c", "r0", "r1"):
        assert np.array_equal(np.array(r[k], np.float32).reshape(-1, 3), sd[k]), k
    # joints and weights: byte-identical to the same vertices written as BDEF2
    assert r["joints"] == f["joints"] and r["weights"] == f["weights"]
    assert f["index"] == []


@needs_node
def test_engine_uploads_sdef_per_shard_only_when_asked():
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "engine_sdef_mock.js")], timeout=60)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["off"]["calls"] == []
    calls, shards = r["on"]["calls"], r["on"]["shards"]
    assert [c["ctx"] for c in calls] == ["ctx0", "ctx1"]
    seen = []
    for call, (b, n) in zip(calls, shards):
        assert call["idx"] == sorted(set(call["idx"])) and all(0 <= i < n for i in call["idx"])
        seen += [b + i for i in call["idx"]]
    assert seen == r["sdefIdx"]
    # the C / R0 / R1 rows travel with their vertex
    rows = [k for k in range(len(r["sdefIdx"]))]
    flat = sum((c["c"] for c in calls), [])
    assert flat == [float(x) for k in rows for x in range(3 * k, 3 * k + 3)]


def test_abi_8_exports_rz_upload_sdef(rz):
    header = open(os.path.join(ROOT, "include", "reze_deform.h")).read()
    assert int(re.search(r"#define RZ_ABI_VERSION (\d+)", header).group(1)) == 8
    assert re.search(r"int rz_upload_sdef\(rz_ctx \*ctx, uint32_t n, const uint32_t \*vert_idx,", header)
    L = rz.capi.load()
    assert L.rz_abi_version() == 8 and hasattr(L, "rz_upload_sdef") and "rz_upload_sdef" in rz.capi.SYMBOLS
    assert hasattr(rz.DeformContext, "upload_sdef")


def test_make_sdef_picks_bdef2_vertices(rz):
    from reze_engine_amd import synth
    mesh = synth.make_mesh(5000, 60)
    t = synth.make_sdef(mesh, 0.15, seed=4)
    idx = t["idx"]
    assert abs(len(idx) - 750) <= 1 and np.all(np.diff(idx.astype(np.int64)) > 0)
    w = mesh["weights"][idx]
    assert np.all(w[:, 1] > 0) and np.all(w[:, 2:] == 0)
    assert np.abs(t["r0"] - t["c"]).max() <= 0.05 + 1e-6
    tc = synth.make_sdef(mesh, 0.05, seed=4, cluster=64)
    assert abs(len(tc["idx"]) - 250) <= 1
