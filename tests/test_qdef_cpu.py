"""CPU checks of opt-in QDEF skinning (PMX 2.1 weight type 4, dual-quaternion blending): the float64 reference (tests/qdef_ref.py) and
its properties, the condition the GPU tests rest on (few listed vertices whose sign s_i float32 and float64 may choose differently) on
every scene they use, the PMX loader listing type-4 vertices (Geometry.qdef) without changing how it encodes them as BDEF4, the engine's
{ qdef } option over a recording stand-in for the addon, and the new symbol. The device pass is tests/test_gpu_qdef.py."""
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import qdef_ref
import qdef_scenes
import sdef_ref
from oracle import rz_oracle_np as onp
from test_sdef_cpu import palette16, rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def random_case(rng, n=300, B=7):
    pos = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    j = rng.integers(0, B, size=(n, 4)).astype(np.uint16)
    w = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
    w[::5, 3] = 0                       # three influences
    w[1::5, 2:] = 0                     # two
    w[2::7] = 0                         # isum == 0: (1, 0, 0, 0)
    pal = palette16(np.stack([rot(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(B)]), rng.uniform(-2, 2, size=(B, 3)))
    return pos, nrm, j, w, pal


def apply_rows(S, p):
    return np.einsum("nij,nj->ni", S[:, :, :3], np.asarray(p, dtype=np.float64)) + S[:, :, 3]


def test_one_influence_is_the_palette_transform():
    rng = np.random.default_rng(12)
    pos, nrm, j, w, pal = random_case(rng)
    w[:] = 0
    slot = rng.integers(0, 4, len(pos))
    w[np.arange(len(pos)), slot] = rng.integers(1, 256, len(pos))
    idx = np.arange(len(pos))
    P, N = qdef_ref.qdef(pos, nrm, j, w, pal, idx)
    S = sdef_ref.rows(pal)[j[idx, slot].astype(np.int64)]
    assert np.abs(P - apply_rows(S, pos)).max() < 1e-6          # (the palette itself is float32: its rotations are orthonormal to ~1e-7)
    assert np.abs(N - np.einsum("nij,nj->ni", S[:, :, :3], nrm.astype(np.float64))).max() < 1e-6
    # joints beyond the skeleton are clamped to its last bone
    j2 = j.copy()
    j2[np.arange(len(pos)), slot] = 1000
    P2, _ = qdef_ref.qdef(pos, nrm, j2, w, pal, idx)
    assert np.abs(P2 - apply_rows(sdef_ref.rows(pal)[np.full(len(pos), len(pal) - 1)], pos)).max() < 1e-6


def test_four_bones_with_the_same_rigid_transform():
    rng = np.random.default_rng(13)
    pos, nrm, j, w, _ = random_case(rng)
    B = 7
    pal = palette16(np.repeat(rot([1, 2, 3], 1.1)[None], B, 0), np.repeat(np.array([[0.3, -1.2, 2.0]]), B, 0))
    P, N = qdef_ref.qdef(pos, nrm, j, w, pal, np.arange(len(pos)))
    S = sdef_ref.rows(pal)[np.zeros(len(pos), dtype=np.int64)]
    assert np.abs(P - apply_rows(S, pos)).max() < 1e-6
    some = np.flatnonzero(w.astype(np.int64).sum(axis=1) > 0)
    Pl, Nl = onp.skin(pos[some], nrm[some], j[some], w[some], pal)
    assert np.abs(P[some] - Pl).max() < 1e-4 and np.abs(N[some] - Nl).max() < 1e-4


def test_a_half_turn_twist_keeps_the_distance_from_the_axis():
    """Two bones twisted 180 degrees about a shared axis at equal weight: linear blending collapses the vertex onto the axis ("candy
    wrapper"), the dual-quaternion blend is the 90 degree twist and keeps its distance."""
    pal = palette16(np.stack([np.eye(3), rot([1, 0, 0], np.pi)]), np.zeros((2, 3)))
    pos = np.array([[0.5, 1.0, 0.0], [0.5, 0.0, 2.0]], np.float32)
    nrm = np.array([[0, 1, 0], [0, 0, 1]], np.float32)
    j = np.array([[0, 1, 0, 0]] * 2, np.uint16)
    w = np.array([[127, 127, 0, 0]] * 2, np.uint8)
    Pl, _ = onp.skin(pos, nrm, j, w, pal)
    assert np.linalg.norm(np.asarray(Pl)[:, 1:], axis=1).max() < 1e-6
    for flip in (None, np.array([[False, True, False, False]] * 2)):      # (exactly 180 degrees: either sign is a 90 degree twist)
        P, N = qdef_ref.qdef(pos, nrm, j, w, pal, [0, 1], flip)
        assert np.allclose(np.linalg.norm(P[:, 1:], axis=1), [1.0, 2.0], atol=1e-6) and np.allclose(P[:, 0], 0.5, atol=1e-6)
        assert np.allclose(np.linalg.norm(N, axis=1), 1.0, atol=1e-12)
    assert qdef_ref.margin(j, w, pal, [0, 1]).max() < 1e-6


def test_the_sign_of_a_bone_quaternion_changes_nothing(monkeypatch):
    rng = np.random.default_rng(14)
    pos, nrm, j, w, pal = random_case(rng)
    idx = np.arange(len(pos))
    P0, N0 = qdef_ref.qdef(pos, nrm, j, w, pal, idx)
    real = sdef_ref.quat_of
    for b in range(len(pal)):
        def negated(m, b=b):
            q = real(m)
            q[b] = -q[b]
            return q
        monkeypatch.setattr(sdef_ref, "quat_of", negated)
        P, N = qdef_ref.qdef(pos, nrm, j, w, pal, idx)
        assert np.abs(P - P0).max() < 1e-12 and np.abs(N - N0).max() < 1e-12, b


def test_few_ambiguous_vertices_in_every_gpu_scene(rz):
    from reze_engine_amd import synth
    for name, m, idx, world in qdef_scenes.poses(synth):
        mg = qdef_ref.margin(m["joints"], m["weights"], onp.palette(world, m["inv_bind"]), idx)
        assert (mg < qdef_ref.AMBIGUOUS).sum() <= 0.01 * len(idx), "%s: %d of %d" % (name, (mg < qdef_ref.AMBIGUOUS).sum(), len(idx))
    s = qdef_scenes.build(synth)
    k = (s["mesh"]["weights"][s["idx"]] > 0).sum(axis=1)
    assert 0 in s["idx"] and qdef_scenes.V - 1 in s["idx"] and len(s["idx"]) % 256 != 0 and 550 <= len(s["idx"]) <= 650
    assert (k == 2).sum() > 100 and (k == 3).sum() > 20 and (k == 4).sum() > 20


def test_make_qdef_draws_multi_influence_vertices(rz):
    from reze_engine_amd import synth
    mesh = synth.make_mesh(5000, 60)
    idx = synth.make_qdef(mesh, 0.15, seed=4)
    assert idx.dtype == np.uint32 and abs(len(idx) - 750) <= 1 and np.all(np.diff(idx.astype(np.int64)) > 0)
    k = (mesh["weights"][idx] > 0).sum(axis=1)
    assert np.all(k >= 2) and (k == 4).sum() > 0
    tc = synth.make_qdef(mesh, 0.05, seed=4, cluster=64)
    assert abs(len(tc) - 250) <= 1 and np.all(np.diff(tc.astype(np.int64)) > 0)
    assert np.all((mesh["weights"][tc] > 0).sum(axis=1) >= 2)


# ---- the PMX loader ----

def _text(s):
    b = s.encode("utf-16le")
    return struct.pack("<i", len(b)) + b


def write_qdef_pmx(V=300, B=40, bone_size=2, seed=3, fold=False):
    """A PMX 2.1 stream with a mix of BDEF1 / BDEF2 / BDEF4 / QDEF vertices and `bone_size`-byte bone indices. fold = True writes every
    QDEF vertex as the BDEF4 vertex the loader encodes it as (same joints, same weights, type 2). A vertex's joints are four consecutive
    bones of the chain in a random slot order, as on a real mesh: influences of bones far apart in a twisted chain would be rotated
    against each other by any angle, 180 degrees included. Returns (bytes, QDEF vertex indices)."""
    rng = np.random.default_rng(seed)
    fmt = {1: "<b", 2: "<h", 4: "<i"}[bone_size]
    out = bytearray(b"PMX ") + struct.pack("<f", 2.1) + bytes([8, 0, 0, 4, 1, 1, bone_size, 1, 1])
    out += _text("qdef") + _text("") + _text("") + _text("")
    kinds = rng.choice([0, 1, 2, 4], size=V, p=[0.2, 0.2, 0.2, 0.4])
    out += struct.pack("<i", V)
    listed = []
    for v in range(V):
        p = rng.uniform(-5, 5, 3).astype(np.float32)
        n = rng.normal(size=3).astype(np.float32)
        out += p.tobytes() + n.tobytes() + struct.pack("<2f", 0.25, 0.75)
        js = [int(x) for x in (rng.integers(0, max(B - 3, 1)) + rng.permutation(4)) % B]
        k = int(kinds[v])
        if k == 0:
            out += bytes([0]) + struct.pack(fmt, js[0])
        elif k == 1:
            out += bytes([1]) + struct.pack(fmt, js[0]) + struct.pack(fmt, js[1]) + struct.pack("<f", float(rng.random()))
        else:
            wt = rng.random(4).astype(np.float32)
            if v % 3 == 0:
                wt[3] = 0                                           # three influences
            out += bytes([2 if (k == 2 or fold) else 4]) + b"".join(struct.pack(fmt, x) for x in js) + wt.tobytes()
            if k == 4:
                listed.append(v)
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
    return bytes(out), np.array(listed, dtype=np.uint32)


def parse(path):
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "qdef_parse.js"), path], timeout=120)
    return json.loads(out.decode().strip().splitlines()[-1])


@needs_node
@pytest.mark.parametrize("bone_size", [1, 2, 4])
def test_loader_lists_qdef_and_encodes_the_skinning_as_before(tmp_path, bone_size):
    data, listed = write_qdef_pmx(bone_size=bone_size, seed=bone_size)
    folded, _ = write_qdef_pmx(bone_size=bone_size, seed=bone_size, fold=True)
    (tmp_path / "q.pmx").write_bytes(data)
    (tmp_path / "f.pmx").write_bytes(folded)
    r, f = parse(str(tmp_path / "q.pmx")), parse(str(tmp_path / "f.pmx"))
    assert len(listed) > 50
    assert r["index"] == listed.tolist() and r["sdef"] == []
    # joints and weights: byte-identical to the same vertices written as BDEF4
    assert r["joints"] == f["joints"] and r["weights"] == f["weights"]
    assert f["index"] == []


@needs_node
def test_few_ambiguous_vertices_in_the_node_scene(tmp_path):
    """The scene of test_gpu_qdef.py::test_node_engine_end_to_end, posed on the host model: the same condition as for the other scenes."""
    data, listed = write_qdef_pmx(V=3000, B=40, bone_size=2, seed=7)
    (tmp_path / "m.pmx").write_bytes(data)
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "qdef_pose.js"), str(tmp_path / "m.pmx"), str(tmp_path)], timeout=120)
    idx = np.array(json.loads(out.decode().strip().splitlines()[-1])["index"], np.int64)
    assert np.array_equal(idx, listed) and len(idx) > 500
    ld = lambda n, dt, k: np.fromfile(str(tmp_path / n), dtype=dt).reshape(-1, k)      # noqa: E731
    joints, weights, inv, world = ld("joints.u16", np.uint16, 4), ld("weights.u8", np.uint8, 4), ld("invbind.f32", np.float32, 16), ld("world.f32", np.float32, 16)
    assert np.abs(world - np.tile(np.eye(4, dtype=np.float32).reshape(16), (len(world), 1)))[:, :11].max() > 0.5      # (the pose is a pose)
    mg = qdef_ref.margin(joints, weights, onp.palette(world, inv), idx)
    assert (mg < qdef_ref.AMBIGUOUS).sum() <= 0.01 * len(idx), "%d of %d" % ((mg < qdef_ref.AMBIGUOUS).sum(), len(idx))


@needs_node
def test_engine_uploads_qdef_per_shard_only_when_asked():
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "qdef_mock.js")], timeout=60)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["off"]["calls"] == []
    calls, shards = r["on"]["calls"], r["on"]["shards"]
    assert [c["ctx"] for c in calls] == ["ctx0", "ctx1"]            # (and no uploadSdef)
    seen = []
    for call, (b, n) in zip(calls, shards):
        assert call["idx"] == sorted(set(call["idx"])) and all(0 <= i < n for i in call["idx"])
        seen += [b + i for i in call["idx"]]
    assert seen == r["qdefIdx"]


def test_the_library_exports_rz_upload_qdef(rz):
    header = open(os.path.join(ROOT, "include", "reze_deform.h")).read()
    assert int(re.search(r"#define RZ_ABI_VERSION (\d+)", header).group(1)) == 8
    assert re.search(r"int rz_upload_qdef\(rz_ctx \*ctx, uint32_t n, const uint32_t \*vert_idx\);", header)
    L = rz.capi.load()
    assert L.rz_abi_version() == 8 and hasattr(L, "rz_upload_qdef")
    assert "rz_upload_qdef" in rz.capi.SYMBOLS and "rz_upload_qdef" in rz.capi.OPTIONAL_SYMBOLS
    assert hasattr(rz.DeformContext, "upload_qdef")
