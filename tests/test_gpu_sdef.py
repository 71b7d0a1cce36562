"""SDEF skinning on the device (rz_upload_sdef, kernels/sdef.hip) against the float64 reference tests/sdef_ref.py, on every frame path.
30 k vertices, 200 bones, ~15 % SDEF vertices, a pose that twists parent-child pairs by 60-120 degrees. The reference takes the world
matrices the frame used from rz_read_world, so device-solved and sampled poses are held to the same definition."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sdef_ref
from helpers import assert_parity, assert_hull

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, M = 30000, 200, 16


def axis_angle(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]]).astype(np.float32)


@pytest.fixture(scope="module")
def scene(rz):
    from reze_engine_amd import synth
    mesh = synth.make_mesh(V, B)
    sd = synth.make_sdef(mesh, 0.15, seed=9)
    rng = np.random.default_rng(21)
    quats = mesh["quats"].copy()
    for b in rng.choice(np.arange(1, B), size=40, replace=False):       # twist 40 bones against their parents
        quats[b] = axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(60, 120)))
    world = synth.fk_world(mesh["parents"], mesh["bind"], quats).reshape(B, 16)
    dense, mw = synth.make_morphs_dense(V, M)
    sparse = synth.make_morphs_sparse(V, M)
    return dict(mesh=mesh, sd=sd, quats=quats, world=world, dense=dense, mw=mw, sparse=sparse, synth=synth)


def make_ctx(rz, s, morphs="none", lib=None, topology=False):
    m = s["mesh"]
    c = rz.DeformContext(0) if lib is None else lib.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    if topology:
        c.upload_skeleton_topology(m["parents"], m["bind"])
    if morphs == "dense":
        c.upload_morphs_dense(s["dense"])
    elif morphs == "sparse":
        c.upload_morphs_sparse(*s["sparse"][:3])
    return c


def weights_of(s, morphs):
    return None if morphs == "none" else (s["mw"] if morphs == "dense" else s["sparse"][3])


def upload_table(c, s, rows=None):
    t = s["sd"]
    r = slice(None) if rows is None else rows
    c.upload_sdef(t["idx"][r], t["c"][r], t["r0"][r], t["r1"][r])


def reference(s, world16, morphs, mw, sdef=True):
    m, t = s["mesh"], s["sd"]
    kw = {}
    if morphs == "dense":
        kw = dict(dense=s["dense"], weights=mw)
    elif morphs == "sparse":
        kw = dict(sparse=s["sparse"][:3], weights=mw)
    idx = t["idx"] if sdef else np.zeros(0, np.uint32)
    return sdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], world16, m["inv_bind"], idx, t["c"], t["r0"], t["r1"], **kw)


def check(c, s, morphs, mw, inst=0, what=""):
    pos, nrm = c.read(inst)
    pr, nr = reference(s, c.read_world(inst), morphs, mw)
    assert_parity(pos, nrm, pr, nr, what)
    return pos, nrm


def test_parity_no_leak_and_lifecycle(rz, scene):
    s = scene
    idx = s["sd"]["idx"].astype(np.int64)
    with make_ctx(rz, s, "dense") as c:
        assert c.get_tuning("sdef_verts") == 0
        c.set_pose(s["world"], s["mw"])
        c.deform()
        p0, n0 = c.read()                                    # BDEF2 for everything
        upload_table(c, s)
        assert c.get_tuning("sdef_verts") == len(idx)
        c.deform()
        p1, n1 = check(c, s, "dense", s["mw"], what="dense world")
        other = np.setdiff1d(np.arange(V), idx)
        assert np.array_equal(p1[other], p0[other]) and np.array_equal(n1[other], n0[other])
        assert np.abs(p1[idx] - p0[idx]).max() > 1e-2
        c.upload_sdef([], [], [], [])                      # removing the table restores the BDEF2 bits
        assert c.get_tuning("sdef_verts") == 0
        c.deform()
        p2, n2 = c.read()
        assert np.array_equal(p2, p0) and np.array_equal(n2, n0)
        # invalid tables are refused with a message and leave the context usable
        upload_table(c, s)
        bad = s["sd"]["idx"].copy()
        bad[[3, 4]] = bad[[4, 3]]
        for ix in (bad, np.concatenate([s["sd"]["idx"][:-1], [V]]).astype(np.uint32)):
            with pytest.raises(rz.RzError) as e:
                c.upload_sdef(ix, s["sd"]["c"], s["sd"]["r0"], s["sd"]["r1"])
            assert e.value.code == -1 and ("ascending" in str(e.value) or "outside" in str(e.value))
        assert c._L.rz_upload_sdef(c._h, 5, None, None, None, None) == -1
        assert b"null" in c._L.rz_last_error()
        c.deform()
        check(c, s, "dense", s["mw"], what="after refused uploads")
        # a fork borrows the table; uploads are refused while it exists
        f = c.fork()
        with pytest.raises(rz.RzError):
            c.upload_sdef([], [], [], [])
        f.set_pose(s["world"], s["mw"])
        c.deform_pair(f, 2)
        check(f, s, "dense", s["mw"], what="fork")
        check(c, s, "dense", s["mw"], what="lender")
        f.close()
        # a new mesh drops the table
        m = s["mesh"]
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        assert c.get_tuning("sdef_verts") == 0


def test_identities_on_the_gpu(rz, scene):
    s = scene
    m = s["mesh"]
    with make_ctx(rz, s) as c:
        upload_table(c, s)
        ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (B, 1))
        ident[:, 12:15] = -m["inv_bind"].reshape(B, 16)[:, 12:15]            # world = bind: palette = identity
        c.set_pose(ident)
        c.deform()
        pos, nrm = c.read()
        idx = s["sd"]["idx"].astype(np.int64)
        assert np.abs(pos[idx] - m["pos"][idx]).max() < 1e-4 and np.abs(nrm[idx] - m["nrm"][idx]).max() < 1e-4
        # every bone the same rotation: SDEF == BDEF2
        x, y, z, ww = (float(v) for v in axis_angle([1, 2, 3], 1.2))
        r3 = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - ww * z), 2 * (x * z + ww * y)],
                       [2 * (x * y + ww * z), 1 - 2 * (x * x + z * z), 2 * (y * z - ww * x)],
                       [2 * (x * z - ww * y), 2 * (y * z + ww * x), 1 - 2 * (x * x + y * y)]], np.float32)
        w = ident.copy().reshape(B, 4, 4)
        w[:, :3, :3] = r3.T                                  # column-major storage: [column][row]
        c.set_pose(w.reshape(B, 16))
        c.deform()
        p1, n1 = c.read()
        c.upload_sdef([], [], [], [])
        c.deform()
        p0, n0 = c.read()
        assert_parity(p1, n1, p0.astype(np.float64), n0.astype(np.float64), "equal rotations")


@pytest.mark.parametrize("morphs", ["none", "dense", "sparse"])
@pytest.mark.parametrize("fast,zero_copy", [(-1, -1), (0, -1), (1, 0), (0, 0)])
def test_world_pose_paths(rz, scene, morphs, fast, zero_copy):
    s = scene
    mw = weights_of(s, morphs)
    with make_ctx(rz, s, morphs) as c:
        c.set_tuning(fast=fast, zero_copy=zero_copy)
        upload_table(c, s)
        for k in range(2):                                   # first frame of a pose, then a replay of it
            if k == 0:
                c.set_pose(s["world"], mw)
            c.deform()
            check(c, s, morphs, mw, what="%s fast=%d zc=%d frame %d" % (morphs, fast, zero_copy, k))


@pytest.mark.parametrize("morphs", ["none", "dense", "sparse"])
@pytest.mark.parametrize("fuse", [0, 1])
def test_local_and_sampled_poses(rz, scene, morphs, fuse):
    s = scene
    mw = weights_of(s, morphs)
    with make_ctx(rz, s, morphs, topology=True) as c:
        c.set_tuning(fuse_fk=fuse)
        upload_table(c, s)
        c.set_pose_local(s["quats"], mw)
        c.deform()
        check(c, s, morphs, mw, what="local %s fuse=%d" % (morphs, fuse))
        nk = 3
        rng = np.random.default_rng(5)
        kq = np.repeat(s["quats"][:, None, :], nk, axis=1).copy()
        kq[:, 1] = [axis_angle(rng.normal(size=3), 1.5) for _ in range(B)]
        c.upload_animation(np.arange(B), np.arange(B + 1) * nk, np.tile(np.arange(nk) * 10.0, B), kq, np.zeros((B, nk, 3), np.float32))
        c.set_pose_sampled([7.5])
        c.deform()
        check(c, s, morphs, None if morphs == "none" else np.zeros(M, np.float32), what="sampled %s fuse=%d" % (morphs, fuse))


def test_graph_replay_takes_a_changed_table(rz, scene):
    s = scene
    with make_ctx(rz, s, "dense") as c:
        c.set_tuning(graph=1)
        upload_table(c, s)
        c.set_pose(s["world"], s["mw"])
        c.deform_n(32)
        check(c, s, "dense", s["mw"], what="graph")
        half = np.arange(len(s["sd"]["idx"])) % 2 == 0
        upload_table(c, s, half)
        c.deform_n(32)
        pos, nrm = c.read()
        t = s["sd"]
        m = s["mesh"]
        pr, nr = sdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], c.read_world(0), m["inv_bind"], t["idx"][half],
                                t["c"][half], t["r0"][half], t["r1"][half], dense=s["dense"], weights=s["mw"])
        assert_parity(pos, nrm, pr, nr, "graph after a changed table")
        c.time_frames(20)                                   # rz_time_frames leaves the SDEF frame behind
        pos2, nrm2 = c.read()
        assert np.array_equal(pos2, pos)


@pytest.mark.parametrize("form", ["whole", "subsets", "subfk"])
def test_crowds(rz, scene, form):
    s = scene
    I = 8
    rng = np.random.default_rng(8)
    quats = np.stack([s["quats"]] * I).copy()
    for i in range(1, I):
        quats[i, rng.choice(np.arange(1, B), 10, replace=False)] = [axis_angle(rng.normal(size=3), 1.0 + 0.1 * i) for _ in range(10)]
    with make_ctx(rz, s, topology=(form == "subfk")) as c:
        c.set_instances(I)
        if form == "whole":
            c.set_tuning(inst_subsets=0)
        upload_table(c, s)
        if form == "subfk":
            nk = 2
            kq = np.stack([quats[0], quats[1]], axis=1)
            c.upload_animation(np.arange(B), np.arange(B + 1) * nk, np.tile(np.arange(nk) * 10.0, B), kq, np.zeros((B, nk, 3), np.float32))
            c.set_pose_sampled(np.linspace(0, 10, I))
        else:
            world = np.stack([s["synth"].fk_world(s["mesh"]["parents"], s["mesh"]["bind"], q).reshape(B, 16) for q in quats])
            c.set_pose(world)
        # the form each case is about: the whole palette, the bone-subset skin kernel (palette_stale), the one-launch device-animated crowd
        # (fk_stale) — the last two leave no palette in memory, so the pass runs the palette kernel their flag names first
        assert c.get_tuning("effective_inst_group") > 0
        assert c.get_tuning("effective_subsets") == (0 if form == "whole" else 1)
        assert (c.get_tuning("effective_closure_bones") > 0) == (form == "subfk")
        c.deform()
        for i in range(I):
            check(c, s, "none", None, inst=i, what="crowd %s instance %d" % (form, i))


def test_dense_crowd_under_the_overlapped_front(rz, scene):
    """Crowd frames with overlap = 1 run their fronts on the upload stream, and the next pose is uploaded there behind this frame's front:
    the pass must take the weights from the ring slot's active list, never from the pose block. Several poses, back to back and read
    after every frame."""
    s = scene
    I = 8
    rng = np.random.default_rng(31)
    with make_ctx(rz, s, "dense") as c:
        c.set_instances(I)
        c.set_tuning(overlap=1)
        upload_table(c, s)
        poses = []
        for k in range(4):
            quats = np.stack([s["quats"]] * I).copy()
            for i in range(I):
                quats[i, rng.choice(np.arange(1, B), 10, replace=False)] = [axis_angle(rng.normal(size=3), rng.uniform(0.5, 2.0)) for _ in range(10)]
            world = np.stack([s["synth"].fk_world(s["mesh"]["parents"], s["mesh"]["bind"], q).reshape(B, 16) for q in quats])
            mw = rng.random((I, M), dtype=np.float32) * (rng.random((I, M)) < 0.6)
            poses.append((world, mw.astype(np.float32)))
        c.set_pose(*poses[0])
        assert c.get_tuning("effective_overlap") == 1
        for rep in range(2):
            for world, mw in poses:                         # rep 0: several frames in flight, rep 1: a read after every frame
                c.set_pose(world, mw)
                c.deform()
                if rep == 1:
                    for i in (0, 3, I - 1):
                        check(c, s, "dense", mw[i], inst=i, what="overlapped dense crowd, instance %d" % i)
            if rep == 0:
                for i in range(I):
                    check(c, s, "dense", poses[-1][1][i], inst=i, what="overlapped dense crowd after back-to-back frames, instance %d" % i)


def test_hull_and_aabb(rz, scene):
    s = scene
    m = s["mesh"]
    edge = np.random.default_rng(3).uniform(0, 1.5, V).astype(np.float32)
    with make_ctx(rz, s, "sparse") as c:
        mw = s["sparse"][3]
        c.upload_edge_scale(edge)
        c.enable_aabb(True)
        c.set_pose(s["world"], mw)
        c.deform()
        pb, _ = c.read()                                    # BDEF2 positions of every vertex
        upload_table(c, s)
        for _ in range(3):                                  # both box slots
            c.deform()
            pos, nrm = check(c, s, "sparse", mw, what="hull / aabb")
            pr, nr = reference(s, c.read_world(0), "sparse", mw)
            assert_hull(c.read_hull(0), pr + nr * edge[:, None].astype(np.float64) * 0.01, "hull")
            box = c.read_aabb(0)
            idx = s["sd"]["idx"].astype(np.int64)
            allp = np.concatenate([pos, pb[idx]])
            assert np.all(box[:3] <= pos.min(axis=0)) and np.all(box[3:] >= pos.max(axis=0))
            assert np.array_equal(box[:3], allp.min(axis=0)) and np.array_equal(box[3:], allp.max(axis=0))


def test_two_shards_on_one_gpu(rz, scene):
    s = scene
    m, t = s["mesh"], s["sd"]
    ref_p, ref_n = None, None
    for r in range(2):
        b, n = rz.shard_range(V, 2, r)
        with rz.DeformContext(0) as c:
            c.upload_mesh(m["pos"][b:b + n], m["nrm"][b:b + n], m["joints"][b:b + n], m["weights"][b:b + n])
            c.upload_skeleton(m["inv_bind"])
            c.upload_morphs_dense(s["dense"][:, b:b + n])
            sel = (t["idx"] >= b) & (t["idx"] < b + n)
            assert sel.sum() > 100
            c.upload_sdef(t["idx"][sel] - b, t["c"][sel], t["r0"][sel], t["r1"][sel])
            c.set_pose(s["world"], s["mw"])
            c.deform()
            pos, nrm = c.read()
            if ref_p is None:
                ref_p, ref_n = reference(s, c.read_world(0), "dense", s["mw"])
            assert_parity(pos, nrm, ref_p[b:b + n], ref_n[b:b + n], "shard %d" % r)


@pytest.mark.parametrize("morphs", ["dense", "sparse"])
def test_variants_library(rzv, scene, morphs):
    s = scene
    mw = weights_of(s, morphs)
    with make_ctx(None, s, morphs, lib=rzv) as c:
        c.set_tuning(geo_lds=1)
        upload_table(c, s)
        c.set_pose(s["world"], mw)
        c.deform()
        check(c, s, morphs, mw, what="variants %s" % morphs)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, scene, tmp_path):
    import test_sdef_cpu as tc
    data, _ = tc.write_sdef_pmx(V=3000, B=40, bone_size=2, seed=7)
    (tmp_path / "m.pmx").write_bytes(data)
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "engine_sdef_e2e.js"), str(tmp_path / "m.pmx"), str(tmp_path)],
                                  timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    ld = lambda n, dt: np.fromfile(str(tmp_path / n), dtype=dt)
    verts = ld("vertices.f32", np.float32).reshape(-1, 8)
    joints = ld("joints.u16", np.uint16).reshape(-1, 4)
    weights = ld("weights.u8", np.uint8).reshape(-1, 4)
    inv = ld("invbind.f32", np.float32).reshape(-1, 16)
    world = ld("world.f32", np.float32).reshape(-1, 16)
    idx = np.array(info["index"], np.uint32)
    c, r0, r1 = (np.array(info[k], np.float32).reshape(-1, 3) for k in ("c", "r0", "r1"))
    assert len(idx) > 500
    for name, table in (("on", idx), ("off", idx[:0])):
        pos = ld("pos_%s.f32" % name, np.float32).reshape(-1, 3)
        nrm = ld("nrm_%s.f32" % name, np.float32).reshape(-1, 3)
        pr, nr = sdef_ref.frame(verts[:, :3], verts[:, 3:6], joints, weights, world, inv, table, c, r0, r1)
        assert_parity(pos, nrm, pr, nr, "node engine sdef %s" % name)
    assert np.abs(ld("pos_on.f32", np.float32) - ld("pos_off.f32", np.float32)).max() > 1e-2
