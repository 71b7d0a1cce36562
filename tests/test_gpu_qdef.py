"""QDEF skinning on the device (rz_upload_qdef, kernels/qdef.hip) against the float64 reference tests/qdef_ref.py, on every frame path.
The scenes are tests/qdef_scenes.py (2 049 vertices, 300 bones, ~600 listed vertices, 9 + 9 morphs, 3 instances). The reference takes the
world matrices the frame used from rz_read_world, so device-solved and sampled poses are held to the same definition. The bar is the
project's (helpers.POS_TOL / NRM_TOL); a vertex whose sign margin (qdef_ref.margin) is under qdef_ref.AMBIGUOUS must meet it against the
reference evaluated with either sign for each slot under the threshold, and such vertices are at most 1 % of a table."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import qdef_ref
import qdef_scenes as qs
import sdef_ref
from helpers import POS_TOL, NRM_TOL, assert_parity, assert_hull, parity_errors
from oracle import rz_oracle_np as onp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, M, I = qs.V, qs.B, qs.M, qs.I


@pytest.fixture(scope="module")
def scene(rz):
    from reze_engine_amd import synth
    return qs.build(synth)


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


def morph_kw(s, morphs, mw):
    if morphs == "dense":
        return dict(dense=s["dense"], weights=mw)
    if morphs == "sparse":
        return dict(sparse=s["sparse"][:3], weights=mw)
    return {}


def hold(pos, nrm, mesh, world16, idx, what, sdef=None, **kw):
    """The listed vertices meet the bar against qdef_ref (ambiguous ones with either sign), every other vertex against the oracle's LBS
    (or sdef_ref for an SDEF table). Returns the float64 reference frame."""
    m = mesh
    idx = np.asarray(idx, dtype=np.int64)
    pr, nr = qdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], world16, m["inv_bind"], idx, **kw)
    if sdef is not None:
        ps, ns = sdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], world16, m["inv_bind"], sdef["idx"], sdef["c"], sdef["r0"], sdef["r1"], **kw)
        si = sdef["idx"].astype(np.int64)
        pr[si], nr[si] = ps[si], ns[si]
    assert np.isfinite(pos).all() and np.isfinite(nrm).all(), "NaN/Inf in GPU output " + what
    skin16 = onp.palette(world16, m["inv_bind"])
    dots, on = qdef_ref.pivot_dots(m["joints"], m["weights"], skin16, idx)
    close = on & (np.abs(dots) < qdef_ref.AMBIGUOUS)
    amb = np.flatnonzero(close.any(axis=1))
    assert len(amb) <= 0.01 * len(idx), "%s: %d of %d listed vertices are ambiguous" % (what, len(amb), len(idx))
    sure = np.ones(len(pos), dtype=bool)
    sure[idx[amb]] = False
    ep, en = assert_parity(pos[sure], nrm[sure], pr[sure], nr[sure], what)
    print("%s: position error %.3e, normal error %.3e, %d ambiguous of %d" % (what, ep, en, len(amb), len(idx)))
    pm = sdef_ref.morphed(m["pos"], kw.get("dense"), kw.get("sparse"), kw.get("weights"))
    for a in amb:                                           # either sign for each slot under the threshold
        slots = np.flatnonzero(close[a])
        best = np.inf
        for bits in itertools.product([False, True], repeat=len(slots)):
            flip = np.zeros((1, 4), dtype=bool)
            flip[0, slots] = bits
            p1, n1 = qdef_ref.qdef(pm, m["nrm"], m["joints"], m["weights"], skin16, idx[a:a + 1], flip)
            e1, e2 = parity_errors(pos[idx[a:a + 1]], nrm[idx[a:a + 1]], p1, n1)
            best = min(best, max(e1[0] / POS_TOL, e2[0] / NRM_TOL))
        assert best <= 1.0, "%s: ambiguous vertex %d misses the bar with every sign (%.3e x the tolerance)" % (what, idx[a], best)
    return pr, nr


def check(c, s, morphs, mw, inst=0, what="", idx=None, sdef=None):
    pos, nrm = c.read(inst)
    hold(pos, nrm, s["mesh"], c.read_world(inst), s["idx"] if idx is None else idx, what, sdef=sdef, **morph_kw(s, morphs, mw))
    return pos, nrm


def test_parity_no_leak_and_lifecycle(rz, scene):
    s = scene
    idx = s["idx"].astype(np.int64)
    assert 0 in idx and V - 1 in idx and len(idx) % 256 != 0
    with make_ctx(rz, s, "dense") as c:
        assert c.get_tuning("qdef_verts") == 0
        c.set_pose(s["world"], s["mw"])
        c.deform()
        p0, n0 = c.read()                                    # BDEF4 for everything
        c.upload_qdef(s["idx"])
        assert c.get_tuning("qdef_verts") == len(idx)
        c.deform()
        p1, n1 = check(c, s, "dense", s["mw"], what="dense world")
        other = np.setdiff1d(np.arange(V), idx)
        assert np.array_equal(p1[other], p0[other]) and np.array_equal(n1[other], n0[other])
        assert np.abs(p1[idx] - p0[idx]).max() > 1e-2
        c.upload_qdef([])                                    # removing the table restores the BDEF4 bits
        assert c.get_tuning("qdef_verts") == 0
        c.deform()
        p2, n2 = c.read()
        assert np.array_equal(p2, p0) and np.array_equal(n2, n0)
        # invalid tables are refused with a message and leave the context usable
        c.upload_qdef(s["idx"])
        bad = s["idx"].copy()
        bad[[3, 4]] = bad[[4, 3]]
        for ix in (bad, np.concatenate([s["idx"][:-1], [V]]).astype(np.uint32)):
            with pytest.raises(rz.RzError) as e:
                c.upload_qdef(ix)
            assert e.value.code == -1 and ("ascending" in str(e.value) or "outside" in str(e.value))
        assert c._L.rz_upload_qdef(c._h, 5, None) == -1
        assert b"null" in c._L.rz_last_error()
        # a vertex has one weight type: whichever upload comes second is refused
        one = dict(idx=s["idx"][5:6], c=np.zeros((1, 3), np.float32), r0=np.zeros((1, 3), np.float32), r1=np.zeros((1, 3), np.float32))
        with pytest.raises(rz.RzError) as e:
            c.upload_sdef(one["idx"], one["c"], one["r0"], one["r1"])
        assert e.value.code == -1 and "QDEF table" in str(e.value)
        assert c.get_tuning("sdef_verts") == 0 and c.get_tuning("qdef_verts") == len(idx)
        c.upload_qdef([])
        c.upload_sdef(one["idx"], one["c"], one["r0"], one["r1"])
        with pytest.raises(rz.RzError) as e:
            c.upload_qdef(s["idx"])
        assert e.value.code == -1 and "SDEF table" in str(e.value)
        assert c.get_tuning("qdef_verts") == 0
        c.upload_sdef([], [], [], [])
        c.upload_qdef(s["idx"])
        c.deform()
        check(c, s, "dense", s["mw"], what="after refused uploads")
        # a new mesh drops the table
        m = s["mesh"]
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        assert c.get_tuning("qdef_verts") == 0


@pytest.mark.parametrize("morphs", ["none", "dense", "sparse"])
def test_world_local_and_sampled_poses(rz, scene, morphs):
    s = scene
    mw = weights_of(s, morphs)
    with make_ctx(rz, s, morphs, topology=True) as c:
        c.upload_qdef(s["idx"])
        for k in range(2):                                   # first frame of a pose, then a replay of it
            if k == 0:
                c.set_pose(s["world"], mw)
            c.deform()
            check(c, s, morphs, mw, what="world %s frame %d" % (morphs, k))
        for fuse in (0, 1):
            c.set_tuning(fuse_fk=fuse)
            c.set_pose_local(s["quats"], mw)
            c.deform()
            check(c, s, morphs, mw, what="local %s fuse=%d" % (morphs, fuse))
        nk = 2
        kq = np.stack([s["quats"], s["key1"]], axis=1)
        c.upload_animation(np.arange(B), np.arange(B + 1) * nk, np.tile(np.arange(nk) * 10.0, B), kq, np.zeros((B, nk, 3), np.float32))
        for fuse in (0, 1):
            c.set_tuning(fuse_fk=fuse)
            c.set_pose_sampled([s["sample_t"]])
            c.deform()
            check(c, s, morphs, None if morphs == "none" else np.zeros(M, np.float32), what="sampled %s fuse=%d" % (morphs, fuse))


@pytest.mark.parametrize("morphs", ["dense", "sparse"])
def test_prep_kernel_frame(rz, scene, morphs):
    s = scene
    mw = weights_of(s, morphs)
    with make_ctx(rz, s, morphs) as c:
        c.set_tuning(fast=0, zero_copy=0)
        assert c.get_tuning("effective_prep") == 1
        c.upload_qdef(s["idx"])
        c.set_pose(s["world"], mw)
        c.deform()
        check(c, s, morphs, mw, what="prep-kernel frame %s" % morphs)


def test_graph_replay_equals_plain_launches(rz, scene):
    s = scene
    with make_ctx(rz, s, "dense") as c:
        c.upload_qdef(s["idx"])
        c.set_pose(s["world"], s["mw"])
        c.deform_n(32)
        p0, n0 = check(c, s, "dense", s["mw"], what="plain launches")
        c.set_tuning(graph=1)
        c.deform_n(32)
        p1, n1 = c.read()
        assert np.array_equal(p1, p0) and np.array_equal(n1, n0)
        half = s["idx"][::2]                                # a changed table drops the captured graph
        c.upload_qdef(half)
        c.deform_n(32)
        check(c, s, "dense", s["mw"], what="graph after a changed table", idx=half)
        c.set_tuning(qdef_chunks=4)                          # several chunks per workgroup: the same bits
        c.upload_qdef(s["idx"])
        c.deform_n(32)
        p2, n2 = c.read()
        assert np.array_equal(p2, p0) and np.array_equal(n2, n0)
        c.time_frames(20)                                   # rz_time_frames leaves the QDEF frame behind
        p3, _ = c.read()
        assert np.array_equal(p3, p0)


@pytest.mark.parametrize("morphs", ["dense", "sparse"])
def test_variants_library(rzv, scene, morphs):
    s = scene
    mw = weights_of(s, morphs)
    with make_ctx(None, s, morphs, lib=rzv) as c:
        c.set_tuning(geo_lds=1)
        c.upload_qdef(s["idx"])
        c.set_pose(s["world"], mw)
        c.deform()
        check(c, s, morphs, mw, what="variants %s" % morphs)


@pytest.mark.parametrize("form", ["whole", "subsets", "subfk", "dense"])
def test_crowds(rz, scene, form):
    """Every instance meets the bar and has the bits of that pose run alone."""
    s = scene
    nk = 2
    kq = np.stack([s["cq"][0], s["cq"][1]], axis=1)
    anim = (np.arange(B), np.arange(B + 1) * nk, np.tile(np.arange(nk) * 10.0, B), kq, np.zeros((B, nk, 3), np.float32))
    morphs = "dense" if form == "dense" else "none"
    with make_ctx(rz, s, morphs, topology=(form == "subfk")) as c:
        mw = np.stack([s["mw"] * (i + 1) / I for i in range(I)]).astype(np.float32) if morphs == "dense" else None
        c.set_instances(I)
        if form == "whole":
            c.set_tuning(inst_subsets=0)
        c.upload_qdef(s["idx"])
        if form == "subfk":
            c.upload_animation(*anim)
            c.set_pose_sampled(s["crowd_t"])
        else:
            c.set_pose(s["cworld"], mw)
        # the form each case is about: the whole palette, the bone-subset skin kernel (palette_stale), the one-launch device-animated crowd
        # (fk_stale) — the last two leave no palette in memory, so the pass runs the palette kernel their flag names first; and, with dense
        # morphs, the generic kernel per instance behind rz_prep_kernel (the pass reads the ring slot's active lists)
        assert (c.get_tuning("effective_inst_group") > 0) == (form != "dense")
        if form != "dense":
            assert c.get_tuning("effective_subsets") == (0 if form == "whole" else 1)
            assert (c.get_tuning("effective_closure_bones") > 0) == (form == "subfk")
        c.deform()
        got = []
        for i in range(I):
            got.append(check(c, s, morphs, None if mw is None else mw[i], inst=i, what="crowd %s instance %d" % (form, i)))
    with make_ctx(rz, s, morphs, topology=(form == "subfk")) as c:
        c.upload_qdef(s["idx"])
        if form == "subfk":
            c.upload_animation(*anim)
        idx = s["idx"].astype(np.int64)
        for i in range(I):
            if form == "subfk":
                c.set_pose_sampled([s["crowd_t"][i]])
            else:
                c.set_pose(s["cworld"][i], None if mw is None else mw[i])
            c.deform()
            pos, nrm = c.read()
            assert np.array_equal(pos[idx], got[i][0][idx]) and np.array_equal(nrm[idx], got[i][1][idx]), "crowd %s instance %d differs from the pose run alone" % (form, i)


def test_hull_and_aabb(rz, scene):
    s = scene
    edge = np.random.default_rng(3).uniform(0, 1.5, V).astype(np.float32)
    with make_ctx(rz, s, "sparse") as c:
        mw = s["sparse"][3]
        c.upload_edge_scale(edge)
        c.enable_aabb(True)
        c.set_pose(s["world"], mw)
        c.deform()
        pb, _ = c.read()                                    # BDEF4 positions of every vertex
        c.upload_qdef(s["idx"])
        idx = s["idx"].astype(np.int64)
        for _ in range(3):                                  # both box slots
            c.deform()
            pos, nrm = c.read()
            pr, nr = hold(pos, nrm, s["mesh"], c.read_world(0), idx, "hull / aabb", **morph_kw(s, "sparse", mw))
            # the hull follows the device's own position and normal: hold it where the frame itself is unambiguous
            amb = qdef_ref.margin(s["mesh"]["joints"], s["mesh"]["weights"], onp.palette(c.read_world(0), s["mesh"]["inv_bind"]), idx) < qdef_ref.AMBIGUOUS
            sure = np.ones(V, dtype=bool)
            sure[idx[amb]] = False
            hull = c.read_hull(0)
            assert_hull(hull[sure], (pr + nr * edge[:, None].astype(np.float64) * 0.01)[sure], "hull")
            assert_hull(hull[~sure], (pos.astype(np.float64) + nrm.astype(np.float64) * edge[:, None] * 0.01)[~sure], "hull of ambiguous vertices")
            box = c.read_aabb(0)
            allp = np.concatenate([pos, pb[idx]])
            assert np.all(box[:3] <= pos.min(axis=0)) and np.all(box[3:] >= pos.max(axis=0))
            assert np.array_equal(box[:3], allp.min(axis=0)) and np.array_equal(box[3:], allp.max(axis=0))


def test_two_shards_and_a_fork(rz, scene):
    s = scene
    m = s["mesh"]
    with make_ctx(rz, s, "dense") as c:
        c.upload_qdef(s["idx"])
        c.set_pose(s["world"], s["mw"])
        c.deform()
        whole_p, whole_n = check(c, s, "dense", s["mw"], what="whole mesh")
        # a fork borrows the table; uploads are refused while it exists; fork and lender alternate
        f = c.fork()
        with pytest.raises(rz.RzError):
            c.upload_qdef([])
        assert f.get_tuning("qdef_verts") == len(s["idx"])
        f.set_pose(s["cworld"][1], s["mw"] * 0.5)
        c.deform_pair(f, 4)
        pf, nf = f.read()
        hold(pf, nf, m, f.read_world(0), s["idx"], "fork", dense=s["dense"], weights=s["mw"] * 0.5)
        pl, nl = c.read()
        assert np.array_equal(pl, whole_p) and np.array_equal(nl, whole_n)
        f.close()
        c.upload_qdef(s["idx"][:10])
    for r in range(2):
        b, n = rz.shard_range(V, 2, r)
        with rz.DeformContext(0) as c:
            c.upload_mesh(m["pos"][b:b + n], m["nrm"][b:b + n], m["joints"][b:b + n], m["weights"][b:b + n])
            c.upload_skeleton(m["inv_bind"])
            c.upload_morphs_dense(s["dense"][:, b:b + n])
            sel = (s["idx"] >= b) & (s["idx"] < b + n)
            assert sel.sum() > 100
            c.upload_qdef(s["idx"][sel] - b)
            c.set_pose(s["world"], s["mw"])
            c.deform()
            pos, nrm = c.read()
            assert np.array_equal(pos, whole_p[b:b + n]) and np.array_equal(nrm, whole_n[b:b + n]), "shard %d" % r


def test_sdef_and_qdef_together(rz, scene):
    s = scene
    sd = s["synth"].make_sdef(s["mesh"], 0.2, seed=9)
    keep = ~np.isin(sd["idx"], s["idx"])
    sd = {k: v[keep] for k, v in sd.items()}
    assert len(sd["idx"]) > 100
    edge = np.random.default_rng(4).uniform(0, 1.5, V).astype(np.float32)
    for first in ("sdef", "qdef"):
        with make_ctx(rz, s, "dense") as c:
            c.upload_edge_scale(edge)
            c.enable_aabb(True)
            if first == "sdef":
                c.upload_sdef(sd["idx"], sd["c"], sd["r0"], sd["r1"])
                c.upload_qdef(s["idx"])
            else:
                c.upload_qdef(s["idx"])
                c.upload_sdef(sd["idx"], sd["c"], sd["r0"], sd["r1"])
            c.set_pose(s["world"], s["mw"])
            c.deform()
            pos, _ = check(c, s, "dense", s["mw"], what="both tables, %s first" % first, sdef=sd)
            box = c.read_aabb(0)
            assert np.all(box[:3] <= pos.min(axis=0)) and np.all(box[3:] >= pos.max(axis=0))
            c.upload_qdef([])                                # one table goes, the other stays
            c.deform()
            p1, n1 = c.read()
            m = s["mesh"]
            pr, nr = sdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], c.read_world(0), m["inv_bind"], sd["idx"], sd["c"], sd["r0"], sd["r1"],
                                    dense=s["dense"], weights=s["mw"])
            assert_parity(p1, n1, pr, nr, "SDEF alone again")


def test_extremes(rz, scene):
    s = scene
    from reze_engine_amd import synth
    with make_ctx(rz, s, "dense") as c:                      # n = 1, n = V
        c.set_pose(s["world"], s["mw"])
        for ix in (s["idx"][7:8], np.arange(V, dtype=np.uint32)):
            c.upload_qdef(ix)
            c.deform()
            check(c, s, "dense", s["mw"], what="n = %d" % len(ix), idx=ix)
    for name, t in (("B = 1", qs.one_bone(synth)), ("B = 3242", qs.big_skeleton(synth))):
        m = t["mesh"]
        with rz.DeformContext(0) as c:
            c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
            c.upload_skeleton(m["inv_bind"])
            c.upload_qdef(t["idx"])
            c.set_pose(t["world"])
            c.deform()
            pos, nrm = c.read()
            hold(pos, nrm, m, c.read_world(0), t["idx"], name)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, scene, tmp_path):
    import test_qdef_cpu as tc
    data, _ = tc.write_qdef_pmx(V=3000, B=40, bone_size=2, seed=7)
    (tmp_path / "m.pmx").write_bytes(data)
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "qdef_e2e.js"), str(tmp_path / "m.pmx"), str(tmp_path)], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    ld = lambda n, dt: np.fromfile(str(tmp_path / n), dtype=dt)      # noqa: E731
    verts = ld("vertices.f32", np.float32).reshape(-1, 8)
    mesh = dict(pos=verts[:, :3], nrm=verts[:, 3:6], joints=ld("joints.u16", np.uint16).reshape(-1, 4), weights=ld("weights.u8", np.uint8).reshape(-1, 4),
                inv_bind=ld("invbind.f32", np.float32).reshape(-1, 16))
    world = ld("world.f32", np.float32).reshape(-1, 16)
    idx = np.array(info["index"], np.uint32)
    assert len(idx) > 500
    for name, table in (("on", idx), ("off", idx[:0])):
        pos = ld("pos_%s.f32" % name, np.float32).reshape(-1, 3)
        nrm = ld("nrm_%s.f32" % name, np.float32).reshape(-1, 3)
        hold(pos, nrm, mesh, world, table, "node engine qdef %s" % name)
    assert np.abs(ld("pos_on.f32", np.float32) - ld("pos_off.f32", np.float32)).max() > 1e-2
