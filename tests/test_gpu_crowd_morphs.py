"""Crowds with sparse morph targets on the crowd skin kernels ("inst_morphs" = 1; kernels/crowd_morph.hip: the MORPH instantiations of
rz_skin_instances_kernel and rz_skin_instances_fk_kernel), on the scenes of tests/crowd_morph_scenes.py. Everything goes through the C
ABI (ctypes).

Every scene, in every form (inst_subsets 0 / 1 x inst_block 256 / 512, and 1024 once; world poses with fast 0 / 1, uploaded local poses
with fuse_fk -1 / 0): the plan says the crowd kernel walks the rows; every instance's positions and normals are, bit for bit, the frame
of the same context with "inst_morphs" = 0 — the generic kernel, one launch row per instance, which is what every such crowd launched
before the key existed; three replays through deform_n give the same bits; a chosen instance equals that pose and those weights run in a
context of one instance, bit for bit; and all of it sits within helpers.assert_parity's bars (1e-4, the bars of
tests/test_gpu_sparse_pieces.py) of the float64 definition — crowd_morph_scenes.reference64, behind helpers.fk_reference for local poses.
No bar is new. Every test prints the launched form and its worst errors before it asserts (profiles/crowd_morph_edges_parity.txt).

On a library without the key every test here fails at set_tuning(inst_morphs=...): unknown tuning key."""
import numpy as np
import pytest

import crowd_morph_scenes as cms
import motion_ref
from helpers import NRM_TOL, POS_TOL, fk_reference, parity_errors, sample_reference

pytestmark = pytest.mark.gpu

RESET = dict(morph_split=0, fast=-1, out_cap=-1, fuse_fk=-1, graph=0, sparse_piece=0, inst_subsets=-1, inst_block=0, inst_order=1, nt_store=-1)
CHOSEN = 6                      # the instance run alone: second group, neither first nor last of it
_refs = {}


def forms():
    out = []
    for sub in (0, 1):
        for blk in (256, 512):
            out += [("world", dict(inst_subsets=sub, inst_block=blk, fast=0)), ("world", dict(inst_subsets=sub, inst_block=blk, fast=1)),
                    ("local", dict(inst_subsets=sub, inst_block=blk, fuse_fk=-1)), ("local", dict(inst_subsets=sub, inst_block=blk, fuse_fk=0))]
    out += [("world", dict(inst_subsets=1, inst_block=1024, fast=1)), ("local", dict(inst_subsets=1, inst_block=1024, fuse_fk=-1))]
    return out


def worlds64(s):
    """float64 world matrices of the local poses, once"""
    if "worlds64" not in _refs:
        m = s["mesh"]
        _refs["worlds64"] = [fk_reference(m["parents"], m["bind"], m["q"][i]) for i in range(cms.I)]
    return _refs["worlds64"]


def reference(s, kind):
    """[(positions, normals)] per instance in float64, computed once per (scene, pose kind) and left alone"""
    key = (s["name"], kind)
    if key not in _refs:
        _refs[key] = [cms.reference64(s, i, None if kind == "world" else worlds64(s)[i % cms.I]) for i in range(s["I"])]
    return _refs[key]


def make_ctx(lib, s, instances=None, targets=True):
    m = s["mesh"]
    c = lib.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"])
    if targets:
        c.upload_morphs_sparse(s["off"], s["idx"], s["d3"])
    c.set_instances(s["I"] if instances is None else instances)
    c.set_tuning(**dict(RESET, **s["tuning"]))
    return c


def put_pose(c, s, kind, only=None):
    m = s["mesh"]
    pick = [i % cms.I for i in range(s["I"])] if only is None else [only % cms.I]
    mw = s["mw"] if only is None else s["mw"][only:only + 1]
    if kind == "world":
        c.set_pose(m["worlds"][pick], mw)
    else:
        c.set_pose_local(m["q"][pick], mw)


def read_all(c, n):
    return [c.read(i) for i in range(n)]


def same_bits(x, y):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for a, b in zip(x, y) for k in (0, 1))


def worst(outs, refs):
    e = np.zeros(2)
    for (pg, ng), (pr, nr) in zip(outs, refs):
        assert np.isfinite(pg).all() and np.isfinite(ng).all()
        ep, en = parity_errors(pg, ng, pr, nr)
        e = np.maximum(e, [ep.max(), en.max()])
    return e


def launched(c):
    g = c.get_tuning
    return dict(morphs=g("effective_inst_morphs"), group=g("effective_inst_group"), block=g("effective_inst_block"), lds=g("effective_inst_lds"),
                subsets=g("effective_subsets"), fuse_fk=g("effective_fuse_fk"), prep=g("effective_prep"), grid=g("effective_grid"), kernel=c.kernel_name())


@pytest.mark.parametrize("name", cms.NAMES)
def test_every_form_equals_the_generic_frame_bit_for_bit(rz, name):
    s = cms.scene(name)
    G = min(s["tuning"]["inst_loop"], s["I"])
    alone = {}
    with make_ctx(rz, s) as c, make_ctx(rz, s, instances=1) as one:
        for kind, form in forms():
            what = "%s %s %r" % (name, kind, form)
            refs = reference(s, kind)
            c.set_tuning(**dict(RESET, **s["tuning"]))
            c.set_tuning(**form)
            # the frame launched without the key: the generic kernel
            c.set_tuning(inst_morphs=0)
            put_pose(c, s, kind)
            off = launched(c)
            c.deform()
            base = read_all(c, s["I"])
            # the crowd kernel
            c.set_tuning(inst_morphs=1)
            put_pose(c, s, kind)
            on = launched(c)
            c.deform()
            got = read_all(c, s["I"])
            c.deform_n(3)
            again = read_all(c, s["I"])
            if kind not in alone:
                one.set_tuning(inst_morphs=1)
                put_pose(one, s, kind, only=CHOSEN)
                one.deform()
                alone[kind] = [one.read(0)]
            e_on, e_off = worst(got, refs), worst(base, refs)
            print("crowd morphs | %s | %s %s: block %d, G %d, subsets %d, one launch %d, front kernel %d, %d B of LDS, grid %d | positions %.3e normals %.3e"
                  " (bars %.0e / %.0e) | generic frame: positions %.3e normals %.3e"
                  % (name, kind, " ".join("%s=%d" % kv for kv in form.items()), on["block"], on["group"], on["subsets"], on["fuse_fk"], on["prep"], on["lds"],
                     on["grid"], e_on[0], e_on[1], POS_TOL, NRM_TOL, e_off[0], e_off[1]))
            assert off["morphs"] == 0 and off["group"] == 0, (what, off)
            assert on["morphs"] == 1 and on["group"] == G and on["block"] == form["inst_block"] and on["grid"] == cms.RUNS, (what, on)
            assert on["subsets"] == form["inst_subsets"], (what, on)
            assert ("_morph_kernel<%d," % form["inst_block"]) in on["kernel"] and "_morph_" not in off["kernel"], (what, on["kernel"], off["kernel"])
            if kind == "local":         # uploaded local poses: the one-launch front where it has an instantiation, else rz_fk_kernel in front
                fused = form["fuse_fk"] != 0 and form["inst_subsets"] == 1 and form["inst_block"] != 1024
                assert (on["fuse_fk"], on["prep"]) == ((1, 0) if fused else (0, 1)), (what, on)
            else:
                assert on["prep"] == (0 if form["fast"] else 1), (what, on)
            per_bone = (112 if on["subsets"] else 64) if (kind == "world" and form["fast"]) else 48
            if not (kind == "local" and on["fuse_fk"]):
                bones = max(len(x) for x in cms.run_bones()) if on["subsets"] else cms.B
                assert on["lds"] == cms.lds_bytes(G, bones, per_bone, s["M"]), (what, on)
            for i in range(s["I"]):
                assert same_bits(got[i:i + 1], base[i:i + 1]), "%s: instance %d differs from the inst_morphs = 0 frame" % (what, i)
            assert same_bits(got, again), "%s: a replay differs from the first frame" % what
            assert same_bits(got[CHOSEN:CHOSEN + 1], alone[kind]), "%s: instance %d differs from that pose run alone" % (what, CHOSEN)
            assert e_on[0] <= POS_TOL and e_on[1] <= NRM_TOL, (what, e_on)
            assert e_off[0] <= POS_TOL and e_off[1] <= NRM_TOL, (what, e_off)


def test_empty_rows_equal_a_context_without_targets(rz):
    """targets uploaded, every row empty: the bits of the same crowd in a context with no targets at all (the morph-free crowd kernel)"""
    s = cms.scene("empty")
    with make_ctx(rz, s) as c, make_ctx(rz, s, targets=False) as bare:
        for kind, form in forms():
            for ctx in (c, bare):
                ctx.set_tuning(**dict(RESET, **s["tuning"]))
                ctx.set_tuning(**form)
            c.set_tuning(inst_morphs=1)
            put_pose(c, s, kind)
            m = s["mesh"]
            if kind == "world":
                bare.set_pose(m["worlds"])
            else:
                bare.set_pose_local(m["q"])
            assert c.get_tuning("effective_inst_morphs") == 1 and bare.get_tuning("effective_inst_morphs") == 0
            assert bare.get_tuning("effective_inst_group") == cms.G
            c.deform()
            bare.deform()
            assert same_bits(read_all(c, cms.I), read_all(bare, cms.I)), "empty %s %r" % (kind, form)
    print("crowd morphs | empty | every form equals the morph-free crowd of a context without targets, bit for bit")


@pytest.mark.parametrize("block", [256, 512])
def test_a_group_that_does_not_fit_keeps_the_generic_frame(rz, block):
    s = cms.scene("nofit")
    with make_ctx(rz, s) as c:
        c.set_tuning(inst_block=block, inst_morphs=1)
        put_pose(c, s, "world")
        on = launched(c)
        print("crowd morphs | nofit | block %d, inst_loop %d, M %d: effective_inst_morphs %d, inst_group %d" % (block, s["tuning"]["inst_loop"], s["M"], on["morphs"], on["group"]))
        assert on["morphs"] == 0 and on["group"] == 0
        c.deform()
        got = [c.read(i) for i in (0, 7, 63)]
        refs = [cms.reference64(s, i, s["mesh"]["worlds"][i % cms.I]) for i in (0, 7, 63)]
        e = worst(got, refs)
        print("crowd morphs | nofit | positions %.3e normals %.3e (bars %.0e / %.0e)" % (e[0], e[1], POS_TOL, NRM_TOL))
        assert e[0] <= POS_TOL and e[1] <= NRM_TOL
        c.set_tuning(inst_loop=8)           # the same targets in groups of 8: 19 KB of weights fit
        assert c.get_tuning("effective_inst_morphs") == 1 and c.get_tuning("effective_inst_group") == 8
        c.deform()
        assert same_bits(got, [c.read(i) for i in (0, 7, 63)])


def _library(s):
    from reze_engine_amd import synth
    base = synth.make_motion_base(cms.B, seed=77)
    return [synth.make_motion(cms.B, s["M"], seed=78, keyed=0.8, base=base, trans=0.05), synth.make_motion(cms.B, s["M"], seed=79, keyed=0.7, base=base, flip=0.5, n_keys=7, trans=0.05)]


def test_a_blended_pose_whose_clips_key_morph_tracks(rz):
    """two clips with morph tracks: rz_motion_kernel leaves rotations, translations AND morph weights in device memory in front of the
    frame, so the crowd kernel may solve the hierarchy in its own front (one launch behind the motion kernel)"""
    s = cms.scene("face")
    clips = _library(s)
    rng = np.random.default_rng(5)
    states = [(int(rng.integers(0, 2)), float(rng.uniform(-2, 30)), int(rng.integers(0, 2)), float(rng.uniform(0, 30)), float(b))
              for b in np.concatenate([[0.0, 1.0], rng.uniform(0.1, 0.9, size=cms.I - 2)])]
    m = s["mesh"]
    refs = []
    for st in states:
        q, t, w = motion_ref.blend_reference(clips, st, cms.B, s["M"])
        world = fk_reference(m["parents"], m["bind"], q, t)
        p, n, _ = cms.sps.skin64(s, cms.sps.morph64(s, w), world)
        refs.append((p, n))
    cols = list(zip(*states))
    with make_ctx(rz, s) as c:
        c.upload_motions(clips)
        out = {}
        for key in (0, 1):
            c.set_tuning(inst_morphs=key)
            c.set_pose_blended(*cols)
            on = launched(c)
            c.deform()
            out[key] = read_all(c, cms.I)
            if key:
                assert on["morphs"] == 1 and on["group"] == cms.G and on["fuse_fk"] == 1 and on["prep"] == 0, on
                c.deform_n(3)
                assert same_bits(out[1], read_all(c, cms.I))
            else:
                assert on["morphs"] == 0 and on["group"] == 0, on
        e = worst(out[1], refs)
        print("crowd morphs | blended pose, two clips with morph tracks | one launch behind rz_motion_kernel | positions %.3e normals %.3e (bars %.0e / %.0e)" % (e[0], e[1], POS_TOL, NRM_TOL))
        assert same_bits(out[0], out[1])
        assert e[0] <= POS_TOL and e[1] <= NRM_TOL


def test_a_sampled_pose_takes_the_two_launch_form(rz):
    """rz_set_pose_sampled: the morph weights are sampled by rz_fk_kernel, which therefore stays in front of the crowd kernel"""
    s = cms.scene("face")
    clip = _library(s)[0]
    frames = np.linspace(-2.0, 40.0, cms.I).astype(np.float32)
    m = s["mesh"]
    refs = []
    for f in frames:
        q, t, w = sample_reference(clip, float(f), cms.B, s["M"])
        p, n, _ = cms.sps.skin64(s, cms.sps.morph64(s, w), fk_reference(m["parents"], m["bind"], q, t))
        refs.append((p, n))
    with make_ctx(rz, s) as c:
        c.upload_animation(**clip)
        out = {}
        for key in (0, 1):
            c.set_tuning(inst_morphs=key)
            c.set_pose_sampled(frames)
            on = launched(c)
            c.deform()
            out[key] = read_all(c, cms.I)
            assert (on["morphs"], on["group"]) == ((1, cms.G) if key else (0, 0)), on
            if key:
                assert on["fuse_fk"] == 0 and on["prep"] == 1, on
        e = worst(out[1], refs)
        print("crowd morphs | sampled pose | rz_fk_kernel in front | positions %.3e normals %.3e (bars %.0e / %.0e)" % (e[0], e[1], POS_TOL, NRM_TOL))
        assert same_bits(out[0], out[1])
        assert e[0] <= POS_TOL and e[1] <= NRM_TOL


@pytest.mark.parametrize("table", ["sdef", "qdef"])
@pytest.mark.parametrize("kind", ["world", "local"])
def test_the_sdef_and_qdef_passes_behind_the_crowd_frame(rz, table, kind):
    """a table that lists morphed vertices: the pass reads the CSR and the weights from the context and writes, behind the crowd frame,
    what it writes behind the generic one"""
    from reze_engine_amd import synth
    s = cms.scene("face")
    m = s["mesh"]
    with make_ctx(rz, s) as c:
        if table == "sdef":
            t = synth.make_sdef(m, 1.0)
            listed = t["idx"]
            c.upload_sdef(t["idx"], t["c"], t["r0"], t["r1"])
        else:
            listed = synth.make_qdef(m, 0.5)
            c.upload_qdef(listed)
        morphed = np.flatnonzero(s["rows"])
        both = np.intersect1d(listed, morphed)
        assert len(both) > 0 and len(np.setdiff1d(morphed, listed)) > 0
        out = {}
        for key in (0, 1):
            c.set_tuning(inst_morphs=key)
            put_pose(c, s, kind)
            assert c.get_tuning("effective_inst_morphs") == key
            c.deform()
            out[key] = read_all(c, cms.I)
        # the pass did something to a listed, morphed vertex (against the frame without the table, which the first test holds to float64)
        with make_ctx(rz, s) as plain:
            plain.set_tuning(inst_morphs=1)
            put_pose(plain, s, kind)
            plain.deform()
            p0 = plain.read(0)[0]
        moved = np.abs(out[1][0][0][both] - p0[both]).max()
        print("crowd morphs | %s table, %d listed vertices with a row, %s poses: key on equals key off; the pass moves a listed vertex by up to %.3e" % (table, len(both), kind, moved))
        assert same_bits(out[0], out[1])
        assert moved > 0


def test_a_fork_inherits_the_key(rz):
    s = cms.scene("edges")
    with make_ctx(rz, s) as c:
        c.set_tuning(inst_morphs=1)
        put_pose(c, s, "world")
        c.deform()
        want = read_all(c, cms.I)
        f = c.fork()
        try:
            assert f.get_tuning("inst_morphs") == 1
            f.set_instances(cms.I)
            put_pose(f, s, "world")
            assert f.get_tuning("effective_inst_morphs") == 1 and f.get_tuning("effective_inst_group") == cms.G
            f.deform()
            assert same_bits(want, read_all(f, cms.I))
            c.deform_pair(f, 4)
            assert same_bits(want, read_all(f, cms.I)) and same_bits(want, read_all(c, cms.I))
        finally:
            f.close()
    print("crowd morphs | fork: inherits inst_morphs = 1, the same bits, alone and through deform_pair")


def test_the_bounding_box_keeps_the_crowd_on_the_generic_kernel(rz):
    s = cms.scene("scattered")
    with make_ctx(rz, s) as c:
        c.set_tuning(inst_morphs=1)
        put_pose(c, s, "world")
        assert c.get_tuning("effective_inst_morphs") == 1
        c.deform()
        want = read_all(c, cms.I)
        c.enable_aabb(True)
        assert c.get_tuning("effective_inst_morphs") == 0 and c.get_tuning("effective_inst_group") == 0
        c.deform()
        assert same_bits(want, read_all(c, cms.I))
    print("crowd morphs | rz_enable_aabb(1): effective_inst_morphs 0, the generic kernel, the same bits")


def test_the_key_is_refused_outside_its_range_and_off_by_default(rz):
    s = cms.scene("edges")
    with make_ctx(rz, s) as c:
        assert c.get_tuning("inst_morphs") == -1
        put_pose(c, s, "world")
        assert c.get_tuning("effective_inst_morphs") == 0 and c.get_tuning("effective_inst_group") == 0       # auto = off
        for bad in (2, -2):
            with pytest.raises(rz.capi.RzError) as e:
                c.set_tuning(inst_morphs=bad)
            assert "inst_morphs must be" in str(e.value)
        c.set_tuning(inst_morphs=1, inst_loop=0)
        assert c.get_tuning("effective_inst_morphs") == 0           # the crowd kernels switched off
