"""PMX after-physics bones solved again behind the overrides on the device (rz_upload_after_physics; kernels/after.hip:
rz_fk_after_kernel) against the float64 definition tests/after_ref.py, on the hand-laid scenes of tests/after_scenes.py.

Bars: world matrices within 5e-5 x max(1, |ref|) of the definition in float64 — the project's bar for world matrices
(tests/test_gpu_follow.py, tests/test_gpu_layers.py); positions and normals of the scene's mesh, which has vertices on every listed
bone, within the layers test's 2e-4 of the oracle on the reference matrices. tests/test_after_cpu.py holds the float32 run of the
definition to a quarter of the world bar on every scene used here. Every parity test prints its worst errors before it asserts; the
maxima per scene go to profiles/after_edges_parity.txt."""
import numpy as np
import pytest

import after_ref as ar
import after_scenes as asc
import physics_gpu as pg

pytestmark = pytest.mark.gpu
W_BAR, P_BAR = 5e-5, 2e-4
ORDER = list(asc.STATIC) + ["c follow"] + ["h " + k for k in asc.SOURCES] + ["j I=1", "j I=3"]
HEAD = ("rz_upload_after_physics against tests/after_ref.py in float64 (tests/test_gpu_after.py): per scene the largest world-matrix error over\n"
        "max(1, |ref|) (bar %.0e), position error over max(1, |p|) and normal error (bar %.0e), with the list and the overrides resident" % (W_BAR, P_BAR))
_rows = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))


def make_ctx(rz, sc, instances=None, after=True, follow=False, chains=True):
    m = sc["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"], sc["ap"], sc["ratio"], sc["move"])
    n = len(sc["instances"]) if instances is None else instances
    if n > 1:
        c.set_instances(n)
    if sc["chains"] and chains:
        c.upload_ik(sc["chains"])
    if follow:
        c.override_follow(True)
    if after:
        c.upload_after_physics(sc["order"])
    return c


def override(c, insts):
    bones = np.concatenate([x["bones"] for x in insts])
    mats = np.concatenate([x["mats"] for x in insts])
    which = np.concatenate([np.full(len(x["bones"]), k, dtype=np.uint32) for k, x in enumerate(insts)])
    c.override_world(bones, mats, instances=which)


def feed(c, insts):
    """the local poses and the override sets of `insts`, as instances 0 .. of the context"""
    c.set_pose_local(np.stack([x["q"] for x in insts]).astype(np.float32), None, np.stack([x["t"] for x in insts]).astype(np.float32))
    override(c, insts)


def frame_of(c, i=0):
    return (c.read_world(i),) + tuple(c.read(i))


def errors(c, oracle, sc, i, ref):
    """(world, position, normal) errors of instance i of the frame that has run against the reference world matrices"""
    m = sc["mesh"]
    wg = c.read_world(i)
    pg_, ng = c.read(i)
    assert np.isfinite(wg).all() and np.isfinite(pg_).all() and np.isfinite(ng).all()
    ew = float(np.abs(wg - ref).max()) / max(1.0, float(np.abs(ref).max()))
    pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], ref.astype(np.float32), m["inv_bind"])
    ep = float((np.linalg.norm(pg_ - pr, axis=1) / np.maximum(np.linalg.norm(pr, axis=1), 1.0)).max())
    en = float(np.linalg.norm(ng - nr, axis=1).max())
    return ew, ep, en


def hold(name, errs, entries, levels):
    worst = np.array(errs).reshape(-1, 3).max(axis=0)
    line = "(%s) world %.2e positions %.2e normals %.2e  [%d entries in %d levels]" % ((name,) + tuple(worst) + (entries, levels))
    print(line)
    _rows[name] = line
    pg.write_parity("after_edges_parity.txt", HEAD, ORDER, _rows)
    assert worst[0] <= W_BAR and worst[1] <= P_BAR and worst[2] <= P_BAR, line


def levels_of(sc):
    return max(ar.levels(sc["parents"], sc["ap"], sc["ratio"], sc["order"])) + 1


@pytest.mark.parametrize("name", list(asc.STATIC))
def test_scene_against_the_definition(rz, oracle, name):
    """fails without the feature (the symbol is absent). Every hand-fed scene, all its instances in one crowd: world matrices, positions
    and normals at the bars, the tuning keys the definition's counts, and the listed bones moved — the frame without the stage is off the
    reference by far more than the bar"""
    sc = asc.scene(name)
    insts = sc["instances"]
    with make_ctx(rz, sc) as c:
        assert c.get_tuning("after_physics") == len(sc["order"]) and c.get_tuning("after_physics_levels") == levels_of(sc)
        feed(c, insts)
        c.deform()
        errs, off = [], 0.0
        for i, x in enumerate(insts):
            ref = asc.reference(sc, x)
            errs.append(errors(c, oracle, sc, i, ref))
            off = max(off, float(np.abs(ref - asc.frame_without(sc, x))[sc["order"]].max()))
    assert off > 0.1, "the scene's listed bones do not move"
    hold(name, errs, len(sc["order"]), levels_of(sc))


def test_listed_bones_below_an_override_with_and_without_follow(rz, oracle):
    """(c): with rz_override_follow on, the listed bones below the overridden bone come out of the follow stage first and are evaluated
    again through their own local transforms; both runs sit within the bar of the same reference"""
    sc = asc.scene("c")
    x = sc["instances"][0]
    ref = asc.reference(sc, x)
    assert float(np.abs(asc.reference(sc, x, follow=True) - ref).max()) < 1e-12
    with make_ctx(rz, sc, follow=True) as c:
        assert c.get_tuning("override_follow") == 1
        feed(c, [x])
        assert c.get_tuning("override_followers") > 0
        c.deform()
        hold("c follow", [errors(c, oracle, sc, 0, ref)], len(sc["order"]), levels_of(sc))


@pytest.mark.parametrize("kind", asc.SOURCES)
def test_pose_sources(rz, oracle, kind):
    """(h): the listed bone's local pose comes from a bone morph on top of an uploaded pose (weights where the solve read them), is
    sampled again from its key record under rz_set_pose_sampled, and is read from the resident pose rz_set_pose_blended left"""
    sc, ex, x = asc.source_case(kind)
    with make_ctx(rz, sc, instances=1) as c:
        if kind == "bone morph":
            bm = ex["bm"]
            c.upload_morphs_sparse(np.zeros(len(ex["mw"]) + 1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32))
            c.upload_bone_morphs(bm["morph"], bm["bone"], bm["t"], bm["q"])
            c.set_pose_local(ex["q0"][None], ex["mw"][None], ex["t0"][None])
        elif kind == "sampled":
            c.upload_animation(**ex["clips"][0])
            c.set_pose_sampled([asc.H_FRAME])
        else:
            c.upload_motions(ex["clips"])
            a, fa, b, fb, bl = asc.H_STATE
            c.set_pose_blended([a], [fa], [b], [fb], [bl])
        override(c, [x])
        c.deform()
        ref = asc.reference(sc, x)
        assert float(np.abs(ref - asc.frame_without(sc, x))[sc["order"]].max()) > 0.1
        hold("h " + kind, [errors(c, oracle, sc, 0, ref)], len(sc["order"]), levels_of(sc))


@pytest.mark.parametrize("I", [1, 3])
def test_physics_helpers_see_the_simulated_bones(rz, oracle, I):
    """(j): rz_physics_step(3) then a frame: the helpers append from the dynamic bones where the step put them"""
    sc = asc.scene("j")
    poses = [asc.physics_pose(sc, i) for i in range(I)]
    with make_ctx(rz, sc, instances=I) as c:
        c.upload_physics(sc["table"])
        pg.set_local(c, poses)
        c.physics_step(asc.SUBSTEPS)
        c.deform()
        errs, off = [], 0.0
        for i in range(I):
            F, W, _ = asc.physics_reference(sc, poses[i])
            errs.append(errors(c, oracle, sc, i, W))
            off = max(off, float(np.abs(W - F)[sc["order"]].max()))
    assert off > 0.1
    hold("j I=%d" % I, errs, len(sc["order"]), levels_of(sc))


def test_unchanged_frames_and_tuning_keys(rz):
    """a resident list without any override is bit-identical to no list; n = 0 after n > 0 gives the bits of a context that never had a
    list; the tuning keys report entries and levels"""
    sc = asc.scene("d")
    x = sc["instances"][0]

    def plain(c):
        c.set_pose_local(x["q"][None], None, x["t"][None])
        c.override_world(np.zeros(0, np.uint32), np.zeros((0, 16), np.float32))
        c.deform()
        return frame_of(c)

    def fed(c):
        feed(c, [x])
        c.deform()
        return frame_of(c)
    with make_ctx(rz, sc, after=False) as c:
        assert c.get_tuning("after_physics") == 0 and c.get_tuning("after_physics_levels") == 0
        never = [plain(c), fed(c)]
    with make_ctx(rz, sc) as c:
        assert (c.get_tuning("after_physics"), c.get_tuning("after_physics_levels")) == (4, 3)
        assert same(plain(c), never[0]), "a resident list without overrides"
        on = fed(c)
        assert not same(on, never[1])
        c.upload_after_physics([])
        assert (c.get_tuning("after_physics"), c.get_tuning("after_physics_levels")) == (0, 0)
        assert same((c.read_world(0),), never[1][:1]), "rz_read_world after the list went, the set still resident"
        c.deform()
        assert same(frame_of(c), never[1]), "n = 0 with the set still resident"
        assert same(fed(c), never[1]) and same(plain(c), never[0])
        c.upload_after_physics(sc["order"])
        assert same(fed(c), on)


def test_replays_fork_and_read_back(rz):
    """rz_deform_n(3) and a graph replay carry the stage: the bits of live frames; a fork inherits the list and produces the lender's
    bits; rz_read_world returns the staged matrices, also when it has to solve on demand; an instance of the crowd (e) equals the same
    instance run alone"""
    sc = asc.scene("e")
    insts = sc["instances"]
    with make_ctx(rz, sc) as c:
        feed(c, insts)
        c.deform()
        crowd = [frame_of(c, i) for i in range(len(insts))]
    x = insts[2]
    with make_ctx(rz, sc, instances=1) as c:
        feed(c, [x])
        for _ in range(3):
            c.deform()
        alone = frame_of(c)
        # the list goes and comes back with the set resident: the matrices in memory are the other setting's, the read solves on demand
        c.upload_after_physics([])
        assert not np.array_equal(bits(c.read_world(0)), bits(alone[0]))
        c.upload_after_physics(sc["order"])
        assert np.array_equal(bits(c.read_world(0)), bits(alone[0])), "rz_read_world solving on demand, through the stage"
        assert same(alone, crowd[2]), "instance 2 alone differs from the crowd's"
        assert float(np.abs(alone[0] - asc.reference(sc, x)).max()) < 1e-3
        c.deform_n(3)
        assert same(frame_of(c), alone), "rz_deform_n"
        c.set_tuning(graph=1)
        c.deform_n(40)                  # (a graph replay: 16 captured frames at a time)
        assert same(frame_of(c), alone), "graph replay"
        c.set_tuning(graph=0)
        f = c.fork()
        try:
            assert f.get_tuning("after_physics") == 2 and f.get_tuning("after_physics_levels") == 2
            feed(f, [x])
            f.deform()
            assert same(frame_of(f), alone), "the fork's frame"
            with pytest.raises(rz.capi.RzError):
                c.upload_after_physics([])              # static data is locked while a fork borrows it
        finally:
            f.close()


def test_refusals(rz):
    sc = asc.scene("i")
    m = sc["mesh"]

    def refused(fn, *words, code=-1):           # RZ_ERR_INVALID unless said otherwise
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert e.value.code == code, (e.value.code, str(e.value))
        return e.value
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        refused(lambda: c.upload_after_physics([9]), "rz_upload_skeleton_topology")
        c.upload_skeleton_topology(m["parents"], m["bind"], sc["ap"], sc["ratio"], sc["move"])
        refused(lambda: c.upload_after_physics([9, 11]), "bone 11 of 11")
        refused(lambda: c.upload_after_physics([9, 10, 9]), "bone 9", "twice")
        # bone 7 hangs below bone 6: its parent listed later
        refused(lambda: c.upload_after_physics([7, 6]), "bone 7", "parent, bone 6")
        assert c.get_tuning("after_physics") == 0
        # the IK table first, then a list that names a link (3), the effector (4), a path bone
        c.upload_ik(sc["chains"])
        for b in (2, 3, 4):
            e = refused(lambda: c.upload_after_physics([b, 9]), "bone %d" % b, "IK", code=-6)      # RZ_ERR_UNSUPPORTED
            assert "rz_upload_after_physics" in str(e)
        c.upload_after_physics([5, 9, 10])              # the goal may be listed
        assert c.get_tuning("after_physics") == 3
        # ... and the list first, then the table
        c.upload_ik([])
        c.upload_after_physics([3, 9])
        e = refused(lambda: c.upload_ik(sc["chains"]), "bone 3", "after-physics", code=-6)
        assert c.get_tuning("ik_chains") == 0 and c.get_tuning("after_physics") == 2
        c.upload_after_physics([9, 10])
        c.upload_ik(sc["chains"])
        # a new topology clears the list
        c.upload_skeleton_topology(m["parents"], m["bind"], sc["ap"], sc["ratio"], sc["move"])
        assert c.get_tuning("after_physics") == 0 and c.get_tuning("after_physics_levels") == 0
    # append parent and append parent's parent listed later: scene (d)'s bone 1 appends from 4; scene (a)'s bone 5 appends from 3, whose parent is 2
    for name, order, words in (("d", [1, 4], ("bone 1", "append parent, bone 4")), ("a", [5, 2], ("bone 5", "append parent's parent, bone 2"))):
        s2 = asc.scene(name)
        with make_ctx(rz, s2, after=False) as c:
            refused(lambda: c.upload_after_physics(order), *words)


@pytest.mark.skipif(__import__("shutil").which("node") is None, reason="node is not installed")
def test_through_node_equals_the_ctypes_path(rz, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, afterPhysics: true }) on the synthetic PMX of (j): the loader's flags and
    levels, Model.afterPhysicsOrder, the N-API call and the engine's upload order give, frame for frame, the bits of the same frames driven
    through ctypes with the table the loader must derive; without the option the listed bones stay where the first solve put them"""
    import json
    import os
    import subprocess
    import physics_scenes as ps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sc = asc.scene("j node")
    data, want = asc.write_pmx(sc)
    q, _ = ps.pose(sc, 70, amount=2.0)
    (tmp_path / "j.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(root, "tests", "js", "after_e2e.js"), str(tmp_path / "j.pmx"), str(tmp_path / "q.f32"), str(tmp_path)]
                                  + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    assert info["order"] == [int(b) for b in sc["order"]]
    assert info["on"] == [len(sc["order"]), levels_of(sc)] and info["off"] == [0, 0]
    calls = ps.node_substeps()
    n, B = len(calls), sc["B"]
    on = np.fromfile(str(tmp_path / "world_on.f32"), dtype=np.float32).reshape(n, B, 16)
    off = np.fromfile(str(tmp_path / "world_off.f32"), dtype=np.float32).reshape(n, B, 16)
    worst = 0.0
    # the skeleton as the loader derives it: a PMX stores absolute bone positions in float32, the bind translations are their differences
    # (taken in doubles, uploaded as float32) — up to an ulp off the scene's own
    bp = __import__("ik_ref").bind_positions(sc["parents"], sc["bind"]).astype(np.float32).astype(np.float64)
    bind = np.array([bp[b] - (bp[p] if p >= 0 else 0.0) for b, p in enumerate(sc["parents"])]).astype(np.float32)
    with make_ctx(rz, dict(sc, table=want, mesh=dict(sc["mesh"], bind=bind)), instances=1) as c:
        c.upload_physics(want)
        for k, steps in enumerate(calls):
            c.set_pose_local(q[None], None, None)
            c.physics_step(steps)
            c.deform()
            w = c.read_world(0)
            worst = max(worst, float(np.abs(w - on[k]).max()))
            assert np.array_equal(bits(w), bits(on[k])), "frame %d: the Node engine's world matrices differ from the ctypes path's by %.3e" % (k, worst)
    listed = [int(b) for b in sc["order"]]
    rest = [b for b in range(B) if b not in listed]
    moved = float(np.abs(on[-1][listed] - off[-1][listed]).max())
    print("node engine, %d frames / %d substeps: bit-identical to the ctypes path; the listed bones moved %.4f against the engine without afterPhysics" % (n, sum(calls), moved))
    assert np.array_equal(bits(on[:, rest]), bits(off[:, rest])) and moved > 1e-3
