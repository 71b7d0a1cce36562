"""Rigid-body physics on the device (rz_upload_physics / rz_physics_step, kernels/physics.hip) against the float64 definition
tests/physics_ref.py, through every pose source that can carry it.

The bar is that of tests/test_gpu_ik.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent of
the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every scene used here is checked for
conditioning on the CPU (tests/test_physics_cpu.py). Every test prints its largest error before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref
import physics_ref
import physics_scenes as ps
from helpers import NRM_TOL, sample_reference
from physics_gpu import BAR, assert_bar, errors, make_ctx, set_local

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["one body", "63 bodies", "65 bodies", "wide colour", "skirt", "one joint"])
def test_body_and_joint_counts(rz, oracle, name):
    """1, 10 and 3 x 10 substeps over five calls, the pose changing between calls: the state persists across calls"""
    sc = ps.scene(name)
    poses = [ps.pose(sc, k) for k in range(len(ps.CALLS))]
    ref = ps.run_reference(sc, poses)
    _, _, ncol = physics_ref.colouring(sc["table"])
    errs = []
    with make_ctx(rz, sc) as c:
        assert (c.get_tuning("physics_bodies"), c.get_tuning("physics_joints"), c.get_tuning("physics_colours")) == (sc["table"]["n_bodies"], sc["table"]["n_joints"], ncol)
        for (q, t), n, (rw, rs) in zip(poses, ps.CALLS, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
        # the physics moved something: without the table the last frame's dynamic bones sit on the solved pose
        w = c.read_world(0)
        c.upload_physics(None)
        c.deform()
        assert np.abs(c.read_world(0) - w).max() > 0.05
    assert_bar(errs, name)


def _crowd(rz, oracle, sc, I, kind, anims):
    """a crowd of I, every instance at its own frame, against the reference AND bit for bit against the same sequence run alone"""
    B = sc["B"]

    def pose_call(c, insts, call):
        fr = np.array([ps.crowd_frames(i, call) for i in insts], dtype=np.float32)
        if kind == "sampled":
            c.set_pose_sampled(fr)
        else:
            c.set_pose_blended(np.array([i % 2 for i in insts]), fr, np.array([(i + 1) % 2 for i in insts]), fr + 0.5, np.array([0.25 * (i % 5) for i in insts], dtype=np.float32))

    def local_of(i, call):
        f = float(np.float32(ps.crowd_frames(i, call)))
        if kind == "sampled":
            return sample_reference(anims[0], f, B, 0)[:2]
        return motion_ref.blend_reference(anims, (i % 2, f, (i + 1) % 2, float(np.float32(f + 0.5)), float(np.float32(0.25 * (i % 5)))), B, 0)[:2]

    def upload(c):
        if kind == "sampled":
            a = anims[0]
            c.upload_animation(a["track_bone"], a["key_off"], a["key_frame"], a["key_rot"], a["key_pos"], a["key_interp"])
        else:
            c.upload_motions(anims)
    dyn_bones = [int(b) for b in physics_ref.prepare(sc["table"], sc["parents"], sc["bind"])["dyn_bodies"]]
    errs, crowd_bits = [], []
    with make_ctx(rz, sc, instances=I) as c:
        upload(c)
        refs = [ps.run_reference(sc, [local_of(i, k) for k in range(len(ps.CROWD_CALLS))], ps.CROWD_CALLS) for i in range(I)]
        for call, n in enumerate(ps.CROWD_CALLS):
            pose_call(c, range(I), call)
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, *refs[i][call]))
        crowd_bits = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "%s crowd of %d" % (kind, I))
    k = I - 2
    with make_ctx(rz, sc) as c:
        upload(c)
        for call, n in enumerate(ps.CROWD_CALLS):
            pose_call(c, [k], call)
            c.physics_step(n)
            c.deform()
        st, w = c.read_physics(0), c.read_world(0)
    bones = [sc["table"]["bone"][b] for b in dyn_bones]
    same = np.array_equal(st.view(np.uint32), crowd_bits[k][0].view(np.uint32)) and np.array_equal(w[bones].view(np.uint32), crowd_bits[k][1][bones].view(np.uint32))
    print("instance %d alone vs in the crowd: state differs by %.2e, overrides by %.2e" % (k, np.abs(st - crowd_bits[k][0]).max(), np.abs(w[bones] - crowd_bits[k][1][bones]).max()))
    assert same, "instance %d of the crowd is not bit-identical to the same sequence run alone" % k


def test_sampled_crowd(rz, oracle):
    sc = ps.scene("crowd")
    _crowd(rz, oracle, sc, 3, "sampled", [ps.motion(sc, 0)])


def test_blended_crowd(rz, oracle):
    sc = ps.scene("crowd")
    _crowd(rz, oracle, sc, 5, "blended", [ps.motion(sc, 0), ps.motion(sc, 1)])


def test_with_ik(rz, oracle):
    """an IK table resident: the following body rides the solved arm, so physics reads the pose after IK"""
    sc = ps.scene("ik")
    poses = [ps.ik_pose(sc, k) for k in range(len(ps.CALLS))]
    ref = ps.run_reference(sc, poses, chains=sc["chains"])
    errs = []
    with make_ctx(rz, sc, chains=sc["chains"]) as c:
        assert c.get_tuning("ik_chains") == 1
        for (q, t), n, (rw, rs) in zip(poses, ps.CALLS, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
    assert_bar(errs, "with IK")
    no_ik = ps.run_reference(sc, poses)
    assert np.abs(no_ik[-1][1][:, :3] - ref[-1][1][:, :3]).max() > 0.1        # (the IK moves the strand's support)


def test_with_bone_morphs_and_sdef_qdef(rz, oracle):
    """a bone morph on a following body's bone, SDEF and QDEF tables behind the frame: state and world matrices against the reference, and
    the frame's output at the bar against the same frame fed the device's own overrides by hand (rz_override_world), the path those passes
    are already held to their references on"""
    from reze_engine_amd import synth
    from helpers import bone_morph_reference
    sc, bm, mw, poses = ps.bone_morph_case()
    m = sc["mesh"]
    sdef = synth.make_sdef(m, 0.2)
    qdef_idx = np.setdiff1d(np.arange(0, len(m["pos"]), 5, dtype=np.uint32), sdef["idx"]).astype(np.uint32)
    morphed = []
    for q, t in poses:
        q2, t2 = bone_morph_reference(q, t, bm["morph"], bm["bone"], bm["t"], bm["q"], mw)
        morphed.append((q2, t2))
    ref = ps.run_reference(sc, morphed, ps.CROWD_CALLS)
    plain = ps.run_reference(sc, poses, ps.CROWD_CALLS)
    assert np.abs(plain[-1][1][:, :3] - ref[-1][1][:, :3]).max() > 0.05          # (the morph moves the strand's support)

    def setup(c):
        c.upload_morphs_sparse(np.zeros(2, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32))
        c.upload_bone_morphs(bm["morph"], bm["bone"], bm["t"], bm["q"])
        c.upload_sdef(sdef["idx"], sdef["c"], sdef["r0"], sdef["r1"])
        c.upload_qdef(qdef_idx)
    worst = 0.0
    with make_ctx(rz, sc) as c:
        setup(c)
        assert c.get_tuning("sdef_verts") > 0 and c.get_tuning("qdef_verts") > 0
        for (q, t), n, (rw, rs) in zip(poses, ps.CROWD_CALLS, ref):
            c.set_pose_local(q[None], mw[None], t[None])
            c.physics_step(n)
            c.deform()
            st, wg = c.read_physics(0).astype(np.float64), c.read_world(0).astype(np.float64)
            worst = max(worst, float(np.abs(st[:, :3] - rs[:, :3]).max()) / sc["extent"], float(np.abs(wg - rw).max()) / sc["extent"])
        out = c.read(0)
        w = c.read_world(0)
    print("bone morph + SDEF + QDEF: body position / world %.2e x extent" % worst)
    assert worst <= BAR
    dyn = physics_ref.prepare(sc["table"], sc["parents"], sc["bind"])["dyn_bodies"]
    bones = np.array([sc["table"]["bone"][b] for b in dyn], dtype=np.uint32)
    with make_ctx(rz, sc, table=False) as c:
        setup(c)
        q, t = poses[-1]
        c.set_pose_local(q[None], mw[None], t[None])
        c.override_world(bones, w[bones])
        c.deform()
        by_hand = c.read(0)
    ep = float(np.abs(out[0].astype(np.float64) - by_hand[0]).max()) / sc["extent"]
    en = float(np.linalg.norm(out[1].astype(np.float64) - by_hand[1], axis=1).max())
    print("frame behind physics against the frame fed the same overrides by hand: positions %.2e x extent, normals %.2e" % (ep, en))
    assert ep <= BAR and en <= NRM_TOL


def test_replays_do_not_advance(rz, oracle):
    sc = ps.scene("crowd")
    poses = [ps.pose(sc, 40 + k) for k in range(3)]
    ref = ps.run_reference(sc, poses, (5, 5, 5))
    with make_ctx(rz, sc) as c:
        set_local(c, poses[:1])
        c.physics_step(5)
        c.deform()
        st, out = c.read_physics(0), c.read(0)
        c.deform_n(3)
        assert np.array_equal(c.read_physics(0).view(np.uint32), st.view(np.uint32)) and np.array_equal(c.read(0)[0].view(np.uint32), out[0].view(np.uint32))
        c.set_tuning(graph=1)
        c.deform_n(40)                  # (a graph replay: 16 captured frames at a time)
        assert np.array_equal(c.read_physics(0).view(np.uint32), st.view(np.uint32)) and np.array_equal(c.read(0)[0].view(np.uint32), out[0].view(np.uint32))
        c.time_span(3, lead=1)          # (rz_time_span: timed back-to-back frames)
        assert np.array_equal(c.read_physics(0).view(np.uint32), st.view(np.uint32)) and np.array_equal(c.read(0)[0].view(np.uint32), out[0].view(np.uint32))
        errs = []
        for k in (1, 2):                # steps after the replays go on from the state before them; the captured graph stays in use
            set_local(c, poses[k:k + 1])
            c.physics_step(5)
            c.deform_n(33)
            errs.append(errors(c, oracle, sc, 0, *ref[k]))
    assert_bar(errs, "steps after replays")


def test_crowd_under_the_overlapped_front(rz):
    """Crowd frames with overlap = 1 run their fronts on the upload stream and skin on the compute stream, two palette slots in turn. The
    step's hierarchy solve rewrites the current slot, so it waits for the frame that read it. Frames and steps back to back, nothing read
    in between: the state is the bits of the same sequence without the protocol, the output within the bar of it."""
    sc = ps.scene("crowd")
    I = 3
    got = {}
    for overlap in (0, 1):
        with make_ctx(rz, sc, instances=I) as c:
            c.set_tuning(overlap=overlap)
            for call, n in enumerate(ps.CROWD_CALLS + ps.CROWD_CALLS):
                set_local(c, [ps.pose(sc, 100 + I * call + i) for i in range(I)])
                c.physics_step(n)
                c.deform()
            assert c.get_tuning("effective_overlap") == overlap
            got[overlap] = ([c.read_physics(i) for i in range(I)], [c.read(i)[0] for i in range(I)])
    for i in range(I):
        assert np.array_equal(got[0][0][i].view(np.uint32), got[1][0][i].view(np.uint32)), "instance %d: the state differs under the overlapped front" % i
        e = float(np.abs(got[0][1][i].astype(np.float64) - got[1][1][i]).max()) / sc["extent"]
        assert e <= BAR, "instance %d: output off by %.3e x extent under the overlapped front" % (i, e)


def test_reset_and_instances(rz, oracle):
    sc = ps.scene("crowd")
    poses = [ps.pose(sc, 60 + k) for k in range(3)]
    sim = physics_ref.Sim(sc["table"], sc["parents"], sc["bind"])
    with make_ctx(rz, sc) as c:
        set_local(c, poses[:1])
        c.physics_step(8)
        c.deform()
        moved = c.read_world(0)
        # reset: the bodies stand on the un-overridden solved pose, the frame is the frame without physics (to the quaternion round trip)
        c.physics_reset()
        c.deform()
        w0 = ps.world_of(sc, *poses[0])
        sim.reset(w0)
        st = c.read_physics(0).astype(np.float64)
        e = max(float(np.abs(st[:, :3] - sim.x).max()), float(np.abs(c.read_world(0) - w0).max())) / sc["extent"]
        print("after reset: %.2e x extent from the solved pose (physics had moved it by %.2f)" % (e, np.abs(moved - w0).max()))
        assert e <= BAR and np.abs(st[:, 7:]).max() == 0.0 and np.abs(moved - w0).max() > 0.05
        # step(0) re-emits the overrides without advancing: same state, same overrides
        c.physics_step(6)
        c.deform()
        st, w = c.read_physics(0), c.read_world(0)
        c.physics_step(0)
        c.deform()
        assert np.array_equal(c.read_physics(0).view(np.uint32), st.view(np.uint32)) and np.array_equal(c.read_world(0).view(np.uint32), w.view(np.uint32))
        # a change of the instance count resets: both instances start from their own solved poses
        c.set_instances(2)
        set_local(c, poses[1:3])
        c.physics_step(4)
        c.deform()
        errs = []
        for i in range(2):
            ref = ps.run_reference(sc, [poses[1 + i]], (4,))
            errs.append(errors(c, oracle, sc, i, *ref[0]))
    assert_bar(errs, "after a change of the instance count")


def test_without_a_table_the_frame_is_the_old_frame(rz):
    sc = ps.scene("crowd")
    q, t = ps.pose(sc, 80)
    keys = ("effective_fuse_fk", "effective_fast", "effective_prep", "effective_grid", "effective_fk_kind", "effective_variant")
    with make_ctx(rz, sc, table=False) as c:
        set_local(c, [(q, t)])
        c.deform()
        before = (c.read(0), [c.get_tuning(k) for k in keys])
        c.upload_physics(sc["table"])
        set_local(c, [(q, t)])
        c.physics_step(5)
        c.deform()
        assert np.abs(c.read(0)[0] - before[0][0]).max() > 0.01
        c.upload_physics(None)
        assert c.get_tuning("physics_bodies") == 0
        set_local(c, [(q, t)])
        c.deform()
        after = (c.read(0), [c.get_tuning(k) for k in keys])
        assert after[1] == before[1]
        assert np.array_equal(after[0][0].view(np.uint32), before[0][0].view(np.uint32)) and np.array_equal(after[0][1].view(np.uint32), before[0][1].view(np.uint32))
        # rz_override_world works again
        w = c.read_world(0)
        m = w[3].copy()
        m[12] += 1.0
        c.override_world([3], m[None])
        c.deform()
        assert np.abs(c.read_world(0)[3] - m).max() == 0.0


def test_misuse(rz):
    import copy
    sc = ps.scene("crowd")
    m, tab = sc["mesh"], sc["table"]
    q, t = ps.pose(sc, 90)

    def refused(fn, *words):
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    def variant(**kw):
        v = copy.deepcopy(tab)
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        refused(lambda: c.upload_physics(tab), "rz_upload_skeleton_topology")
        c.upload_skeleton_topology(m["parents"], m["bind"])
        refused(lambda: c.physics_step(1), "no physics table")
        for bad, word in ((variant(bone=(2, sc["B"])), "names bone"), (variant(body_b=(1, 999)), "names bodies"), (variant(body_b=(1, int(tab["body_a"][1]))), "to itself"),
                          (variant(mass=(3, np.nan)), "not finite"), (variant(position=((0, 1), np.inf)), "not finite"), (variant(mass=(3, -1.0)), "negative mass"),
                          (variant(linear_damping=(3, 1.5)), "damping"), (variant(bone=(2, int(tab["bone"][1]))), "both drive bone"),
                          (variant(type=(3, 7)), "has type"), (variant(shape=(3, 5)), "has shape")):
            refused(lambda: c.upload_physics(bad), word)
            assert c.get_tuning("physics_bodies") == 0
        neg_h = copy.deepcopy(tab)
        neg_h["h"] = np.float32(-0.01)
        refused(lambda: c.upload_physics(neg_h), "h must be")
        big = physics_ref.make_table([dict(bone=0, type=1, mass=1.0) if k else dict(bone=0, type=0) for k in range(1800)], [])
        big["bone"][1:] = -1
        refused(lambda: c.upload_physics(big), "too large", "160 KB")
        c.upload_physics(tab)
        refused(lambda: c.physics_step(1), "no pose")
        c.set_pose(np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (sc["B"], 1)))
        refused(lambda: c.physics_step(1), "device-solved")
        refused(lambda: c.override_world([1], np.eye(4, dtype=np.float32).reshape(1, 16)), "physics table is resident")
        set_local(c, [(q, t)])
        c.physics_step(2)
        c.deform()
        f = c.fork()
        try:
            refused(lambda: c.physics_step(1), "fork")
            refused(lambda: c.physics_reset(), "fork")
            refused(lambda: c.upload_physics(None), "fork")
        finally:
            f.close()
        c.physics_step(1)
        # a new topology drops the table
        c.upload_skeleton_topology(m["parents"], m["bind"])
        assert c.get_tuning("physics_bodies") == 0


# ---- the edges of the launch shape (kernels/physics.hip: rz_launch_physics) and of what a table may hold ----

def form_of(c):
    """(lanes per workgroup, joints in registers?, bytes of LDS) of the resident table"""
    return c.get_tuning("physics_block"), c.get_tuning("physics_own"), c.get_tuning("physics_lds")


def run_sequence(rz, oracle, name, calls=ps.CALLS):
    """the standard sequence on one instance against the reference; returns (errors per call, counts, form, last state)"""
    sc = ps.scene(name)
    poses = [ps.pose(sc, k) for k in range(len(calls))]
    ref = ps.run_reference(sc, poses, calls)
    errs = []
    with make_ctx(rz, sc) as c:
        counts = (c.get_tuning("physics_bodies"), c.get_tuning("physics_joints"), c.get_tuning("physics_colours"))
        form = form_of(c)
        for (q, t), n, (rw, rs) in zip(poses, calls, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
        st = c.read_physics(0)
    return errs, counts, form, st


@pytest.mark.parametrize("name", ["params", "params h", "params iterations", "params gravity"])
def test_table_parameters(rz, oracle, name):
    """h, iterations and gravity3 away from their defaults (RzPhysicsParams h, iterations, gx / gy / gz): all three at once — 1 / 120 s, 7
    passes, (3, -40, 25) — and one at a time. tests/test_physics_cpu.py: test_every_parameter_moves_the_reference shows that each of them,
    and each component of gravity, moves the definition by more than 100 x this test's bar."""
    errs, _, form, _ = run_sequence(rz, oracle, name)
    assert form == (64, 1, ps.lds_bytes(25, 20))
    assert_bar(errs, name)


@pytest.mark.parametrize("name", [n for n in ps.FORMS if not n.startswith("most")])
def test_switch_points(rz, oracle, name):
    """The counts at which the launch changes its form, exactly: block = 64 iff nb <= 64 and the widest colour <= 64; joints in registers
    iff nj <= block (64 / 65 joints in a wave: lane 63 owns a joint / <64, false>; 256 / 257 joints under 256 lanes); and above 48 KB of
    LDS ("257 joints": 52 428 B) the launch first raises the kernel's dynamic shared memory limit."""
    sc = ps.scene(name)
    nb, nj, block, own = ps.FORMS[name]
    _, _, ncol = physics_ref.colouring(sc["table"])
    errs, counts, form, _ = run_sequence(rz, oracle, name)
    print("%s: %d bodies %d joints %d colours -> %d lanes, joints %s, %d B of LDS" % ((name,) + counts + (form[0], "in registers" if form[1] else "strided", form[2])))
    assert counts == (nb, nj, ncol) and (sc["table"]["n_bodies"], sc["table"]["n_joints"]) == (nb, nj)
    assert form == (block, own, ps.lds_bytes(nb, nj))
    if name == "257 joints":
        assert form[2] > 48 * 1024
    assert_bar(errs, name)


@pytest.mark.parametrize("name", ["most strands", "most bodies"])
def test_largest_tables(rz, oracle, name):
    """The largest tables the upload accepts, from the documented formula — 96 B per body, + 12 B per joint once the joints outnumber the
    lanes, at most 163 840 B: 1 516 strands of one body under one shared base (1 517 bodies, 1 516 joints in one colour, 163 824 B; 1 000
    of the strands drive bones, the bodies of the rest have bone = -1, because the hierarchy solve takes 1 412 bones and no more) and
    1 706 falling bodies without a joint (163 776 B), 100 of them on bones of their own, the rest with bone = -1. Both launch with the
    raised dynamic shared memory limit. One strand or one body more is refused by the upload."""
    sc = ps.scene(name)
    nb, nj, block, own = ps.FORMS[name]
    lds = ps.lds_bytes(nb, nj)
    assert (nb, nj) == ((1517, 1516) if name == "most strands" else (1706, 0)) and lds == (163824 if name == "most strands" else 163776)
    assert lds <= ps.LDS_LIMIT < ps.lds_bytes(nb + 1, nj + (1 if nj else 0))
    errs, counts, form, st = run_sequence(rz, oracle, name, ps.EDGE_CALLS)
    print("%s: %d bodies %d joints -> %d lanes, joints %s, %d B of LDS" % (name, counts[0], counts[1], form[0], "in registers" if form[1] else "strided", form[2]))
    assert counts[:2] == (nb, nj) and form == (block, own, lds)
    assert_bar(errs, name)
    more = ps.strands(ps.MOST_STRANDS + 1, 1, base=False, seed=28, n_verts=64, sprung=True, boned=1000) if nj else ps.falling_bodies(ps.MOST_BODIES + 1, n_verts=64)
    with make_ctx(rz, more, table=False) as c:
        with pytest.raises(rz.capi.RzError) as e:
            c.upload_physics(more["table"])
        assert "too large" in str(e.value) and "%d B of LDS" % ps.lds_bytes(nb + 1, nj + (1 if nj else 0)) in str(e.value), str(e.value)
        assert c.get_tuning("physics_bodies") == 0 and form_of(c) == (0, 0, 0)


@pytest.mark.parametrize("name", ["65 bodies 64 joints", "257 joints"])
def test_256_lane_forms_in_a_crowd(rz, oracle, name):
    """<256, true> and <256, false> with inst > 0: three instances, each at a pose of its own through rz_set_pose_local, against the
    reference per instance (the per-instance state, world and override addressing), and instance I - 2 bit for bit, state and overrides,
    against the same sequence run alone."""
    sc = ps.scene(name)
    I, calls = 3, ps.CROWD_CALLS
    dyn = physics_ref.prepare(sc["table"], sc["parents"], sc["bind"])["dyn_bodies"]
    bones = [int(sc["table"]["bone"][b]) for b in dyn]
    refs = [ps.run_reference(sc, [ps.local_crowd_pose(sc, i, k) for k in range(len(calls))], calls) for i in range(I)]
    errs = []
    with make_ctx(rz, sc, instances=I) as c:
        assert form_of(c)[:2] == ps.FORMS[name][2:]
        for call, n in enumerate(calls):
            set_local(c, [ps.local_crowd_pose(sc, i, call) for i in range(I)])
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, *refs[i][call]))
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "%s, crowd of %d" % (name, I))
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01                  # (the instances are not copies of each other)
    k = I - 2
    with make_ctx(rz, sc) as c:
        for call, n in enumerate(calls):
            set_local(c, [ps.local_crowd_pose(sc, k, call)])
            c.physics_step(n)
            c.deform()
        st, w = c.read_physics(0), c.read_world(0)
    print("instance %d alone vs in the crowd: state differs by %.2e, overrides by %.2e" % (k, np.abs(st - crowd[k][0]).max(), np.abs(w[bones] - crowd[k][1][bones]).max()))
    assert np.array_equal(st.view(np.uint32), crowd[k][0].view(np.uint32)) and np.array_equal(w[bones].view(np.uint32), crowd[k][1][bones].view(np.uint32)), \
        "instance %d of the crowd is not bit-identical to the same sequence run alone" % k


def test_table_contents(rz, oracle):
    """What no strand scene holds (physics_scenes.contents): bone = -1 on a following and on a dynamic body, a type-2 follower, a joint
    between two followers (det K = 0 in both stages: a no-op, and no NaN), a dynamic sphere of size 0 — zero inertia — under a follower in
    a limited, sprung joint, dampings of exactly 0 and 1, rotation limits given max first, and position play with rotation limits and
    springs in one joint. Held to the reference over the standard sequence; the followers' records are their placement."""
    sc = ps.scene("contents")
    t = sc["table"]
    assert t["bone"][0] == -1 and t["bone"][1] == -1 and t["type"][5] == 2 and not physics_ref.is_dynamic(t)[[0, 2, 5]].any() and physics_ref.is_dynamic(t)[[1, 3, 4, 6, 7]].all()
    assert (t["rotation_min"][1] > t["rotation_max"][1]).all() and t["size"][6][0] == 0 and t["linear_damping"][3] == 1 and t["linear_damping"][4] == 0
    poses = [ps.pose(sc, k) for k in range(len(ps.CALLS))]
    ref = ps.run_reference(sc, poses)
    errs, place = [], 0.0
    with make_ctx(rz, sc) as c:
        assert c.get_tuning("physics_bodies") == 8 and c.get_tuning("physics_joints") == 6 and form_of(c) == (64, 1, 8 * 96)
        for (q, tr), n, (rw, rs) in zip(poses, ps.CALLS, ref):
            set_local(c, [(q, tr)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
            st = c.read_physics(0).astype(np.float64)
            assert np.isfinite(st).all()
            # a following body's record: boneWorld x offset (the offset itself without a bone), zero velocities
            sim = physics_ref.Sim(t, sc["parents"], sc["bind"])
            sim.reset(ps.world_of(sc, q, tr))
            for b in (0, 2, 5):
                place = max(place, float(np.abs(st[b, :3] - sim.x[b]).max()) / sc["extent"], float(np.minimum(np.abs(st[b, 3:7] - sim.q[b]).max(), np.abs(st[b, 3:7] + sim.q[b]).max())))
                assert np.abs(st[b, 7:]).max() == 0.0
        assert np.array_equal(c.read_physics(0)[0, :3], t["offset_pos"][0])         # (the anchor without a bone is its offset, bit for bit)
    print("followers against their placement: %.2e" % place)
    assert place <= BAR
    assert_bar(errs, "table contents")


@pytest.mark.parametrize("name", ["crowd", "wide colour"])
def test_steps_add_up_bit_for_bit(rz, name):
    """With one resident pose physics_step(30) is 30 x physics_step(1) and physics_step(1000) is 4 x physics_step(250), bit for bit in
    the state and in the dynamic bones' world matrices: the state is stored and reloaded exactly, a following body is re-placed on the same
    matrices, and the spring multipliers start at zero in every substep. One wave with its joints in registers ("crowd") and 256 lanes
    striding with the multipliers in LDS ("wide colour"). No float64 bar applies over 1000 substeps (the float32 probe of the definition
    itself drifts to 4e-3 x extent by then), which is why this is an identity and not a parity check. And physics_step(0) as the very first
    call — a reset without a substep — leaves every body on the solved pose."""
    sc = ps.scene(name)
    q, t = ps.pose(sc, 30)
    dyn = physics_ref.prepare(sc["table"], sc["parents"], sc["bind"])["dyn_bodies"]
    bones = [int(sc["table"]["bone"][b]) for b in dyn]

    def run(steps):
        with make_ctx(rz, sc) as c:
            set_local(c, [(q, t)])
            for n in steps:
                c.physics_step(n)
            c.deform()
            st, w = c.read_physics(0), c.read_world(0)
        assert np.isfinite(st).all() and np.isfinite(w).all()
        return st, w
    for whole, parts in (((30,), (1,) * 30), ((1000,), (250,) * 4)):
        (sa, wa), (sb, wb) = run(whole), run(parts)
        print("%s, %d substeps in one call vs %d calls: state differs by %.2e, overrides by %.2e" % (name, whole[0], len(parts), np.abs(sa - sb).max(), np.abs(wa[bones] - wb[bones]).max()))
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)) and np.array_equal(wa[bones].view(np.uint32), wb[bones].view(np.uint32))
    assert np.abs(sa[dyn, 7:]).max() > 0                 # (something is still moving: the comparison is not of a scene at rest)
    st, w = run((0,))
    w0 = ps.world_of(sc, q, t)
    sim = physics_ref.Sim(sc["table"], sc["parents"], sc["bind"])
    sim.reset(w0)
    e = max(float(np.abs(st[:, :3] - sim.x).max()), float(np.abs(w - w0).max())) / sc["extent"]
    eq = float(np.minimum(np.abs(st[:, 3:7] - sim.q).max(axis=1), np.abs(st[:, 3:7] + sim.q).max(axis=1)).max())
    print("%s, physics_step(0) as the first call: %.2e x extent from the solved pose, quaternions %.2e" % (name, e, eq))
    assert e <= BAR and eq <= BAR and np.abs(st[:, 7:]).max() == 0.0


def test_joint_locked_at_the_gimbal_angle(rz):
    """rotation_min.y = rotation_max.y = pi / 2: the joint is held where euler_xyz changes its branch (|m02| < 0.9999999) on the last bits
    of one matrix entry, so the float32 and the float64 run of the definition legitimately take different branches and part (the probe
    deviates by 5.5e-3 x extent): there is NO parity bar here. What must hold in any branch: the state stays finite and the quaternions
    stay unit to 1e-5 over the standard sequence."""
    sc = ps.scene("gimbal")
    worst = 0.0
    with make_ctx(rz, sc) as c:
        for k, n in enumerate(ps.CALLS):
            set_local(c, [ps.pose(sc, k)])
            c.physics_step(n)
            c.deform()
            st = c.read_physics(0).astype(np.float64)
            assert np.isfinite(st).all() and np.isfinite(c.read_world(0)).all() and np.isfinite(c.read(0)[0]).all()
            worst = max(worst, float(np.abs(np.linalg.norm(st[:, 3:7], axis=1) - 1).max()))
    print("gimbal lock: quaternion norms off 1 by %.2e" % worst)
    assert worst <= 1e-5


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true }) on a PMX with a strand scene: loadModel uploads Model.physicsTables(), every
    step(timeMs) turns the clock's advance (16.7 ms a frame) into substeps of 1/75 s. The frames are held to the float64 reference run with
    the table the loader must derive and the same substeps; the strands move against the engine without devicePhysics; resetPhysics()
    restores the first frame bit for bit (under the same pose the reset puts every body where the first frame had it)."""
    sc, data, q = ps.node_case()
    m, B, ext = sc["mesh"], sc["B"], sc["extent"]
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "physics_e2e.js"), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"), str(tmp_path)]
                                  + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    calls = ps.node_substeps()
    assert tuple(info["on"]) == calls and info["off"] == [] and info["bodies"] == sc["table"]["n_bodies"] and info["offRefusesReset"]
    assert sum(calls) >= 12 and max(calls) >= 2
    n, V = len(calls), len(m["pos"])
    on = np.fromfile(str(tmp_path / "pos_on.f32"), dtype=np.float32).reshape(n, V, 3)
    off = np.fromfile(str(tmp_path / "pos_off.f32"), dtype=np.float32).reshape(n, V, 3)
    world = np.fromfile(str(tmp_path / "world_on.f32"), dtype=np.float32).reshape(n, B, 16)
    state = np.fromfile(str(tmp_path / "state_on.f32"), dtype=np.float32).reshape(n, -1, 13)
    reset = np.fromfile(str(tmp_path / "reset_on.f32"), dtype=np.float32).reshape(V, 3)
    ref = ps.run_reference(sc, [(q, np.zeros((B, 3), dtype=np.float32))] * n, calls)
    ex = ew = ep = eq = 0.0
    for k, (rw, rs) in enumerate(ref):
        ex = max(ex, float(np.abs(state[k][:, :3] - rs[:, :3]).max()) / ext)
        eq = max(eq, float(np.minimum(np.abs(state[k][:, 3:7] - rs[:, 3:7]).max(axis=1), np.abs(state[k][:, 3:7] + rs[:, 3:7]).max(axis=1)).max()))
        ew = max(ew, float(np.abs(world[k] - rw).max()) / ext)
        pr_, _ = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], rw.astype(np.float32), m["inv_bind"])
        ep = max(ep, float(np.abs(on[k].astype(np.float64) - pr_).max()) / ext)
    moved = float(np.abs(on[-1] - off[-1]).max())
    print("node engine, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f); the strands moved %.3f against "
          "the engine without devicePhysics" % (n, sum(calls), ex, eq, ew, ep, ext, moved))
    assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    assert moved > 0.05 and np.abs(on[0] - on[-1]).max() > 0.05
    assert np.array_equal(reset.view(np.uint32), on[0].view(np.uint32)), "resetPhysics() did not restore the first frame: off by %.3e" % np.abs(reset - on[0]).max()
