"""Bones below an overridden bone follow it on the device (rz_override_follow; kernels/fk.hip.h: FOLLOW, rz_fk_kernel<RzFollowParams> and
rz_fk_kernel<RzIkParams, RzFollowParams>) against the float64 definition tests/follow_ref.py, on the hand-laid scenes of tests/follow_scenes.py.

Bars: world matrices within 5e-5 x max(1, |ref|) of the definition in float64 — the project's bar for world matrices
(tests/test_gpu_layers.py, tests/test_gpu_fuzz.py); positions and normals of the scene's mesh, which has vertices on every follower
bone, within the layers test's 2e-4 of the oracle on the reference matrices. tests/test_follow_cpu.py holds the float32 run of the
definition to a quarter of the world bar on every scene used here. Every parity test prints its worst errors before it asserts; the
maxima per scene go to profiles/follow_edges_parity.txt."""
import os

import numpy as np
import pytest

import follow_ref as fr
import follow_scenes as fs
import ik_ref
import physics_gpu as pg
from helpers import assert_parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_BAR, P_BAR = 5e-5, 2e-4
ORDER = list("abcdefghi") + ["j I=1", "j I=3"]
HEAD = ("rz_override_follow against tests/follow_ref.py in float64 (tests/test_gpu_follow.py): per scene the largest world-matrix error over\n"
        "max(1, |ref|) (bar %.0e), position error over max(1, |p|) and normal error (bar %.0e), with the follower entries resident" % (W_BAR, P_BAR))
_rows = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_ctx(rz, sc, instances=None, follow=True):
    m = sc["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"], sc["ap"], sc["ratio"], sc["move"])
    n = len(sc["instances"]) if instances is None else instances
    if n > 1:
        c.set_instances(n)
    if sc["chains"]:
        c.upload_ik(sc["chains"])
    if follow:
        c.override_follow(True)
    return c


def feed(c, insts):
    """the local poses and the override sets of `insts`, as instances 0 .. of the context"""
    c.set_pose_local(np.stack([x["q"] for x in insts]), None, np.stack([x["t"] for x in insts]))
    bones = np.concatenate([x["bones"] for x in insts])
    mats = np.concatenate([x["mats"] for x in insts])
    which = np.concatenate([np.full(len(x["bones"]), k, dtype=np.uint32) for k, x in enumerate(insts)])
    c.override_world(bones, mats, instances=which)


def reference(sc, inst):
    return fr.follow(sc["parents"], fs.solved(sc, inst["q"], inst["t"]), inst["bones"], inst["mats"])


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


def hold(name, errs, followers):
    worst = np.array(errs).reshape(-1, 3).max(axis=0)
    line = "(%s) world %.2e positions %.2e normals %.2e  [%d follower entries]" % ((name,) + tuple(worst) + (followers,))
    print(line)
    _rows[name] = line
    pg.write_parity("follow_edges_parity.txt", HEAD, ORDER, _rows)
    assert worst[0] <= W_BAR and worst[1] <= P_BAR and worst[2] <= P_BAR, line


@pytest.mark.parametrize("name", list(fs.STATIC))
def test_scene_against_the_definition(rz, oracle, name):
    """fails without the feature (the symbol is absent). Every hand-fed scene, all its instances in one crowd: world matrices, positions
    and normals at the bars, the follower count the definition's, and the followers moved — the un-followed seam is off the reference by
    far more than the bar"""
    sc = fs.scene(name)
    insts = sc["instances"]
    want = sum(len(fr.followers(sc["parents"], x["bones"])) for x in insts)
    with make_ctx(rz, sc) as c:
        assert c.get_tuning("override_follow") == 1 and c.get_tuning("override_followers") == 0
        feed(c, insts)
        assert c.get_tuning("override_followers") == want
        c.deform()
        errs, off = [], 0.0
        for i, x in enumerate(insts):
            ref = reference(sc, x)
            errs.append(errors(c, oracle, sc, i, ref))
            off = max(off, float(np.abs(ref - fr.replaced(fs.solved(sc, x["q"], x["t"]), x["bones"], x["mats"])).max()))
    assert off > 0.1, "the scene's followers do not move"
    hold(name, errs, want)


def test_off_after_on_and_nothing_to_follow_are_the_old_frame(rz):
    """the flag off after on gives the bits of a context that never had it on; on with no overrides, or with overrides nothing hangs
    below, is bit-identical to off with no follower entry resident"""
    sc = fs.scene("a")
    x = sc["instances"][0]
    leaf = dict(x, bones=np.array([5, 7], dtype=np.uint32), mats=np.tile(x["mats"][:1], (2, 1)))       # the two leaves of (a)

    def frame(c, inst, overrides=True):
        if overrides:
            feed(c, [inst])
        else:
            c.set_pose_local(inst["q"][None], None, inst["t"][None])
            c.override_world(np.zeros(0, np.uint32), np.zeros((0, 16), np.float32))
        c.deform()
        return (c.read_world(0),) + tuple(c.read(0))

    def same(a, b):
        return all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
    with make_ctx(rz, sc, follow=False) as c:
        never = [frame(c, x), frame(c, leaf), frame(c, x, overrides=False)]
    with make_ctx(rz, sc) as c:
        on = frame(c, x)
        assert not same(on, never[0])
        c.override_follow(False)
        assert c.get_tuning("override_follow") == 0 and c.get_tuning("override_followers") == 0
        c.deform()
        assert same((c.read_world(0),) + tuple(c.read(0)), never[0]), "flag off with the set still resident"
        assert same(frame(c, x), never[0]), "flag off, the set fed again"
        c.override_follow(True)             # flips with the set resident: the lists are built by the flip
        assert c.get_tuning("override_followers") == 3
        c.deform()
        assert same((c.read_world(0),) + tuple(c.read(0)), on)
        assert same(frame(c, leaf), never[1]) and c.get_tuning("override_followers") == 0, "overrides without descendants"
        assert same(frame(c, x, overrides=False), never[2]) and c.get_tuning("override_followers") == 0, "no overrides"


def test_crowd_instance_alone_fork_replays(rz):
    """an instance of the crowd (h) equals the same instance run alone, bit for bit; a fork inherits the flag and follows its own set;
    rz_deform_n and a graph replay show the same followed pose"""
    sc = fs.scene("h")
    insts = sc["instances"]
    with make_ctx(rz, sc) as c:
        feed(c, insts)
        c.deform()
        crowd = [(c.read_world(i),) + tuple(c.read(i)) for i in range(len(insts))]
    for i, x in enumerate(insts):
        with make_ctx(rz, sc, instances=1) as c:
            feed(c, [x])
            c.deform()
            alone = (c.read_world(0),) + tuple(c.read(0))
            assert np.array_equal(bits(alone[0]), bits(crowd[i][0])), "instance %d alone differs from the crowd's" % i
            if i != 1:
                continue
            c.deform_n(3)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((c.read_world(0),) + tuple(c.read(0)), alone)), "rz_deform_n"
            c.set_tuning(graph=1)
            c.deform_n(40)                  # (a graph replay: 16 captured frames at a time)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((c.read_world(0),) + tuple(c.read(0)), alone)), "graph replay"
            c.set_tuning(graph=0)
            f = c.fork()
            try:
                assert f.get_tuning("override_follow") == 1 and f.get_tuning("override_followers") == 0
                feed(f, [x])
                assert f.get_tuning("override_followers") == len(fr.followers(sc["parents"], x["bones"]))
                f.deform()
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((f.read_world(0),) + tuple(f.read(0)), alone)), "the fork's frame"
                f.override_follow(False)    # a fork sets it like its lender, and only for itself
                assert f.get_tuning("override_follow") == 0 and c.get_tuning("override_follow") == 1
            finally:
                f.close()


def test_refusals_and_persistence(rz):
    sc = fs.scene("a")
    m = sc["mesh"]

    def refused(fn, *words):
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        refused(lambda: c.override_follow(True), "rz_upload_skeleton_topology")
        c.upload_skeleton_topology(m["parents"], m["bind"])
        refused(lambda: c.override_follow(2), "0 or 1")
        assert c.get_tuning("override_follow") == 0
        c.override_follow(True)
        refused(lambda: c.override_follow(2), "0 or 1")
        assert c.get_tuning("override_follow") == 1
        # persists across override sets and a change of the instance count; a new topology clears it
        feed(c, sc["instances"])
        c.override_world(np.zeros(0, np.uint32), np.zeros((0, 16), np.float32))
        c.set_instances(2)
        assert c.get_tuning("override_follow") == 1 and c.get_tuning("override_followers") == 0
        c.set_instances(1)
        c.upload_skeleton_topology(m["parents"], m["bind"])
        assert c.get_tuning("override_follow") == 0


@pytest.mark.parametrize("I", [1, 3])
def test_physics_tips_ride_their_strands(rz, oracle, I):
    """(j): the strands' body-less tip bones and the ornament ride the dynamic bones above them — each stays at its bind-pose offset from
    the bone it hangs from, within the bar — and the frame is the definition's on the overrides the step wrote. Without the flag the same
    bones stay with the animation: more than 100 x the bar away, so the scene shows the defect. The flag persists across the table's
    upload and removal."""
    sc = fs.scene("j")
    poses = [fs.physics_poses(sc, i) for i in range(I)]
    refs = [fs.physics_reference(sc, poses[i]) for i in range(I)]
    bp = ik_ref.bind_positions(sc["parents"], sc["bind"])
    scale = max(1.0, float(np.abs(refs[0][-1][0]).max()))

    def rigid_gap(w):
        """largest distance of a riding bone from its bind-pose offset in the frame of the bone it hangs from (the pose carries no
        translation below the centre, so a child's origin sits at its bind translation in its parent's frame; the ornament's second
        bone is turned about the first by the pose and is held to the definition only)"""
        worst = 0.0
        for b, a in sc["ride"].items():
            if sc["parents"][b] != a:
                continue
            A = w[a].reshape(4, 4).T.astype(np.float64)
            worst = max(worst, float(np.abs(A[:3, :3] @ (bp[b] - bp[a]) + A[:3, 3] - w[b].reshape(4, 4).T[:3, 3]).max()))
        return worst

    def run(follow):
        with pg.make_ctx(rz, sc, instances=I, table=False) as c:
            if follow and I == 1:
                c.override_follow(True)     # ahead of the table: the lists are built with the table's per-instance buffers
            c.upload_physics(sc["table"])
            for k, n in enumerate(fs.SUBSTEPS):
                pg.set_local(c, [poses[i][k] for i in range(I)])
                c.physics_step(n)
                c.deform()
                if follow and I > 1 and k == 0:
                    assert c.get_tuning("override_followers") == 0
                    c.override_follow(True)     # with the table's overrides resident: the lists are built by the flip
                    assert c.get_tuning("override_followers") == I * len(sc["ride"])
            followers = c.get_tuning("override_followers")
            out = [(c.read_world(i),) + tuple(c.read(i)) for i in range(I)]
            errs = []
            if follow:
                assert c.get_tuning("override_follow") == 1
                for i in range(I):
                    S, bones, O = refs[i][-1]
                    errs.append(errors(c, oracle, sc, i, fr.follow(sc["parents"], S, bones, O)))
                c.upload_physics(None)
                assert c.get_tuning("override_follow") == 1 and c.get_tuning("override_followers") == 0
            return out, errs, followers
    on, errs, followers = run(True)
    off, _, none = run(False)
    assert none == 0 and followers == I * len(sc["ride"])
    gap_on = max(rigid_gap(w) for w, _, _ in on)
    gap_off = min(rigid_gap(w) for w, _, _ in off)
    print("(j) I = %d: riding bones off their bind-pose offsets by %.2e with the flag (bar %.1e), %.3f without" % (I, gap_on, W_BAR * scale, gap_off))
    assert gap_on <= W_BAR * scale
    assert gap_off > 100 * W_BAR * scale, "the scene does not show the defect"
    hold("j I=%d" % I, errs, followers)


def test_sdef_and_qdef_on_follower_bones(rz):
    """the SDEF and QDEF passes behind a followed frame match their references on the followed matrices: tables on vertices of follower
    bones of scene (e)"""
    import qdef_ref
    import sdef_ref
    from reze_engine_amd import synth
    sc = fs.scene("e")
    m, x = sc["mesh"], sc["instances"][0]
    sd = synth.make_sdef(m, 0.3)
    qd = np.setdiff1d(synth.make_qdef(m, 0.4), sd["idx"]).astype(np.uint32)
    on_followers = lambda idx: int((m["joints"][idx, 0] >= 2).sum())
    assert on_followers(sd["idx"]) > 5 and on_followers(qd) > 5
    with make_ctx(rz, sc) as c:
        c.upload_sdef(sd["idx"], sd["c"], sd["r0"], sd["r1"])
        feed(c, [x])
        c.deform()
        w = c.read_world(0)
        assert float(np.abs(w - reference(sc, x)).max()) <= W_BAR * max(1.0, float(np.abs(w).max()))
        pr, nr = sdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], w, m["inv_bind"], sd["idx"], sd["c"], sd["r0"], sd["r1"])
        print("SDEF on follower bones: %.2e / %.2e" % assert_parity(*c.read(0), pr, nr, "SDEF on follower bones"))
        c.upload_sdef([], None, None, None)
        c.upload_qdef(qd)
        c.deform()
        pr, nr = qdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], w, m["inv_bind"], qd)
        print("QDEF on follower bones: %.2e / %.2e" % assert_parity(*c.read(0), pr, nr, "QDEF on follower bones"))
