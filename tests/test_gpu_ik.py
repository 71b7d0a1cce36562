"""PMX inverse kinematics on the device (rz_upload_ik, kernels/ik.hip.h: the IK stage of rz_fk_kernel<RzIkParams>) against the float64 restatement
tests/ik_ref.py, through every pose source and frame form that can carry it.

The bar: world-matrix entries and deformed positions within 1e-4 x the skeleton's extent of the float64 restatement (1e-4 is the project's
parity tolerance); normals within the suite's 1e-4. A case may be left out only when the restatement itself marks it ill-conditioned — its
float32 run differs from its float64 run by more than 2.5e-5 x extent — and at most 2 % of a test's cases may be. Every test prints its
largest error before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ik_ref
import ik_scenes as iks
from helpers import NRM_TOL, bone_morph_reference, sample_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR, ILL = 1e-4, 2.5e-5


def skel_of(mesh, ap=None, ratio=None):
    return dict(parents=mesh["parents"], bind=mesh["bind"], ap=ap, ratio=ratio,
                extent=ik_ref.extent(ik_ref.bind_positions(mesh["parents"], mesh["bind"])))


def make_ctx(rz, mesh, chains, ap=None, ratio=None, instances=1, rows=None):
    r = slice(None) if rows is None else rows
    c = rz.DeformContext(0)
    c.upload_mesh(mesh["pos"][r], mesh["nrm"][r], mesh["joints"][r], mesh["weights"][r])
    c.upload_skeleton(mesh["inv_bind"])
    c.upload_skeleton_topology(mesh["parents"], mesh["bind"], ap, ratio)
    if instances > 1:
        c.set_instances(instances)
    if chains is not None:
        c.upload_ik(chains)
    return c


def reference(sk, chains, q, t):
    """(float64 world [B,16], ill-conditioned?) of one local pose"""
    w64, _ = ik_ref.solve(sk["parents"], sk["bind"], q, t, chains, sk["ap"], sk["ratio"])
    w32, _ = ik_ref.solve(sk["parents"], sk["bind"], q, t, chains, sk["ap"], sk["ratio"], dtype=np.float32)
    return w64, float(np.abs(w32.astype(np.float64) - w64).max()) > ILL * sk["extent"]


def check(c, oracle, mesh, sk, chains, poses, what, rows=None, overrides=None):
    """every instance of the frame `c` has just run against the restatement; poses = [(q, t)] per instance. Returns the largest error / extent."""
    errs, left_out = [], 0
    r = slice(None) if rows is None else rows
    for i, (q, t) in enumerate(poses):
        w64, ill = reference(sk, chains, q, t)
        if ill:
            left_out += 1
            continue
        if overrides:
            for b, m in overrides.items():
                w64[b] = m
        wg = c.read_world(i)
        assert np.isfinite(wg).all(), what
        ew = float(np.abs(wg.astype(np.float64) - w64).max()) / sk["extent"]
        pg, ng = c.read(i)
        pr, nr = oracle.deform(mesh["pos"][r], mesh["nrm"][r], mesh["joints"][r], mesh["weights"][r], w64.astype(np.float32), mesh["inv_bind"])
        ep = float(np.abs(pg.astype(np.float64) - pr).max()) / sk["extent"]
        en = float(np.linalg.norm(ng.astype(np.float64) - nr, axis=1).max())
        errs.append((ew, ep, en))
    e = np.array(errs).reshape(-1, 3)
    print("%s: %d poses, %d left out as ill-conditioned; world %.2e position %.2e (x extent %.1f), normals %.2e"
          % (what, len(poses), left_out, e[:, 0].max(), e[:, 1].max(), sk["extent"], e[:, 2].max()))
    assert left_out <= 0.02 * len(poses), "%s: %d of %d poses ill-conditioned" % (what, left_out, len(poses))
    assert e[:, 0].max() <= BAR and e[:, 1].max() <= BAR, "%s: world %.3e position %.3e x extent" % (what, e[:, 0].max(), e[:, 1].max())
    assert e[:, 2].max() <= NRM_TOL, "%s: normals %.3e" % (what, e[:, 2].max())
    return float(e[:, :2].max())


_memo = {}


def _rig():
    if "rig" not in _memo:
        from reze_engine_amd import synth
        m = synth.make_leg_rig(n_verts=3000)
        _memo["rig"] = dict(mesh=m, sk=skel_of(m), chains=m["chains"], synth=synth)
    return _memo["rig"]


def _tree():
    if "tree" not in _memo:
        from reze_engine_amd import synth
        m = synth.make_mesh(6000, 120, seed=31)
        _memo["tree"] = dict(mesh=m, sk=skel_of(m), synth=synth)
    return _memo["tree"]


@pytest.fixture(scope="module")
def rig(rz):
    return _rig()


@pytest.fixture(scope="module")
def tree(rz):
    return _tree()


def tree_pose(synth, mesh, seed):
    rng = np.random.default_rng(seed)
    B = len(mesh["parents"])
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-0.6, 0.6, size=B)
    q = np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1).astype(np.float32)
    t = (rng.uniform(-0.3, 0.3, size=(B, 3))).astype(np.float32)
    return q, t


def set_local(c, poses, mw=None):
    q = np.stack([p[0] for p in poses])
    t = np.stack([p[1] for p in poses])
    c.set_pose_local(q, mw, t)


def local_poses(s, I=24):
    poses = [s["synth"].leg_rig_pose(s["mesh"], 500 + k) for k in range(I // 2)]
    return poses + [s["synth"].leg_rig_pose(s["mesh"], 600 + k, reach=(1.05, 1.4)) for k in range(I // 2)]      # out of reach, the worst case: all N iterations


def test_local_poses_in_reach_and_out_of_reach(rz, oracle, rig):
    s = rig
    I = 24
    poses = local_poses(s, I)
    with make_ctx(rz, s["mesh"], s["chains"], instances=I) as c:
        assert c.get_tuning("ik_chains") == 4 and c.get_tuning("effective_fuse_fk") == 0
        set_local(c, poses)
        c.deform()
        check(c, oracle, s["mesh"], s["sk"], s["chains"], poses, "leg rig, local poses")
        # one character: the same kernel, and the plan keeps away from the fused one-launch frame
        c.set_instances(1)
        set_local(c, poses[3:4])
        assert c.get_tuning("effective_fuse_fk") == 0
        c.deform()
        check(c, oracle, s["mesh"], s["sk"], s["chains"], poses[3:4], "leg rig, one character")
        # the IK actually moved the legs: the knee is bent in the solved pose, straight without the table
        w = c.read_world(0)
        c.upload_ik([])
        c.deform()
        assert np.abs(c.read_world(0) - w).max() > 0.1


def leg_motion(rig_mesh, rng, nk=8):
    """keys for the centre and the four goals only, as a VMD dance has them"""
    bones = np.array([1, 10, 11, 12, 13], dtype=np.int32)
    n = len(bones)
    kq = np.zeros((n, nk, 4), dtype=np.float32)
    kq[..., 3] = 1
    ax = rng.normal(size=(nk, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-0.4, 0.4, size=nk)
    kq[0] = np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1)
    kp = np.zeros((n, nk, 3), dtype=np.float32)
    kp[0] = rng.uniform(-1.0, 1.0, size=(nk, 3))
    kp[0, :, 1] = rng.uniform(-3.0, 0.5, size=nk)            # the centre squats: knees bend
    for r in (1, 3):
        kp[r] = rng.uniform(-1.5, 1.5, size=(nk, 3))
        kp[r, :, 1] = rng.uniform(0.0, 2.5, size=nk)
        kp[r + 1] = rng.uniform(-0.3, 0.3, size=(nk, 3))
    return dict(track_bone=bones, key_off=(np.arange(n + 1) * nk).astype(np.uint32),
                key_frame=np.tile(np.cumsum(rng.integers(2, 9, size=nk)).astype(np.float32), n),
                key_rot=kq.reshape(-1, 4), key_pos=kp.reshape(-1, 3), key_interp=rng.integers(1, 127, size=(n * nk, 16)).astype(np.uint8))


def upload_motion(c, anim):
    c.upload_animation(anim["track_bone"], anim["key_off"], anim["key_frame"], anim["key_rot"], anim["key_pos"], anim["key_interp"])


def sampled_poses(anim, frames, B):
    out = []
    for f in frames:
        q, t, _ = sample_reference(anim, float(f), B, 0)
        out.append((q, t))
    return out


def crowd_frames(anim, I=256):
    return np.linspace(-1.0, float(anim["key_frame"].max()) + 2.0, I).astype(np.float32)          # every instance at its own frame


def test_sampled_pose_and_sampled_crowd(rz, oracle, rig):
    s = rig
    anim = leg_motion(s["mesh"], np.random.default_rng(3))
    with make_ctx(rz, s["mesh"], s["chains"]) as c:
        upload_motion(c, anim)
        c.set_pose_sampled([11.3])
        assert c.get_tuning("effective_fuse_fk") == 0
        c.deform()
        check(c, oracle, s["mesh"], s["sk"], s["chains"], sampled_poses(anim, [11.3], 14), "leg rig, one sampled pose")
        I = 256
        c.set_instances(I)
        frames = crowd_frames(anim, I)
        c.set_pose_sampled(frames)
        assert c.get_tuning("effective_fuse_fk") == 0
        c.deform()
        check(c, oracle, s["mesh"], s["sk"], s["chains"], sampled_poses(anim, frames, 14), "leg rig, 256-instance sampled crowd")


def bone_morph_case(s):
    bm = dict(morph=[0, 1], bone=[1, 1], t3=np.array([[0.4, -2.0, 0.3], [0.0, -0.5, 0.2]], dtype=np.float32),
              q4=np.array([[0.2, 0.1, 0.0, 0.97], [0.0, 0.3, 0.1, 0.95]], dtype=np.float32))
    bm["q4"] /= np.linalg.norm(bm["q4"], axis=1, keepdims=True)
    mw = np.array([0.8, 0.5], dtype=np.float32)
    q, t = s["synth"].leg_rig_pose(s["mesh"], 77)
    q2, t2 = bone_morph_reference(q, t, bm["morph"], bm["bone"], bm["t3"], bm["q4"], mw)
    return bm, mw, q, t, q2, t2


def test_bone_morph_on_a_links_parent_and_override_on_a_descendant(rz, oracle, rig):
    s = rig
    m = s["mesh"]
    V = len(m["pos"])
    with make_ctx(rz, m, s["chains"]) as c:
        c.upload_morphs_sparse(np.array([0, 1, 2], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.zeros((2, 3), dtype=np.float32))
        bm, mw, q, t, q2, t2 = bone_morph_case(s)
        c.upload_bone_morphs(bm["morph"], bm["bone"], bm["t3"], bm["q4"])
        c.set_pose_local(q, mw, t)
        c.deform()
        assert np.abs(t2[1] - t[1]).max() > 0.5
        check(c, oracle, m, s["sk"], s["chains"], [(q2, t2)], "bone morphs on the centre (parent of both leg links)")
        # physics override on the left toe, a descendant of the left leg chain: it lands after IK and wins
        ov = np.eye(4)
        ov[:3, 3] = (3.0, 1.0, -2.0)
        ov16 = ov.T.reshape(16).astype(np.float32)
        c.override_world([5], ov16[None])
        c.deform()
        assert np.array_equal(c.read_world(0)[5], ov16)
        check(c, oracle, m, s["sk"], s["chains"], [(q2, t2)], "override on a chain's descendant", overrides={5: ov16.astype(np.float64)})
    assert V > 0


def test_loops_zero_is_the_plain_hierarchy(rz, oracle, rig):
    s = rig
    chains = [dict(ch, loops=0) for ch in s["chains"]]
    poses = [s["synth"].leg_rig_pose(s["mesh"], 900)]
    with make_ctx(rz, s["mesh"], chains) as c:
        assert c.get_tuning("ik_chains") == 4
        set_local(c, poses)
        c.deform()
        w = c.read_world(0)
        check(c, oracle, s["mesh"], s["sk"], chains, poses, "loops = 0")
    from helpers import fk_reference
    plain = fk_reference(s["mesh"]["parents"], s["mesh"]["bind"], poses[0][0], poses[0][1])
    assert np.abs(w - plain.reshape(-1, 16)).max() <= BAR * s["sk"]["extent"]


def tree_chains(s, rigid):
    return s["synth"].make_ik(s["mesh"], n_chains=6, seed=41 + rigid, links=3 if not rigid else 2, rigid=rigid)


@pytest.mark.parametrize("rigid", [False, True])
def test_random_tree_chains(rz, oracle, tree, rigid):
    s = tree
    chains = tree_chains(s, rigid)
    assert len(chains) >= 4 and ik_ref.validate(120, s["mesh"]["parents"], chains) is None
    if rigid:          # a rigid bone sits between two links of every chain
        for ch in chains:
            assert int(s["mesh"]["parents"][ch["effector"]]) != ch["links"][0]["bone"]
    I = 8
    poses = [tree_pose(s["synth"], s["mesh"], 70 + k) for k in range(I)]
    with make_ctx(rz, s["mesh"], chains, instances=I) as c:
        set_local(c, poses)
        c.deform()
        check(c, oracle, s["mesh"], s["sk"], chains, poses, "random tree, rigid=%s" % rigid)


def big_case():
    if "big" in _memo:
        return _memo["big"]
    from reze_engine_amd import synth
    B = 600
    m = synth.make_mesh(8000, B, seed=33)
    chains = synth.make_ik(m, n_chains=5, seed=5, links=2)
    # append children of links (the "D" bones of a modern model): bones outside every chain's path that copy a link's rotation
    ap = np.full(B, -1, dtype=np.int32)
    ratio = np.ones(B, dtype=np.float32)
    on_path = set()
    for ch in chains:
        b = ch["effector"]
        while b != ch["links"][-1]["bone"]:
            on_path.add(int(b))
            b = int(m["parents"][b])
        on_path.add(int(b))
    # ... and above none of them: a "D" bone is a sibling of the leg it copies, never an ancestor of the chain (that would be refused)
    above = set()
    for ch in chains:
        for s in (ch["effector"], ch["goal"]):
            p = int(m["parents"][s])
            while p >= 0:
                above.add(p)
                p = int(m["parents"][p])
    free = [b for b in range(B) if b not in on_path and b not in above]
    for k, ch in enumerate(chains):
        ap[free[10 + k]] = ch["links"][-1]["bone"]
        ratio[free[10 + k]] = (1.0, 0.5, -0.5)[k % 3]
    sk = skel_of(m, ap, ratio)
    poses = [tree_pose(synth, m, 90 + k) for k in range(3)]
    _memo["big"] = (m, sk, chains, ap, ratio, poses)
    return _memo["big"]


def test_append_children_follow_and_more_than_512_bones(rz, oracle):
    m, sk, chains, ap, ratio, poses = big_case()
    with make_ctx(rz, m, chains, ap, ratio, instances=3) as c:
        set_local(c, poses)
        c.deform()
        check(c, oracle, m, sk, chains, poses, "600 bones with append children of links")


def test_shards_fork_and_graph_give_the_same_bits(rz, oracle, rig):
    s = rig
    m = s["mesh"]
    V = len(m["pos"])
    poses = [s["synth"].leg_rig_pose(m, 321)]
    with make_ctx(rz, m, s["chains"]) as c:
        set_local(c, poses)
        c.deform()
        pos, nrm = c.read()
        world = c.read_world(0)
        check(c, oracle, m, s["sk"], s["chains"], poses, "unsharded")
        f = c.fork()
        with pytest.raises(rz.RzError):
            c.upload_ik([])                       # refused while a fork borrows the table
        assert f.get_tuning("ik_chains") == 4
        set_local(f, poses)
        f.deform()
        pf, nf = f.read()
        assert np.array_equal(pf, pos) and np.array_equal(nf, nrm) and np.array_equal(f.read_world(0), world)
        f.close()
        c.set_tuning(graph=1)
        c.deform_n(64)
        pg, ng = c.read()
        assert np.array_equal(pg, pos) and np.array_equal(ng, nrm) and np.array_equal(c.read_world(0), world)
    for r in range(2):
        b, n = rz.shard_range(V, 2, r)
        with make_ctx(rz, m, s["chains"], rows=slice(b, b + n)) as c:
            set_local(c, poses)
            c.deform()
            ps, ns = c.read()
            assert np.array_equal(ps, pos[b:b + n]) and np.array_equal(ns, nrm[b:b + n]) and np.array_equal(c.read_world(0), world)


def test_without_a_table_the_frame_is_the_old_frame(rz, rig, tree):
    for s, I in ((rig, 1), (tree, 1), (tree, 12)):
        m = s["mesh"]
        chains = s.get("chains") or s["synth"].make_ik(m, n_chains=4, seed=8)
        poses = [tree_pose(s["synth"], m, 11 + k) for k in range(I)]
        with make_ctx(rz, m, None, instances=I) as never, make_ctx(rz, m, None, instances=I) as c:
            set_local(never, poses)
            never.deform()
            fuse0, name0 = never.get_tuning("effective_fuse_fk"), never.kernel_name()
            set_local(c, poses)
            c.deform()
            c.upload_ik(chains)
            assert c.get_tuning("ik_chains") == len(chains) and c.get_tuning("effective_fuse_fk") == 0
            c.deform()
            moved = c.read_world(0)
            c.upload_ik([])
            assert c.get_tuning("ik_chains") == 0 and c.get_tuning("effective_fuse_fk") == fuse0
            set_local(c, poses)
            c.deform()
            assert c.kernel_name() == name0
            for i in range(I):
                a, b = never.read(i), c.read(i)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert np.array_equal(never.read_world(i), c.read_world(i)) and np.array_equal(never.read_palette(i), c.read_palette(i))
            assert np.abs(moved - c.read_world(0)).max() > 1e-3


def test_misuse_is_refused_with_a_message(rz, rig):
    s = rig
    m = s["mesh"]
    ch = s["chains"]

    def bad(c, chains, code, word):
        with pytest.raises(rz.RzError) as e:
            c.upload_ik(chains)
        assert e.value.code == code and word in str(e.value), str(e.value)
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        bad(c, ch, -1, "rz_upload_skeleton_topology")
        c.upload_skeleton_topology(m["parents"], m["bind"])
        L = c._L
        assert L.rz_upload_ik(c._h, 2, None, None, None, None, None, None, None, None, None) == -1 and b"null" in L.rz_last_error()
        bad(c, [dict(ch[0], goal=14)], -1, "names bone")
        bad(c, [dict(ch[0], goal=ch[0]["effector"])], -1, "effector is the goal")
        bad(c, [dict(ch[0], links=[dict(bone=7, min=None, max=None)])], -1, "proper ancestor")              # the other leg's knee
        bad(c, [dict(ch[0], links=list(reversed(ch[0]["links"])))], -1, "proper ancestor")                    # links out of order
        bad(c, [dict(ch[0], links=[dict(bone=4, min=None, max=None)])], -1, "proper ancestor")              # the effector itself
        bad(c, [ch[0], dict(ch[2], goal=ch[0]["goal"])], -1, "share")
        bad(c, [dict(ch[0], goal=5)], -6, "goal")                                                            # the goal hangs below its own links
        assert c.get_tuning("ik_chains") == 0
        c.upload_ik(ch)
        assert c.get_tuning("ik_chains") == 4
        c.upload_skeleton_topology(m["parents"], m["bind"])            # a new topology drops the table
        assert c.get_tuning("ik_chains") == 0
        c.upload_ik(ch)
        c.upload_skeleton(m["inv_bind"])                               # ... and so does a new skeleton
        assert c.get_tuning("ik_chains") == 0
    # an append rotation taken from a link by a bone on a chain's path is refused, and the header says so
    ap = np.full(14, -1, dtype=np.int32)
    ap[4] = 7
    with make_ctx(rz, m, None, ap, np.ones(14, dtype=np.float32)) as c:
        bad(c, ch, -6, "append")
    # ... and so is an ancestor of the effector that copies the rotation of the chain's own link
    ap = np.full(14, -1, dtype=np.int32)
    ap[1] = 2
    with make_ctx(rz, m, None, ap, np.ones(14, dtype=np.float32)) as c:
        bad(c, ch, -6, "ancestor of the effector")


# ---- the edges of the launch shape: kernels/ik.hip.h solves a chain with one wave, one path bone per lane, and a stage with four waves ----

def _edge(name):
    """(mesh, skeleton, chains, poses) of a case of tests/ik_scenes.py, built once"""
    if name not in _memo:
        if name.startswith("path of 64"):
            m = iks.long_chain(64, LONG_LINKS[name])
            _memo[name] = (m, skel_of(m), m["chains"], iks.poses(m, 0))
        elif name == "nine legs":
            m = iks.nine_legs()
            _memo[name] = (m, skel_of(m), m["chains"], iks.poses(m, 10))
        elif name == "root link":
            m = iks.root_link()
            _memo[name] = (m, skel_of(m), m["chains"], iks.poses(m, 20))
        elif name == "three stages":
            m = iks.three_stages()
            _memo[name] = (m, skel_of(m), m["chains"], iks.poses(m, 30))
        else:
            s = _rig()
            chains = {"limits max first": lambda: iks.swapped(s["chains"], 0, 0), "limit_angle = 0": lambda: [dict(ch, limit_angle=0.0) for ch in s["chains"]],
                      "limit_angle = 0, no limits": lambda: iks.unlimited(s["chains"], limit_angle=0.0)}[name]()
            _memo[name] = (s["mesh"], s["sk"], chains, [s["synth"].leg_rig_pose(s["mesh"], 700 + k) for k in range(8)])
    return _memo[name]


LONG_LINKS = {"path of 64, links at 40 20 1": (40, 20, 1), "path of 64, links at 60 1": (60, 1), "path of 64, one link": (1,)}
EDGES = tuple(LONG_LINKS) + ("nine legs", "root link", "three stages", "limits max first", "limit_angle = 0", "limit_angle = 0, no limits")


def _run_edge(rz, oracle, name, I=8):
    """the case's 8 poses as crowds of I; returns the world matrices of every pose"""
    m, sk, chains, poses = _edge(name)
    worlds, worst = [], 0.0
    with make_ctx(rz, m, chains, instances=I) as c:
        for k in range(0, len(poses), I):
            set_local(c, poses[k:k + I])
            c.deform()
            worst = max(worst, check(c, oracle, m, sk, chains, poses[k:k + I], "%s, poses %d .. %d" % (name, k, k + I - 1)))
            worlds += [c.read_world(i) for i in range(I)]
        info = (c.get_tuning("ik_chains"), c.get_tuning("ik_stages"))
    print("%s: %d chain(s) in %d stage(s), largest error %.2e x extent" % (name, info[0], info[1], worst))
    return worlds, info


@pytest.mark.parametrize("name", list(LONG_LINKS))
def test_path_of_64_bones(rz, oracle, name):
    """The longest path rz_upload_ik accepts: bones 1 .. 64 of a line, the effector in lane P - 1 = 63 (v_readlane of the wave's last lane
    in every step), links at path bones 40 / 20 / 1, 60 / 1 or bone 1 alone with rigid bones between them, so a step re-solves up to 64
    bones serially. The IK moves bones by 5 to 17 units. A path of 65 bones is refused."""
    m, sk, chains, poses = _edge(name)
    _, info = _run_edge(rz, oracle, name)
    assert info == (1, 1)
    plain = ik_ref.solve(sk["parents"], sk["bind"], *poses[0])[0]
    assert np.abs(ik_ref.solve(sk["parents"], sk["bind"], *poses[0], chains)[0] - plain).max() > 1.0          # (the chain is not at rest)
    if name == "path of 64, one link":
        m65 = iks.long_chain(65, (1,))
        with make_ctx(rz, m65, None) as c:
            with pytest.raises(rz.RzError) as e:
                c.upload_ik(m65["chains"])
            assert e.value.code == -6 and "at most 64" in str(e.value) and "65 bones" in str(e.value), str(e.value)
            assert c.get_tuning("ik_chains") == 0 and c.get_tuning("ik_stages") == 0


def test_a_stage_wider_than_the_block(rz, oracle):
    """Nine independent two-link legs under one root form ONE stage (ik_stages): the workgroup's four waves stride over it (c += kBlock / 64),
    so wave 0 solves chains 0, 4 and 8 and every other wave two. As crowds of 4, every instance at its own pose."""
    _, info = _run_edge(rz, oracle, "nine legs", I=4)
    assert info == (9, 1)


def test_outermost_link_is_a_root_bone(rz, oracle):
    """par = -1: the chain's outermost link has no parent, the path is re-solved under the identity rows of ik_solve_chain; a limited knee
    below it, the goal a root bone of its own."""
    m, _, chains, _ = _edge("root link")
    assert m["parents"][chains[0]["links"][-1]["bone"]] == -1
    _, info = _run_edge(rz, oracle, "root link")
    assert info == (1, 1)


def test_limits_given_max_first_are_the_sorted_table(rz, oracle, rig):
    """The left knee's limits with min and max exchanged: the kernel sorts them per axis (fminf / fmaxf) as the restatement does, so the
    frame is the bits of the frame under the table as the rig gives it."""
    m, sk, chains, poses = _edge("limits max first")
    assert chains[0]["links"][0]["min"][0] > chains[0]["links"][0]["max"][0]
    swapped, _ = _run_edge(rz, oracle, "limits max first")
    with make_ctx(rz, m, rig["chains"], instances=len(poses)) as c:
        set_local(c, poses)
        c.deform()
        for i in range(len(poses)):
            assert np.array_equal(c.read_world(i).view(np.uint32), swapped[i].view(np.uint32)), "pose %d differs under limits given max first" % i
        w = c.read_world(0)
        c.upload_ik([])
        c.deform()
        assert np.abs(c.read_world(0) - w).max() > 0.1


def test_limit_angle_zero(rz, oracle, rig):
    """A per-step angle of 0: every step turns its link by nothing. Without limits the pose is the plain hierarchy within the bar although
    all 40 iterations run (a step of angle 0 still counts as a rotation); with the rig's limits the restatement still clamps the straight
    knee to its maximum of -0.5 degrees (0.05 units at the ankle), and the kernel is held to that."""
    from helpers import fk_reference
    m, sk, _, poses = _edge("limit_angle = 0, no limits")
    worlds, _ = _run_edge(rz, oracle, "limit_angle = 0, no limits")
    worst = 0.0
    for (q, t), w in zip(poses, worlds):
        worst = max(worst, float(np.abs(w - fk_reference(m["parents"], m["bind"], q, t).reshape(-1, 16)).max()) / sk["extent"])
    print("limit_angle = 0 without limits against the plain hierarchy: %.2e x extent" % worst)
    assert worst <= BAR
    _run_edge(rz, oracle, "limit_angle = 0")


def test_three_stages_each_on_the_pose_before(rz, oracle):
    """leg chain, toe chain, and a chain below the toe: the upload orders them into three stages, and each stage starts from the whole
    skeleton as the stage before left it (ik_resolve). The restatement without the earlier chains differs by far more than the bar."""
    m, sk, chains, poses = _edge("three stages")
    _, info = _run_edge(rz, oracle, "three stages")
    assert info == (3, 3)
    tip = chains[2]["effector"]
    full = ik_ref.solve(sk["parents"], sk["bind"], *poses[0], chains)[0]
    alone = ik_ref.solve(sk["parents"], sk["bind"], *poses[0], chains[2:])[0]
    assert np.abs(full[tip] - alone[tip]).max() > 100 * BAR * sk["extent"]


def _sampled_case(frames_of):
    s = _rig()
    anim = leg_motion(s["mesh"], np.random.default_rng(3))
    return s["sk"], s["chains"], sampled_poses(anim, frames_of(anim), 14)


# every (skeleton, chains, poses) set a test above holds the kernel to; tests/test_ik_cpu.py asserts that none of them is ill-conditioned
CASES = {
    "leg rig, local poses": lambda: (_rig()["sk"], _rig()["chains"], local_poses(_rig())),
    "leg rig, one sampled pose": lambda: _sampled_case(lambda anim: [11.3]),
    "leg rig, sampled crowd": lambda: _sampled_case(crowd_frames),
    "bone morphs": lambda: (_rig()["sk"], _rig()["chains"], [bone_morph_case(_rig())[4:6]]),
    "loops = 0, shards, fork, graph": lambda: (_rig()["sk"], _rig()["chains"], [_rig()["synth"].leg_rig_pose(_rig()["mesh"], k) for k in (900, 321)]),
    "random tree": lambda: (_tree()["sk"], tree_chains(_tree(), False), [tree_pose(_tree()["synth"], _tree()["mesh"], 70 + k) for k in range(8)]),
    "random tree, rigid": lambda: (_tree()["sk"], tree_chains(_tree(), True), [tree_pose(_tree()["synth"], _tree()["mesh"], 70 + k) for k in range(8)]),
    "append children, 600 bones": lambda: (big_case()[1], big_case()[2], big_case()[5]),
}
CASES.update({name: (lambda name=name: _edge(name)[1:]) for name in EDGES})


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, tmp_path):
    import test_ik_cpu as tc
    pmx, vmd = tc.write_leg_pmx_vmd(tmp_path)
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "ik_e2e.js"), pmx, vmd, str(tmp_path)], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    assert info["device"]["chains"] == 4 and not info["device"]["hostIK"] and info["host"]["hostIK"] and not info["off"]["hostIK"]
    ext = _rig()["sk"]["extent"]
    dev = np.fromfile(str(tmp_path / "pos_device.f32"), dtype=np.float32)
    host = np.fromfile(str(tmp_path / "pos_host.f32"), dtype=np.float32)
    off = np.fromfile(str(tmp_path / "pos_off.f32"), dtype=np.float32)
    e = float(np.abs(dev.astype(np.float64) - host).max()) / ext
    print("node engine: device-solved vs host-solved IK, position error %.2e x extent %.1f" % (e, ext))
    assert e <= BAR
    assert np.abs(host - off).max() > 0.1          # IK moved the mesh
