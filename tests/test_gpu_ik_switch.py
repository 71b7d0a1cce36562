"""Per-instance switches of the IK chains on the device (rz_set_ik_enabled / rz_upload_ik_keys / rz_read_ik_enabled; kernels/ik.hip.h:
ik_stage<SW>, rz_fk_kernel<RzIkParams, RzIkSwitchParams> and <RzIkParams, RzFollowParams, RzIkSwitchParams>) against the float64 definition tests/ik_switch_ref.py, on the scenes and
key tracks of tests/ik_switch_scenes.py.

Bars, the IK suite's own (tests/test_gpu_ik.py): world-matrix entries and positions within 1e-4 x the skeleton's extent of the definition,
normals within helpers.NRM_TOL; a pose may be left out only when the definition's float32 run strays more than 2.5e-5 x extent from its
float64 run, at most 2 % of a test's poses (tests/test_ik_switch_cpu.py shows none does). Masks and switch states are compared exactly.
Every test prints its largest error before it asserts; the maxima per scene go to profiles/ik_switch_edges_parity.txt."""
import os

import numpy as np
import pytest

import ik_ref
import ik_switch_ref as sw
import ik_switch_scenes as sc
import motion_ref
import physics_gpu as pg
from helpers import NRM_TOL, bone_morph_reference, sample_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR, ILL = 1e-4, 2.5e-5
HEAD = ("rz_set_ik_enabled / rz_upload_ik_keys against tests/ik_switch_ref.py in float64 (tests/test_gpu_ik_switch.py): per scene the largest\n"
        "world-matrix and position error in units of the skeleton's extent (bar %.0e) and the largest normal error (bar %.0e), with the\n"
        "(instance, chain) bits that were off" % (BAR, NRM_TOL))
ORDER = list(sc.SCENES) + ["sampled, one character", "sampled, crowd of 8", "blended", "layered"]
_rows = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_ctx(rz, mesh, chains, instances=1):
    c = rz.DeformContext(0)
    c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
    c.upload_skeleton(mesh["inv_bind"])
    c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
    if instances > 1:
        c.set_instances(instances)
    if chains is not None:
        c.upload_ik(chains)
    return c


def set_local(c, poses, mw=None):
    c.set_pose_local(np.stack([p[0] for p in poses]), mw, np.stack([p[1] for p in poses]))


def errors(c, oracle, mesh, ext, i, w64):
    wg = c.read_world(i)
    pg_, ng = c.read(i)
    assert np.isfinite(wg).all() and np.isfinite(pg_).all() and np.isfinite(ng).all()
    pr, nr = oracle.deform(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"], w64.astype(np.float32), mesh["inv_bind"])
    return (float(np.abs(wg.astype(np.float64) - w64).max()) / ext, float(np.abs(pg_.astype(np.float64) - pr).max()) / ext,
            float(np.linalg.norm(ng.astype(np.float64) - nr, axis=1).max()))


def hold(name, errs, left_out, n, off_bits, record=True):
    e = np.array(errs).reshape(-1, 3)
    worst = e.max(axis=0)
    line = "(%s) world %.2e positions %.2e normals %.2e  [%d poses, %d left out as ill-conditioned, %d bits off]" % ((name,) + tuple(worst) + (n, left_out, off_bits))
    print(line)
    if record:
        _rows[name] = line
        pg.write_parity("ik_switch_edges_parity.txt", HEAD, ORDER, _rows)
    assert left_out <= 0.02 * n, line
    assert worst[0] <= BAR and worst[1] <= BAR and worst[2] <= NRM_TOL, line


def ill(sk, chains, q, t, mask, w64):
    w32 = sw.solve(sk["parents"], sk["bind"], q, t, chains, mask, dtype=np.float32)[0]
    return float(np.abs(w32.astype(np.float64) - w64).max()) > ILL * sk["extent"]


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_scene_against_the_definition(rz, oracle, name):
    """fails without the feature: the parent solves the chains that are off and lands more than 100 x the bar from the definition
    (tests/test_ik_switch_cpu.py: test_restatement_is_not_vacuous). rz_set_pose_local + rz_set_ik_enabled, every pose of the scene."""
    s = sc.scene(name)
    m, sk, I = s["mesh"], s["sk"], s["I"]
    off = int((s["masks"] == 0).sum())
    errs, left, n = [], 0, 0
    with make_ctx(rz, m, s["chains"], instances=I) as c:
        assert c.get_tuning("ik_switched") == 0
        c.set_ik_enabled(s["masks"])
        assert c.get_tuning("ik_switched") == off and np.array_equal(c.read_ik_enabled(), s["masks"])
        for batch in sc.batches(s):
            set_local(c, [s["poses"][p] for p in batch])
            c.deform()
            for i, p in enumerate(batch):
                w64 = sc.reference(name, p, i)
                n += 1
                if float(np.abs(sc.reference(name, p, i, np.float32).astype(np.float64) - w64).max()) > ILL * sk["extent"]:
                    left += 1
                    continue
                errs.append(errors(c, oracle, m, sk["extent"], i, w64))
        assert np.array_equal(c.read_ik_enabled(), s["masks"])          # rz_set_pose_local leaves the mask alone
    hold(name, errs, left, n, off)


def _rig_ctx(rz, instances=1):
    s = sc.scene("leg rig, crowd of 3")
    return s, make_ctx(rz, s["mesh"], s["chains"], instances=instances)


def upload_motion(c, anim):
    c.upload_animation(anim["track_bone"], anim["key_off"], anim["key_frame"], anim["key_rot"], anim["key_pos"], anim["key_interp"])


def test_sampled_pose_follows_the_keys(rz, oracle):
    """rz_upload_animation + rz_upload_ik_keys(RZ_NO_CLIP) + rz_set_pose_sampled: one character frame by frame, then a crowd with a frame
    per instance; the mask read back is the definition's row, exactly"""
    s, c = _rig_ctx(rz)
    m, sk, chains = s["mesh"], s["sk"], s["chains"]
    anim = sc.rig_motion()
    kf, ke = sw.flatten(sc.tracks()["eight keys"][0], sc.rig_chain_names())
    frames = sc.SAMPLED_FRAMES
    poses = [sample_reference(anim, float(f), 14, 0)[:2] for f in frames]
    rows = np.stack([sw.state_at(kf, ke, f) for f in frames])
    assert len({tuple(r) for r in rows}) >= 3
    refs = [sw.solve(sk["parents"], sk["bind"], q, t, chains, r)[0] for (q, t), r in zip(poses, rows)]
    with c:
        upload_motion(c, anim)
        c.upload_ik_keys((kf, ke))
        assert c.get_tuning("ik_key_sets") == 1
        errs = []
        for k, f in enumerate(frames):
            c.set_pose_sampled([f])
            assert np.array_equal(c.read_ik_enabled()[0], rows[k]), f
            assert c.get_tuning("ik_switched") == int((rows[k] == 0).sum())
            c.deform()
            assert not ill(sk, chains, *poses[k], rows[k], refs[k])
            errs.append(errors(c, oracle, m, sk["extent"], 0, refs[k]))
        hold("sampled, one character", errs, 0, len(frames), int((rows == 0).sum()))
        c.set_instances(len(frames))
        c.set_pose_sampled(frames)
        assert np.array_equal(c.read_ik_enabled(), rows)
        c.deform()
        hold("sampled, crowd of 8", [errors(c, oracle, m, sk["extent"], i, refs[i]) for i in range(len(frames))], 0, len(frames), int((rows == 0).sum()))


def _library():
    """two clips of the leg rig and a third; key sets on clips 0 and 1, clip 2 without; states on both sides of 0.5"""
    clips = [sc.rig_motion(3), sc.rig_motion(4, nk=6), sc.rig_motion(5, nk=5)]
    names = sc.rig_chain_names()
    sets = {0: sw.flatten(sc.tracks()["eight keys"][0], names), 1: sw.flatten(sc.tracks()["one key"][0], names), 2: None}
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    states = [(0, 11.3, 1, 7.7, 0.5), (0, 11.3, 1, 7.7, below), (1, 3.25, 0, 20.5, 0.25), (0, 15.5, 1, 9.0, 0.75), (1, 12.5, sw.NO_CLIP, 0.0, 0.0),
              (0, 21.0, 2, 4.0, 0.75), (2, 6.0, 0, 31.0, 0.25), (2, 6.0, 0, 31.0, 0.5)]
    return clips, sets, states


def test_blended_and_layered_poses_choose_a_clip(rz, oracle):
    """library keys: mask[i] = choose(states[i]) exactly — A below 0.5, B from 0.5 on, all on for a chosen clip without keys — and the
    frame is the definition's on the float64 blend. Layers never switch IK: a layered pose with the same base chooses the same rows."""
    s, c = _rig_ctx(rz, instances=8)
    m, sk, chains = s["mesh"], s["sk"], s["chains"]
    clips, sets, states = _library()
    rows = np.stack([sw.choose(st, sets, 4) for st in states])
    assert rows.min() == 0 and any(r.all() for r in rows)
    with c:
        c.upload_motions(clips)
        for k, ks in sets.items():
            if ks is not None:
                c.upload_ik_keys(ks, clip=k)
        assert c.get_tuning("ik_key_sets") == 2
        cols = list(zip(*states))
        c.set_pose_blended(cols[0], cols[1], [int(x) if x != sw.NO_CLIP else -1 for x in cols[2]], cols[3], cols[4])
        assert np.array_equal(c.read_ik_enabled(), rows)
        c.deform()
        errs, left = [], 0
        for i, st in enumerate(states):
            q, t, _ = motion_ref.blend_reference(clips, st, 14, 0)
            q, t = q.astype(np.float32), t.astype(np.float32)          # (the device blends in float32: the definition starts from the blend it is held to elsewhere)
            w64 = sw.solve(sk["parents"], sk["bind"], q, t, chains, rows[i])[0]
            if ill(sk, chains, q, t, rows[i], w64):
                left += 1
                continue
            errs.append(errors(c, oracle, m, sk["extent"], i, w64))
        hold("blended", errs, left, len(states), int((rows == 0).sum()))
        # layered: a layer of clip 1 (which has keys that differ) over the bones of the left leg's goal only, on top of the same base
        c.set_ik_enabled(None)
        mask = np.zeros((1, 14), dtype=np.uint8)
        mask[0, 10] = 1
        c.upload_motion_masks(mask)
        base = rz.DeformContext.pack_motion_states(8, cols[0], cols[1], [int(x) if x != sw.NO_CLIP else -1 for x in cols[2]], cols[3], cols[4])
        layer = dict(clip=1, frame=20.0, weight=1.0, mask=0, mode=0)
        c.set_pose_layered(base, [[layer]] * 8)
        assert np.array_equal(c.read_ik_enabled(), rows)
        c.deform()
        import layer_ref
        errs, left = [], 0
        for i, st in enumerate(states):
            q, t, _ = layer_ref.layered_reference(clips, st, [(1, 20.0, 1.0, 0, 0)], 14, 0, mask)
            q, t = q.astype(np.float32), t.astype(np.float32)
            w64 = sw.solve(sk["parents"], sk["bind"], q, t, chains, rows[i])[0]
            if ill(sk, chains, q, t, rows[i], w64):
                left += 1
                continue
            errs.append(errors(c, oracle, m, sk["extent"], i, w64))
        hold("layered", errs, left, len(states), int((rows == 0).sum()))


@pytest.mark.parametrize("track", ["eight keys", "one key", "300 keys", "no keys"])
def test_switch_states_are_the_definitions_exactly(rz, track):
    """rz_read_ik_enabled after rz_set_pose_sampled equals state_at for every frame asked of the track, for one character and for a crowd
    with a frame per instance; key chains uploaded in descending goal order go through the host-order -> device-order permutation"""
    s = sc.scene("leg rig, descending goals")
    names = [s["mesh"]["names"][ch["goal"]] for ch in s["chains"]]
    keys, ask = sc.tracks()[track]
    kf, ke = sw.flatten(keys, names)
    rows = np.stack([sw.state_at(kf, ke, f, 4) for f in ask])
    anim = sc.rig_motion()
    with make_ctx(rz, s["mesh"], s["chains"]) as c:
        upload_motion(c, anim)
        c.upload_ik_keys((kf, ke))
        for f, r in zip(ask, rows):
            c.set_pose_sampled([f])
            assert np.array_equal(c.read_ik_enabled()[0], r), (track, f)
        c.set_instances(len(ask))
        c.set_pose_sampled(ask)
        got = c.read_ik_enabled()
        print("%s: %d frames, %d bits off, %d mismatches" % (track, len(ask), int((rows == 0).sum()), int((got != rows).sum())))
        assert np.array_equal(got, rows)
        assert c.get_tuning("ik_switched") == int((rows == 0).sum())


def frame_of(c, i=0):
    return (c.read_world(i),) + tuple(c.read(i))


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_bit_identities(rz):
    """an all-on instance inside a crowd that runs the switched instantiation is the pose run alone under rz_fk_kernel<RzIkParams>; an all-off instance is, in
    world matrices, the pose on a context whose table was removed; a mask of all ones leaves ik_switched at 0 and is the parent path's bits"""
    s = sc.scene("leg rig, crowd of 3")
    m, chains, poses = s["mesh"], s["chains"], s["poses"][:3]
    with make_ctx(rz, m, chains, instances=3) as c:
        c.set_ik_enabled(s["masks"])
        assert c.get_tuning("ik_switched") == 6
        set_local(c, poses)
        c.deform()
        crowd = [frame_of(c, i) for i in range(3)]
    with make_ctx(rz, m, chains) as c:
        set_local(c, poses[0:1])
        c.deform()
        never = frame_of(c)
        assert c.get_tuning("ik_switched") == 0 and same(never, crowd[0]), "an all-on instance of a switched crowd"
        c.set_ik_enabled(np.ones((1, 4), dtype=np.uint8))
        assert c.get_tuning("ik_switched") == 0
        c.deform()
        assert same(frame_of(c), never), "a mask of all ones"
        c.set_ik_enabled([1, 0, 1, 1])
        c.deform()
        assert not same(frame_of(c), never)
        c.set_ik_enabled(None)
        c.deform()
        assert same(frame_of(c), never), "all on again"
        c.upload_ik([])
        set_local(c, poses[1:2])
        c.deform()
        assert np.array_equal(bits(c.read_world(0)), bits(crowd[1][0])), "an all-off instance against the solve without a table"


def test_composition_follow_bone_morphs_replays_fork(rz, oracle):
    """with an override set and rz_override_follow (the _sw_follow entry), with bone morphs, under rz_deform_n and a graph replay, and on
    a fork, which keeps a mask of its own"""
    import follow_ref as fr
    s = sc.scene("leg rig, crowd of 3")
    m, sk, chains = s["mesh"], s["sk"], s["chains"]
    mask = np.array([0, 1, 1, 1], dtype=np.uint8)                   # the left leg chain is off; its toe chain still runs
    q, t = s["poses"][2]
    with make_ctx(rz, m, chains) as c:
        c.upload_morphs_sparse(np.array([0, 1, 2], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.zeros((2, 3), dtype=np.float32))
        bm = dict(morph=[0, 1], bone=[1, 1], t3=np.array([[0.4, -2.0, 0.3], [0.0, -0.5, 0.2]], dtype=np.float32),
                  q4=np.array([[0.2, 0.1, 0.0, 0.97], [0.0, 0.3, 0.1, 0.95]], dtype=np.float32))
        bm["q4"] /= np.linalg.norm(bm["q4"], axis=1, keepdims=True)
        mw = np.array([0.8, 0.5], dtype=np.float32)
        c.upload_bone_morphs(bm["morph"], bm["bone"], bm["t3"], bm["q4"])
        q2, t2 = bone_morph_reference(q, t, bm["morph"], bm["bone"], bm["t3"], bm["q4"], mw)
        c.set_ik_enabled(mask)
        c.set_pose_local(q, mw, t)
        c.deform()
        w64 = sw.solve(sk["parents"], sk["bind"], q2, t2, chains, mask)[0]
        assert not ill(sk, chains, q2, t2, mask, w64)
        hold("bone morphs", [errors(c, oracle, m, sk["extent"], 0, w64)], 0, 1, 1, record=False)
        alone = frame_of(c)
        c.deform_n(3)
        assert same(frame_of(c), alone), "rz_deform_n"
        c.set_tuning(graph=1)
        c.deform_n(40)
        assert same(frame_of(c), alone), "graph replay"
        c.set_ik_enabled(None)              # the launched entry changes under a cached graph: the replay must show the full solve
        c.deform_n(40)
        full = frame_of(c)
        assert not same(full, alone)
        c.set_ik_enabled(mask)
        c.deform_n(40)
        assert same(frame_of(c), alone), "graph replay after the mask came back"
        c.set_tuning(graph=0)
        # override on the left knee with followers below it: rz_fk_kernel<RzIkParams, RzFollowParams, RzIkSwitchParams>
        ov = np.eye(4)
        ov[:3, 3] = (2.0, 5.0, 1.0)
        ov16 = ov.T.reshape(1, 16).astype(np.float32)
        c.override_follow(True)
        c.override_world([3], ov16)
        assert c.get_tuning("override_followers") == 2 and c.get_tuning("ik_switched") == 1
        c.deform()
        ref = fr.follow(sk["parents"], w64, np.array([3]), ov16.astype(np.float64))
        hold("override + follow", [errors(c, oracle, m, sk["extent"], 0, ref)], 0, 1, 1, record=False)
        c.override_world(np.zeros(0, np.uint32), np.zeros((0, 16), np.float32))
        c.override_follow(False)
        # a fork sees the table, starts all on and keeps a mask of its own
        f = c.fork()
        try:
            assert f.get_tuning("ik_switched") == 0 and f.read_ik_enabled().all()
            f.set_pose_local(q, mw, t)
            f.deform()
            assert same(frame_of(f), full), "the fork's all-on frame"
            f.set_ik_enabled([1, 1, 0, 0])
            assert c.get_tuning("ik_switched") == 1 and np.array_equal(c.read_ik_enabled()[0], mask)
            c.deform()
            assert same(frame_of(c), alone), "the lender's frame under the fork's other mask"
            with pytest.raises(rz.capi.RzError) as e:
                c.upload_ik_keys((np.zeros(1, np.float32), np.ones((1, 4), np.uint8)))
            assert "fork" in str(e.value), str(e.value)
        finally:
            f.close()


def test_refusals_and_lifetime(rz):
    """every refusal of the header leaves the context producing the bits it produced before; the lifetime rules of the mask and the keys"""
    s = sc.scene("leg rig, crowd of 3")
    m, chains = s["mesh"], s["chains"]
    anim = sc.rig_motion()
    keys = sw.flatten(sc.tracks()["eight keys"][0], sc.rig_chain_names())

    def refused(fn, *words):
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        assert e.value.code == -1, e.value.code
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    with make_ctx(rz, m, None) as c:
        set_local(c, s["poses"][:1])
        c.deform()
        before = frame_of(c)
        L = c._L
        assert L.rz_set_ik_enabled(c._h, None) == -1 and b"no IK table" in L.rz_last_error()
        assert L.rz_read_ik_enabled(c._h, np.zeros(4, np.uint8).ctypes.data_as(rz.capi.ctypes.POINTER(rz.capi.ctypes.c_uint8))) == -1
        k = rz.capi.RzIkKeys(0, None, None)
        assert L.rz_upload_ik_keys(c._h, rz.capi.NO_CLIP, rz.capi.ctypes.byref(k)) == -1 and b"no IK table" in L.rz_last_error()
        c.deform()
        assert same(frame_of(c), before)
        c.upload_ik(chains)
        upload_motion(c, anim)
        c.upload_ik_keys(keys)
        c.set_pose_sampled([12.0])
        c.deform()
        before, mask = frame_of(c), c.read_ik_enabled().copy()
        assert c.get_tuning("ik_switched") == 1 and c.get_tuning("ik_key_sets") == 1
        refused(lambda: c.upload_ik_keys(keys, clip=0), "clip 0 of 0")
        bad = (keys[0].copy(), keys[1])
        bad[0][3] = np.inf
        refused(lambda: c.upload_ik_keys(bad), "not finite")
        bad[0][3] = np.nan
        refused(lambda: c.upload_ik_keys(bad), "not finite")
        bad[0][3] = 19.0
        refused(lambda: c.upload_ik_keys(bad), "descend")
        k = rz.capi.RzIkKeys(2, None, None)
        assert L.rz_upload_ik_keys(c._h, rz.capi.NO_CLIP, rz.capi.ctypes.byref(k)) == -1 and b"null" in L.rz_last_error()
        assert c.get_tuning("ik_key_sets") == 1 and np.array_equal(c.read_ik_enabled(), mask)
        c.set_pose_sampled([12.0])
        c.deform()
        assert same(frame_of(c), before), "after the refused calls"
        # rz_set_pose_local and a sampling call without keys for its source leave the mask alone; rz_set_ik_enabled is the last writer
        c.set_ik_enabled([0, 0, 1, 1])
        set_local(c, s["poses"][:1])
        assert c.read_ik_enabled().tolist() == [[0, 0, 1, 1]]
        c.set_pose_sampled([12.0])
        assert np.array_equal(c.read_ik_enabled(), mask)
        c.upload_ik_keys(None)
        assert c.get_tuning("ik_key_sets") == 0
        c.set_ik_enabled([0, 0, 1, 1])
        c.set_pose_sampled([12.0])
        assert c.read_ik_enabled().tolist() == [[0, 0, 1, 1]]
        # rz_set_instances: shrinking keeps the mask, members that appear are all on
        c.set_instances(3)
        assert c.read_ik_enabled().tolist() == [[0, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]] and c.get_tuning("ik_switched") == 2
        c.set_ik_enabled([[1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 0, 0]])
        c.set_instances(2)
        assert c.read_ik_enabled().tolist() == [[1, 1, 1, 1], [1, 0, 1, 1]] and c.get_tuning("ik_switched") == 1
        c.set_instances(1)
        assert c.get_tuning("ik_switched") == 0
        # rz_upload_animation drops the RZ_NO_CLIP keys, rz_upload_motions the library's, rz_upload_ik everything and resets the mask
        c.upload_ik_keys(keys)
        c.upload_motions([anim, anim])
        c.upload_ik_keys(keys, clip=1)
        refused(lambda: c.upload_ik_keys(keys, clip=2), "clip 2 of 2")
        assert c.get_tuning("ik_key_sets") == 2
        upload_motion(c, anim)
        assert c.get_tuning("ik_key_sets") == 1
        c.upload_ik_keys(keys)
        c.upload_motions([anim])
        assert c.get_tuning("ik_key_sets") == 1
        c.upload_ik_keys(keys, clip=0)
        c.set_ik_enabled([0, 1, 1, 1])
        c.upload_ik(chains)
        assert c.get_tuning("ik_key_sets") == 0 and c.get_tuning("ik_switched") == 0 and c.read_ik_enabled().all()
        c.upload_ik_keys(keys)
        c.set_ik_enabled([0, 1, 1, 1])
        c.upload_ik([])
        c.upload_ik(chains)
        assert c.get_tuning("ik_key_sets") == 0 and c.get_tuning("ik_switched") == 0
        c.upload_ik_keys(keys)
        c.set_ik_enabled([0, 1, 1, 1])
        c.upload_skeleton_topology(m["parents"], m["bind"])            # a new topology drops everything
        c.upload_ik(chains)
        assert c.get_tuning("ik_key_sets") == 0 and c.get_tuning("ik_switched") == 0 and c.read_ik_enabled().all()
        upload_motion(c, anim)
        c.upload_motions([anim])
        c.upload_ik_keys(keys)
        c.upload_ik_keys(keys, clip=0)
        c.set_ik_enabled([0, 1, 1, 1])
        assert c.get_tuning("ik_key_sets") == 2 and c.get_tuning("ik_switched") == 1
        c.upload_skeleton(m["inv_bind"])                               # ... and so does a new skeleton
        assert c.get_tuning("ik_chains") == 0 and c.get_tuning("ik_key_sets") == 0 and c.get_tuning("ik_switched") == 0
        c.upload_skeleton_topology(m["parents"], m["bind"])
        c.upload_ik(chains)
        assert c.get_tuning("ik_key_sets") == 0 and c.get_tuning("ik_switched") == 0 and c.read_ik_enabled().all()


def test_physics_first_solve_uses_the_mask(rz, oracle):
    """rz_physics_step's first solve goes through the same launch: with the arm's chain switched off, the following body on the lower arm
    (a link of the chain) is placed on the un-solved bone and the strand hangs from there — the physics suite's IK scene against its
    reference WITHOUT the chain, at the physics bar; the reference with the chain is far away"""
    import physics_scenes as ps
    s = ps.scene("ik")
    poses = [ps.ik_pose(s, k) for k in range(len(ps.CALLS))]
    off_ref = ps.run_reference(s, poses)
    on_ref = ps.run_reference(s, poses, chains=s["chains"])
    assert np.abs(off_ref[-1][1][:, :3] - on_ref[-1][1][:, :3]).max() > 0.1
    errs = []
    with pg.make_ctx(rz, s, chains=s["chains"]) as c:
        c.set_ik_enabled([0])
        assert c.get_tuning("ik_chains") == 1 and c.get_tuning("ik_switched") == 1
        for (q, t), n, (rw, rs) in zip(poses, ps.CALLS, off_ref):
            pg.set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(pg.errors(c, oracle, s, 0, rw, rs))
        st = c.read_physics(0)
    pg.assert_bar(errs, "physics with the arm's chain switched off")
    assert np.abs(st[:, :3] - on_ref[-1][1][:, :3]).max() > 0.1


@pytest.mark.skipif(__import__("shutil").which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, tmp_path):
    """a PMX leg rig and a VMD whose show / IK keys switch the right leg (and its toe) off at frame 30: frames 29 and 31 through
    { deviceFK, deviceSampling, ik, ikKeys } and through host-sampled { deviceFK, ik, ikKeys } against the host path of the same engine"""
    import json
    import subprocess
    import test_ik_cpu as tc
    import test_ik_switch_cpu as tsc
    from reze_engine_amd import synth
    rig = synth.make_leg_rig(n_verts=1500)
    rng = np.random.default_rng(23)
    keys = []
    for f in (0, 10, 20, 30, 40):
        a = rng.uniform(-0.3, 0.3)
        keys.append(("centre", f, (0.0, float(np.sin(a / 2)), 0.0, float(np.cos(a / 2))), (float(rng.uniform(-1, 1)), float(rng.uniform(-3, -0.5)), float(rng.uniform(-1, 1)))))
        for g in ("leg_ik_L", "leg_ik_R"):
            keys.append((g, f, (0, 0, 0, 1), (float(rng.uniform(-1.5, 1.5)), float(rng.uniform(0, 2.5)), float(rng.uniform(-1.5, 1.5)))))
    ik_keys = [(0, True, [("leg_ik_L", True), ("toe_ik_L", True), ("leg_ik_R", True), ("toe_ik_R", True)]), (30, True, [("leg_ik_R", False), ("toe_ik_R", False)])]
    (tmp_path / "legs.pmx").write_bytes(tc.write_ik_pmx(rig))
    (tmp_path / "legs.vmd").write_bytes(tsc.write_vmd_with_ik(keys, [], ik_keys)[0])
    from pmx_synth import write_vmd
    (tmp_path / "plain.vmd").write_bytes(write_vmd(keys))             # the same motion without a show / IK block, loaded behind it
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "ik_switch_e2e.js"), str(tmp_path / "legs.pmx"), str(tmp_path / "legs.vmd"), str(tmp_path),
                                   str(tmp_path / "plain.vmd")], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    for tag in ("device", "local", "host"):
        # frames 29 and 31 of the motion with keys, then frame 31 of the motion without: every chain on again
        assert info[tag]["masks"] == [[1, 1, 1, 1], [1, 1, 0, 0], [1, 1, 1, 1]] and info[tag]["ikFrames"] == 2, (tag, info[tag])
    assert info["device"]["keySets"] == 1 and info["device"]["switched"] == 2 and info["local"]["keySets"] == 0 and info["local"]["switched"] == 2
    assert info["nokeys"]["masks"] == [[1, 1, 1, 1]] * 3
    ext = ik_ref.extent(ik_ref.bind_positions(rig["parents"], rig["bind"]))
    pos = {tag: np.fromfile(str(tmp_path / ("pos_%s.f32" % tag)), dtype=np.float32).reshape(3, -1) for tag in ("device", "local", "host", "nokeys")}
    e_dev = float(np.abs(pos["device"].astype(np.float64) - pos["host"]).max()) / ext
    e_loc = float(np.abs(pos["local"].astype(np.float64) - pos["host"]).max()) / ext
    moved = float(np.abs(pos["host"][1] - pos["nokeys"][1]).max()) / ext
    print("node engine, frames 29 and 31: device-sampled vs host %.2e, host-sampled device vs host %.2e x extent %.1f; the keys move frame 31 by %.3f x extent"
          % (e_dev, e_loc, ext, moved))
    assert e_dev <= BAR and e_loc <= BAR
    assert np.array_equal(pos["host"][0], pos["nokeys"][0]) and moved > 100 * BAR
    assert np.array_equal(pos["host"][2], pos["nokeys"][2]), "the motion without keys plays with every chain on"


def test_a_motion_without_keys_behind_one_with_keys(rz):
    """rz_upload_animation drops the keys and leaves the mask: a sampling call without keys would keep the old switches. A set of NO keys
    uploaded behind the new motion is resident and says "all on" (what Engine { ikKeys } uploads behind a motion without a show / IK
    block): the next pose call writes an all-on mask and the frame is the bits of a context that never saw keys. The same for a library."""
    s = sc.scene("leg rig, crowd of 3")
    m, chains = s["mesh"], s["chains"]
    anim, plain = sc.rig_motion(3), sc.rig_motion(4, nk=6)
    keys = sw.flatten(sc.tracks()["eight keys"][0], sc.rig_chain_names())
    none = (np.zeros(0, np.float32), np.zeros((0, 4), np.uint8))
    with make_ctx(rz, m, chains) as never:
        upload_motion(never, plain)
        never.set_pose_sampled([7.5])
        never.deform()
        want = frame_of(never)
        never.upload_motions([plain])
        never.set_pose_blended(0, 7.5)
        never.deform()
        want_lib = frame_of(never)
    with make_ctx(rz, m, chains) as c:
        upload_motion(c, anim)
        c.upload_ik_keys(keys)
        c.set_pose_sampled([7.5])
        c.deform()
        assert c.read_ik_enabled().tolist() == [[0, 1, 1, 1]]
        upload_motion(c, plain)
        assert c.get_tuning("ik_key_sets") == 0
        c.set_pose_sampled([7.5])
        assert c.read_ik_enabled().tolist() == [[0, 1, 1, 1]], "a sampling call without keys leaves the mask alone"
        c.upload_ik_keys(none)
        assert c.get_tuning("ik_key_sets") == 1
        c.set_pose_sampled([7.5])
        assert c.read_ik_enabled().all() and c.get_tuning("ik_switched") == 0
        c.deform()
        assert same(frame_of(c), want)
        # the library: clip 0 with keys, then a library whose only clip has none
        c.upload_motions([anim])
        c.upload_ik_keys(keys, clip=0)
        c.set_pose_blended(0, 7.5)
        assert c.read_ik_enabled().tolist() == [[0, 1, 1, 1]]
        c.upload_motions([plain])
        c.upload_ik_keys(none, clip=0)
        c.set_pose_blended(0, 7.5)
        assert c.read_ik_enabled().all()
        c.deform()
        assert same(frame_of(c), want_lib)


def test_forks_see_the_keys(rz, oracle):
    """key sets are static data: a fork made after the upload reports them and its own sampling pose calls evaluate them - the mask it
    reads back is state_at / choose exactly, its frame the definition's - while its mask stays its own"""
    s = sc.scene("leg rig, crowd of 3")
    m, sk, chains = s["mesh"], s["sk"], s["chains"]
    anim = sc.rig_motion()
    names = sc.rig_chain_names()
    keys, one = sw.flatten(sc.tracks()["eight keys"][0], names), sw.flatten(sc.tracks()["one key"][0], names)
    with make_ctx(rz, m, chains, instances=4) as c:
        upload_motion(c, anim)
        c.upload_motions([anim, sc.rig_motion(4, nk=6)])
        c.upload_ik_keys(keys)
        c.upload_ik_keys(one, clip=1)
        f = c.fork()
        try:
            assert f.get_tuning("ik_key_sets") == 2 and f.get_tuning("ik_switched") == 0
            frames = [2.0, 10.0, 20.0, 31.0]
            rows = np.stack([sw.state_at(keys[0], keys[1], x) for x in frames])
            f.set_pose_sampled(frames)
            assert np.array_equal(f.read_ik_enabled(), rows) and c.read_ik_enabled().all()
            f.deform()
            errs = []
            for i, x in enumerate(frames):
                q, t, _ = sample_reference(anim, x, 14, 0)
                errs.append(errors(f, oracle, m, sk["extent"], i, sw.solve(sk["parents"], sk["bind"], q, t, chains, rows[i])[0]))
            hold("sampled on a fork", errs, 0, len(frames), int((rows == 0).sum()), record=False)
            states = [(0, 11.3, 1, 7.7, 0.25), (0, 11.3, 1, 7.7, 0.75), (1, 3.0, sw.NO_CLIP, 0.0, 0.0), (0, 5.0, sw.NO_CLIP, 0.0, 0.0)]
            want = np.stack([sw.choose(st, {0: None, 1: one}, 4) for st in states])
            cols = list(zip(*states))
            f.set_pose_blended(cols[0], cols[1], [int(x) if x != sw.NO_CLIP else -1 for x in cols[2]], cols[3], cols[4])
            assert np.array_equal(f.read_ik_enabled(), want) and want.min() == 0 and c.read_ik_enabled().all()
        finally:
            f.close()


@pytest.mark.parametrize("chain", [31, 32])
def test_one_character_with_two_words_in_the_arguments(rz, oracle, chain):
    """one character of the 33-leg scene: its two mask words ride in the kernel arguments, and the bit either side of the word boundary is
    found by the select between them (a crowd of it goes through the device array: the scene tests)"""
    name = "33 legs, chain %d off" % chain
    s = sc.scene(name)
    m, sk = s["mesh"], s["sk"]
    with make_ctx(rz, m, s["chains"]) as c:
        c.set_ik_enabled(s["masks"][:1])
        assert c.get_tuning("ik_switched") == 1 and np.array_equal(c.read_ik_enabled(), s["masks"][:1])
        errs = []
        for p in (0, 1):
            set_local(c, [s["poses"][p]])
            c.deform()
            errs.append(errors(c, oracle, m, sk["extent"], 0, sc.reference(name, p, 0)))
        hold(name + ", one character", errs, 0, 2, 1, record=False)
        full = ik_ref.solve(sk["parents"], sk["bind"], *s["poses"][1], s["chains"])[0]
        eff = s["chains"][chain]["effector"]
        assert np.abs(c.read_world(0)[eff] - full[eff]).max() > 100 * BAR * sk["extent"]          # (the chain that is off is not solved)
        other = s["chains"][63 - chain]["effector"]                                                 # its neighbour across the boundary is
        assert np.abs(c.read_world(0)[other] - full[other]).max() <= BAR * sk["extent"]


def test_crowd_graph_replay_reads_the_mask_of_the_moment(rz):
    """a crowd's words lie in a device array that keeps its address: a captured graph is replayed across mask changes that arrive by the
    copy outside it, and every replay shows the frame of the mask of that moment (bit for bit the plain frame's)"""
    s = sc.scene("leg rig, crowd of 3")
    m, chains, poses = s["mesh"], s["chains"], s["poses"][:3]
    a, b = s["masks"], np.array([[0, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1]], dtype=np.uint8)

    def frames(c):
        return [frame_of(c, i) for i in range(3)]
    with make_ctx(rz, m, chains, instances=3) as c:
        set_local(c, poses)
        plain = {}
        for tag, mask in (("a", a), ("b", b), ("on", None)):
            c.set_ik_enabled(mask)
            c.deform()
            plain[tag] = frames(c)
        assert not all(same(x, y) for x, y in zip(plain["a"], plain["b"]))
        c.set_tuning(graph=1)
        for tag, mask in (("a", a), ("b", b), ("a", a), ("on", None), ("b", b)):      # ("on": the entry point changes, a graph of its own)
            c.set_ik_enabled(mask)
            c.deform_n(40)
            assert all(same(x, y) for x, y in zip(frames(c), plain[tag])), "graph replay under mask " + tag
