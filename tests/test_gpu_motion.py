"""The device motion library (rz_upload_motions / rz_set_pose_blended, rz_motion_kernel<RzMotionParams> of kernels/motion.hip) against its float64 definition
tests/motion_ref.py, and through everything that runs behind a local pose.

Inputs follow one rule (tests/test_motion_cpu.py asserts it on exactly these states): every key of a bone, across all clips, lies within a
45 degree rotation of a per-bone base rotation — identity for a bone some clip leaves at rest — so any two samples of a bone have
|dot| >= 0.7 and the precision the blend's sign choice is taken in cannot flip it. Half of clip 1's keys are stored with the opposite
sign, key frames are unevenly spaced with one duplicate per track, interpolation bytes are random in 1 .. 126.

Bars: world matrices within 5e-5 x max(1, |ref|) of fk_reference(motion_ref), positions and normals within 2e-4 of the oracle on those
matrices and weights — the project's own for this sampler arithmetic (tests/test_gpu_round6.py); the blend adds one slerp of the form
the sampler already ends with. Every parity test prints its worst error before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref
import motion_scenes as ms
from helpers import assert_parity, bone_morph_reference, fk_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = motion_ref.NO_CLIP
W_BAR, P_BAR = 5e-5, 2e-4


@pytest.fixture(scope="module")
def scene(rz):
    return ms.main_scene()


@pytest.fixture(scope="module")
def refs(scene, oracle):
    """float64 references of the five states of the main scene, computed once: (q, t, w, world [B,16], positions, normals)"""
    s, m = scene, scene["mesh"]
    out = []
    for st in s["states"]:
        q, t, w = motion_ref.blend_reference(s["clips"], st, ms.B, ms.M)
        world = fk_reference(m["parents"], m["bind"], q, t)
        pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], world.reshape(ms.B, 16).astype(np.float32), m["inv_bind"],
                               s["dense"], w.astype(np.float32))
        out.append((q, t, w, world, pr, nr))
    return out


def make_ctx(rz, s, instances=1, morphs="dense", library=True, topology=True):
    m = s["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    if topology:
        c.upload_skeleton_topology(m["parents"], m["bind"])
    if morphs == "dense":
        c.upload_morphs_dense(s["dense"])
    if instances > 1:
        c.set_instances(instances)
    if library:
        c.upload_motions(s["clips"])
    return c


def blended(c, states):
    a, fa, b, fb, bl = zip(*states)
    c.set_pose_blended(a, fa, [NO if x is None else x for x in b], fb, bl)


def snapshot(c, inst=0):
    p, n = c.read(inst)
    return c.read_world(inst), p, n


def same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def hold(c, inst, ref, what):
    _q, _t, _w, world, pr, nr = ref
    wg, pg, ng = snapshot(c, inst)
    assert np.isfinite(wg).all() and np.isfinite(pg).all() and np.isfinite(ng).all(), what
    ew = float(np.abs(wg - world).max()) / max(1.0, float(np.abs(world).max()))
    ep = float((np.linalg.norm(pg - pr, axis=1) / np.maximum(np.linalg.norm(pr, axis=1), 1.0)).max())
    en = float(np.linalg.norm(ng - nr, axis=1).max())
    return ew, ep, en


def test_parity_against_float64_one_character_and_crowd(rz, scene, refs):
    s = scene
    worst = np.zeros(3)
    with make_ctx(rz, s) as c:
        assert c.get_tuning("motion_clips") == 3
        for k, st in enumerate(s["states"]):
            blended(c, [st])
            c.deform()
            worst = np.maximum(worst, hold(c, 0, refs[k], "one character, state %d" % k))
    with make_ctx(rz, s, instances=len(s["states"])) as c:
        blended(c, s["states"])
        c.deform()
        for k in range(len(s["states"])):
            worst = np.maximum(worst, hold(c, k, refs[k], "crowd, instance %d" % k))
    print("blended pose vs float64: world %.3e (bar %.0e x max(1, |ref|)), positions %.3e, normals %.3e (bar %.0e)" % (worst[0], W_BAR, worst[1], worst[2], P_BAR))
    assert worst[0] <= W_BAR and worst[1] <= P_BAR and worst[2] <= P_BAR, worst


def test_endpoints_in_bits(rz, scene):
    s = scene
    with make_ctx(rz, s) as c:
        blended(c, [(0, 4.37, 1, 8.5, 0.0)]); c.deform()
        a = snapshot(c)
        blended(c, [(0, 4.37, 2, -77.0, 0.0)]); c.deform()
        assert same_bits(a, snapshot(c)), "blend 0: the second clip's fields reached the output"
        blended(c, [(0, 4.37, None, 0.0, 0.0)]); c.deform()
        assert same_bits(a, snapshot(c))
        blended(c, [(0, 4.37, 1, 8.5, 1.0)]); c.deform()
        b = snapshot(c)
        blended(c, [(1, 8.5, None, 0.0, 0.0)]); c.deform()
        assert same_bits(b, snapshot(c)), "blend 1 is not exactly the second clip"
        assert not same_bits(a, b)
        alone = []
        for st in s["states"]:
            blended(c, [st]); c.deform()
            alone.append(snapshot(c))
    I = len(s["states"])
    with make_ctx(rz, s, instances=I) as c:
        blended(c, s["states"]); c.deform()
        for k in (1, 2, I - 1):
            assert same_bits(alone[k], snapshot(c, k)), "instance %d of the crowd differs from its state run alone" % k


def test_against_the_existing_sampler(rz, scene):
    s = scene
    worst = 0.0
    with make_ctx(rz, s) as c, make_ctx(rz, s, library=False) as d:
        for k, f in ((0, -2.0), (0, 6.25), (1, 13.5), (2, 9.75), (2, 500.0)):
            d.upload_animation(**s["clips"][k])
            d.set_pose_sampled([f]); d.deform()
            blended(c, [(k, f, None, 0.0, 0.0)]); c.deform()
            (wc, pc, nc), (wd, pd, nd) = snapshot(c), snapshot(d)
            ew = float(np.abs(wc - wd).max()) / max(1.0, float(np.abs(wd).max()))
            ep = float((np.linalg.norm(pc - pd, axis=1) / np.maximum(np.linalg.norm(pd, axis=1), 1.0)).max())
            en = float(np.linalg.norm(nc - nd, axis=1).max())
            worst = max(worst, ew, ep, en)
            assert ew <= 2 * W_BAR and ep <= 2 * P_BAR and en <= 2 * P_BAR, (k, f, ew, ep, en)
    print("library clip alone vs rz_set_pose_sampled: worst difference %.3e" % worst)


def test_replays_do_not_resample(rz, scene):
    s = scene
    with make_ctx(rz, s) as c:
        blended(c, [s["states"][1]])
        assert "motion" not in c.kernel_name()
        c.deform_n(3)
        a = snapshot(c)
        c.deform()
        assert same_bits(a, snapshot(c))
        c.set_tuning(graph=1)
        c.deform_n(40)
        assert same_bits(a, snapshot(c))
        c.time_span(4)
        assert same_bits(a, snapshot(c))


def test_big_pose_ring(rz):
    """B = 300, I = 32: 268 800 bytes of local pose, above the 256 KB that send a pose through the big-pose ring. Eleven poses wrap its
    eight blocks; two instances of every frame against their states alone."""
    s = ms.ring_scene()
    I, n = 32, 11
    rng = np.random.default_rng(12)
    frames = []
    for _ in range(n):
        frames.append([(int(rng.integers(0, 3)), float(rng.uniform(-2, 40)), int(rng.integers(0, 3)), float(rng.uniform(-2, 40)),
                        float(rng.choice([0.0, 0.3, 0.5, 0.8, 1.0]))) for _ in range(I)])
    with make_ctx(rz, s, instances=I, morphs="none") as c, make_ctx(rz, s, morphs="none") as one:
        for k, states in enumerate(frames):
            blended(c, states); c.deform()
            for i in (k % I, I - 1):
                blended(one, [states[i]]); one.deform()
                assert same_bits(snapshot(one), snapshot(c, i)), "frame %d instance %d" % (k, i)


def test_second_chunk_of_morphs_on_the_single_character_path(rz, oracle):
    """M = 260 sparse morphs: the morphs beyond 256 are sampled by a second workgroup. Eleven poses on one context alternate its two pose
    blocks; every one equals the same state on a context that runs them in the opposite order, and one is held to float64."""
    s = ms.sparse_scene()
    m = s["mesh"]
    rng = np.random.default_rng(13)
    states = [(int(rng.integers(0, 2)), float(rng.uniform(-2, 30)), int(rng.integers(0, 2)), float(rng.uniform(-2, 30)), float(rng.choice([0.0, 0.4, 1.0])))
              for _ in range(11)]
    states[3] = ms.SPARSE_STATE

    def ctx():
        c = rz.DeformContext(0)
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"]); c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        c.upload_morphs_sparse(*s["sparse"][:3])
        c.upload_motions(s["clips"])
        return c
    with ctx() as c, ctx() as d:
        fwd, bwd = [], {}
        for st in states:
            blended(c, [st]); c.deform()
            fwd.append(snapshot(c))
        for k in reversed(range(len(states))):
            blended(d, [states[k]]); d.deform()
            bwd[k] = snapshot(d)
        for k in range(len(states)):
            assert same_bits(fwd[k], bwd[k]), "state %d" % k
    q, t, w = motion_ref.blend_reference(s["clips"], states[3], ms.B, ms.M_SPARSE)
    assert np.abs(w[256:]).max() > 0.05                        # the second chunk's weights matter to the frame
    world = fk_reference(m["parents"], m["bind"], q, t)
    from reze_engine_amd import synth
    dense = synth.sparse_to_dense(len(m["pos"]), *s["sparse"][:3])
    pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], world.reshape(ms.B, 16).astype(np.float32), m["inv_bind"], dense, w.astype(np.float32))
    ep = float((np.linalg.norm(fwd[3][1] - pr, axis=1) / np.maximum(np.linalg.norm(pr, axis=1), 1.0)).max())
    print("260 sparse morphs vs float64: positions %.3e" % ep)
    assert ep <= P_BAR


def test_downstream_ik(rz):
    """The leg rig with its IK table: the pose blended on the device against rz_set_pose_local of the float64 blend cast to f32, both through
    rz_fk_kernel<RzIkParams>. Bar: IK's own, 1e-4 of the skeleton's extent (tests/test_gpu_ik.py)."""
    import ik_ref
    s = ms.leg_scene()
    m = s["mesh"]
    extent = ik_ref.extent(ik_ref.bind_positions(m["parents"], m["bind"]))
    worst = 0.0
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"]); c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        c.upload_ik(m["chains"])
        c.upload_motions(s["clips"])
        for st in s["states"]:
            blended(c, [st]); c.deform()
            assert c.get_tuning("effective_fuse_fk") == 0
            wa = c.read_world(0)
            q, t, _ = motion_ref.blend_reference(s["clips"], st, 14, 0)
            c.set_pose_local(q.astype(np.float32), None, t.astype(np.float32)); c.deform()
            wb = c.read_world(0)
            plain = fk_reference(m["parents"], m["bind"], q, t).reshape(14, 16)
            assert np.abs(wb - plain).max() > 0.1, "the IK stage did not move this pose"
            worst = max(worst, float(np.abs(wa.astype(np.float64) - wb).max()) / extent)
    print("blended pose through IK vs the float64 blend uploaded as a local pose: %.3e x extent %.1f" % (worst, extent))
    assert worst <= 1e-4


def test_downstream_bone_morphs_and_sdef(rz, scene, refs):
    import sdef_ref
    from reze_engine_amd import synth
    s, m = scene, scene["mesh"]
    rng = np.random.default_rng(14)
    n = 12
    bm = dict(morph=rng.integers(0, ms.M, size=n), bone=rng.integers(0, ms.B, size=n), t3=rng.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32),
              q4=rng.normal(size=(n, 4)).astype(np.float32) * np.array([0.2, 0.2, 0.2, 0.0], dtype=np.float32) + np.array([0, 0, 0, 1], dtype=np.float32))
    bm["q4"] /= np.linalg.norm(bm["q4"], axis=1, keepdims=True)
    order = np.lexsort((bm["morph"], bm["bone"]))             # folded per bone in ascending morph order
    sd = synth.make_sdef(m, 0.15, seed=9)
    with make_ctx(rz, s) as c:
        c.upload_bone_morphs(bm["morph"], bm["bone"], bm["t3"], bm["q4"])
        c.upload_sdef(sd["idx"], sd["c"], sd["r0"], sd["r1"])
        for k in (1, 2):
            blended(c, [s["states"][k]]); c.deform()
            q, t, w = refs[k][:3]
            q2, t2 = bone_morph_reference(q, t, bm["morph"][order], bm["bone"][order], bm["t3"][order], bm["q4"][order], w)
            world = fk_reference(m["parents"], m["bind"], q2, t2)
            wg, pg, ng = snapshot(c)
            ew = float(np.abs(wg - world).max()) / max(1.0, float(np.abs(world).max()))
            print("bone morphs behind a blended pose, state %d: world %.3e" % (k, ew))
            assert np.abs(world - refs[k][3]).max() > 1e-2 and ew <= W_BAR
            pr, nr = sdef_ref.frame(m["pos"], m["nrm"], m["joints"], m["weights"], wg, m["inv_bind"], sd["idx"], sd["c"], sd["r0"], sd["r1"],
                                    dense=s["dense"], weights=w.astype(np.float32))
            assert_parity(pg, ng, pr, nr, "SDEF pass behind a blended pose, state %d" % k)


def test_forks_and_misuse(rz, scene):
    s = scene
    st = s["states"]
    with make_ctx(rz, s) as c:
        blended(c, [st[1]]); c.deform()
        a = snapshot(c)
        blended(c, [st[2]]); c.deform()
        b = snapshot(c)
        f = c.fork()
        assert f.get_tuning("motion_clips") == 3
        with pytest.raises(rz.RzError):
            c.upload_motions(s["clips"][:2])                  # refused while a fork borrows the library
        for _ in range(2):                                    # two frames in flight, alternating poses
            blended(c, [st[1]]); c.deform()
            blended(f, [st[2]]); f.deform()
        assert same_bits(a, snapshot(c)) and same_bits(b, snapshot(f))
        f.close()
        # refusals leave the resident pose as it was
        for bad in ((3, 1.0, None, 0.0, 0.0), (0, 1.0, 3, 1.0, 0.5), (0, 1.0, 1, 1.0, -0.1), (0, 1.0, 1, 1.0, 1.5), (0, 1.0, 1, 1.0, float("nan")),
                    (0, float("inf"), 1, 1.0, 0.5), (0, 1.0, 1, float("nan"), 0.5), (0, float("nan"), None, 0.0, 0.0)):
            with pytest.raises(rz.RzError) as e:
                blended(c, [bad])
            assert e.value.code == -1, bad
        blended(c, [(0, 1.0, 1, float("nan"), 0.0)])          # a frame that is not used may be anything
        blended(c, [(0, float("nan"), 1, 2.0, 1.0)])
        blended(c, [st[1]])
        c.deform()
        assert same_bits(a, snapshot(c))
        with pytest.raises(rz.RzError):
            blended(c, [(3, 1.0, None, 0.0, 0.0)])
        c.deform()
        assert same_bits(a, snapshot(c)), "a refused call changed the resident pose"
        # map -> set_pose_blended -> commit: the mapping is cancelled
        c.map_pose()
        blended(c, [st[2]])
        with pytest.raises(rz.RzError):
            c.commit_pose()
        c.deform()
        assert same_bits(b, snapshot(c))
        # another morph set: refused until the library is uploaded again
        c.upload_morphs_dense(s["dense"][:5])
        with pytest.raises(rz.RzError):
            blended(c, [st[1]])
        clips5 = ms.clips_for_morphs(s, 5)
        c.upload_motions(clips5)
        blended(c, [st[1]]); c.deform()
        c.upload_motions([])
        assert c.get_tuning("motion_clips") == 0
        with pytest.raises(rz.RzError):
            blended(c, [st[1]])
        c.deform()                                            # the resident pose outlives its library
    with make_ctx(rz, s, topology=False) as c:
        with pytest.raises(rz.RzError):
            blended(c, [st[1]])
    with make_ctx(rz, s, library=False) as c:
        with pytest.raises(rz.RzError):
            blended(c, [st[1]])
        bad = dict(s["clips"][0])
        bad["key_frame"] = bad["key_frame"].copy(); bad["key_frame"][1] = bad["key_frame"][0] - 1.0
        with pytest.raises(rz.RzError):
            c.upload_motions([s["clips"][1], bad])            # checked like rz_upload_animation, clip by clip
        assert c.get_tuning("motion_clips") == 0
        c.upload_motions(s["clips"])
        c.upload_skeleton(s["mesh"]["inv_bind"])              # a new skeleton drops the library
        assert c.get_tuning("motion_clips") == 0


@pytest.mark.parametrize("I", [1, 3])
def test_both_motion_stores_in_one_context(rz, scene, I):
    """One context holds the single motion (clip 1) AND the library with masks; sampled, blended and layered poses alternate, a frame after each.
    Every frame equals, in bits, the frame of a context that holds only the store that pose reads — a parameter block built from the wrong
    store would not. Then the library is replaced under the sampled pose and the motion under the blended one: neither moves. I = 1: frames
    and states ride in the kernel arguments; I = 3: in device arrays."""
    s = scene
    rng = np.random.default_rng(31)
    masks = (rng.random((2, ms.B)) < 0.5).astype(np.uint8), (rng.random((2, ms.M)) < 0.5).astype(np.uint8)
    pack = rz.DeformContext.pack_motion_states

    def pose(c, kind, t):
        if kind == "sampled":
            c.set_pose_sampled([3.25 + 2.5 * i + 4.0 * t for i in range(I)])
            return
        a, fa, b, fb, bl = zip(*[s["states"][(t + i) % len(s["states"])] for i in range(I)])
        b = [NO if x is None else x for x in b]
        if kind == "blended":
            c.set_pose_blended(a, fa, b, fb, bl)
        else:
            c.set_pose_layered(pack(I, a, fa, b, fb, bl),
                               [[dict(clip=(i + t) % 3, frame=5.5 + i, weight=0.6, mask=i % 2), dict(clip=2, frame=7.25 + t, mask=1 - i % 2, additive=True)] for i in range(I)])

    def frame(c, kind, t):
        pose(c, kind, t)
        c.deform()
        return [snapshot(c, i) for i in range(I)]

    def same(x, y):
        return all(same_bits(a, b) for a, b in zip(x, y))
    with make_ctx(rz, s, instances=I) as both, make_ctx(rz, s, instances=I, library=False) as single, make_ctx(rz, s, instances=I) as lib:
        both.upload_animation(**s["clips"][1])
        single.upload_animation(**s["clips"][1])
        both.upload_motion_masks(*masks)
        lib.upload_motion_masks(*masks)
        seen = []
        for t in range(2):
            for kind in ("sampled", "blended", "layered"):
                got = frame(both, kind, t)
                assert same(got, frame(single if kind == "sampled" else lib, kind, t)), (kind, t)
                seen.append(got)
        assert not same(seen[0], seen[1]) and not same(seen[1], seen[2]) and not same(seen[0], seen[3])
        # another library under the sampled pose
        both.upload_motions(s["clips"][::-1])
        assert same(frame(both, "sampled", 1), seen[3])
        lib.upload_motions(s["clips"][::-1])
        other = frame(both, "blended", 1)
        assert same(other, frame(lib, "blended", 1)) and not same(other, seen[4])
        # another motion under the blended pose
        both.upload_animation(**s["clips"][2])
        assert same(frame(both, "blended", 1), other)
        assert same(frame(both, "layered", 1), frame(lib, "layered", 1))
        single.upload_animation(**s["clips"][2])
        assert same(frame(both, "sampled", 0), frame(single, "sampled", 0))


def test_variants_build_equals_the_product(rz, rzv, scene):
    s = scene
    out = []
    for lib in (rz, rzv):
        with make_ctx(lib, s) as c:
            got = []
            for st in s["states"]:
                blended(c, [st]); c.deform()
                got.append(snapshot(c))
            out.append(got)
    for k in range(len(s["states"])):
        assert same_bits(out[0][k], out[1][k]), "state %d" % k


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_end_to_end(rz, tmp_path):
    """tests/js/motion_e2e.js: a host engine (seekMotions -> applyBlendedFrame) and a { deviceFK, deviceSampling } engine on the same
    synthetic PMX and two VMDs at six states, then a crowd of three."""
    import pmx_synth
    files = ms.write_node_scene(pmx_synth, str(tmp_path))
    (tmp_path / "states.json").write_text(json.dumps(ms.NODE_STATES))
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "motion_e2e.js"), files["pmx"], files["vmd_a"], files["vmd_b"], str(tmp_path / "states.json")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print("node: device vs host positions %.3e over %d states; crowd of %d" % (out["worst"], out["states"], out["crowd"]))
    assert out["states"] == 6 and out["crowd"] == 3 and out["moved"] > 0.2
    assert out["worst"] <= P_BAR
    assert out["crowd_bits_equal"] is True
