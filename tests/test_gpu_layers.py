"""Layered device poses (rz_upload_motion_masks / rz_set_pose_layered, rz_motion_kernel<RzLayerParams> of kernels/motion.hip) against their float64 definition
tests/layer_ref.py, and through everything that runs behind a local pose.

Inputs follow one rule (tests/layer_scenes.py; tests/test_layer_cpu.py asserts it on exactly these states): override clips keep every key
of a bone within 45 degrees of a per-bone base, additive clips within 15 degrees of identity, at most two additive layers below an override
layer — so every slerp spans at most 120 degrees (|dot| >= 0.5) and the precision its sign choice is taken in cannot flip it.

Shapes are those of tests/test_gpu_motion.py, the smallest that reach every path: V = 2048, B = 300 (a second chunk of bones), M = 8 dense;
M = 260 sparse (a second chunk of morphs); B = 300 x I = 32 = 268 800 bytes of local pose (the big-pose ring).

Bars: world matrices within 5e-5 x max(1, |ref|) of fk_reference(layer_ref), positions and normals within 2e-4 of the oracle on those
matrices and weights — the project's own for this sampler arithmetic (tests/test_gpu_motion.py); each layer adds one slerp and one product
of forms already under those bars. Every parity test prints its worst error before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import layer_ref
import layer_scenes as ls
from helpers import fk_reference
from layer_ref import ADDITIVE as ADD, NO_CLIP, OVERRIDE as OVR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_BAR, P_BAR = 5e-5, 2e-4
NAN = float("nan")


@pytest.fixture(scope="module")
def scene(rz):
    return ls.main_scene()


@pytest.fixture(scope="module")
def refs(scene, oracle):
    """float64 references of the six states of the main scene, computed once: (world [B,16], positions, normals)"""
    s, m = scene, scene["mesh"]
    out = []
    for base, layers in s["states"]:
        q, t, w = layer_ref.layered_reference(s["clips"], base, layers, ls.B, ls.M, s["bone_masks"], s["morph_masks"])
        world = fk_reference(m["parents"], m["bind"], q, t)
        pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], world.reshape(ls.B, 16).astype(np.float32), m["inv_bind"],
                               s["dense"], w.astype(np.float32))
        out.append((world, pr, nr))
    return out


def make_ctx(rz, s, instances=1, morphs="dense", masks=True, clips=None):
    m = s["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"])
    if morphs == "dense":
        c.upload_morphs_dense(s["dense"])
    elif morphs == "sparse":
        c.upload_morphs_sparse(*s["sparse"][:3])
    if instances > 1:
        c.set_instances(instances)
    c.upload_motions(s["clips"] if clips is None else clips)
    if masks:
        c.upload_motion_masks(s["bone_masks"], s.get("morph_masks") if morphs != "none" else None)
    return c


def pack(rz, states):
    """(base records [I], layer records [I, n]) of a list of (base, layers)"""
    a, fa, b, fb, bl = zip(*[st for st, _ in states])
    base = rz.DeformContext.pack_motion_states(len(states), a, fa, [-1 if x is None else x for x in b], fb, bl)
    rows = [[dict(clip=-1 if ly[0] is None or ly[0] == NO_CLIP else ly[0], frame=ly[1], weight=ly[2], mask=ly[3], mode=ly[4]) for ly in layers] for _, layers in states]
    return base, rz.DeformContext.pack_motion_layers(len(states), rows)


def layered(rz, c, states):
    c.set_pose_layered(*pack(rz, states))


def blended(c, bases):
    a, fa, b, fb, bl = zip(*bases)
    c.set_pose_blended(a, fa, [-1 if x is None else x for x in b], fb, bl)


def snapshot(c, inst=0):
    p, n = c.read(inst)
    return c.read_world(inst), p, n


def same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def hold(c, inst, ref, what):
    world, pr, nr = ref
    wg, pg, ng = snapshot(c, inst)
    assert np.isfinite(wg).all() and np.isfinite(pg).all() and np.isfinite(ng).all(), what
    ew = float(np.abs(wg - world).max()) / max(1.0, float(np.abs(world).max()))
    ep = float((np.linalg.norm(pg - pr, axis=1) / np.maximum(np.linalg.norm(pr, axis=1), 1.0)).max())
    en = float(np.linalg.norm(ng - nr, axis=1).max())
    return ew, ep, en


def test_parity_against_float64_one_character_and_crowd(rz, scene, refs):
    s = scene
    worst = np.zeros(3)
    moved = 0.0
    with make_ctx(rz, s) as c:
        assert c.get_tuning("motion_masks") == 4 and c.get_tuning("motion_clips") == 5
        for k, st in enumerate(s["states"]):
            layered(rz, c, [st])
            c.deform()
            worst = np.maximum(worst, hold(c, 0, refs[k], "one character, state %d" % k))
            if st[1]:
                a = snapshot(c)[0]
                blended(c, [st[0]]); c.deform()
                moved = max(moved, float(np.abs(a - snapshot(c)[0]).max()))
    assert moved > 0.1, "the layers did not move the pose"
    with make_ctx(rz, s, instances=len(s["states"])) as c:
        layered(rz, c, s["states"])
        c.deform()
        for k in range(len(s["states"])):
            worst = np.maximum(worst, hold(c, k, refs[k], "crowd, instance %d" % k))
    print("layered pose vs float64: world %.3e (bar %.0e x max(1, |ref|)), positions %.3e, normals %.3e (bar %.0e)" % (worst[0], W_BAR, worst[1], worst[2], P_BAR))
    assert worst[0] <= W_BAR and worst[1] <= P_BAR and worst[2] <= P_BAR, worst


def test_second_chunk_of_morphs_and_morph_masks(rz, oracle):
    """M = 260 sparse morphs, morph masks that flip at 255|256: two states against float64"""
    from reze_engine_amd import synth
    s = ls.sparse_scene()
    m = s["mesh"]
    dense = synth.sparse_to_dense(len(m["pos"]), *s["sparse"][:3])
    worst = np.zeros(3)
    with make_ctx(rz, s, morphs="sparse") as c:
        for k, (base, layers) in enumerate(s["states"]):
            q, t, w = layer_ref.layered_reference(s["clips"], base, layers, ls.B, ls.M_SPARSE, s["bone_masks"], s["morph_masks"])
            w0 = layer_ref.layered_reference(s["clips"], base, layers, ls.B, ls.M_SPARSE, s["bone_masks"], None)[2]
            assert np.abs(w[250:] - w0[250:]).max() > 0.05           # the morph masks matter on both sides of 255|256
            world = fk_reference(m["parents"], m["bind"], q, t)
            pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], world.reshape(ls.B, 16).astype(np.float32), m["inv_bind"], dense, w.astype(np.float32))
            layered(rz, c, [(base, layers)]); c.deform()
            worst = np.maximum(worst, hold(c, 0, (world, pr, nr), "sparse state %d" % k))
    print("layered pose, 260 sparse morphs vs float64: world %.3e, positions %.3e, normals %.3e" % tuple(worst))
    assert worst[0] <= W_BAR and worst[1] <= P_BAR and worst[2] <= P_BAR, worst


def test_nothing_to_apply_is_the_blended_pose_in_bits(rz, scene):
    s = scene
    bases = [st for st, _ in s["states"]]
    nothing = [[], [(NO_CLIP, NAN, 0.5, 0, OVR), (3, NAN, 0.0, 9, 7)], [(3, 5.0, 0.35, 2, OVR), (4, 6.0, 1.0, 2, ADD), (0, 1.0, 1.0, 2, OVR), (1, 2.0, 0.6, 2, ADD)]]
    with make_ctx(rz, s) as c:
        for base in bases:
            blended(c, [base]); c.deform()
            want = snapshot(c)
            for layers in nothing:
                layered(rz, c, [(base, layers)]); c.deform()
                assert same_bits(want, snapshot(c)), (base, layers)
    I = len(bases)
    with make_ctx(rz, s, instances=I) as c:
        blended(c, bases); c.deform()
        want = [snapshot(c, k) for k in range(I)]
        for layers in nothing:
            layered(rz, c, [(b, layers) for b in bases]); c.deform()
            for k in range(I):
                assert same_bits(want[k], snapshot(c, k)), (k, layers)


def test_body_with_face_on_top_is_their_concatenation_in_bits(rz, scene):
    s = scene
    body, face, cat = ls.body_and_face()
    with make_ctx(rz, s, clips=[body, face, cat], masks=False) as c:
        for f in (-1.0, 6.25, 13.5, 400.0):
            blended(c, [(2, f, None, 0.0, 0.0)]); c.deform()
            want = snapshot(c)
            layered(rz, c, [((0, f, None, 0.0, 0.0), [(1, f, 1.0, None, OVR)])]); c.deform()
            assert same_bits(want, snapshot(c)), f
            blended(c, [(0, f, None, 0.0, 0.0)]); c.deform()
            assert not same_bits(want, snapshot(c))


def test_crowd_instances_equal_their_states_alone_and_the_variants_build(rz, rzv, scene):
    s = scene
    alone = []
    for lib in (rz, rzv):
        with make_ctx(lib, s) as c:
            got = []
            for st in s["states"]:
                layered(rz, c, [st]); c.deform()
                got.append(snapshot(c))
            alone.append(got)
    I = len(s["states"])
    for k in range(I):
        assert same_bits(alone[0][k], alone[1][k]), "state %d: the variants build differs from the product" % k
    with make_ctx(rz, s, instances=I) as c:
        layered(rz, c, s["states"]); c.deform()
        for k in range(I):
            assert same_bits(alone[0][k], snapshot(c, k)), "instance %d of the crowd differs from its state run alone" % k


def test_replays_do_not_resample(rz, scene):
    s = scene
    with make_ctx(rz, s) as c:
        layered(rz, c, [s["states"][3]])
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
    """B = 300, I = 32: 268 800 bytes of local pose, above the 256 KB that send a pose through the big-pose ring. Eleven layered poses wrap
    its eight blocks; two instances of every frame against their states alone."""
    s = ls.ring_scene()
    I, n = 32, 11
    rng = np.random.default_rng(12)
    frames = []
    for k in range(n):
        nl = (4, 1, 3)[k % 3]
        frames.append([((int(rng.integers(0, 3)), float(rng.uniform(-2, 40)), int(rng.integers(0, 3)), float(rng.uniform(-2, 40)), float(rng.choice([0.0, 0.3, 0.5, 1.0]))),
                        ls.random_layers(rng, nl)) for _ in range(I)])
    with make_ctx(rz, s, instances=I, morphs="none") as c, make_ctx(rz, s, morphs="none") as one:
        for k, states in enumerate(frames):
            layered(rz, c, states); c.deform()
            for i in (k % I, I - 1):
                layered(rz, one, [states[i]]); one.deform()
                assert same_bits(snapshot(one), snapshot(c, i)), "frame %d instance %d" % (k, i)


def test_downstream_ik(rz):
    """The leg rig with its IK table: the layered pose on the device against rz_set_pose_local of the float64 layered pose cast to f32, both
    through rz_fk_kernel<RzIkParams>. Bar: IK's own, 1e-4 of the skeleton's extent (tests/test_gpu_ik.py)."""
    import ik_ref
    s = ls.leg_scene()
    m = s["mesh"]
    extent = ik_ref.extent(ik_ref.bind_positions(m["parents"], m["bind"]))
    worst = 0.0
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"]); c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        c.upload_ik(m["chains"])
        c.upload_motions(s["clips"])
        c.upload_motion_masks(s["bone_masks"])
        for base, layers in s["states"]:
            layered(rz, c, [(base, layers)]); c.deform()
            wa = c.read_world(0)
            q, t, _ = layer_ref.layered_reference(s["clips"], base, layers, 14, 0, s["bone_masks"], None)
            q0, t0, _ = layer_ref.layered_reference(s["clips"], base, [], 14, 0)
            assert max(np.abs(q - q0).max(), np.abs(t - t0).max()) > 0.05, "the layers did not move this pose"
            c.set_pose_local(q.astype(np.float32), None, t.astype(np.float32)); c.deform()
            wb = c.read_world(0)
            plain = fk_reference(m["parents"], m["bind"], q, t).reshape(14, 16)
            assert np.abs(wb - plain).max() > 0.1, "the IK stage did not move this pose"
            worst = max(worst, float(np.abs(wa.astype(np.float64) - wb).max()) / extent)
    print("layered pose through IK vs the float64 layered pose uploaded as a local pose: %.3e x extent %.1f" % (worst, extent))
    assert worst <= 1e-4


def test_forks_and_misuse(rz, scene):
    s = scene
    st = s["states"]
    with make_ctx(rz, s) as c:
        layered(rz, c, [st[3]]); c.deform()
        a = snapshot(c)
        layered(rz, c, [st[4]]); c.deform()
        b = snapshot(c)
        f = c.fork()
        assert f.get_tuning("motion_masks") == 4
        with pytest.raises(rz.RzError):
            c.upload_motion_masks(s["bone_masks"][:2])            # refused while a fork borrows the masks
        for _ in range(2):                                        # two frames in flight, alternating poses
            layered(rz, c, [st[3]]); c.deform()
            layered(rz, f, [st[4]]); f.deform()
        assert same_bits(a, snapshot(c)) and same_bits(b, snapshot(f))
        f.close()
        # every refusal returns -1, names instance and layer, and leaves the resident pose as it was
        base = st[3][0]
        ok = (3, 5.0, 0.5, 0, OVR)
        for layers in ([(5, 1.0, 0.5, None, OVR)], [ok, (3, 1.0, 0.5, 4, OVR)], [(3, 1.0, 0.5, None, 2)], [(3, 1.0, -0.1, None, OVR)], [(3, 1.0, 1.5, None, ADD)],
                       [ok, ok, (3, 1.0, NAN, None, OVR)], [(3, float("inf"), 0.5, None, OVR)], [(3, NAN, 1.0, None, ADD)], [ok] * 5):
            with pytest.raises(rz.RzError) as e:
                layered(rz, c, [(base, layers)])
            assert e.value.code == -1, layers
            if len(layers) <= 4:
                assert "instance 0 layer %d" % (len(layers) - 1) in str(e.value), str(e.value)
        for bad_base in ((5, 1.0, None, 0.0, 0.0), (0, 1.0, 1, 1.0, 1.5), (0, NAN, None, 0.0, 0.0)):      # what rz_set_pose_blended refuses of the base
            with pytest.raises(rz.RzError) as e:
                layered(rz, c, [(bad_base, [ok])])
            assert e.value.code == -1, bad_base
        L = rz.capi.load()
        base_rec, _ = pack(rz, [(base, [])])
        assert L.rz_set_pose_layered(c._h, base_rec.ctypes.data_as(__import__("ctypes").POINTER(rz.capi.RzMotionState)), 2, None) == -1      # layers == NULL with n_layers > 0
        c.deform()
        assert same_bits(a, snapshot(c)), "a refused call changed the resident pose"
        layered(rz, c, [(base, [(NO_CLIP, NAN, NAN, 77, 9), (3, NAN, 0.0, 77, 9)])])      # a skipped layer may carry anything
        layered(rz, c, [st[3]]); c.deform()
        assert same_bits(a, snapshot(c))
        # map -> set_pose_layered -> commit: the mapping is cancelled
        c.map_pose()
        layered(rz, c, [st[4]])
        with pytest.raises(rz.RzError):
            c.commit_pose()
        c.deform()
        assert same_bits(b, snapshot(c))
        # another morph set: masked layers are refused until the masks are uploaded again (and the library, by its own rule)
        c.upload_morphs_dense(s["dense"][:5])
        clips5 = ls.ms.clips_for_morphs(s, 5)
        c.upload_motions(clips5)
        layered(rz, c, [((0, 2.0, None, 0.0, 0.0), [(1, 3.0, 0.5, None, OVR)])])
        with pytest.raises(rz.RzError) as e:
            layered(rz, c, [((0, 2.0, None, 0.0, 0.0), [(1, 3.0, 0.5, 0, OVR)])])
        assert e.value.code == -1
        c.upload_motion_masks(s["bone_masks"], s["morph_masks"][:, :5])
        layered(rz, c, [((0, 2.0, None, 0.0, 0.0), [(1, 3.0, 0.5, 0, OVR)])]); c.deform()
        c.upload_motion_masks(np.zeros((0, ls.B), dtype=np.uint8))
        assert c.get_tuning("motion_masks") == 0
        with pytest.raises(rz.RzError):
            layered(rz, c, [((0, 2.0, None, 0.0, 0.0), [(1, 3.0, 0.5, 0, OVR)])])
        layered(rz, c, [((0, 2.0, None, 0.0, 0.0), [(1, 3.0, 0.5, None, OVR)])]); c.deform()      # layers without a mask need none
        c.upload_motion_masks(s["bone_masks"])
        assert c.get_tuning("motion_masks") == 4
        c.upload_skeleton(s["mesh"]["inv_bind"])                  # a new skeleton drops the masks
        assert c.get_tuning("motion_masks") == 0


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_end_to_end(rz, tmp_path):
    """tests/js/motion_layers_e2e.js: a host engine (seekMotions with layers -> applyLayeredFrame) and a { deviceFK, deviceSampling } engine
    on the same synthetic PMX and three VMDs (a body pair and a morph-only face file) with setMotionMask(withDescendants), then a crowd of
    three against the single runs."""
    import pmx_synth
    files = ls.write_node_scene(pmx_synth, str(tmp_path))
    (tmp_path / "states.json").write_text(json.dumps(dict(masks=ls.NODE_MASKS, states=ls.NODE_STATES)))
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "motion_layers_e2e.js"), files["pmx"], files["vmd_a"], files["vmd_b"], files["vmd_c"],
                        str(tmp_path / "states.json")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print("node: device vs host positions %.3e over %d layered states; crowd of %d" % (out["worst"], out["states"], out["crowd"]))
    assert out["states"] == len(ls.NODE_STATES) and out["crowd"] == 3 and out["moved"] > 0.05
    assert out["worst"] <= P_BAR
    assert out["crowd_bits_equal"] is True
