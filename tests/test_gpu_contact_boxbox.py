"""Contacts between two PMX boxes in the device contact stage (rz_physics_contacts(ctx, 3), the CONTACT = 3 instantiations of
kernels/physics.hip) against the float64 definition tests/contact_boxbox_ref.py.

The bar is that of tests/test_gpu_contacts.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning (the
float32 probe of the definition within 2.5e-5 x extent: a 4 x margin) and for box - box contact activity on the CPU
(tests/test_contact_boxbox_cpu.py). Every test prints its largest error before it asserts; when every case has run, the largest errors per
case go to profiles/contact_boxbox_edges_parity.txt."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_box_ref
import contact_box_scenes as bs
import contact_boxbox_ref as xr
import contact_boxbox_scenes as xs
import physics_scenes as ps
from physics_gpu import BAR, assert_bar, bits, dyn_bones, errors, make_ctx, same, set_local

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("physics_contacts", "physics_contact_follow", "physics_contact_pairs", "physics_contact_colours", "physics_contact_boxes", "physics_contact_box_pairs",
        "physics_contact_box_box")
PARITY = os.path.join(ROOT, "profiles", "contact_boxbox_edges_parity.txt")
HEAD = """Contacts between two PMX boxes on the device (rz_physics_contacts(ctx, 3), the CONTACT = 3 instantiations of kernels/physics.hip): largest
errors of the GPU tests against the float64 definition (tests/contact_boxbox_ref.py) on an MI355X, written by
  python -m pytest tests/test_gpu_contact_boxbox.py -q -m gpu
when every case has run. The bars: body positions, world-matrix entries and deformed positions 1e-4 x extent, quaternions 1e-4 up to sign,
normals 1e-4. Per case: its lists (follow entries, dynamic pairs, colours, pairs of two boxes among them), how far the contacts between boxes
move the last state against the definition of mode 2 on the same table, then the errors. The four launch forms are "own 64" (<64, OWN, 3>),
"stride 64", "own 256" and "stride 256"; fd / df / dd = following box first / dynamic box first / both dynamic. The identities (crowd
instance against the sequence run alone, whole calls against calls of one substep, no pair of two boxes under mode 3 against mode 2, a pair
separated along one axis against the pair masked apart, 2 -> 3 -> 2) are bit for bit.
"""
_rows = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    if set(_rows) >= set(xs._CASES):
        with open(PARITY, "w") as f:
            f.write(HEAD + "\n" + "".join(_rows[name] + "\n" for name in xs._CASES))


def set_mode(c, mode):
    """the contact stage's mode: 0 off, 1 spheres and capsules, 2 boxes too, 3 and boxes against boxes"""
    c.physics_contacts(bool(mode), boxes=mode >= 2, box_pairs=mode == 3)


def ctx_of(rz, sc, mode=3, instances=1):
    c = make_ctx(rz, sc, instances=instances)
    set_mode(c, mode)
    return c


def keys_of(L, mode=3):
    return [mode, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"], L["box_pairs"], L["n_box_box"]]


def run(rz, sc, poses, calls, mode=3, split=False, detour=()):
    """one instance through the calls; (state, world) after the last frame. split: every call of n substeps as n calls of one. detour: the
    modes to pass through (ending in `mode` again) behind the first call, a substep under each that is not `mode`"""
    with ctx_of(rz, sc, mode) as c:
        for k, ((q, t), n) in enumerate(zip(poses, calls)):
            set_local(c, [(q, t)])
            for part in ([1] * n if split else [n]):
                c.physics_step(part)
            c.deform()
            if k == 0:
                for m in detour:
                    set_mode(c, m)
                    assert c.get_tuning("physics_contacts") == m
                    if m != mode:
                        c.physics_step(1)
        return c.read_physics(0), c.read_world(0)


@pytest.mark.parametrize("name", list(xs._CASES))
def test_case_against_the_definition(rz, oracle, name):
    """every case of contact_boxbox_scenes (the four instantiations, the three roles, the kinds of contact — a face of A, a face of B, edge
    on edge, a vertex on a face, an edge lying on a face, face on face, the footprint clamp, a near-parallel pair whose edge axes are
    skipped —, friction off and on, a table with its own h, iterations and gravity) over its calls, the pose changing between calls; the
    lists' counts are the definition's, the launch takes the form the case is there for, and the contacts between boxes moved something"""
    sc, poses, calls = xs.case(name)
    ref, _ = xs.reference(name)
    L = xr.contact_lists(sc["table"])
    errs = []
    with ctx_of(rz, sc) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L) and L["n_box_box"] > 0
        if name in xs.FORMS:
            assert (c.get_tuning("physics_block"), c.get_tuning("physics_own")) == xs.FORMS[name]
        for (q, t), n, (rw, rs) in zip(poses, calls, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
    moved = float(np.abs(xs.mode2(name)[-1][1][:, :3] - ref[-1][1][:, :3]).max())
    head = "%s: %d follow entries, %d dynamic pairs in %d colours, %d pairs of two boxes; their contacts move the last state by %.3f" % (name, L["n_follow"], L["n_pairs"], L["n_colours"], L["n_box_box"], moved)
    print(head)
    assert moved > 0.01
    _rows[name] = head + "\n" + assert_bar(errs, name)


def test_crowd_instances_equal_the_sequence_run_alone(rz, oracle):
    """three instances, each at poses of its own, against the reference per instance, and instance 1 bit for bit, state and overrides,
    against the same sequence run alone"""
    sc, _, _ = xs.case(xs.CROWD)
    I, calls = 3, xs.SHORT
    amounts = (0.5, 0.35, 0.6)
    bones = dyn_bones(sc)
    poses = [[xs.pose(sc, k, amounts[i], turn=0.05 + 0.02 * i) for k in range(len(calls))] for i in range(I)]
    refs = [xs.run_reference(sc, poses[i], calls, sim=xs.sim_of(sc)) for i in range(I)]
    errs = []
    with ctx_of(rz, sc, instances=I) as c:
        for call, n in enumerate(calls):
            set_local(c, [poses[i][call] for i in range(I)])
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, *refs[i][call]))
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "crowd of %d with contacts between boxes" % I)
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01
    alone = run(rz, sc, poses[1], calls)
    print("instance 1 alone vs in the crowd: state differs by %.2e" % np.abs(alone[0] - crowd[1][0]).max())
    assert same(alone, crowd[1], bones)


@pytest.mark.parametrize("name", ["own 64", "box box dd"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with pairs of two boxes taking part (follow entries; a dynamic pair)"""
    sc, poses, calls = xs.case(name)
    a, b = run(rz, sc, poses, calls), run(rz, sc, poses, calls, split=True)
    print("%s: whole calls vs calls of one substep: state differs by %.2e" % (name, np.abs(a[0] - b[0]).max()))
    assert same(a, b, dyn_bones(sc))


def test_without_a_pair_of_two_boxes_mode_3_is_mode_2(rz):
    """state and overrides, bit for bit: a table with boxes and no pair of two of them (the box pair scene with the pair masked apart)
    under on = 3 against on = 2, the keys but for the mode the same"""
    sc = bs.with_box_pair(apart=True)
    L = xr.contact_lists(sc["table"])
    assert L["n_box_box"] == 0 and L["box"].any() and L["n_follow"] > 0
    calls = xs.SHORT
    poses = [xs.pose(sc, k, 0.3) for k in range(len(calls))]
    a, b = run(rz, sc, poses, calls, mode=3), run(rz, sc, poses, calls, mode=2)
    print("no pair of two boxes, mode 3 vs mode 2: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(sc))
    with ctx_of(rz, sc) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L)


def test_the_box_pair_scene_differs_from_mode_2(rz):
    """contact_box_scenes' "box pair" (a dynamic box plate whose only partner is the following box): mode 2 counts the pair and leaves it
    out, mode 3 takes it — the keys say so and the run differs"""
    sc, poses, calls = bs.case("box pair")
    L2, L3 = contact_box_ref.contact_lists(sc["table"], boxes=True), xr.contact_lists(sc["table"])
    assert (L2["box_pairs"], L3["box_pairs"], L3["n_box_box"]) == (1, 0, 1) and L3["n_follow"] == L2["n_follow"] + 1
    with ctx_of(rz, sc, 2) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(dict(L2, n_box_box=0), 2)
        set_mode(c, 3)
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L3)
    a, b = run(rz, sc, poses, calls, mode=3), run(rz, sc, poses, calls, mode=2)
    d = float(np.abs(a[0][:, :3] - b[0][:, :3]).max())
    print("box pair under mode 3 vs mode 2: positions differ by %.3f" % d)
    assert np.isfinite(a[0]).all() and d > 0.01


@pytest.mark.parametrize("kind", ["A", "B", "edge"])
def test_a_pair_separated_along_one_axis_changes_nothing(rz, kind):
    """two boxes that overlap along fourteen of the fifteen axes (the one left: a face axis of A, a face axis of B, an edge pair) against the
    same pair masked apart: the count differs, the run does not"""
    a_sc, b_sc = xs.single_axis(kind), xs.single_axis(kind, apart=True)
    La, Lb = xr.contact_lists(a_sc["table"]), xr.contact_lists(b_sc["table"])
    assert (La["n_box_box"], Lb["n_box_box"]) == (1, 0) and La["n_follow"] == Lb["n_follow"] + 1 > 1
    poses, calls = xs.single_axis_poses(a_sc), xs.SHORT
    a, b = run(rz, a_sc, poses, calls), run(rz, b_sc, poses, calls)
    print("separated along %s only vs masked apart: state differs by %.2e" % (kind, np.abs(a[0] - b[0]).max()))
    assert same(a, b, dyn_bones(a_sc))


def test_switching_between_the_modes(rz):
    """3 -> 0 zeroes every key; 2 -> 3 -> 2 (a substep under 3 in between) leaves the state bit-identical to never having left 2 when the
    boxes are out of each other's reach; the simulation is not reset by any switch"""
    sc, poses, _ = xs.case("own 64")
    with ctx_of(rz, sc) as c:
        set_local(c, [poses[1]])
        c.physics_step(3)
        before = c.read_physics(0)
        assert c.get_tuning("physics_contacts") == 3 and c.get_tuning("physics_contact_box_box") > 0
        c.physics_contacts(False)
        assert [c.get_tuning(k) for k in KEYS] == [0] * len(KEYS)
        assert np.array_equal(bits(before), bits(c.read_physics(0)))
        for mode in (1, 2, 3, 2, 1, 3):
            set_mode(c, mode)
            assert c.get_tuning("physics_contacts") == mode and (c.get_tuning("physics_contact_box_box") > 0) == (mode == 3)
            assert (c.get_tuning("physics_contact_box_pairs") > 0) == (mode == 2)
            assert np.array_equal(bits(before), bits(c.read_physics(0)))
    far = bs.far_boxes()
    L2, L3 = xr.contact_lists(far["table"], box_pairs=False), xr.contact_lists(far["table"])
    assert L3["n_follow"] > L2["n_follow"] > 0 and L3["n_box_box"] == L2["box_pairs"] > 0
    calls = xs.SHORT
    poses = [xs.pose(far, k) for k in range(len(calls))]
    # (the detour takes one substep under mode 3 behind the first call: the straight run takes it under mode 2)
    a, b = run(rz, far, poses, calls, mode=2, detour=(3, 2)), run(rz, far, poses, (calls[0] + 1,) + calls[1:], mode=2)
    print("2 -> 3 -> 2 against mode 2 throughout: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(far))


def test_refusals(rz):
    """the 65 536-candidate limit with pairs of two boxes counted (taken at the limit, refused one past it with the counts in the message,
    the context left as it was: contacts, keys and state), and the fork refusal under on = 3"""
    import test_contact_boxbox_cpu as tc
    sc, poses, _ = xs.case("own 64")
    m = sc["mesh"]

    def refused(fn, word, code=None):
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        assert word in str(e.value), str(e.value)
        if code is not None:
            assert e.value.code == code, e.value.code
    with ctx_of(rz, sc) as c:
        before = [c.get_tuning(k) for k in KEYS]
        f = c.fork()
        try:
            refused(lambda: set_mode(c, 3), "fork")
            refused(lambda: set_mode(c, 2), "fork")
            refused(lambda: c.physics_contacts(False), "fork")
        finally:
            f.close()
        assert [c.get_tuning(k) for k in KEYS] == before and before[0] == 3
    big, ok = tc.limit_table(257), tc.limit_table(256)
    Lbig, Lok = xr.contact_lists(big), xr.contact_lists(ok)
    assert Lok["n_follow"] == Lok["n_box_box"] == 65536 and Lbig["n_follow"] == Lbig["n_box_box"] == 65792
    B = 2
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], np.zeros_like(m["joints"]), m["weights"])
        inv = np.zeros((B, 16), dtype=np.float32); inv[:, [0, 5, 10, 15]] = 1
        c.upload_skeleton(inv)
        c.upload_skeleton_topology(np.array([-1, 0], dtype=np.int32), np.zeros((B, 3), dtype=np.float32))
        c.upload_physics(ok)
        set_mode(c, 2)
        assert [c.get_tuning(k) for k in KEYS] == [2, 0, 0, 0, 0, 65536, 0]
        set_mode(c, 3)
        assert [c.get_tuning(k) for k in KEYS] == keys_of(Lok)
        c.upload_physics(big)
        set_mode(c, 2)
        q = np.zeros((1, B, 4), dtype=np.float32); q[..., 3] = 1
        c.set_pose_local(q, None, np.zeros((1, B, 3), dtype=np.float32))
        c.physics_step(1)
        state, keys = c.read_physics(0), [c.get_tuning(k) for k in KEYS]
        assert keys == [2, 0, 0, 0, 0, 65792, 0]
        refused(lambda: set_mode(c, 3), xr.refusal(Lbig), code=-6)
        assert "65792 follow entries and 0 dynamic pairs (65792 of them pairs of two boxes)" == xr.refusal(Lbig)
        assert [c.get_tuning(k) for k in KEYS] == keys and np.array_equal(bits(state), bits(c.read_physics(0)))


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, physicsContacts: 'all' }) on the PMX physics_scenes.write_pmx writes for
    the box strands (a box torso, box plates): the frames are held to the float64 definition, run with the table the loader must derive
    and the same substeps"""
    sc, data, q = xs.node_case()
    m, B, ext = sc["mesh"], sc["B"], sc["extent"]
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "contact_boxbox_e2e.js"), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"), str(tmp_path)]
                                  + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    calls = ps.node_substeps()
    L = xr.contact_lists(sc["table"])
    assert tuple(info["substeps"]) == calls
    assert info["keys"] == keys_of(L) and L["n_box_box"] > 0
    n, V = len(calls), len(m["pos"])
    poses = [(q, np.zeros((B, 3), dtype=np.float32))] * n
    sim = xs.sim_of(sc)
    ref = xs.run_reference(sc, poses, calls, sim=sim)
    pos = np.fromfile(str(tmp_path / "pos.f32"), dtype=np.float32).reshape(n, V, 3)
    world = np.fromfile(str(tmp_path / "world.f32"), dtype=np.float32).reshape(n, B, 16)
    state = np.fromfile(str(tmp_path / "state.f32"), dtype=np.float32).reshape(n, -1, 13)
    ex = ew = ep = eq = 0.0
    for k, (rw, rs) in enumerate(ref):
        ex = max(ex, float(np.abs(state[k][:, :3] - rs[:, :3]).max()) / ext)
        eq = max(eq, float(np.minimum(np.abs(state[k][:, 3:7] - rs[:, 3:7]).max(axis=1), np.abs(state[k][:, 3:7] + rs[:, 3:7]).max(axis=1)).max()))
        ew = max(ew, float(np.abs(world[k] - rw).max()) / ext)
        pr_, _ = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], rw.astype(np.float32), m["inv_bind"])
        ep = max(ep, float(np.abs(pos[k].astype(np.float64) - pr_).max()) / ext)
    print("node engine, contacts between boxes, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (n, sum(calls), ex, eq, ew, ep, ext))
    assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    plain = xs.run_reference(sc, poses, calls, sim=xs.sim_of(sc, box_pairs=False))
    moved = float(np.abs(ref[-1][1][:, :3] - plain[-1][1][:, :3]).max())
    print("contacts between boxes move the last frame's bodies by %.3f against mode 2; %d of them" % (moved, sim.n_boxbox))
    assert moved > 0.01 and sim.n_boxbox > 0
