"""Contacts between two PMX boxes in the device contact stage (rz_physics_contacts(ctx, 3), the CONTACT = 3 instantiations of
kernels/physics.hip) against the float64 definition tests/contact_boxbox_ref.py.

The bar is that of tests/test_gpu_contacts.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning (the
float32 probe of the definition within 2.5e-5 x extent: a 4 x margin) and for box - box contact activity on the CPU
(tests/test_contact_boxbox_cpu.py). Every test prints its largest error before it asserts; when every case has run, the largest errors per
case go to profiles/contact_boxbox_edges_parity.txt."""
import shutil

import numpy as np
import pytest

import contact_box_scenes as bs
import contact_boxbox_scenes as xs
import contact_ref
import physics_gpu as pg
import physics_scenes as ps
from physics_gpu import BAR, KEYS, assert_bar, bits, dyn_bones, errors, keys_of, make_ctx, run, same, set_local, set_mode

pytestmark = pytest.mark.gpu
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
    pg.write_parity("contact_boxbox_edges_parity.txt", HEAD, list(xs._CASES), _rows)


@pytest.mark.parametrize("name", list(xs._CASES))
def test_case_against_the_definition(rz, oracle, name):
    """every case of contact_boxbox_scenes (the four instantiations, the three roles, the kinds of contact — a face of A, a face of B, edge
    on edge, a vertex on a face, an edge lying on a face, face on face, the footprint clamp, a near-parallel pair whose edge axes are
    skipped —, friction off and on, a table with its own h, iterations and gravity) over its calls, the pose changing between calls; the
    lists' counts are the definition's, the launch takes the form the case is there for, and the contacts between boxes moved something"""
    sc, poses, calls = xs.case(name)
    ref, _ = xs.reference(name)
    L = contact_ref.contact_lists(sc["table"], 3)
    errs = []
    with make_ctx(rz, sc, contacts=3) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L, 3) and L["n_box_box"] > 0
        if name in xs.FORMS:
            assert (c.get_tuning("physics_block"), c.get_tuning("physics_own")) == xs.FORMS[name]
        for (q, t), n, (rw, rs) in zip(poses, calls, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
    moved = float(np.abs(xs.reference(name, mode=2)[0][-1][1][:, :3] - ref[-1][1][:, :3]).max())
    head = "%s: %d follow entries, %d dynamic pairs in %d colours, %d pairs of two boxes; their contacts move the last state by %.3f" % (name, L["n_follow"], L["n_pairs"], L["n_colours"], L["n_box_box"], moved)
    print(head)
    assert moved > 0.01
    _rows[name] = head + "\n" + assert_bar(errs, name)


def test_crowd_instances_equal_the_sequence_run_alone(rz, oracle):
    """three instances, each at poses of its own, against the reference per instance, and instance 1 bit for bit, state and overrides,
    against the same sequence run alone"""
    pg.crowd_against_alone(rz, oracle, xs, 3, "contacts between boxes")


@pytest.mark.parametrize("name", ["own 64", "box box dd"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with pairs of two boxes taking part (follow entries; a dynamic pair)"""
    sc, poses, calls = xs.case(name)
    pg.steps_add_up(rz, sc, poses, calls, 3, name)


def test_without_a_pair_of_two_boxes_mode_3_is_mode_2(rz):
    """state and overrides, bit for bit: a table with boxes and no pair of two of them (the box pair scene with the pair masked apart)
    under on = 3 against on = 2, the keys but for the mode the same"""
    sc = bs.with_box_pair(apart=True)
    L = contact_ref.contact_lists(sc["table"], 3)
    assert L["n_box_box"] == 0 and L["box"].any() and L["n_follow"] > 0
    calls = xs.SHORT
    poses = [xs.pose(sc, k, 0.3) for k in range(len(calls))]
    a, b = run(rz, sc, poses, calls, 3), run(rz, sc, poses, calls, 2)
    print("no pair of two boxes, mode 3 vs mode 2: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(sc))
    with make_ctx(rz, sc, contacts=3) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L, 3)


def test_the_box_pair_scene_differs_from_mode_2(rz):
    """contact_box_scenes' "box pair" (a dynamic box plate whose only partner is the following box): mode 2 counts the pair and leaves it
    out, mode 3 takes it — the keys say so and the run differs"""
    sc, poses, calls = bs.case("box pair")
    L2, L3 = contact_ref.contact_lists(sc["table"], 2), contact_ref.contact_lists(sc["table"], 3)
    assert (L2["box_pairs"], L3["box_pairs"], L3["n_box_box"]) == (1, 0, 1) and L3["n_follow"] == L2["n_follow"] + 1
    with make_ctx(rz, sc, contacts=2) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L2, 2, 7)
        set_mode(c, 3)
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L3, 3)
    a, b = run(rz, sc, poses, calls, 3), run(rz, sc, poses, calls, 2)
    d = float(np.abs(a[0][:, :3] - b[0][:, :3]).max())
    print("box pair under mode 3 vs mode 2: positions differ by %.3f" % d)
    assert np.isfinite(a[0]).all() and d > 0.01


@pytest.mark.parametrize("kind", ["A", "B", "edge"])
def test_a_pair_separated_along_one_axis_changes_nothing(rz, kind):
    """two boxes that overlap along fourteen of the fifteen axes (the one left: a face axis of A, a face axis of B, an edge pair) against the
    same pair masked apart: the count differs, the run does not"""
    a_sc, b_sc = xs.single_axis(kind), xs.single_axis(kind, apart=True)
    La, Lb = contact_ref.contact_lists(a_sc["table"], 3), contact_ref.contact_lists(b_sc["table"], 3)
    assert (La["n_box_box"], Lb["n_box_box"]) == (1, 0) and La["n_follow"] == Lb["n_follow"] + 1 > 1
    poses, calls = xs.single_axis_poses(a_sc), xs.SHORT
    a, b = run(rz, a_sc, poses, calls, 3), run(rz, b_sc, poses, calls, 3)
    print("separated along %s only vs masked apart: state differs by %.2e" % (kind, np.abs(a[0] - b[0]).max()))
    assert same(a, b, dyn_bones(a_sc))


def test_switching_between_the_modes(rz):
    """3 -> 0 zeroes every key; 2 -> 3 -> 2 (a substep under 3 in between) leaves the state bit-identical to never having left 2 when the
    boxes are out of each other's reach; the simulation is not reset by any switch"""
    sc, poses, _ = xs.case("own 64")
    with make_ctx(rz, sc, contacts=3) as c:
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
    L2, L3 = contact_ref.contact_lists(far["table"], 2), contact_ref.contact_lists(far["table"], 3)
    assert L3["n_follow"] > L2["n_follow"] > 0 and L3["n_box_box"] == L2["box_pairs"] > 0
    calls = xs.SHORT
    poses = [xs.pose(far, k) for k in range(len(calls))]
    # (the detour takes one substep under mode 3 behind the first call: the straight run takes it under mode 2)
    a, b = run(rz, far, poses, calls, 2, detour=(3, 2)), run(rz, far, poses, (calls[0] + 1,) + calls[1:], 2)
    print("2 -> 3 -> 2 against mode 2 throughout: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(far))


def test_refusals(rz):
    """the 65 536-candidate limit with pairs of two boxes counted (taken at the limit, refused one past it with the counts in the message,
    the context left as it was: contacts, keys and state), and the fork refusal under on = 3"""
    sc, poses, _ = xs.case("own 64")
    m = sc["mesh"]
    refused = lambda fn, word, code=None: pg.refused(rz, fn, word, code)
    with make_ctx(rz, sc, contacts=3) as c:
        before = [c.get_tuning(k) for k in KEYS]
        f = c.fork()
        try:
            refused(lambda: set_mode(c, 3), "fork")
            refused(lambda: set_mode(c, 2), "fork")
            refused(lambda: c.physics_contacts(False), "fork")
        finally:
            f.close()
        assert [c.get_tuning(k) for k in KEYS] == before and before[0] == 3
    big, ok = xs.limit_table(257), xs.limit_table(256)
    Lbig, Lok = contact_ref.contact_lists(big, 3), contact_ref.contact_lists(ok, 3)
    assert Lok["n_follow"] == Lok["n_box_box"] == 65536 and Lbig["n_follow"] == Lbig["n_box_box"] == 65792
    B = 2
    with pg.two_bone_ctx(rz, m) as c:
        c.upload_physics(ok)
        set_mode(c, 2)
        assert [c.get_tuning(k) for k in KEYS] == [2, 0, 0, 0, 0, 65536, 0]
        set_mode(c, 3)
        assert [c.get_tuning(k) for k in KEYS] == keys_of(Lok, 3)
        c.upload_physics(big)
        set_mode(c, 2)
        q = np.zeros((1, B, 4), dtype=np.float32); q[..., 3] = 1
        c.set_pose_local(q, None, np.zeros((1, B, 3), dtype=np.float32))
        c.physics_step(1)
        state, keys = c.read_physics(0), [c.get_tuning(k) for k in KEYS]
        assert keys == [2, 0, 0, 0, 0, 65792, 0]
        refused(lambda: set_mode(c, 3), contact_ref.refusal(Lbig), code=-6)
        assert "65792 follow entries and 0 dynamic pairs (65792 of them pairs of two boxes)" == contact_ref.refusal(Lbig)
        assert [c.get_tuning(k) for k in KEYS] == keys and np.array_equal(bits(state), bits(c.read_physics(0)))


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, physicsContacts: 'all' }) on the PMX physics_scenes.write_pmx writes for
    the box strands (a box torso, box plates): the frames are held to the float64 definition, run with the table the loader must derive
    and the same substeps"""
    sc, data, q = xs.node_case()
    info = pg.node_run(tmp_path, data, q, ("all",), KEYS)["all"]
    calls = ps.node_substeps()
    L = contact_ref.contact_lists(sc["table"], 3)
    assert tuple(info["substeps"]) == calls
    assert info["keys"] == keys_of(L, 3) and L["n_box_box"] > 0
    n, ext = len(calls), sc["extent"]
    poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * n
    sim = xs.sim_of(sc)
    ref = xs.run_reference(sc, poses, calls, sim=sim)
    ex, eq, ew, ep = pg.node_errors(tmp_path, "all", oracle, sc, ref)
    print("node engine, contacts between boxes, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (n, sum(calls), ex, eq, ew, ep, ext))
    assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    plain = xs.run_reference(sc, poses, calls, sim=xs.sim_of(sc, mode=2))
    moved = float(np.abs(ref[-1][1][:, :3] - plain[-1][1][:, :3]).max())
    print("contacts between boxes move the last frame's bodies by %.3f against mode 2; %d of them" % (moved, sim.n_boxbox))
    assert moved > 0.01 and sim.n_boxbox > 0
