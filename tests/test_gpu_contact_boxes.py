"""PMX boxes in the device contact stage (rz_physics_contacts(ctx, 2), the CONTACT = 2 instantiations of kernels/physics.hip) against the
float64 definition tests/contact_box_ref.py.

The bar is that of tests/test_gpu_contacts.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning (the
float32 probe of the definition within 2.5e-5 x extent: a 4 x margin) and for contact activity on the CPU (tests/test_contact_box_cpu.py).
Every test prints its largest error before it asserts; when every case has run, the largest errors per case go to
profiles/contact_box_edges_parity.txt."""
import shutil

import numpy as np
import pytest

import contact_box_scenes as bs
import contact_ref
import physics_gpu as pg
import physics_scenes as ps
from physics_gpu import BAR, assert_bar, bits, dyn_bones, errors, keys_of, make_ctx, run, same, set_local

pytestmark = pytest.mark.gpu
KEYS = pg.KEYS[:6]
HEAD = """Contacts with PMX boxes on the device (rz_physics_contacts(ctx, 2), the CONTACT = 2 instantiations of kernels/physics.hip): largest errors
of the GPU tests against the float64 definition (tests/contact_box_ref.py) on an MI355X, written by
  python -m pytest tests/test_gpu_contact_boxes.py -q -m gpu
when every case has run. The bars: body positions, world-matrix entries and deformed positions 1e-4 x extent, quaternions 1e-4 up to sign,
normals 1e-4. Per case: its lists (follow entries, dynamic pairs, colours, pairs of two boxes left out), how far contacts move the last state
against the same table stepped without them, then the errors. The four launch forms are "own 64" (<64, OWN, 2>), "stride 64", "own 256" and
"stride 256"; fd / df / dd = following body first / dynamic body first / both dynamic. The identities (crowd instance against the sequence
run alone, whole calls against calls of one substep, boxes masked out under mode 1, no box under mode 2, 1 -> 2 -> 1) are bit for bit.
"""
_rows = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    pg.write_parity("contact_box_edges_parity.txt", HEAD, list(bs._CASES), _rows)


@pytest.mark.parametrize("name", list(bs._CASES))
def test_case_against_the_definition(rz, oracle, name):
    """every case of contact_box_scenes (the four instantiations, the shape pairs in both index orders and three roles, the regions of the
    box, the deep case, friction off and on, a pair of two boxes left out, a table with its own h, iterations and gravity) over its calls,
    the pose changing between calls; the lists' counts are the definition's, the launch takes the form the case is there for, and contacts
    moved something"""
    sc, poses, calls = bs.case(name)
    ref, _ = bs.reference(name)
    L = contact_ref.contact_lists(sc["table"], 2)
    errs = []
    with make_ctx(rz, sc, contacts=2) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L, 2)
        if name in bs.FORMS:
            assert (c.get_tuning("physics_block"), c.get_tuning("physics_own")) == bs.FORMS[name]
        for (q, t), n, (rw, rs) in zip(poses, calls, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
    plain = bs.run_reference(sc, poses, calls)
    moved = float(np.abs(plain[-1][1][:, :3] - ref[-1][1][:, :3]).max())
    head = "%s: %d follow entries, %d dynamic pairs in %d colours, %d pairs of two boxes; contacts move the last state by %.3f" % (name, L["n_follow"], L["n_pairs"], L["n_colours"], L["box_pairs"], moved)
    print(head)
    assert moved > 0.01
    _rows[name] = head + "\n" + assert_bar(errs, name)


def test_crowd_instances_equal_the_sequence_run_alone(rz, oracle):
    """three instances, each at poses of its own, against the reference per instance, and instance 1 bit for bit, state and overrides,
    against the same sequence run alone"""
    pg.crowd_against_alone(rz, oracle, bs, 2, "box contacts")


@pytest.mark.parametrize("name", ["own 64", "box capsule dd"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with boxes taking part (follow entries against a box; a dynamic pair with a box)"""
    sc, poses, calls = bs.case(name)
    pg.steps_add_up(rz, sc, poses, calls, 2, name)


@pytest.mark.parametrize("kind", ["boxes under mode 1", "no box under mode 2"])
def test_the_old_paths_are_what_they_were(rz, kind):
    """state and overrides, bit for bit: a table with boxes under on = 1 against the same table with the boxes' masks 0 (mode 1 leaves
    boxes out: same lists but for the count), and a table without any box under on = 2 against on = 1"""
    if kind == "boxes under mode 1":
        sc = bs.case("own 64")[0]
        a_sc, b_sc, a_mode, b_mode = sc, bs.masked_boxes(sc), 1, 1
        L = contact_ref.contact_lists(sc["table"])
        assert L["boxes"] > 0 and L["n_follow"] > 0 and contact_ref.contact_lists(b_sc["table"])["boxes"] == 0
    else:
        sc = bs.no_boxes()
        a_sc, b_sc, a_mode, b_mode = sc, sc, 2, 1
        assert not (sc["table"]["shape"] == 1).any() and contact_ref.contact_lists(sc["table"])["n_follow"] > 0
    calls = bs.SHORT
    poses = [bs.pose(sc, k) for k in range(len(calls))]
    a, b = run(rz, a_sc, poses, calls, a_mode), run(rz, b_sc, poses, calls, b_mode)
    print("%s: state differs by %.2e" % (kind, np.abs(a[0] - b[0]).max()))
    assert same(a, b, dyn_bones(sc))
    with make_ctx(rz, a_sc, contacts=a_mode) as c:
        L = contact_ref.contact_lists(a_sc["table"])
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L, a_mode, 6) and L["box_pairs"] == 0


def test_a_pair_of_two_boxes_is_counted_and_changes_nothing(rz):
    """the table with a pair of two boxes against the same table with that pair masked apart: the count differs, the run does not"""
    a_sc, b_sc = bs.case("box pair")[0], bs.with_box_pair(apart=True)
    _, poses, calls = bs.case("box pair")
    La, Lb = (contact_ref.contact_lists(s["table"], 2) for s in (a_sc, b_sc))
    assert (La["box_pairs"], Lb["box_pairs"]) == (1, 0) and La["n_follow"] == Lb["n_follow"] > 0
    with make_ctx(rz, b_sc, contacts=2) as c:
        assert c.get_tuning("physics_contact_box_pairs") == 0 and c.get_tuning("physics_contact_follow") == Lb["n_follow"]
    a, b = run(rz, a_sc, poses, calls, 2), run(rz, b_sc, poses, calls, 2)
    print("box pair counted vs masked apart: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(a_sc))


def test_switching_between_the_modes(rz):
    """2 -> 0 zeroes every key; 1 -> 2 -> 1 (a substep under 2 in between) leaves the state bit-identical to never having left 1 when the
    boxes are out of reach; the simulation is not reset by any switch"""
    sc, poses, _ = bs.case("own 64")
    with make_ctx(rz, sc, contacts=2) as c:
        set_local(c, [poses[1]])
        c.physics_step(3)
        before = c.read_physics(0)
        assert c.get_tuning("physics_contacts") == 2 and c.get_tuning("physics_contact_follow") > 0
        c.physics_contacts(False)
        assert [c.get_tuning(k) for k in KEYS] == [0] * 6
        assert np.array_equal(bits(before), bits(c.read_physics(0)))
        c.physics_contacts(True)
        assert c.get_tuning("physics_contacts") == 1 and c.get_tuning("physics_contact_box_pairs") == 0
        c.physics_contacts(True, boxes=True)
        assert c.get_tuning("physics_contacts") == 2 and np.array_equal(bits(before), bits(c.read_physics(0)))
    far = bs.far_boxes()
    L1, L2 = contact_ref.contact_lists(far["table"]), contact_ref.contact_lists(far["table"], 2)
    assert L2["n_follow"] > L1["n_follow"] > 0
    calls = bs.SHORT
    poses = [bs.pose(far, k) for k in range(len(calls))]
    # (the detour takes one substep under mode 2 behind the first call: the straight run takes it under mode 1)
    a, b = run(rz, far, poses, calls, 1, detour=(2, 1)), run(rz, far, poses, (calls[0] + 1,) + calls[1:], 1)
    print("1 -> 2 -> 1 against mode 1 throughout: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(far))


def test_refusals(rz):
    """the 65 536-candidate limit with follow entries against boxes (taken at the limit, refused one past it with both counts in the
    message, the context left without contacts), and the fork refusal under on = 2"""
    sc = bs.case("own 64")[0]
    m = sc["mesh"]
    refused = lambda fn, word, code=None: pg.refused(rz, fn, word, code)
    with make_ctx(rz, sc, contacts=2) as c:
        before = [c.get_tuning(k) for k in KEYS]
        f = c.fork()
        try:
            refused(lambda: c.physics_contacts(True, boxes=True), "fork")
            refused(lambda: c.physics_contacts(False), "fork")
        finally:
            f.close()
        assert [c.get_tuning(k) for k in KEYS] == before and before[0] == 2
        c.upload_physics(sc["table"])
        assert [c.get_tuning(k) for k in KEYS] == [0] * 6
    big, ok = bs.limit_table(257), bs.limit_table(256)
    with pg.two_bone_ctx(rz, m) as c:
        c.upload_physics(ok)
        c.physics_contacts(True)
        assert [c.get_tuning(k) for k in KEYS] == [1, 0, 0, 0, 256, 0]
        c.physics_contacts(True, boxes=True)
        assert [c.get_tuning(k) for k in KEYS] == [2, 65536, 0, 0, 0, 0]
        c.upload_physics(big)
        refused(lambda: c.physics_contacts(True, boxes=True), "65792 follow entries and 0 dynamic pairs", code=-6)
        assert [c.get_tuning(k) for k in KEYS] == [0] * 6 and c.get_tuning("physics_bodies") == 513
        c.physics_contacts(True)
        assert [c.get_tuning(k) for k in KEYS] == [1, 0, 0, 0, 257, 0]


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, physicsContacts: 'boxes' }) on the PMX physics_scenes.write_pmx writes for
    the box strands (a box torso, box plates): the frames are held to the float64 definition, run with the table the loader must derive
    and the same substeps"""
    sc, data, q = bs.node_case()
    info = pg.node_run(tmp_path, data, q, ("boxes",), KEYS)["boxes"]
    calls = ps.node_substeps()
    L = contact_ref.contact_lists(sc["table"], 2)
    assert tuple(info["substeps"]) == calls
    assert info["keys"] == keys_of(L, 2) and L["box"].any()
    n, ext = len(calls), sc["extent"]
    poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * n
    sim = bs.sim_of(sc)
    ref = bs.run_reference(sc, poses, calls, sim=sim)
    ex, eq, ew, ep = pg.node_errors(tmp_path, "boxes", oracle, sc, ref)
    print("node engine, box contacts, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (n, sum(calls), ex, eq, ew, ep, ext))
    assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    plain = bs.run_reference(sc, poses, calls, sim=bs.sim_of(sc, mode=1))
    moved = float(np.abs(ref[-1][1][:, :3] - plain[-1][1][:, :3]).max())
    print("boxes move the last frame's bodies by %.3f against contacts without them; %d box contacts" % (moved, sum(sim.regions.values())))
    assert moved > 0.05
