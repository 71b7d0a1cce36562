"""PMX boxes in the device contact stage (rz_physics_contacts(ctx, 2), the CONTACT = 2 instantiations of kernels/physics.hip) against the
float64 definition tests/contact_box_ref.py.

The bar is that of tests/test_gpu_contacts.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning (the
float32 probe of the definition within 2.5e-5 x extent: a 4 x margin) and for contact activity on the CPU (tests/test_contact_box_cpu.py).
Every test prints its largest error before it asserts; when every case has run, the largest errors per case go to
profiles/contact_box_edges_parity.txt."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_box_ref
import contact_box_scenes as bs
import contact_ref
import physics_scenes as ps
from physics_gpu import BAR, assert_bar, bits, dyn_bones, errors, make_ctx, same, set_local, set_mode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("physics_contacts", "physics_contact_follow", "physics_contact_pairs", "physics_contact_colours", "physics_contact_boxes", "physics_contact_box_pairs")
PARITY = os.path.join(ROOT, "profiles", "contact_box_edges_parity.txt")
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
    if set(_rows) >= set(bs._CASES):
        with open(PARITY, "w") as f:
            f.write(HEAD + "\n" + "".join(_rows[name] + "\n" for name in bs._CASES))


def run(rz, sc, poses, calls, mode=2, split=False, detour=()):
    """one instance through the calls; (state, world) after the last frame. split: every call of n substeps as n calls of one. detour: the
    modes to pass through (ending in `mode` again) behind the first call"""
    with make_ctx(rz, sc, contacts=mode) as c:
        for k, ((q, t), n) in enumerate(zip(poses, calls)):
            set_local(c, [(q, t)])
            for part in ([1] * n if split else [n]):
                c.physics_step(part)
            c.deform()
            if k == 0:
                for m in detour:
                    set_mode(c, m)
                    assert c.get_tuning("physics_contacts") == m
                    if m == 2:
                        c.physics_step(1)
        return c.read_physics(0), c.read_world(0)


@pytest.mark.parametrize("name", list(bs._CASES))
def test_case_against_the_definition(rz, oracle, name):
    """every case of contact_box_scenes (the four instantiations, the shape pairs in both index orders and three roles, the regions of the
    box, the deep case, friction off and on, a pair of two boxes left out, a table with its own h, iterations and gravity) over its calls,
    the pose changing between calls; the lists' counts are the definition's, the launch takes the form the case is there for, and contacts
    moved something"""
    sc, poses, calls = bs.case(name)
    ref, _ = bs.reference(name)
    L = contact_box_ref.contact_lists(sc["table"], boxes=True)
    errs = []
    with make_ctx(rz, sc, contacts=2) as c:
        assert [c.get_tuning(k) for k in KEYS] == [2, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"], L["box_pairs"]]
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
    sc, _, _ = bs.case(bs.CROWD)
    I, calls = 3, bs.SHORT
    amounts = (0.5, 0.35, 0.6)
    bones = dyn_bones(sc)
    poses = [[bs.pose(sc, k, amounts[i], turn=0.05 + 0.02 * i) for k in range(len(calls))] for i in range(I)]
    refs = [bs.run_reference(sc, poses[i], calls, sim=bs.sim_of(sc)) for i in range(I)]
    errs = []
    with make_ctx(rz, sc, instances=I, contacts=2) as c:
        for call, n in enumerate(calls):
            set_local(c, [poses[i][call] for i in range(I)])
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, *refs[i][call]))
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "crowd of %d with box contacts" % I)
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01
    alone = run(rz, sc, poses[1], calls)
    print("instance 1 alone vs in the crowd: state differs by %.2e" % np.abs(alone[0] - crowd[1][0]).max())
    assert same(alone, crowd[1], bones)


@pytest.mark.parametrize("name", ["own 64", "box capsule dd"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with boxes taking part (follow entries against a box; a dynamic pair with a box)"""
    sc, poses, calls = bs.case(name)
    a, b = run(rz, sc, poses, calls), run(rz, sc, poses, calls, split=True)
    print("%s: whole calls vs calls of one substep: state differs by %.2e" % (name, np.abs(a[0] - b[0]).max()))
    assert same(a, b, dyn_bones(sc))


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
    a, b = run(rz, a_sc, poses, calls, mode=a_mode), run(rz, b_sc, poses, calls, mode=b_mode)
    print("%s: state differs by %.2e" % (kind, np.abs(a[0] - b[0]).max()))
    assert same(a, b, dyn_bones(sc))
    with make_ctx(rz, a_sc, contacts=a_mode) as c:
        L = contact_ref.contact_lists(a_sc["table"])
        assert [c.get_tuning(k) for k in KEYS] == [a_mode, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"], 0]


def test_a_pair_of_two_boxes_is_counted_and_changes_nothing(rz):
    """the table with a pair of two boxes against the same table with that pair masked apart: the count differs, the run does not"""
    a_sc, b_sc = bs.case("box pair")[0], bs.with_box_pair(apart=True)
    _, poses, calls = bs.case("box pair")
    La, Lb = (contact_box_ref.contact_lists(s["table"], boxes=True) for s in (a_sc, b_sc))
    assert (La["box_pairs"], Lb["box_pairs"]) == (1, 0) and La["n_follow"] == Lb["n_follow"] > 0
    with make_ctx(rz, b_sc, contacts=2) as c:
        assert c.get_tuning("physics_contact_box_pairs") == 0 and c.get_tuning("physics_contact_follow") == Lb["n_follow"]
    a, b = run(rz, a_sc, poses, calls), run(rz, b_sc, poses, calls)
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
    L1, L2 = contact_ref.contact_lists(far["table"]), contact_box_ref.contact_lists(far["table"], boxes=True)
    assert L2["n_follow"] > L1["n_follow"] > 0
    calls = bs.SHORT
    poses = [bs.pose(far, k) for k in range(len(calls))]
    # (the detour takes one substep under mode 2 behind the first call: the straight run takes it under mode 1)
    a, b = run(rz, far, poses, calls, mode=1, detour=(2, 1)), run(rz, far, poses, (calls[0] + 1,) + calls[1:], mode=1)
    print("1 -> 2 -> 1 against mode 1 throughout: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, dyn_bones(far))


def test_refusals(rz):
    """the 65 536-candidate limit with follow entries against boxes (taken at the limit, refused one past it with both counts in the
    message, the context left without contacts), and the fork refusal under on = 2"""
    import test_contact_box_cpu as tc
    sc = bs.case("own 64")[0]
    m = sc["mesh"]

    def refused(fn, word, code=None):
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        assert word in str(e.value), str(e.value)
        if code is not None:
            assert e.value.code == code, e.value.code
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
    big, ok = tc.limit_table(257), tc.limit_table(256)
    B = 2
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], np.zeros_like(m["joints"]), m["weights"])
        inv = np.zeros((B, 16), dtype=np.float32); inv[:, [0, 5, 10, 15]] = 1
        c.upload_skeleton(inv)
        c.upload_skeleton_topology(np.array([-1, 0], dtype=np.int32), np.zeros((B, 3), dtype=np.float32))
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
    m, B, ext = sc["mesh"], sc["B"], sc["extent"]
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "contact_boxes_e2e.js"), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"), str(tmp_path)]
                                  + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    calls = ps.node_substeps()
    L = contact_box_ref.contact_lists(sc["table"], boxes=True)
    assert tuple(info["substeps"]) == calls
    assert info["keys"] == [2, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"], L["box_pairs"]] and L["box"].any()
    n, V = len(calls), len(m["pos"])
    poses = [(q, np.zeros((B, 3), dtype=np.float32))] * n
    sim = bs.sim_of(sc)
    ref = bs.run_reference(sc, poses, calls, sim=sim)
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
    print("node engine, box contacts, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (n, sum(calls), ex, eq, ew, ep, ext))
    assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    plain = bs.run_reference(sc, poses, calls, sim=contact_ref.Sim(sc["table"], sc["parents"], sc["bind"]))
    moved = float(np.abs(ref[-1][1][:, :3] - plain[-1][1][:, :3]).max())
    print("boxes move the last frame's bodies by %.3f against contacts without them; %d box contacts" % (moved, sum(sim.regions.values())))
    assert moved > 0.05
