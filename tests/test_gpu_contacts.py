"""Contacts between PMX rigid bodies on the device (rz_physics_contacts, the CONTACT instantiations of kernels/physics.hip) against the float64
definition tests/contact_ref.py.

The bar is that of tests/test_gpu_physics.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning and for
contact activity on the CPU (tests/test_contact_cpu.py). Every test prints its largest error before it asserts."""
import shutil

import numpy as np
import pytest

import contact_ref
import contact_scenes as cs
import physics_gpu as pg
import physics_scenes as ps
from physics_gpu import BAR, assert_bar, bits, dyn_bones, errors, keys_of, make_ctx, run, set_local

pytestmark = pytest.mark.gpu
KEYS = pg.KEYS[:5]


@pytest.mark.parametrize("name", list(cs._CASES))
def test_case_against_the_definition(rz, oracle, name):
    """every case of contact_scenes (the four instantiations, the strides of pass F and pass D, the shape pairs in both index orders,
    friction on and off, the reset into penetration, a table with its own h, iterations and gravity) over its calls, the pose changing
    between calls; the lists' counts are the definition's, the launch takes the form the case is there for, and contacts moved something"""
    sc, poses, calls = cs.case(name)
    ref, _ = cs.reference(name)
    L = contact_ref.contact_lists(sc["table"])
    errs = []
    with make_ctx(rz, sc, contacts=1) as c:
        assert [c.get_tuning(k) for k in KEYS] == keys_of(L, 1)
        if name in cs.FORMS:
            assert (c.get_tuning("physics_block"), c.get_tuning("physics_own")) == cs.FORMS[name]
        for (q, t), n, (rw, rs) in zip(poses, calls, ref):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
    plain = cs.run_reference(sc, poses, calls)
    moved = float(np.abs(plain[-1][1][:, :3] - ref[-1][1][:, :3]).max())
    print("%s: %d follow entries, %d dynamic pairs in %d colours; contacts move the last state by %.3f" % (name, L["n_follow"], L["n_pairs"], L["n_colours"], moved))
    assert moved > 0.01
    assert_bar(errs, name)


def test_crowd_instances_equal_the_sequence_run_alone(rz, oracle):
    """three instances, each at poses of its own, against the reference per instance, and instance 1 bit for bit, state and overrides,
    against the same sequence run alone"""
    pg.crowd_against_alone(rz, oracle, cs, 1, "contacts")


@pytest.mark.parametrize("name", ["own 64", "three colours"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with contacts on (follow entries; dynamic pairs in several colours)"""
    sc, poses, calls = cs.case(name)
    pg.steps_add_up(rz, sc, poses[:3], cs.SHORT, 1, name)


@pytest.mark.parametrize("kind", ["no candidate pair", "pairs out of reach", "on and off again"])
def test_bit_identical_to_contacts_never_enabled(rz, kind):
    """state and overrides, bit for bit, against the same table stepped without rz_physics_contacts: with every mask 0 (empty lists), with
    pairs that never come within reach (the stage runs and corrects nothing), and with contacts turned on and off again"""
    if kind == "pairs out of reach":
        sc = cs.apart()
    else:
        sc = cs.case("own 64")[0]
        if kind == "no candidate pair":
            sc = cs.masked(sc)
    calls = cs.SHORT
    poses = [cs.pose(sc, k) for k in range(len(calls))]
    bones = dyn_bones(sc)
    L = contact_ref.contact_lists(sc["table"])
    if kind == "no candidate pair":
        assert L["n_follow"] + L["n_pairs"] == 0
    if kind == "pairs out of reach":
        assert L["n_follow"] > 0 and L["n_pairs"] > 0
    sa, wa = run(rz, sc, poses, calls, 0)
    sb, wb = run(rz, sc, poses, calls, int(kind != "on and off again"), toggle=kind == "on and off again")
    print("%s: state differs by %.2e, overrides by %.2e" % (kind, np.abs(sa - sb).max(), np.abs(wa[bones] - wb[bones]).max()))
    assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(bits(wa[bones]), bits(wb[bones]))


def test_replays_do_not_advance(rz):
    """rz_deform_n replays the resident overrides with contacts on: the state and the frame stay where the step left them; enabling and
    disabling between replays changes no frame either (the overrides are resident, the simulation is not reset)"""
    sc, poses, _ = cs.case("own 64")
    with make_ctx(rz, sc, contacts=1) as c:
        for k, n in enumerate(cs.SHORT):
            set_local(c, [poses[k]])
            c.physics_step(n)
        c.deform()
        st, w, p = c.read_physics(0), c.read_world(0), c.read(0)[0]
        c.deform_n(5)
        assert np.array_equal(bits(st), bits(c.read_physics(0))) and np.array_equal(bits(w), bits(c.read_world(0))) and np.array_equal(bits(p), bits(c.read(0)[0]))
        c.physics_contacts(False)
        c.deform_n(3)
        c.physics_contacts(True)
        c.deform()
        assert np.array_equal(bits(st), bits(c.read_physics(0))) and np.array_equal(bits(p), bits(c.read(0)[0]))
        c.physics_step(1)
        assert not np.array_equal(bits(st), bits(c.read_physics(0)))


def test_misuse(rz):
    """every refusal of rz_physics_contacts with its message, and the context untouched afterwards"""
    sc, poses, _ = cs.case("own 64")
    m = sc["mesh"]
    refused = lambda fn, word, code=None: pg.refused(rz, fn, word, code)
    with make_ctx(rz, sc) as c:
        # no table
        c.upload_physics(None)
        refused(lambda: c.physics_contacts(True), "no physics table", code=-1)
        refused(lambda: c.physics_contacts(False), "no physics table", code=-1)
        # a table without group / mask / friction: rz_upload_physics takes it, contacts do not
        for keys in (("group",), ("mask", "friction")):
            t = dict(sc["table"])
            for k in keys:
                t[k] = None
            c.upload_physics(t)
            for k in keys:
                refused(lambda: c.physics_contacts(True), " " + k, code=-1)
            assert c.get_tuning("physics_contacts") == 0 and c.get_tuning("physics_bodies") == sc["table"]["n_bodies"]
        c.upload_physics(sc["table"])
        # forks
        c.physics_contacts(True)
        before = [c.get_tuning(k) for k in KEYS]
        f = c.fork()
        try:
            refused(lambda: c.physics_contacts(False), "fork")
            refused(lambda: c.physics_contacts(True), "fork")
        finally:
            f.close()
        assert [c.get_tuning(k) for k in KEYS] == before and before[0] == 1
        set_local(c, [poses[1]])
        c.physics_step(2)
        # a new table, a removal, a new topology: off again
        c.upload_physics(sc["table"])
        assert [c.get_tuning(k) for k in KEYS] == [0] * 5
        c.physics_contacts(True)
        c.upload_skeleton_topology(m["parents"], m["bind"])
        assert [c.get_tuning(k) for k in KEYS] == [0] * 5 and c.get_tuning("physics_bodies") == 0
    # beyond the candidate limit: 256 dynamic x 257 following bodies; the previous lists stay
    big, ok = cs.limit_table(257), cs.limit_table(256)
    with pg.two_bone_ctx(rz, m) as c:
        c.upload_physics(ok)
        c.physics_contacts(True)
        assert [c.get_tuning(k) for k in KEYS] == [1, 65536, 0, 0, 0]
        c.upload_physics(big)
        refused(lambda: c.physics_contacts(True), "65792 follow entries and 0 dynamic pairs", code=-6)
        with pytest.raises(rz.capi.RzError) as e:
            c.physics_contacts(True)
        assert "broad phase" in str(e.value)
        assert [c.get_tuning(k) for k in KEYS] == [0] * 5 and c.get_tuning("physics_bodies") == 513


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, physicsContacts: true }) on the PMX physics_scenes.write_pmx writes for a
    contact scene (it carries group, mask and friction): the frames are held to the float64 reference with contacts, run with the table the
    loader must derive and the same substeps; the same engine without the option is held to the contact-free reference"""
    sc, data, q = cs.node_case()
    info = pg.node_run(tmp_path, data, q, ("true", "off"), KEYS)
    calls = ps.node_substeps()
    L = contact_ref.contact_lists(sc["table"])
    assert tuple(info["true"]["substeps"]) == calls and tuple(info["off"]["substeps"]) == calls
    assert info["true"]["keys"] == keys_of(L, 1) and info["off"]["keys"] == [0] * 5
    n, ext = len(calls), sc["extent"]
    poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * n
    refs = dict(on=cs.run_reference(sc, poses, calls, sim=cs.sim_of(sc)), off=cs.run_reference(sc, poses, calls))
    for tag, option in (("on", "true"), ("off", "off")):
        ex, eq, ew, ep = pg.node_errors(tmp_path, option, oracle, sc, refs[tag])
        print("node engine, contacts %s, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (tag, n, sum(calls), ex, eq, ew, ep, ext))
        assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    moved = float(np.abs(refs["on"][-1][1][:, :3] - refs["off"][-1][1][:, :3]).max())
    print("contacts move the last frame's bodies by %.3f" % moved)
    assert moved > 0.05
