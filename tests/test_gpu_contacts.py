"""Contacts between PMX rigid bodies on the device (rz_physics_contacts, the CONTACT instantiations of kernels/physics.hip) against the float64
definition tests/contact_ref.py.

The bar is that of tests/test_gpu_physics.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning and for
contact activity on the CPU (tests/test_contact_cpu.py). Every test prints its largest error before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_ref
import contact_scenes as cs
import physics_scenes as ps
from physics_gpu import BAR, assert_bar, bits, dyn_bones, errors, make_ctx, set_local

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("physics_contacts", "physics_contact_follow", "physics_contact_pairs", "physics_contact_colours", "physics_contact_boxes")


def run(rz, sc, poses, calls, contacts=True, toggle=False, split=False):
    """one instance through the calls; (state, world) after the last frame. toggle: contacts on and off again before the first step.
    split: every call of n substeps as n calls of one"""
    with make_ctx(rz, sc, contacts=int(contacts)) as c:
        if toggle:
            c.physics_contacts(True)
            assert c.get_tuning("physics_contacts") == 1
            c.physics_contacts(False)
            assert [c.get_tuning(k) for k in KEYS] == [0] * 5
        for (q, t), n in zip(poses, calls):
            set_local(c, [(q, t)])
            for part in ([1] * n if split else [n]):
                c.physics_step(part)
            c.deform()
        return c.read_physics(0), c.read_world(0)


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
        assert [c.get_tuning(k) for k in KEYS] == [1, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"]]
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
    sc, _, _ = cs.case(cs.CROWD)
    I, calls = 3, cs.SHORT
    amounts = (0.5, 0.35, 0.6)
    bones = dyn_bones(sc)
    poses = [[cs.pose(sc, k, amounts[i], turn=0.05 + 0.02 * i) for k in range(len(calls))] for i in range(I)]
    refs = [cs.run_reference(sc, poses[i], calls, sim=contact_ref.Sim(sc["table"], sc["parents"], sc["bind"])) for i in range(I)]
    errs = []
    with make_ctx(rz, sc, instances=I, contacts=1) as c:
        for call, n in enumerate(calls):
            set_local(c, [poses[i][call] for i in range(I)])
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, *refs[i][call]))
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "crowd of %d with contacts" % I)
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01
    st, w = run(rz, sc, poses[1], calls)
    print("instance 1 alone vs in the crowd: state differs by %.2e, overrides by %.2e" % (np.abs(st - crowd[1][0]).max(), np.abs(w[bones] - crowd[1][1][bones]).max()))
    assert np.array_equal(bits(st), bits(crowd[1][0])) and np.array_equal(bits(w[bones]), bits(crowd[1][1][bones]))


@pytest.mark.parametrize("name", ["own 64", "three colours"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with contacts on (follow entries; dynamic pairs in several colours)"""
    sc, poses, calls = cs.case(name)
    bones = dyn_bones(sc)
    (sa, wa), (sb, wb) = run(rz, sc, poses[:3], cs.SHORT), run(rz, sc, poses[:3], cs.SHORT, split=True)
    print("%s: whole calls vs calls of one substep: state differs by %.2e, overrides by %.2e" % (name, np.abs(sa - sb).max(), np.abs(wa[bones] - wb[bones]).max()))
    assert np.isfinite(sa).all() and np.array_equal(bits(sa), bits(sb)) and np.array_equal(bits(wa[bones]), bits(wb[bones]))


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
    sa, wa = run(rz, sc, poses, calls, contacts=False)
    sb, wb = run(rz, sc, poses, calls, contacts=kind != "on and off again", toggle=kind == "on and off again")
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

    def refused(fn, word, code=None):
        with pytest.raises(rz.capi.RzError) as e:
            fn()
        assert word in str(e.value), str(e.value)
        if code is not None:
            assert e.value.code == code, e.value.code
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
    import test_contact_cpu as tc
    big, ok = tc.limit_table(257), tc.limit_table(256)
    B = 2
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], np.zeros_like(m["joints"]), m["weights"])
        inv = np.zeros((B, 16), dtype=np.float32); inv[:, [0, 5, 10, 15]] = 1
        c.upload_skeleton(inv)
        c.upload_skeleton_topology(np.array([-1, 0], dtype=np.int32), np.zeros((B, 3), dtype=np.float32))
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
    m, B, ext = sc["mesh"], sc["B"], sc["extent"]
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "contacts_e2e.js"), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"), str(tmp_path)]
                                  + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    calls = ps.node_substeps()
    L = contact_ref.contact_lists(sc["table"])
    assert tuple(info["on"]) == calls and tuple(info["off"]) == calls
    assert info["onKeys"] == [1, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"]] and info["offKeys"] == [0] * 5
    n, V = len(calls), len(m["pos"])
    poses = [(q, np.zeros((B, 3), dtype=np.float32))] * n
    refs = dict(on=cs.run_reference(sc, poses, calls, sim=contact_ref.Sim(sc["table"], sc["parents"], sc["bind"])), off=cs.run_reference(sc, poses, calls))
    for tag in ("on", "off"):
        pos = np.fromfile(str(tmp_path / ("pos_%s.f32" % tag)), dtype=np.float32).reshape(n, V, 3)
        world = np.fromfile(str(tmp_path / ("world_%s.f32" % tag)), dtype=np.float32).reshape(n, B, 16)
        state = np.fromfile(str(tmp_path / ("state_%s.f32" % tag)), dtype=np.float32).reshape(n, -1, 13)
        ex = ew = ep = eq = 0.0
        for k, (rw, rs) in enumerate(refs[tag]):
            ex = max(ex, float(np.abs(state[k][:, :3] - rs[:, :3]).max()) / ext)
            eq = max(eq, float(np.minimum(np.abs(state[k][:, 3:7] - rs[:, 3:7]).max(axis=1), np.abs(state[k][:, 3:7] + rs[:, 3:7]).max(axis=1)).max()))
            ew = max(ew, float(np.abs(world[k] - rw).max()) / ext)
            pr_, _ = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], rw.astype(np.float32), m["inv_bind"])
            ep = max(ep, float(np.abs(pos[k].astype(np.float64) - pr_).max()) / ext)
        print("node engine, contacts %s, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (tag, n, sum(calls), ex, eq, ew, ep, ext))
        assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    moved = float(np.abs(refs["on"][-1][1][:, :3] - refs["off"][-1][1][:, :3]).max())
    print("contacts move the last frame's bodies by %.3f" % moved)
    assert moved > 0.05
