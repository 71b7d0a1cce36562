"""Linear joint springs on the device (rz_physics_springs, the LSPRING instantiations of kernels/physics.hip) against the float64 definition
tests/spring_ref.py.

The bar is that of tests/test_gpu_physics.py: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent
of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4. Every case is checked for conditioning and for
the springs' effect on the CPU (tests/test_spring_cpu.py). Every test prints its largest error before it asserts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import physics_gpu as pg
import physics_scenes as ps
import spring_ref
import spring_scenes as ss
from physics_gpu import BAR, assert_bar, bits, dyn_bones, errors, make_ctx, same, set_local

pytestmark = pytest.mark.gpu
FORM_KEYS = ("physics_block", "physics_own", "physics_contacts", "physics_springs")
_rows = {}
HEAD = ("Linear joint springs on the device against tests/spring_ref.py in float64, per case of tests/spring_scenes.py: the largest errors over the\n"
        "case's calls and the form the launch took (lanes per workgroup, joints in registers, contact mode, springs). Written by\n"
        "tests/test_gpu_springs.py on an MI355X.")


def form_of(c):
    return tuple(c.get_tuning(k) for k in FORM_KEYS)


def lds_of(t, own, springs):
    return t["n_bodies"] * 96 + (0 if own else t["n_joints"] * (24 if springs else 12))


def run(rz, sc, poses, calls, mode=0, springs="on", split=False, toggle_between=False):
    """one instance through the calls; (state, world) after the last frame. springs: "never" — no call; "on"; "on off" — on and off again
    before the first step. split: every call of n substeps as n calls of one. toggle_between: off and on again between the frames"""
    with make_ctx(rz, sc) as c:
        if springs != "never":
            c.physics_springs(True)
            assert c.get_tuning("physics_springs") == 1
        if springs == "on off":
            c.physics_springs(False)
            assert c.get_tuning("physics_springs") == 0 and c.get_tuning("physics_spring_axes") == 0
        if mode:
            pg.set_mode(c, mode)
        for (q, t), n in zip(poses, calls):
            set_local(c, [(q, t)])
            for part in ([1] * n if split else [n]):
                c.physics_step(part)
            c.deform()
            if toggle_between:
                before = c.read_physics(0)
                c.physics_springs(False)
                assert np.array_equal(bits(before), bits(c.read_physics(0)))
                c.physics_springs(True)
                assert np.array_equal(bits(before), bits(c.read_physics(0)))
        return c.read_physics(0), c.read_world(0)


@pytest.mark.parametrize("name", ss.ORDER)
def test_case_against_the_definition(rz, oracle, name):
    """every case of spring_scenes — the four launch forms without contacts and under each contact mode (the sixteen LSPRING
    instantiations), one axis at a time in frames turned away from the bodies', the roles a joint's bodies can have, a table with its own
    h and one iteration, the largest strands table the doubled multipliers admit — over its calls, the pose changing between calls; the
    launch takes the form the case is there for, with the LDS the header states"""
    sc, poses, calls = ss.case(name)
    _, mode, (block, own) = ss.CASES[name]
    ref = ss.reference(name)
    t = sc["table"]
    errs = []
    with make_ctx(rz, sc) as c:
        c.physics_springs(True)
        if mode:
            pg.set_mode(c, mode)
        form = form_of(c)
        assert form == (block, own, mode, 1), form
        assert c.get_tuning("physics_spring_axes") == ss.axes_of(t) and c.get_tuning("physics_lds") == lds_of(t, own, True)
        for (q, tr), n, (rw, rs) in zip(poses, calls, ref):
            set_local(c, [(q, tr)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
    line = assert_bar(errs, name)
    _rows[name] = "%s  [%d lanes, own %d, contacts %d, springs %d; %d bodies, %d joints, %d spring axes]" % ((line,) + form + (t["n_bodies"], t["n_joints"], ss.axes_of(t)))
    pg.write_parity("spring_edges_parity.txt", HEAD, ss.ORDER, _rows)


def test_every_new_instantiation_is_launched():
    """the cases' forms cover (64 | 256 lanes) x (joints in registers | striding) x (contact mode 0 .. 3), all with the springs on"""
    forms = {ss.CASES[n][2] + (ss.CASES[n][1],) for n in ss.ORDER}
    assert forms == {(b, o, m) for b in (64, 256) for o in (0, 1) for m in (0, 1, 2, 3)}


def test_the_springs_move_the_crowd_scene(rz):
    """fails without the feature: on the "own 64" case the stepped state with the springs differs from the state without the call by what
    the definition says, at least 100 x the bar (tests/test_spring_cpu.py asserts that margin of the definition)"""
    sc, poses, calls = ss.case(ss.CROWD)
    on, off = run(rz, sc, poses, calls), run(rz, sc, poses, calls, springs="never")
    moved = float(np.abs(on[0][:, :3] - off[0][:, :3]).max()) / sc["extent"]
    want = float(np.abs(ss.reference(ss.CROWD)[-1][1][:, :3] - ss.reference(ss.CROWD, springs=False)[-1][1][:, :3]).max()) / sc["extent"]
    print("the springs move the last state by %.3e x extent on the device, %.3e in the definition" % (moved, want))
    assert moved >= 100 * BAR and abs(moved - want) <= 2 * BAR


@pytest.mark.parametrize("kind", ["no call", "on and off again", "an all-zero column"])
@pytest.mark.parametrize("name", ["own 64", "stride 64"])
def test_bit_identical_without_springs(rz, name, kind):
    """state and overrides, bit for bit: a table with nonzero spring_position and no call against the same table with the column zeroed;
    on then off against never on; on with an all-zero column against off (the call is taken, reports no spring axis and launches the old
    kernels with the old LDS)"""
    sc, poses, calls = ss.case(name)
    poses, calls = poses[:3], ps.CROWD_CALLS
    zero = ss.with_columns(sc, np.zeros((sc["table"]["n_joints"], 3)))
    bones = dyn_bones(sc)
    if kind == "no call":
        a, b = run(rz, sc, poses, calls, springs="never"), run(rz, zero, poses, calls, springs="never")
    elif kind == "on and off again":
        a, b = run(rz, sc, poses, calls, springs="never"), run(rz, sc, poses, calls, springs="on off")
    else:
        with make_ctx(rz, zero) as c:
            before = c.get_tuning("physics_lds")
            c.physics_springs(True)
            assert (c.get_tuning("physics_springs"), c.get_tuning("physics_spring_axes"), c.get_tuning("physics_lds")) == (1, 0, before)
            assert before == lds_of(sc["table"], ss.CASES[name][2][1], False)
        a, b = run(rz, zero, poses, calls, springs="never"), run(rz, zero, poses, calls, springs="on")
    print("%s, %s: state differs by %.2e, overrides by %.2e" % (name, kind, np.abs(a[0] - b[0]).max(), np.abs(a[1][bones] - b[1][bones]).max()))
    assert same(a, b, bones)


@pytest.mark.parametrize("name", ["own 64", "stride 64"])
def test_steps_add_up_bit_for_bit(rz, name):
    """physics_step(n) is n x physics_step(1) bit for bit with the springs on, joints in registers and striding"""
    sc, poses, _ = ss.case(name)
    bones = dyn_bones(sc)
    a, b = run(rz, sc, poses[:3], ps.CROWD_CALLS), run(rz, sc, poses[:3], ps.CROWD_CALLS, split=True)
    print("%s: whole calls vs calls of one substep: state differs by %.2e, overrides by %.2e" % (name, np.abs(a[0] - b[0]).max(), np.abs(a[1][bones] - b[1][bones]).max()))
    assert same(a, b, bones)


@pytest.mark.parametrize("name", ["own 64", "stride 64"])
def test_crowd_instance_equals_the_sequence_run_alone(rz, name):
    """three instances, each at poses of its own: instance 1 bit for bit, state and overrides, against the same sequence run alone"""
    sc = ss.case(name)[0]
    I, calls = 3, ps.CROWD_CALLS
    bones = dyn_bones(sc)
    poses = [[ps.local_crowd_pose(sc, i, k) for k in range(len(calls))] for i in range(I)]
    with make_ctx(rz, sc, instances=I) as c:
        c.physics_springs(True)
        for k, n in enumerate(calls):
            set_local(c, [poses[i][k] for i in range(I)])
            c.physics_step(n)
            c.deform()
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01
    alone = run(rz, sc, poses[1], calls)
    print("%s: instance 1 alone vs in the crowd: state differs by %.2e" % (name, np.abs(alone[0] - crowd[1][0]).max()))
    assert same(alone, crowd[1], bones)


def test_toggling_between_frames_leaves_the_state(rz):
    """off and on again between two stepped frames: the state stays where the step left it, and the run ends bit for bit where the run
    that never toggled ends"""
    sc, poses, _ = ss.case("stride 64")
    a = run(rz, sc, poses[:3], ps.CROWD_CALLS)
    b = run(rz, sc, poses[:3], ps.CROWD_CALLS, toggle_between=True)
    assert same(a, b, dyn_bones(sc))


def test_misuse(rz):
    """every refusal of rz_physics_springs with its message and the context untouched afterwards; a new table and a new topology turn the
    stage off"""
    sc, poses, _ = ss.case("own 64")
    m = sc["mesh"]
    refused = lambda fn, word, code=None: pg.refused(rz, fn, word, code)
    keys = ("physics_springs", "physics_spring_axes")
    with make_ctx(rz, sc) as c:
        # no table
        c.upload_physics(None)
        refused(lambda: c.physics_springs(True), "no physics table", code=-1)
        refused(lambda: c.physics_springs(False), "no physics table", code=-1)
        # a table without spring_position: rz_upload_physics takes it, the springs do not
        t = dict(sc["table"])
        t["spring_position"] = None
        c.upload_physics(t)
        refused(lambda: c.physics_springs(True), "spring_position", code=-1)
        assert [c.get_tuning(k) for k in keys] == [0, 0] and c.get_tuning("physics_bodies") == sc["table"]["n_bodies"]
        c.upload_physics(sc["table"])
        # forks
        c.physics_springs(True)
        before = [c.get_tuning(k) for k in keys]
        assert before == [1, ss.axes_of(sc["table"])]
        f = c.fork()
        try:
            refused(lambda: c.physics_springs(False), "fork", code=-1)
            refused(lambda: c.physics_springs(True), "fork", code=-1)
        finally:
            f.close()
        assert [c.get_tuning(k) for k in keys] == before
        set_local(c, [poses[1]])
        c.physics_step(2)
        # a new table, a new topology: off again
        c.upload_physics(sc["table"])
        assert [c.get_tuning(k) for k in keys] == [0, 0]
        c.physics_springs(True)
        c.upload_skeleton_topology(m["parents"], m["bind"])
        assert [c.get_tuning(k) for k in keys] == [0, 0] and c.get_tuning("physics_bodies") == 0


def test_the_lds_limit_refuses_and_leaves_the_table(rz):
    """physics_scenes' "most strands" with springs on its joints: 1517 bodies and 1516 joints fit with 12 B per joint and not with 24;
    refused with RZ_ERR_UNSUPPORTED, and the table then steps bit for bit as in a context that never made the call"""
    sc = ss.sprung(ps.scene("most strands"), 28)
    t = sc["table"]
    poses, calls = [ps.pose(sc, k) for k in range(2)], (1, 4)
    with make_ctx(rz, sc) as c:
        before = [c.get_tuning(k) for k in FORM_KEYS + ("physics_lds", "physics_spring_axes")]
        pg.refused(rz, lambda: c.physics_springs(True), "24 B per joint", code=-6)
        with pytest.raises(rz.capi.RzError) as e:
            c.physics_springs(True)
        print(str(e.value))
        assert all(w in str(e.value) for w in ("%d bodies" % t["n_bodies"], "%d joints" % t["n_joints"], "%d B of LDS" % lds_of(t, 0, True)))
        assert [c.get_tuning(k) for k in FORM_KEYS + ("physics_lds", "physics_spring_axes")] == before and before[3] == 0
        for (q, tr), n in zip(poses, calls):
            set_local(c, [(q, tr)])
            c.physics_step(n)
            c.deform()
        a = c.read_physics(0), c.read_world(0)
    b = run(rz, sc, poses, calls, springs="never")
    assert same(a, b, dyn_bones(sc))


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, physicsSprings: true }) on the PMX physics_scenes.write_pmx writes for the
    sprung "crowd" strands: the frames are held to the float64 definition with the springs, run with the table the loader must derive and
    the same substeps; the same engine without the option is held to the definition without them"""
    sc, data, q = ss.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    keys = ("physics_springs", "physics_spring_axes")
    out = subprocess.check_output(["node", os.path.join(pg.ROOT, "tests", "js", "springs_e2e.js"), "springs,off", ",".join(keys), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"),
                                   str(tmp_path)] + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    calls = ps.node_substeps()
    assert tuple(info["springs"]["substeps"]) == calls and tuple(info["off"]["substeps"]) == calls
    assert info["springs"]["keys"] == [1, ss.axes_of(sc["table"])] and info["off"]["keys"] == [0, 0]
    n, ext = len(calls), sc["extent"]
    poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * n
    sim = lambda springs: spring_ref.Sim(sc["table"], sc["parents"], sc["bind"], springs=springs)
    refs = dict(springs=ps.run_reference(sc, poses, calls, sim=sim(True)), off=ps.run_reference(sc, poses, calls, sim=sim(False)))
    for option in ("springs", "off"):
        ex, eq, ew, ep = pg.node_errors(tmp_path, option, oracle, sc, refs[option])
        print("node engine, %s, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (option, n, sum(calls), ex, eq, ew, ep, ext))
        assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    moved = float(np.abs(refs["springs"][-1][1][:, :3] - refs["off"][-1][1][:, :3]).max()) / ext
    print("the springs move the last frame's bodies by %.3e x extent" % moved)
    assert moved >= 100 * BAR
