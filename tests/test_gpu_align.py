"""PMX type-2 bodies on the device (rz_physics_aligned, the ALIGN instantiations of kernels/physics.hip) against the float64 definition
tests/align_ref.py, on the scenes of tests/align_scenes.py.

The bar is that of tests/test_gpu_physics.py (physics_gpu.BAR): body positions, world-matrix entries and deformed positions within
1e-4 x the skeleton's extent of the float64 reference, quaternions within 1e-4 up to sign, normals within the suite's 1e-4 — per call,
over a handful of calls of 1 - 3 substeps with a pose that moves between calls. tests/test_align_cpu.py holds the float32 run of the
definition to a tenth of that on every scene and every sequence of calls used here. Every test prints its largest error before it
asserts; the maxima per scene go to profiles/align_edges_parity.txt. A build without rz_physics_aligned fails every test here: the
binding raises where the symbol is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import align_ref
import align_scenes as als
import physics_gpu as pg
import physics_scenes as ps
from physics_gpu import BAR, assert_bar, bits, errors, same, set_local

pytestmark = pytest.mark.gpu
KEYS = ("physics_aligned", "physics_aligned_bodies")
FORM_KEYS = ("physics_block", "physics_own", "physics_contacts", "physics_springs")
_rows = {}
HEAD = ("PMX type-2 bodies on the device (rz_physics_aligned) against tests/align_ref.py in float64, per case of tests/align_scenes.py: the largest\n"
        "errors over the case's calls (substeps %s, the pose moving between calls) and the form the launch took (lanes per workgroup, joints in\n"
        "registers, contact mode, springs). Written by tests/test_gpu_align.py on an MI355X." % (als.CALLS,))


def ctx_of(rz, sc, instances=1, aligned=True, mode=0, springs=False, behind=None, table=True):
    """a context with the scene's mesh and skeleton (with its append columns, if it has them), the stage the frame runs behind the
    overrides, the physics table, and then, in the order callers owe: aligned -> springs -> contacts"""
    m = sc["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"], sc.get("ap"), sc.get("ratio"), sc.get("move"))
    if instances > 1:
        c.set_instances(instances)
    if behind == "follow":
        c.override_follow(True)
    if behind == "after":
        c.upload_after_physics(sc["order"])
    if table:
        c.upload_physics(sc["table"])
        if aligned:
            c.physics_aligned(True)
        if springs:
            c.physics_springs(True)
        if mode:
            pg.set_mode(c, mode)
    return c


def solved_on_device(rz, sc, poses):
    """the un-overridden hierarchy solve of every pose as the device makes it: a context without a physics table, [len(poses)][B,16]"""
    out = []
    with ctx_of(rz, sc, table=False) as c:
        for q, t in poses:
            set_local(c, [(q, t)])
            c.deform()
            out.append(c.read_world(0))
    return out


def assert_pinned(world, solved, sc, what):
    """the pin: the translation column of every aligned bone is the un-overridden solve's bit for bit; its rotation is the body's"""
    bones = als.aligned_bones(sc)
    assert bones
    assert np.array_equal(bits(world[bones][:, 12:16]), bits(solved[bones][:, 12:16])), "%s: an aligned bone left its solved position" % what
    return float(np.abs(world[bones][:, :12] - solved[bones][:, :12]).max())


def run(rz, sc, poses, calls, aligned=True, mode=0, springs=False, split=False, toggle=False):
    """one instance through the calls; (state, world) after the last frame. split: every call of n substeps as n calls of one. toggle: on
    and off again before the first step (with aligned=False)"""
    with ctx_of(rz, sc, aligned=aligned, mode=mode, springs=springs) as c:
        if toggle:
            c.physics_aligned(True)
            assert c.get_tuning("physics_aligned") == 1
            c.physics_aligned(False)
            assert [c.get_tuning(k) for k in KEYS] == [0, 0]
        for (q, t), n in zip(poses, calls):
            set_local(c, [(q, t)])
            for part in ([1] * n if split else [n]):
                c.physics_step(part)
            c.deform()
        return c.read_physics(0), c.read_world(0)


def overridden_bones(sc, aligned=True):
    t = align_ref.read_table(sc["table"], aligned)
    return pg.dyn_bones(dict(sc, table=t))


@pytest.mark.parametrize("name", als.ORDER)
def test_case_against_the_definition(rz, oracle, name):
    """every case of align_scenes — the three launch forms, contacts in mode 1, an aligned box against a following box in mode 3, the
    linear springs, a body-less tip below an aligned bone under rz_override_follow, an after-physics helper appending from an aligned
    bone — per call against the definition, the first call being the implicit reset; after every call every aligned bone's translation
    column is the un-overridden solve's bit for bit while its rotation is not; the launch takes the form the case is there for"""
    sc, poses, calls = als.case(name)
    _, mode, springs, (block, own), behind = als.CASES[name]
    ref = als.reference(name)
    t = sc["table"]
    n_aligned = int(align_ref.aligned_bodies(t).sum())
    solved = solved_on_device(rz, sc, poses)
    errs, turned = [], 0.0
    with ctx_of(rz, sc, mode=mode, springs=springs, behind=behind) as c:
        form = tuple(c.get_tuning(k) for k in FORM_KEYS)
        assert form == (block, own, mode, int(springs)), form
        assert [c.get_tuning(k) for k in KEYS] == [1, n_aligned] and n_aligned > 0
        for k, ((q, tr), n, (rw, rs, _)) in enumerate(zip(poses, calls, ref)):
            set_local(c, [(q, tr)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, rw, rs))
            turned = max(turned, assert_pinned(c.read_world(0), solved[k], sc, "%s, call %d" % (name, k)))
    print("%s: the aligned bones' rotations leave the solved ones by up to %.3e" % (name, turned))
    assert turned > 1e-3
    line = assert_bar(errs, name)
    _rows[name] = "%s  [%d lanes, own %d, contacts %d, springs %d; %d bodies, %d joints, %d aligned]" % ((line,) + form + (t["n_bodies"], t["n_joints"], n_aligned))
    pg.write_parity("align_edges_parity.txt", HEAD, als.ORDER, _rows)


def test_the_feature_moves_the_scene(rz):
    """fails without the feature: on the "own 64" case the stepped state with the call differs from the state without it by what the
    definition says, at least 100 x the bar"""
    sc, poses, calls = als.case(als.CROWD)
    on, off = run(rz, sc, poses, calls), run(rz, sc, poses, calls, aligned=False)
    moved = float(np.abs(on[0][:, :3] - off[0][:, :3]).max()) / sc["extent"]
    want = float(np.abs(als.reference(als.CROWD)[-1][1][:, :3] - als.reference(als.CROWD, aligned=False)[-1][1][:, :3]).max()) / sc["extent"]
    print("the call moves the last state by %.3e x extent on the device, %.3e in the definition" % (moved, want))
    assert moved >= 100 * BAR and abs(moved - want) <= 2 * BAR


def test_crowd_instances_equal_the_sequences_run_alone(rz, oracle):
    """a crowd of three, every instance at poses of its own: each against the definition, and each bit for bit, state and overrides,
    against the same sequence run alone"""
    sc = als.case(als.CROWD)[0]
    I, calls = 3, als.CALLS
    bones = overridden_bones(sc)
    poses = [als.crowd_poses(sc, i) for i in range(I)]
    refs = [als.run(sc, poses[i], calls)[0] for i in range(I)]
    errs = []
    with ctx_of(rz, sc, instances=I) as c:
        for k, n in enumerate(calls):
            set_local(c, [poses[i][k] for i in range(I)])
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, refs[i][k][0], refs[i][k][1]))
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "crowd of %d" % I)
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01
    for i in range(I):
        alone = run(rz, sc, poses[i], calls)
        print("instance %d alone vs in the crowd: state differs by %.2e" % (i, np.abs(alone[0] - crowd[i][0]).max()))
        assert same(alone, crowd[i], bones)


def test_zero_substeps_repin_and_reemit(rz, oracle):
    """rz_physics_step(0) after a pose change: the aligned bodies go back onto their bones' new positions with the rotation and the
    velocities they had, every other dynamic body stays, and the overrides are emitted with the new bone positions"""
    sc, poses, _ = als.case(als.CROWD)
    calls = als.ZERO_CALLS
    ref = als.run(sc, poses, calls)[0]
    solved = solved_on_device(rz, sc, poses[:len(calls)])
    al = align_ref.aligned_bodies(sc["table"])
    errs, states = [], []
    with ctx_of(rz, sc) as c:
        for k, ((q, t), n) in enumerate(zip(poses, calls)):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, ref[k][0], ref[k][1]))
            assert_pinned(c.read_world(0), solved[k], sc, "call %d" % k)
            states.append(c.read_physics(0))
    assert_bar(errs, "substeps 1, 3, 0, 2")
    before, after = states[1], states[2]
    dyn = align_ref.Sim(sc["table"], sc["parents"], sc["bind"]).c["dyn"]
    assert np.array_equal(bits(before[dyn][:, 3:]), bits(after[dyn][:, 3:])), "a call without substeps changed a rotation or a velocity"
    assert np.array_equal(bits(before[dyn & ~al][:, :3]), bits(after[dyn & ~al][:, :3])), "a call without substeps moved a body that is not aligned"
    moved = float(np.abs(before[al][:, :3] - after[al][:, :3]).max()) / sc["extent"]
    print("the call without substeps moves the aligned bodies by %.3e x extent" % moved)
    assert moved > BAR


def test_reset_places_every_body(rz, oracle):
    """rz_physics_reset under a new pose in the middle of a sequence, and the implicit reset of the first step: every body, the aligned
    ones included, stands on its bone with zero velocity, which satisfies the pin; the sequence goes on from there as the definition's"""
    sc, poses, _ = als.case(als.CROWD)
    calls = als.RESET_CALLS
    ref = [(w, s) for w, s, _ in als.run(sc, poses, calls)[0]]
    solved = solved_on_device(rz, sc, poses[:len(calls)])
    errs = []
    with ctx_of(rz, sc) as c:
        for k, ((q, t), n) in enumerate(zip(poses, calls)):
            set_local(c, [(q, t)])
            if n == "reset":
                c.physics_reset()
            else:
                c.physics_step(n)
            c.deform()
            errs.append(errors(c, oracle, sc, 0, *ref[k]))
            assert_pinned(c.read_world(0), solved[k], sc, "call %d" % k)
            if n == "reset":
                st = c.read_physics(0)
                assert not st[:, 7:].any()
    assert_bar(errs, "steps, a reset, a step")
    # the first step alone: the implicit reset, then no substep
    with ctx_of(rz, sc) as c:
        set_local(c, [poses[0]])
        c.physics_step(0)
        c.deform()
        sim = als.sim_of(sc)
        S = als.solved(sc, *poses[0])
        ovr = sim.step(S, 0)
        assert_bar([errors(c, oracle, sc, 0, als.frame(sc, poses[0][0], poses[0][1], S, ovr), sim.state13().astype(np.float64))], "the implicit reset")
        assert not c.read_physics(0)[:, 7:].any()


def test_off_after_on_is_a_fresh_upload(rz):
    """on and off again before the first step: state and overrides bit for bit those of a context that never made the call"""
    sc, poses, calls = als.case(als.CROWD)
    bones = overridden_bones(sc, aligned=False)
    a, b = run(rz, sc, poses, calls, aligned=False), run(rz, sc, poses, calls, aligned=False, toggle=True)
    print("never on vs on and off again: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, bones)


def test_a_table_without_type_2_keeps_its_bits_and_its_steps_add_up(rz):
    """on = 1 on a table without a type-2 body: the call is taken, reports no aligned body and the table steps bit for bit as without it;
    physics_step(2) is two physics_step(1) there, bit for bit"""
    (sc, poses), calls = als.plain_scene(), als.SPLIT_CALLS
    bones = overridden_bones(sc)
    with ctx_of(rz, sc) as c:
        assert [c.get_tuning(k) for k in KEYS] == [1, 0]
    a, b = run(rz, sc, poses, calls, aligned=False), run(rz, sc, poses, calls)
    print("no type 2: without the call vs with it: state differs by %.2e" % np.abs(a[0] - b[0]).max())
    assert same(a, b, bones)
    s = run(rz, sc, poses, calls, split=True)
    assert same(b, s, bones)


def test_steps_do_not_add_up_with_aligned_bodies(rz):
    """the re-pin is per call: physics_step(2) is not two physics_step(1) on a table with aligned bodies (the free aligned body of "own 64"
    falls through the first substep and is back on its bone before the second), and the definition says by how much"""
    sc, poses, _ = als.case(als.CROWD)
    calls = als.SPLIT_CALLS
    a, b = run(rz, sc, poses, calls), run(rz, sc, poses, calls, split=True)
    diff = float(np.abs(a[0][:, :3] - b[0][:, :3]).max()) / sc["extent"]
    want = float(np.abs(als.run(sc, poses, calls)[0][-1][1][:, :3] - als.run(sc, *als.split(poses, calls))[0][-1][1][:, :3]).max()) / sc["extent"]
    print("whole calls vs calls of one substep: the state differs by %.3e x extent on the device, %.3e in the definition" % (diff, want))
    assert not same(a, b, overridden_bones(sc))
    assert diff >= 10 * BAR and abs(diff - want) <= 2 * BAR


def test_refusals_leave_the_table_stepping(rz):
    """no table; forks; two bodies that would both be dynamic on one bone, both named: each refusal leaves the keys and the resident
    table as they were, stepping bit for bit as a context that never made the call; a new table and a new topology turn the feature off"""
    sc, poses, calls = als.case(als.CROWD)
    m = sc["mesh"]
    refused = lambda fn, word, code=None: pg.refused(rz, fn, word, code)
    with ctx_of(rz, sc, table=False) as c:
        refused(lambda: c.physics_aligned(True), "no physics table", code=-1)
        refused(lambda: c.physics_aligned(False), "no physics table", code=-1)
        assert [c.get_tuning(k) for k in KEYS] == [0, 0]
    # forks: the call is refused either way and the table steps on as it was, aligned
    with ctx_of(rz, sc) as c:
        before = [c.get_tuning(k) for k in KEYS + FORM_KEYS + ("physics_colours", "physics_lds")]
        f = c.fork()
        try:
            refused(lambda: c.physics_aligned(False), "fork", code=-1)
            refused(lambda: c.physics_aligned(True), "fork", code=-1)
        finally:
            f.close()
        assert [c.get_tuning(k) for k in KEYS + FORM_KEYS + ("physics_colours", "physics_lds")] == before
        for (q, t), n in zip(poses, calls):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
        assert same((c.read_physics(0), c.read_world(0)), run(rz, sc, poses, calls), overridden_bones(sc))
        # a new table, a new topology: off again
        c.upload_physics(sc["table"])
        assert [c.get_tuning(k) for k in KEYS] == [0, 0]
        c.physics_aligned(True)
        c.upload_skeleton_topology(m["parents"], m["bind"])
        assert [c.get_tuning(k) for k in KEYS] == [0, 0] and c.get_tuning("physics_bodies") == 0
    # two on one bone
    two, first, extra = als.two_on_one_bone(sc)
    with ctx_of(rz, two, aligned=False) as c:
        before = [c.get_tuning(k) for k in KEYS + FORM_KEYS + ("physics_colours", "physics_lds")]
        with pytest.raises(rz.capi.RzError) as e:
            c.physics_aligned(True)
        print(str(e.value))
        assert e.value.code == -1 and "bodies %d and %d both drive bone %d" % (first, extra, int(two["table"]["bone"][first])) in str(e.value)
        assert [c.get_tuning(k) for k in KEYS + FORM_KEYS + ("physics_colours", "physics_lds")] == before
        for (q, t), n in zip(poses, calls):
            set_local(c, [(q, t)])
            c.physics_step(n)
            c.deform()
        assert same((c.read_physics(0), c.read_world(0)), run(rz, two, poses, calls, aligned=False), overridden_bones(two, aligned=False))


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_engine_end_to_end(rz, oracle, tmp_path):
    """new Engine(null, { deviceFK: true, devicePhysics: true, physicsAligned: true }) on the PMX physics_scenes.write_pmx writes for the
    "crowd" strands with type-2 first links: the frames are held to the float64 definition, run with the table the loader must derive
    (it passes the type through) and the same substeps; the same engine without the option is held to the definition with the feature off"""
    sc, data, q = als.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(pg.ROOT, "tests", "js", "align_e2e.js"), "aligned,off", ",".join(KEYS), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"),
                                   str(tmp_path)] + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    info = json.loads(out.decode().strip().splitlines()[-1])
    calls = ps.node_substeps()
    assert tuple(info["aligned"]["substeps"]) == calls and tuple(info["off"]["substeps"]) == calls
    assert info["aligned"]["keys"] == [1, int(align_ref.aligned_bodies(sc["table"]).sum())] and info["off"]["keys"] == [0, 0]
    n, ext = len(calls), sc["extent"]
    poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * n
    refs = {option: [(w, s) for w, s, _ in als.run(sc, poses, calls, aligned=option == "aligned")[0]] for option in ("aligned", "off")}
    for option in ("aligned", "off"):
        ex, eq, ew, ep = pg.node_errors(tmp_path, option, oracle, sc, refs[option])
        print("node engine, %s, %d frames / %d substeps: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent %.1f)" % (option, n, sum(calls), ex, eq, ew, ep, ext))
        assert ex <= BAR and ew <= BAR and ep <= BAR and eq <= BAR
    moved = float(np.abs(refs["aligned"][-1][1][:, :3] - refs["off"][-1][1][:, :3]).max()) / ext
    print("the option moves the last frame's bodies by %.3e x extent" % moved)
    # (a figure of the two definitions, not of the device: ten times the bar and the two engines' frames cannot pass for each other; the
    # strands have only begun to swing after these 15 substeps — tests/test_align_cpu.py prints the figure, 97 x the bar)
    assert moved >= 10 * BAR
