"""What the GPU tests of the device physics share (tests/test_gpu_physics.py, tests/test_gpu_contacts.py, tests/test_gpu_contact_boxes.py,
tests/test_gpu_contact_boxbox.py): the context a scene runs in, the errors of a frame against the float64 reference and their bar, the
bit-for-bit comparisons, and for the three contact files the run of one instance, the tuning keys, the refusals, the Node end-to-end run
and the parity file.

The bar: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent of the float64 reference,
quaternions within 1e-4 up to sign, normals within the suite's 1e-4."""
import json
import os
import subprocess

import numpy as np
import pytest

import physics_ref
import physics_scenes as ps
from helpers import NRM_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
# the contact stage's tuning keys, in the order the modes brought them: mode 1 knows the first five, mode 2 six, mode 3 all
KEYS = ("physics_contacts", "physics_contact_follow", "physics_contact_pairs", "physics_contact_colours", "physics_contact_boxes", "physics_contact_box_pairs",
        "physics_contact_box_box")


def set_mode(c, mode):
    """the contact stage's mode: 0 off, 1 spheres and capsules, 2 boxes against them too, 3 and boxes against boxes"""
    c.physics_contacts(bool(mode), boxes=mode >= 2, box_pairs=mode == 3)


def keys_of(L, mode, n=None):
    """what the first n of KEYS (those the mode's build knows, unless given) read under `mode` with the definition's lists L"""
    return [mode, L["n_follow"], L["n_pairs"], L["n_colours"], L["boxes"], L["box_pairs"], L["n_box_box"]][:n or 4 + mode]


def make_ctx(rz, sc, instances=1, contacts=0, table=True, chains=None):
    """a context with the scene's mesh and skeleton, its IK chains, its physics table and the contact stage in mode `contacts` (0: never
    enabled)"""
    m = sc["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"])
    if instances > 1:
        c.set_instances(instances)
    if chains:
        c.upload_ik(chains)
    if table:
        c.upload_physics(sc["table"])
    if contacts:
        set_mode(c, contacts)
    return c


def set_local(c, poses):
    c.set_pose_local(np.stack([p[0] for p in poses]), None, np.stack([p[1] for p in poses]))


def errors(c, oracle, sc, i, ref_world, ref_state):
    """(position, quaternion, world, deformed position [all but the quaternion in units of extent], normal) errors of instance i against
    the reference's (world [B,16] with overrides, state [nb,13]); the frame has run"""
    m, ext = sc["mesh"], sc["extent"]
    st = c.read_physics(i).astype(np.float64)
    assert np.isfinite(st).all()
    ex = float(np.abs(st[:, :3] - ref_state[:, :3]).max()) / ext
    eq = float(np.minimum(np.abs(st[:, 3:7] - ref_state[:, 3:7]).max(axis=1), np.abs(st[:, 3:7] + ref_state[:, 3:7]).max(axis=1)).max())
    wg = c.read_world(i).astype(np.float64)
    ew = float(np.abs(wg - ref_world).max()) / ext
    pg, ng = c.read(i)
    pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], ref_world.astype(np.float32), m["inv_bind"])
    ep = float(np.abs(pg.astype(np.float64) - pr).max()) / ext
    en = float(np.linalg.norm(ng.astype(np.float64) - nr, axis=1).max())
    return ex, eq, ew, ep, en


def assert_bar(e, what):
    """prints the largest of the errors, holds them to the bar and returns the printed line"""
    e = np.array(e).reshape(-1, 5)
    worst = e.max(axis=0)
    line = "%s: body position %.2e quaternion %.2e world %.2e deformed %.2e (x extent), normals %.2e" % ((what,) + tuple(worst))
    print(line)
    assert worst[0] <= BAR and worst[2] <= BAR and worst[3] <= BAR, "%s: position %.3e world %.3e deformed %.3e x extent" % (what, worst[0], worst[2], worst[3])
    assert worst[1] <= BAR, "%s: quaternion %.3e" % (what, worst[1])
    assert worst[4] <= NRM_TOL, "%s: normals %.3e" % (what, worst[4])
    return line


def dyn_bones(sc):
    dyn = physics_ref.prepare(sc["table"], sc["parents"], sc["bind"])["dyn_bodies"]
    return [int(sc["table"]["bone"][b]) for b in dyn]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, bones):
    """two runs' (state, world): finite, and bit for bit the same in the state and in the world matrices of `bones`"""
    (sa, wa), (sb, wb) = a, b
    return np.isfinite(sa).all() and np.array_equal(bits(sa), bits(sb)) and np.array_equal(bits(wa[bones]), bits(wb[bones]))


# ---- what the three contact files share ----

def run(rz, sc, poses, calls, mode, split=False, detour=(), toggle=False):
    """one instance through the calls under the mode; (state, world) after the last frame. split: every call of n substeps as n calls of
    one. detour: the modes to pass through (ending in `mode` again) behind the first call, a substep under each that is not `mode`.
    toggle: contacts on and off again before the first step"""
    with make_ctx(rz, sc, contacts=mode) as c:
        if toggle:
            c.physics_contacts(True)
            assert c.get_tuning("physics_contacts") == 1
            c.physics_contacts(False)
            assert [c.get_tuning(k) for k in KEYS[:5]] == [0] * 5
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


def refused(rz, fn, word, code=None):
    """fn raises RzError with `word` in its message (and the code, when given)"""
    with pytest.raises(rz.capi.RzError) as e:
        fn()
    assert word in str(e.value), str(e.value)
    if code is not None:
        assert e.value.code == code, e.value.code


def two_bone_ctx(rz, m):
    """a context with the mesh m on a skeleton of two bones at the origin: what the limit tables (contact_scenes.limit_table) stand on"""
    B = 2
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], np.zeros_like(m["joints"]), m["weights"])
    inv = np.zeros((B, 16), dtype=np.float32); inv[:, [0, 5, 10, 15]] = 1
    c.upload_skeleton(inv)
    c.upload_skeleton_topology(np.array([-1, 0], dtype=np.int32), np.zeros((B, 3), dtype=np.float32))
    return c


def crowd_against_alone(rz, oracle, scenes, mode, what):
    """three instances of the scenes module's CROWD case, each at poses of its own, against the reference per instance, and instance 1 bit
    for bit, state and overrides, against the same sequence run alone"""
    sc, _, _ = scenes.case(scenes.CROWD)
    I, calls = 3, scenes.SHORT
    amounts = (0.5, 0.35, 0.6)
    bones = dyn_bones(sc)
    poses = [[scenes.pose(sc, k, amounts[i], turn=0.05 + 0.02 * i) for k in range(len(calls))] for i in range(I)]
    refs = [scenes.run_reference(sc, poses[i], calls, sim=scenes.sim_of(sc)) for i in range(I)]
    errs = []
    with make_ctx(rz, sc, instances=I, contacts=mode) as c:
        for call, n in enumerate(calls):
            set_local(c, [poses[i][call] for i in range(I)])
            c.physics_step(n)
            c.deform()
            for i in range(I):
                errs.append(errors(c, oracle, sc, i, *refs[i][call]))
        crowd = [(c.read_physics(i), c.read_world(i)) for i in range(I)]
    assert_bar(errs, "crowd of %d with %s" % (I, what))
    assert np.abs(crowd[0][0] - crowd[1][0]).max() > 0.01
    alone = run(rz, sc, poses[1], calls, mode)
    print("instance 1 alone vs in the crowd: state differs by %.2e, overrides by %.2e" % (np.abs(alone[0] - crowd[1][0]).max(), np.abs(alone[1][bones] - crowd[1][1][bones]).max()))
    assert same(alone, crowd[1], bones)


def steps_add_up(rz, sc, poses, calls, mode, name):
    """physics_step(n) is n x physics_step(1) bit for bit, state and overrides"""
    bones = dyn_bones(sc)
    a, b = run(rz, sc, poses, calls, mode), run(rz, sc, poses, calls, mode, split=True)
    print("%s: whole calls vs calls of one substep: state differs by %.2e, overrides by %.2e" % (name, np.abs(a[0] - b[0]).max(), np.abs(a[1][bones] - b[1][bones]).max()))
    assert same(a, b, bones)


def node_run(tmp_path, data, q, options, keys):
    """tests/js/contacts_e2e.js on the PMX bytes `data` under the local rotations q, one engine per physicsContacts option (true, off,
    boxes, all): per option {substeps, keys} as the script prints them; the frames are left in tmp_path for node_errors"""
    (tmp_path / "s.pmx").write_bytes(data)
    q.tofile(str(tmp_path / "q.f32"))
    out = subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "contacts_e2e.js"), ",".join(options), ",".join(keys), str(tmp_path / "s.pmx"), str(tmp_path / "q.f32"),
                                   str(tmp_path)] + ["%r" % t for t in ps.NODE_TIMES], timeout=300)
    return json.loads(out.decode().strip().splitlines()[-1])


def node_errors(tmp_path, option, oracle, sc, ref):
    """the largest (body position, quaternion, world, deformed position) errors of the frames node_run dumped for the option against the
    reference's per-call (world, state), all but the quaternion in units of extent"""
    m, B, ext = sc["mesh"], sc["B"], sc["extent"]
    n, V = len(ref), len(m["pos"])
    pos = np.fromfile(str(tmp_path / ("pos_%s.f32" % option)), dtype=np.float32).reshape(n, V, 3)
    world = np.fromfile(str(tmp_path / ("world_%s.f32" % option)), dtype=np.float32).reshape(n, B, 16)
    state = np.fromfile(str(tmp_path / ("state_%s.f32" % option)), dtype=np.float32).reshape(n, -1, 13)
    ex = ew = ep = eq = 0.0
    for k, (rw, rs) in enumerate(ref):
        ex = max(ex, float(np.abs(state[k][:, :3] - rs[:, :3]).max()) / ext)
        eq = max(eq, float(np.minimum(np.abs(state[k][:, 3:7] - rs[:, 3:7]).max(axis=1), np.abs(state[k][:, 3:7] + rs[:, 3:7]).max(axis=1)).max()))
        ew = max(ew, float(np.abs(world[k] - rw).max()) / ext)
        pr_, _ = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], rw.astype(np.float32), m["inv_bind"])
        ep = max(ep, float(np.abs(pos[k].astype(np.float64) - pr_).max()) / ext)
    return ex, eq, ew, ep


def write_parity(name, head, order, rows):
    """profiles/<name>: the head and the rows of the cases in `order`, once every one of them has run"""
    if set(rows) >= set(order):
        with open(os.path.join(ROOT, "profiles", name), "w") as f:
            f.write(head + "\n" + "".join(rows[case] + "\n" for case in order))
