"""What the GPU tests of the device physics share (tests/test_gpu_physics.py, tests/test_gpu_contacts.py, tests/test_gpu_contact_boxes.py): the
context a scene runs in, the errors of a frame against the float64 reference and their bar, and the bit-for-bit comparisons.

The bar: body positions, world-matrix entries and deformed positions within 1e-4 x the skeleton's extent of the float64 reference,
quaternions within 1e-4 up to sign, normals within the suite's 1e-4."""
import numpy as np

import physics_ref
from helpers import NRM_TOL

BAR = 1e-4


def set_mode(c, mode):
    """the contact stage's mode: 0 off, 1 spheres and capsules, 2 boxes too"""
    if mode == 2:
        c.physics_contacts(True, boxes=True)
    else:
        c.physics_contacts(bool(mode))


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
