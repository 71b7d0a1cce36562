"""The per-frame pose transport as a whole: every way to set a pose, cycled through more uploads than its rings have slots, each frame held
BIT FOR BIT to the same pose on a context created fresh for that step (one upload, one frame). A characterisation test: the zero-copy ring
(32 slots, with and without the pose prefetch's hand-over), the two pose blocks (zero_copy = 0), the staging ring (8 slots) and the
big-pose ring (8 blocks) each wrap at least twice while the KIND of pose changes under them with every upload — a slot reused early, a tag
of another kind matched, a resident flag left over from the pose before would show as wrong bits.

Shapes are the smallest that reach those paths: V = 256, B = 8, M = 2 for the one character; V = 256, B = 16, I = 264 for the crowd, whose
world-matrix pose is 264 x 16 x 64 B = 270 336 B, above the 256 KB that send a pose through the big-pose ring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZC_SLOTS, BIG_BLOCKS = 32, 8


def _scene(rz, V, B, M, seed):
    synth = rz.synth
    mesh = synth.make_mesh(V, B, seed=seed)
    s = dict(mesh=mesh, B=B, M=M, dense=synth.make_morphs_dense(V, M, seed=seed + 1)[0] if M else None,
             clips=[synth.make_motion(B, M, seed=seed + 2), synth.make_motion(B, M, seed=seed + 3, n_keys=5, flip=0.3)],
             single=synth.make_motion(B, M, seed=seed + 4, n_keys=7))
    return s


def _ctx(rz, s, instances=1, tuning=None):
    m = s["mesh"]
    c = rz.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    c.upload_skeleton_topology(m["parents"], m["bind"])
    if s["M"]:
        c.upload_morphs_dense(s["dense"])
    if instances > 1:
        c.set_instances(instances)
    c.upload_motions(s["clips"])
    if instances == 1:
        c.upload_animation(**s["single"])
    if tuning:
        c.set_tuning(**tuning)
    return c


def _frame(c, instances):
    c.deform()
    return [c.read(i) for i in range(instances)]


def _same(a, b):
    return all(np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def _inputs(rz, s, I, k):
    """the k-th pose of a run, in every form a step may hand over"""
    m, B, M = s["mesh"], s["B"], s["M"]
    rng = np.random.default_rng(1000 + k)
    world = np.stack([rz.synth.make_pose(m["parents"], m["bind"], B, seed=5000 + 7 * k + i % 5) for i in range(I)]).astype(np.float32)
    q = rng.normal(size=(I, B, 4))
    q = (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float32)
    t = rng.uniform(-0.2, 0.2, size=(I, B, 3)).astype(np.float32)
    mw = None
    if M:
        mw = rng.random((I, M)).astype(np.float32)
        mw[:, k % M] = 0.0                                      # the host-compacted list changes shape from pose to pose
    state = (rng.integers(0, 2, size=I), rng.uniform(-2, 30, size=I), rng.integers(0, 2, size=I), rng.uniform(-2, 30, size=I),
             rng.choice([0.0, 0.25, 1.0], size=I))
    layers = [[dict(clip=int(rng.integers(0, 2)), frame=float(rng.uniform(0, 30)), weight=0.5, additive=bool(k & 1))] for _ in range(I)]
    return dict(world=world, q=q, t=t, mw=mw, state=state, layers=layers, frame=rng.uniform(-2, 40, size=I))


def _mapped(rz, c, p, layout):
    mats, mw = c.map_pose(layout)
    I, B = p["world"].shape[:2]
    w4 = p["world"].reshape(I, B, 4, 4)
    mats[:] = w4[..., :3].reshape(I, B, 12) if layout == rz.capi.POSE_ROWS12 else w4.reshape(I, B, 16)
    if mw is not None:
        mw[:] = p["mw"]
    c.commit_pose()


def _one(x):
    return x[0] if len(x) == 1 else x


WAYS = {
    "world": lambda rz, c, p: c.set_pose(_one(p["world"]), p["mw"]),
    "local_t": lambda rz, c, p: c.set_pose_local(p["q"], p["mw"], p["t"]),
    "local": lambda rz, c, p: c.set_pose_local(p["q"], p["mw"]),
    "mapped": lambda rz, c, p: _mapped(rz, c, p, rz.capi.POSE_WORLD16),
    "rows": lambda rz, c, p: _mapped(rz, c, p, rz.capi.POSE_ROWS12),
    "sampled": lambda rz, c, p: c.set_pose_sampled(p["frame"]),
    "blended": lambda rz, c, p: c.set_pose_blended(*p["state"]),
    "layered": lambda rz, c, p: c.set_pose_layered(rz.DeformContext.pack_motion_states(len(p["frame"]), *p["state"]), p["layers"]),
}


def _fresh(rz, s, I, tuning, way, p):
    with _ctx(rz, s, I, tuning) as f:
        WAYS[way](rz, f, p)
        return _frame(f, I)


def test_one_character_every_way_to_set_a_pose_across_the_zero_copy_ring(rz):
    s = _scene(rz, 256, 8, 2, seed=11)
    cycle = ("world", "local_t", "local", "mapped", "sampled", "blended", "layered")
    for zero_copy in (-1, 0):                                   # read in place with the prefetch's hand-over; then every pose copied
        tuning = dict(pose_prefetch=1, zero_copy=zero_copy)
        with _ctx(rz, s, 1, tuning) as c:
            for k in range(2 * ZC_SLOTS + 3):
                way = cycle[k % len(cycle)]
                p = _inputs(rz, s, 1, k)
                WAYS[way](rz, c, p)
                got = _frame(c, 1)
                assert _same(got, _fresh(rz, s, 1, tuning, way, p)), "upload %d (%s, zero_copy = %d)" % (k, way, zero_copy)


def test_crowd_above_256_kb_every_way_to_set_a_pose_across_the_big_pose_ring(rz):
    I = 264
    s = _scene(rz, 256, 16, 0, seed=23)
    assert I * 16 * 64 == 270336 > (256 << 10)
    cycle = ("world", "mapped", "rows", "local_t", "blended")
    big, k, rows_refused = 0, 0, 0
    with _ctx(rz, s, I) as c:
        while big < 2 * BIG_BLOCKS + 3:                         # uploads that take a block of the big-pose ring: never fewer than 2 x 8 + 3 uploads in all
            way = cycle[k % len(cycle)]
            p = _inputs(rz, s, I, k)
            k += 1
            try:
                WAYS[way](rz, c, p)
            except rz.RzError as e:
                if way == "rows" and e.code == -6:              # this context cannot pull rows (no device-mapped ring): the other steps cross the ring
                    rows_refused += 1
                    continue
                raise
            big += way in ("world", "mapped", "rows")
            got = _frame(c, I)
            want = _fresh(rz, s, I, None, way, p)
            assert _same(got, want), "upload %d (%s)" % (k - 1, way)
    print("crowd: %d uploads, %d through the big-pose ring, rows refused %d times" % (k - rows_refused, big, rows_refused))
