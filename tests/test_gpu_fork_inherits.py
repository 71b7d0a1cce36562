"""What rz_fork hands a fork (csrc/ctx.h): it BORROWS every static table (RzStatic), INHERITS every settable tuning key (RzTuning) and owns
the rest. Two runs of the same kernels on the same inputs are compared, so every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Every settable key with a legal value that is not its default. Written out on purpose: a key that joins the table in csrc/tune.cpp
# belongs here too. The product refuses the values that select a tools-only kernel variant, so it keeps the only value it accepts there.
KEYS = dict(morph_split=2, grid_cap=7, nt_store=1, out_cap=64, graph=1, inst_loop=4, pose_prefetch=0, inst_subsets=0, fuse_fk=0,
            zero_copy=0, fuse_fk_plain=0, pose_pull=0, overlap=1, inst_order=0, inst_block=512, qdef_chunks=3, fast=0, sparse_piece=48)
PRODUCT_ONLY = dict(unroll=8, geo_lds=0, nontemporal=1)
VARIANTS_ONLY = dict(unroll=4, geo_lds=1, nontemporal=0)
DEFAULTS = dict(morph_split=0, grid_cap=0, nt_store=-1, out_cap=-1, graph=0, inst_loop=-1, pose_prefetch=-1, inst_subsets=-1, fuse_fk=-1,
                zero_copy=-1, fuse_fk_plain=-1, pose_pull=-1, overlap=-1, inst_order=1, inst_block=0, qdef_chunks=0, fast=-1, sparse_piece=0,
                unroll=0, geo_lds=0, nontemporal=1)


@pytest.mark.parametrize("build", ["product", "variants"])
def test_a_fork_inherits_every_tuning_key_by_value(request, rz, build):
    from reze_engine_amd import synth
    lib = rz if build == "product" else request.getfixturevalue("rzv")
    want = dict(KEYS, **(PRODUCT_ONLY if build == "product" else VARIANTS_ONLY))
    assert set(want) == set(DEFAULTS)
    mesh = synth.make_mesh(64, 2)
    with lib.DeformContext(0) as c:
        c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
        c.upload_skeleton(mesh["inv_bind"])
        assert {k: c.get_tuning(k) for k in DEFAULTS} == DEFAULTS
        c.set_tuning(**want)
        assert {k: c.get_tuning(k) for k in want} == want
        f = c.fork()
        assert {k: f.get_tuning(k) for k in want} == want
        for k in want:                                        # by value: what the fork is told stays with the fork
            f.set_tuning(**{k: DEFAULTS[k]})
            assert f.get_tuning(k) == DEFAULTS[k] and c.get_tuning(k) == want[k], k
        c.set_tuning(grid_cap=9)                              # ... and the other way round
        assert f.get_tuning("grid_cap") == 0
        f.close()
        assert {k: c.get_tuning(k) for k in want} == dict(want, grid_cap=9)


V, B, M = 1500, 24, 3               # 1500: the second 1024-vertex tile is partly padding
STATE = (0, 4.37, 1, 6.6, 0.25)     # clip 0 at frame 4.37 cross-faded by 0.25 into clip 1 at frame 6.6
COUNTS = ("verts", "bones", "morphs", "morph_mode", "sdef_verts", "qdef_verts", "ik_chains", "motion_clips")


@pytest.fixture(scope="module")
def scene(rz):
    """Everything that can be resident together, each table at the smallest size at which it is not trivial."""
    from reze_engine_amd import synth
    mesh = synth.make_mesh(V, B)
    depth = np.zeros(B, dtype=int)
    for b in range(B):
        depth[b] = 0 if mesh["parents"][b] < 0 else depth[mesh["parents"][b]] + 1
    assert depth.max() >= 2
    rng = np.random.default_rng(77)
    sd = synth.make_sdef(mesh, 0.02, seed=9)
    qd = np.setdiff1d(synth.make_qdef(mesh, 0.03, seed=10), sd["idx"]).astype(np.uint32)
    chains = synth.make_ik(mesh, n_chains=1, seed=8)
    assert 0 < len(sd["idx"]) < 256 and 0 < len(qd) < 256 and len(chains) == 1
    q = rng.normal(size=4)
    return dict(mesh=mesh, dense=synth.make_morphs_dense(V, M)[0], sd=sd, qd=qd, chains=chains,
                bone_morph=([1], [3], [[0.1, -0.2, 0.05]], [(q / np.linalg.norm(q)).astype(np.float32)]),
                motion=synth.make_motion(B, M, seed=30), clips=[synth.make_motion(B, M, seed=31), synth.make_motion(B, M, seed=32, flip=0.5)],
                edge=rng.uniform(0.5, 2.0, size=V).astype(np.float32))


def uploads(c, s):
    """(name, upload) of every static table, in an order in which no upload drops what an earlier one brought"""
    m, sd = s["mesh"], s["sd"]
    return [("mesh", lambda: c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])),
            ("skeleton", lambda: c.upload_skeleton(m["inv_bind"])),
            ("topology", lambda: c.upload_skeleton_topology(m["parents"], m["bind"])),
            ("dense morphs", lambda: c.upload_morphs_dense(s["dense"])),
            ("bone morphs", lambda: c.upload_bone_morphs(*s["bone_morph"])),
            ("animation", lambda: c.upload_animation(**s["motion"])),
            ("motions", lambda: c.upload_motions(s["clips"])),
            ("edge scale", lambda: c.upload_edge_scale(s["edge"])),
            ("sdef", lambda: c.upload_sdef(sd["idx"], sd["c"], sd["r0"], sd["r1"])),
            ("qdef", lambda: c.upload_qdef(s["qd"])),
            ("ik", lambda: c.upload_ik(s["chains"]))]


def frames(c):
    """positions, normals and hull of a pose blended from the library and of one sampled from the single motion"""
    out = []
    for pose in (lambda: c.set_pose_blended(*STATE), lambda: c.set_pose_sampled([7.5])):
        pose()
        c.deform()
        out.extend(c.read() + (c.read_hull(),))
    assert all(np.isfinite(a).all() for a in out)
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_fork_borrows_every_static_table_and_frees_none(rz, scene):
    s = scene
    c = rz.DeformContext(0)
    for _name, up in uploads(c, s):
        up()
    counts = {k: c.get_tuning(k) for k in COUNTS}
    assert counts == dict(verts=V, bones=B, morphs=M, morph_mode=1, sdef_verts=len(s["sd"]["idx"]), qdef_verts=len(s["qd"]), ik_chains=1, motion_clips=2)
    first = frames(c)
    assert not np.array_equal(first[2], first[0]) and not np.array_equal(first[3], first[0])     # a hull, and two different poses
    f = c.fork()
    assert {k: f.get_tuning(k) for k in COUNTS} == counts
    assert same(frames(f), first)
    for ctx, who in ((c, "lender"), (f, "fork")):
        for name, up in uploads(ctx, s):
            with pytest.raises(rz.RzError) as e:
                up()
            assert e.value.code == -1 and "fork" in str(e.value), (who, name)
    assert same(frames(f), first) and same(frames(c), first)  # a refused upload changed nothing
    f.close()
    assert same(frames(c), first)                             # the fork took nothing with it
    for _name, up in uploads(c, s):
        up()
    assert {k: c.get_tuning(k) for k in COUNTS} == counts
    assert same(frames(c), first)
    h, c._h = c._h, None
    assert c._L.rz_destroy(h) == 0
