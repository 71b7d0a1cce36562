"""The sparse morph row walk (kernels/deform_small.hip, MODE 2) at its LDS piece edges: every scene of tests/sparse_piece_scenes.py at every
piece size the "sparse_piece" key takes here, in both frame forms, both wave-step sizes, fused behind the hierarchy solve and as two
instances. Two bars: the frames of one scene are the same BITS at every piece size, and the frames at the plan's own size and at the
smallest one match the oracle — which, with the per-entry condition tests/test_sparse_pieces_cpu.py holds the scenes to, means every
single entry was staged, walked and weighted once.

Why the bits cannot depend on the piece size (read off the kernel): a lane accumulates its row with one fmaf chain per component, in
entry order, from +0; a piece boundary only splits the chain between two entries (lo = max(b0, c0), hi = min(b1, c1)), the accumulators
live across pieces. The masked tail of a group of eight adds fmaf(0, finite, acc) = acc — exactly, unless acc is -0, and a sum that
starts at +0 is never -0 under round-to-nearest (x + (-x) = +0, and nothing here underflows). So a differing bit is a kernel bug."""
import numpy as np
import pytest

import sparse_piece_scenes as sps
from helpers import assert_parity

pytestmark = pytest.mark.gpu

RESET = dict(morph_split=0, grid_cap=0, fast=-1, out_cap=-1, fuse_fk=-1, graph=0, sparse_piece=0)
FORMS = [dict(fast=1, morph_split=4), dict(fast=0, morph_split=4), dict(fast=1, morph_split=1), dict(fast=0, morph_split=1)]
BIG = 3242                  # bones: 152 KB of palette, the largest skeleton the LDS holds
WORST = {}                  # (scene, P designed for, piece run) -> worst (position, normal) error against the float64 reference


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nsparse piece edges: worst error against the float64 reference (bar 1e-4), per scene and piece size run")
    for (name, P, run), (ep, en) in sorted(WORST.items()):
        print("  %-9s designed for %4d, piece %-4s  position %.3e  normal %.3e" % (name, P, run or "auto", ep, en))


def references(oracle, s, mw=None, world=None, inv_bind=None):
    """the project's oracle (binary32, the reference's operation order) and the float64 restatement"""
    m = s["mesh"]
    mw = s["mw"] if mw is None else mw
    pm = oracle.morph_sparse(s["V"], s["off"], s["idx"], s["d3"], mw, m["pos"])
    S = oracle.palette(m["world"] if world is None else world, m["inv_bind"] if inv_bind is None else inv_bind)
    return oracle.skin(pm, m["nrm"], m["joints"], m["weights"], S), sps.reference64(s, mw)


def check(pg, ng, refs, s, run, what):
    (pr, nr), (p64, n64) = refs
    assert_parity(pg, ng, pr, nr, what + " (oracle)")
    e = assert_parity(pg, ng, p64, n64, what + " (float64)")
    key = (s["name"], s["P"], run)
    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0, 0.0)), e))


def upload(c, s, world=None, inv_bind=None):
    m = s["mesh"]
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"] if inv_bind is None else inv_bind)
    c.upload_morphs_sparse(s["off"], s["idx"], s["d3"])
    c.set_instances(1)
    c.set_tuning(**RESET)


def frames_at_every_piece(c, pose, what, pieces=sps.PIECES, instances=1):
    """{P: [(positions, normals) per instance]}, with the piece the plan reports checked against the one asked for"""
    out = {}
    for P in pieces:
        c.set_tuning(sparse_piece=P)
        eff = c.get_tuning("effective_sparse_piece")
        if P:
            assert eff == P, what
        else:
            print("%s: the plan's own piece is %d entries" % (what, eff))
            assert eff >= 64 and eff % 64 == 0, what
        pose()
        c.deform()
        out[P] = [c.read(instance=i) for i in range(instances)]
    first = out[pieces[0]]
    for P in pieces[1:]:
        for i in range(instances):
            assert np.array_equal(first[i][0], out[P][i][0]) and np.array_equal(first[i][1], out[P][i][1]), \
                "%s: piece %d and piece %d give different bits (instance %d)" % (what, pieces[0], P, i)
    return out


@pytest.mark.parametrize("name,P", sps.DESIGNS)
def test_bits_do_not_depend_on_the_piece_and_the_frame_is_right(rz, oracle, name, P):
    s = sps.scene(name, P)
    refs = references(oracle, s)
    forms = list(FORMS)
    if name == "bursts":
        forms.append(dict(fast=1, morph_split=4, out_cap=0))         # (every other form: out_cap auto = one 64-vertex step parked)
    if name == "straddle":
        forms.append(dict(fast=1, morph_split=4, grid_cap=1))        # one workgroup: a wave takes a second, steady-state step
    if name == "tall":                                               # one workgroup: 256-vertex steps of four rounds; 64-vertex steps five per wave
        forms += [dict(fast=1, morph_split=1, grid_cap=1), dict(fast=0, morph_split=1, grid_cap=1), dict(fast=1, morph_split=4, grid_cap=1)]
    with rz.DeformContext(0) as c:
        upload(c, s)
        for form in forms:
            what = "%s P=%d %r" % (name, P, form)
            c.set_tuning(**dict(RESET, **form))
            assert c.get_tuning("effective_split") == form["morph_split"] and c.get_tuning("effective_fast") == form["fast"]
            if "grid_cap" not in form:
                assert c.get_tuning("effective_out_cap") == (0 if form.get("out_cap") == 0 else 256 // form["morph_split"])     # auto: one step parked
            assert c.get_tuning("effective_grid") == sps.step_quads(s["V"], form["morph_split"], form.get("grid_cap", 0))[0]     # the steps are where the CPU test has them
            out = frames_at_every_piece(c, lambda: c.set_pose(s["mesh"]["world"], s["mw"]), what)
            for run in (0, 16):
                check(out[run][0][0], out[run][0][1], refs, s, run, "%s piece %d" % (what, run))


@pytest.mark.parametrize("name,P", [d for d in sps.DESIGNS if d[0] in ("straddle", "long_row")])
def test_behind_the_fused_hierarchy_solve(rz, oracle, name, P):
    """the hierarchy solved in the deform kernel's prologue: its scratch aliases the buffers the pieces land in"""
    s = sps.scene(name, P)
    m = s["mesh"]
    refs = references(oracle, s)
    with rz.DeformContext(0) as c:
        upload(c, s)
        c.upload_skeleton_topology(m["parents"], m["bind"])
        for split in (4, 1):
            what = "%s P=%d fused split=%d" % (name, P, split)
            c.set_tuning(**dict(RESET, fuse_fk=1, morph_split=split))
            c.set_pose_local(m["quats"], s["mw"])
            assert c.get_tuning("effective_fuse_fk") == 1 and c.get_tuning("effective_prep") == 0
            out = frames_at_every_piece(c, lambda: c.set_pose_local(m["quats"], s["mw"]), what)
            for run in (0, 16):
                check(out[run][0][0], out[run][0][1], refs, s, run, "%s piece %d" % (what, run))


@pytest.mark.parametrize("P", [p for n, p in sps.DESIGNS if n == "exact"])
def test_two_instances_with_their_own_weights(rz, oracle, P):
    s = sps.scene("exact", P)
    m = s["mesh"]
    refs = [references(oracle, s, mw) for mw in (s["mw"], s["mw2"])]
    with rz.DeformContext(0) as c:
        upload(c, s)
        c.set_instances(2)
        for split in (4, 1):
            what = "exact P=%d two instances split=%d" % (P, split)
            c.set_tuning(**dict(RESET, morph_split=split))
            out = frames_at_every_piece(c, lambda: c.set_pose(np.stack([m["world"], m["world"]]), np.stack([s["mw"], s["mw2"]])), what, instances=2)
            for run in (0, 16):
                for i in range(2):
                    check(out[run][i][0], out[run][i][1], refs[i], s, run, "%s piece %d instance %d" % (what, run, i))


def big_skeleton_frame(c, s, refs, world, what):
    c.set_pose(world, s["mw"])
    c.deform()
    pg, ng = c.read()
    check(pg, ng, refs, s, c.get_tuning("effective_sparse_piece"), what)
    return pg, ng


@pytest.mark.parametrize("name", ["straddle", "long_row"])
def test_a_skeleton_near_the_limit_through_the_front_door(rz, oracle, name):
    """sparse_piece = 0 and 3 242 bones: the palette leaves the pieces less than a burst. 163 840 B - 3 242 x 48 B of palette - 576 B of
    morph list and weights - 3 072 B of step scratch (morph_split 4) = 4 576 B; less the 1 KiB the plan keeps back, over 4 waves x 16 B:
    55 entries per wave, 48 as a multiple of 16 — and no room for the write-batching buffer. Going down from there the piece only grows."""
    found = None
    with rz.DeformContext(0) as c:
        s = sps.scene(name, 16)
        upload(c, s)
        for B in range(BIG, BIG - 64, -1):
            world, inv_bind = sps.padded_skeleton(s, B)
            c.upload_skeleton(inv_bind)
            eff = c.get_tuning("effective_sparse_piece")
            if eff < 64:
                found = (B, eff)
                break
        assert found is not None, "no skeleton of %d..%d bones leaves less than a burst" % (BIG - 63, BIG)
        B, eff = found
        print("%s: %d bones leave a piece of %d entries" % (name, B, eff))
        assert eff >= 16 and eff % 16 == 0
        if (name, eff) in sps.DESIGNS:              # the scene built around that very size
            s = sps.scene(name, eff)
            world, inv_bind = sps.padded_skeleton(s, B)
            upload(c, s, inv_bind=inv_bind)
            assert c.get_tuning("effective_sparse_piece") == eff
        refs = references(oracle, s, world=world, inv_bind=inv_bind)
        auto = big_skeleton_frame(c, s, refs, world, "%s %d bones, the plan's piece" % (name, B))
        c.set_tuning(sparse_piece=eff)
        assert c.get_tuning("effective_sparse_piece") == eff
        forced = big_skeleton_frame(c, s, refs, world, "%s %d bones, piece %d forced" % (name, B, eff))
        assert np.array_equal(auto[0], forced[0]) and np.array_equal(auto[1], forced[1])
        # a request that does not fit is lowered, never an LDS overflow — to the same frame
        c.set_tuning(sparse_piece=2048)
        low = c.get_tuning("effective_sparse_piece")
        assert 16 <= low < 2048 and low % 16 == 0
        lowered = big_skeleton_frame(c, s, refs, world, "%s %d bones, 2048 asked for" % (name, B))
        assert np.array_equal(auto[0], lowered[0]) and np.array_equal(auto[1], lowered[1])


def test_the_last_bytes_of_the_lds_at_256_vertex_steps(rz, oracle):
    """The branch of the plan that takes what the CU's 160 KB still hold (`hard`, csrc/plan.cpp) proper: at morph_split = 1 the step
    scratch is 12 KB, and a skeleton a little under the limit leaves the pieces 2-4 KB. Found through the front door: going down from
    3 242 bones, the first skeleton beside which a forced piece of 32 entries is not lowered. There the plan's own piece is those 32."""
    s = sps.scene("straddle", 32)
    with rz.DeformContext(0) as c:
        upload(c, s)
        c.set_tuning(morph_split=1, sparse_piece=32)
        for B in range(BIG, BIG - 256, -1):
            world, inv_bind = sps.padded_skeleton(s, B)
            c.upload_skeleton(inv_bind)
            if c.get_tuning("effective_sparse_piece") == 32:
                break
        else:
            pytest.fail("a piece of 32 entries fits beside no skeleton of %d..%d bones" % (BIG - 255, BIG))
        refs = references(oracle, s, world=world, inv_bind=inv_bind)
        forced = big_skeleton_frame(c, s, refs, world, "%d bones, 256-vertex steps, piece 32 forced" % B)
        c.set_tuning(sparse_piece=0)
        eff = c.get_tuning("effective_sparse_piece")
        print("256-vertex steps: %d bones leave a piece of %d entries" % (B, eff))
        assert eff == 32 and c.get_tuning("effective_out_cap") == 0
        auto = big_skeleton_frame(c, s, refs, world, "%d bones, 256-vertex steps, the plan's piece" % B)
        assert np.array_equal(auto[0], forced[0]) and np.array_equal(auto[1], forced[1])
        c.set_tuning(sparse_piece=16)
        small = big_skeleton_frame(c, s, refs, world, "%d bones, 256-vertex steps, piece 16" % B)
        assert np.array_equal(auto[0], small[0]) and np.array_equal(auto[1], small[1])


def test_the_write_batching_buffer_leaves_room_for_a_piece(rz, oracle):
    """3 200 bones: the 6 KB write-batching buffer of a 64-vertex step still fits beside the palette, but not together with the smallest
    piece — the plan has to do without the buffer (it is optional) instead of handing the frame a piece that overflows the LDS."""
    s = sps.scene("straddle", 64)
    world, inv_bind = sps.padded_skeleton(s, 3200)
    refs = references(oracle, s, world=world, inv_bind=inv_bind)
    with rz.DeformContext(0) as c:
        upload(c, s, inv_bind=inv_bind)
        assert c.get_tuning("effective_out_cap") == 0 and c.get_tuning("effective_sparse_piece") >= 16
        big_skeleton_frame(c, s, refs, world, "3200 bones, everything automatic")


def test_refusals_and_a_replayed_graph(rz, oracle):
    s = sps.scene("straddle", 16)
    refs = references(oracle, s)
    with rz.DeformContext(0) as c:
        upload(c, s)
        c.set_tuning(sparse_piece=48)
        for bad in (8, 24, 2064, -1):
            with pytest.raises(rz.capi.RzError) as e:
                c.set_tuning(sparse_piece=bad)
            assert "sparse_piece must be" in str(e.value)
            assert c.get_tuning("sparse_piece") == 48 and c.get_tuning("effective_sparse_piece") == 48
        c.upload_morphs_sparse(np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32))
        assert c.get_tuning("effective_sparse_piece") == 0          # no sparse targets resident
        c.upload_morphs_sparse(s["off"], s["idx"], s["d3"])
        # a captured graph bakes the piece in (RzDeformParams.sp_cap is part of the replay key): a new piece is a new graph
        c.set_tuning(graph=1, sparse_piece=16)
        c.set_pose(s["mesh"]["world"], s["mw"])
        c.deform_n(40)
        first = c.read()
        check(first[0], first[1], refs, s, 16, "graph replay, piece 16")
        c.set_tuning(sparse_piece=48)
        c.deform_n(40)
        assert c.get_tuning("effective_sparse_piece") == 48
        second = c.read()
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
        c.set_tuning(graph=0)
        c.deform()
        plain = c.read()
        assert np.array_equal(first[0], plain[0]) and np.array_equal(first[1], plain[1])
