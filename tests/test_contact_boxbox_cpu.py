"""Contacts between two boxes without a GPU: what the definition (tests/contact_boxbox_ref.py) promises, its separating-axis search alone
against a dense scan, the host half of rz_physics_contacts(ctx, 3) (reze-engine_amd/csrc/contact_table.h, through
tests/contact_table_main.cpp built with -fsanitize=address,undefined) against the definition's lists, the conditioning and contact
activity of every case tests/test_gpu_contact_boxbox.py runs, and the Engine option 'all' against a recording addon."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_box_scenes as bs
import contact_boxbox_ref as xr
import contact_boxbox_scenes as xs
import contact_ref as cr
import contact_scenes as cs
import physics_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILL = 2.5e-5                            # the conditioning bar of tests/test_contact_cpu.py
IDENT = np.eye(4).T.reshape(1, 16)


def surface(e, n=7):
    """points on the surface of the box |y_i| <= e_i in its own frame: an n x n grid on every face (vertices and edges among them)"""
    g = np.linspace(-1.0, 1.0, n)
    u, v = [a.reshape(-1) for a in np.meshgrid(g, g)]
    pts = []
    for i in range(3):
        for s in (-1.0, 1.0):
            p = np.zeros((len(u), 3))
            p[:, i], p[:, (i + 1) % 3], p[:, (i + 2) % 3] = s, u, v
            pts.append(p * np.asarray(e))
    return np.concatenate(pts)


def gap_and_depth(xa, qa, ea, xb, qb, eb, n=7):
    """Independent of the separating-axis search: over a dense scan of each box's surface points taken into the other's frame, the smallest
    distance to the other box (0 when a point is inside) and the largest depth of a point inside it (its distance to the nearest face)"""
    gap, depth = np.inf, 0.0
    for (x1, q1, e1), (x2, q2, e2) in (((xa, qa, ea), (xb, qb, eb)), ((xb, qb, eb), (xa, qa, ea))):
        p = pr.qrot(np.asarray(q1, dtype=np.float64)[None], surface(e1, n)) + x1
        c = pr.qrot(pr.qconj(np.asarray(q2, dtype=np.float64))[None], p - x2)
        out = np.linalg.norm(c - np.clip(c, -np.asarray(e2), np.asarray(e2)), axis=1)
        gap = min(gap, float(out.min()))
        depth = max(depth, float(np.maximum((np.asarray(e2) - np.abs(c)).min(axis=1), 0.0).max()))
    return gap, depth


CORNER_DOWN = cs._quat(np.cross([1.0, 1.0, 1.0], [0.0, -1.0, 0.0]), float(np.arccos(-1 / np.sqrt(3))))      # a cube's diagonal turned onto -y
# name: (the dropped box's half extents, its rotation at release, the following box's half extents)
DROPS = {
    "flat cube": ((0.5, 0.5, 0.5), (0, 0, 0, 1), (1.5, 1.0, 1.2)),
    "cube tilted by 0.3": ((0.5, 0.5, 0.5), cs._quat([0, 0, 1], 0.3), (1.5, 1.0, 1.2)),
    "cube corner first": ((0.5, 0.5, 0.5), CORNER_DOWN, (1.5, 1.0, 1.2)),
    "thin tilted plate": ((0.8, 0.05, 0.8), cs._quat([0, 0, 1], 0.3), (1.5, 1.0, 1.2)),
    "wide plate on a narrow box": ((2.0, 0.2, 2.0), (0, 0, 0, 1), (0.5, 1.0, 0.5)),
    "box tilted about two axes": ((0.6, 0.3, 0.4), cs._quat([1, 0, 0.7], 0.5), (1.5, 1.0, 1.2)),
}


def drop_sim(e, rot, base, dtype=np.float64):
    """the drop: the box released from rest with its centre 1.8 x its largest half extent above the top face of a following box
    at the origin, a little off its middle; default h, iterations and gravity, both dampings and both frictions 0.5"""
    t = pr.make_table([dict(bone=0, type=0, shape=1, size=list(base), mass=0.0, friction=0.5),
                       dict(bone=-1, type=1, shape=1, size=list(e), mass=1.0, offset_pos=[0.1, base[1] + 1.8 * max(e), -0.05], offset_rot=rot,
                            linear_damping=0.5, angular_damping=0.5, friction=0.5)], [])
    return cr.Sim(t, [-1], [[0, 0, 0]], dtype=dtype, mode=3), IDENT.copy()


@pytest.mark.parametrize("name", list(DROPS))
def test_a_dropped_box_comes_to_rest_on_a_face(name):
    """300 substeps after its release the box rests on a face of the following box: one of its axes is the face's normal, the gap or
    penetration left is below 2 % of its smallest half extent (the project's resting bar), and in no substep did it penetrate by more than
    10 % of that. Gap and depth come from a scan of surface points, not from the search under test.
    (The thin plate is 0.8 wide: at the default step and gravity a plate lying flat turns by about 60 g h^2 / e times its tilt per
    contact — the point of 1c slides by e tilt / 0.05 off the middle, the plate's inertia is m e^2 / 3 —, which is 1.04 / e: once that
    overshoots, a resting thin plate rattles at about 0.007 rad — measured at e = 0.5 and 0.6, not at 0.8)"""
    e, rot, base = DROPS[name]
    sim, W = drop_sim(e, rot, base)
    worst = 0.0
    for _ in range(300):
        sim.step(W, 1)
        worst = max(worst, gap_and_depth(sim.x[0], sim.q[0], base, sim.x[1], sim.q[1], e)[1])
    gap, depth = gap_and_depth(sim.x[0], sim.q[0], base, sim.x[1], sim.q[1], e, n=21)
    up = np.abs(np.stack(xr.axes_of(sim.q[1:2]), axis=1)[0][:, 1]).max()
    print("%s: at rest gap %.2e depth %.2e (%.2f %% of the smallest half extent), deepest over the run %.4f (%.1f %%), an axis within %.1e of the normal, speed %.1e; %s"
          % (name, gap, depth, 100 * max(gap, depth) / min(e), worst, 100 * worst / min(e), 1 - up, np.linalg.norm(sim.v[1]), sim.kinds))
    assert max(gap, depth) < 0.02 * min(e) and worst < 0.1 * min(e)
    assert up > 1 - 1e-4 and sim.x[1, 1] > base[1] and sim.n_boxbox > 100


def test_crossed_bars_are_held_by_their_edges():
    """a bar along z with an edge down, released just above a following bar along x with an edge up: the pair meets edge on edge, the
    edge contacts of 1d hold it — it never passes through: the scan's depth stays below 10 % of the bars' thickness in every substep, and
    while only edges touch the bar's centre stays above the edge it lies on (it tips about that edge, which lowers it) —, and it rolls onto a face (and then, a bar balanced across a
    bar turned by 45 degrees, slides off: nothing is asserted about where it ends)"""
    fol = dict(bone=0, type=0, shape=1, size=[2.0, 0.2, 0.2], mass=0.0, offset_rot=cs._quat([1, 0, 0], np.pi / 4), friction=0.5)
    top = 0.2 * np.sqrt(2)
    dyn = dict(bone=-1, type=1, shape=1, size=[0.2, 0.2, 2.0], mass=1.0, offset_pos=[0.05, 2 * top + 0.02, 0.03], offset_rot=cs._quat([0, 0, 1], np.pi / 4 + 0.02),
               linear_damping=0.5, angular_damping=0.5, friction=0.5)
    sim = cr.Sim(pr.make_table([fol, dyn], []), [-1], [[0, 0, 0]], mode=3)
    W = IDENT.copy()
    worst, low, first = 0.0, np.inf, None
    for k in range(200):
        sim.step(W, 1)
        worst = max(worst, gap_and_depth(sim.x[0], sim.q[0], fol["size"], sim.x[1], sim.q[1], dyn["size"], n=21)[1])
        if first is None and sim.kinds:
            first = dict(sim.kinds)
        if all(key[0] == "edge" for key in sim.kinds):
            low = min(low, sim.x[1, 1])
    edges = sum(n for key, n in sim.kinds.items() if key[0] == "edge")
    faces = sum(n for key, n in sim.kinds.items() if key[0] != "edge")
    print("crossed bars: first contacts %s; %d edge and %d face contacts; deepest %.4f, lowest centre while only edges touch %.3f (edge on edge at %.3f)" % (first, edges, faces, worst, low, 2 * top))
    assert first and all(key[0] == "edge" for key in first) and edges >= 4 and faces > 0
    assert worst < 0.1 * 0.2 and low > top + 0.2 and np.isfinite(sim.state13()).all()


def _slide(mu):
    """a box lying on the top face of a following box tilted by 0.5 rad (under 45 degrees): its drift down the face over 30 substeps, its
    drift off the face, the substeps in contact"""
    tilt = cs._quat([0, 0, 1], -0.5)
    down, normal = pr.qrot(tilt, np.array([1.0, 0.0, 0.0])), pr.qrot(tilt, np.array([0.0, 1.0, 0.0]))
    sim = cr.Sim(pr.make_table([dict(bone=0, type=0, shape=1, size=[12.0, 0.5, 2.0], mass=0.0, offset_rot=tilt, friction=1.0),
                                dict(bone=-1, type=1, shape=1, size=[0.6, 0.3, 0.5], mass=1.0, offset_pos=list(normal * 0.8), offset_rot=tilt, friction=mu)], []), [-1], [[0, 0, 0]], mode=3)
    W = IDENT.copy()
    sim.step(W, 0)
    x0 = sim.x[1].copy()
    sim.step(W, 30)
    return float(np.dot(sim.x[1] - x0, down)), float(np.dot(sim.x[1] - x0, normal)), sum(a > 0 for a in sim.active)


def test_friction_holds_a_box_that_slides_without_it():
    """mu = 0 (the dynamic box's friction; the product is 0): the box slides down the tilted face by g sin(0.5) t^2 / 2 within 5 %. mu = 1
    with tan(0.5) = 0.55 < 1: the contact sticks — its drift is below 5 % of the frictionless one. The bars of the capsule test."""
    free, off0, n0 = _slide(0.0)
    held, off1, n1 = _slide(1.0)
    t = 30 * pr.DEFAULT_H
    want = 0.5 * 98 * np.sin(0.5) * t * t
    print("drift down the face over 30 substeps: %.4f without friction (g sin(0.5) t^2 / 2 = %.4f), %.4f with mu = 1 (ratio %.3f); off the face %.3f / %.3f; %d / %d substeps in contact"
          % (free, want, held, held / free, off0, off1, n0, n1))
    assert abs(free / want - 1) < 0.05
    assert abs(held) < 0.05 * free and n0 >= 28 and n1 >= 28 and abs(off0) < 0.05 and abs(off1) < 0.05


def _random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    eA, eB = rng.uniform(0.1, 1.2, size=(n, 3)), rng.uniform(0.1, 1.2, size=(n, 3))
    xB = rng.uniform(-1.6, 1.6, size=(n, 3))
    q = rng.normal(size=(2, n, 4))
    q[0, : n // 8] = [0, 0, 0, 1]
    q[1, : n // 8] = q[0, : n // 8] + 1e-4 * rng.normal(size=(n // 8, 4))         # near-parallel pairs: edge axes are skipped
    q /= np.linalg.norm(q, axis=2)[:, :, None]
    return np.zeros((n, 3)), q[0], eA, xB, q[1], eB


def test_the_search_alone_against_a_dense_scan():
    """1500 seeded box pairs, an eighth of them near parallel. Against a scan of 11 x 11 surface points per face: where the scan finds
    the boxes apart by more than its own resolution (the distance to a box is 1-Lipschitz in the point, a surface point lies within half
    a grid diagonal of a sample), the search reports no contact; where a sample lies inside the other box by more than that, it reports
    one. pen is the chosen overlap, and the smallest overlap over the axes considered up to the 0.95 that favours a face; n is a unit
    vector from A to B; on a face cB = cA - n pen; in float32 the verdict is the same wherever no overlap is within 1e-4 of 0."""
    n = 1500
    xA, qA, eA, xB, qB, eB = _random_pairs(n, 17)
    f = xr.front_end(xA, qA, eA, xB, qB, eB)
    scan = np.array([gap_and_depth(xA[k], qA[k], eA[k], xB[k], qB[k], eB[k], n=11) for k in range(n)])
    res = np.maximum(eA, eB).max(axis=1) * 2 / 10 * np.sqrt(2) / 2
    apart, inside = scan[:, 0] > res, scan[:, 1] > res
    print("search vs scan over %d pairs: %d in contact, %d apart by the scan, %d inside by the scan, %d with an edge axis skipped, %d edge contacts" % (
        n, int(f["ok"].sum()), int(apart.sum()), int(inside.sum()), int((~f["considered"].all(axis=1)).sum()), int((f["ok"] & f["edge"]).sum())))
    assert not (f["ok"] & apart).any() and f["ok"][inside].all()
    assert apart.sum() > n // 10 and inside.sum() > n // 10 and (~f["considered"].all(axis=1)).sum() >= n // 8 and (f["ok"] & f["edge"]).sum() > 20
    ok = f["ok"]
    smallest = np.minimum(f["face"].min(axis=1), np.where(f["considered"], f["edges"], np.inf).min(axis=1))
    chosen = np.where(f["edge"], f["edges"][np.arange(n), f["axis"] % 9], f["face"][np.arange(n), f["axis"] % 6])
    assert np.array_equal(f["pen"][ok], chosen[ok]) and (f["pen"][ok] >= smallest[ok]).all() and (f["pen"][ok] * 0.95 <= smallest[ok] * (1 + 1e-12)).all()
    assert np.array_equal(f["pen"][ok & f["edge"]], smallest[ok & f["edge"]])
    assert np.allclose(np.linalg.norm(f["n"][ok], axis=1), 1, atol=1e-12) and (pr.dot(f["n"], xB - xA)[ok] >= 0).all()
    face = ok & ~f["edge"]
    assert np.allclose((f["cB"] - f["cA"])[face], (-f["n"] * f["pen"][:, None])[face], atol=1e-12)
    f32 = xr.front_end(*[a.astype(np.float32) for a in (xA, qA, eA, xB, qB, eB)])
    clear = (np.abs(f["face"]) > 1e-4).all(axis=1) & (~f["considered"] | (np.abs(f["edges"]) > 1e-4)).all(axis=1)
    assert f32["pen"].dtype == np.float32 and np.array_equal(f32["ok"][clear], ok[clear]) and clear.sum() > n // 2


def test_what_is_a_candidate_with_box_pairs():
    """two boxes pair like any two shapes, in either role; mode 2 counts the same pairs and leaves them out; a table without a pair of two
    boxes has the same lists either way"""
    dyn = dict(type=1, mass=1.0, shape=0, size=[0.3, 0, 0])
    fol = dict(type=0, mass=0.0, shape=0, size=[0.3, 0, 0])
    bx = dict(shape=1, size=[0.3, 0.2, 0.1])
    t = pr.make_table([dict(fol, **bx), dict(dyn), dict(dyn, **bx), dict(fol, shape=2, size=[0.2, 0.5, 0]), dict(dyn, **bx), dict(fol, **bx)], [])
    L = cr.contact_lists(t, 3)
    assert (L["n_follow"], L["n_pairs"], L["box_pairs"], L["n_box_box"], L["boxes"]) == (9, 3, 0, 5, 0)
    assert L["follow_off"].tolist() == [0, 0, 3, 6, 6, 9, 9] and L["follow_idx"].tolist() == [0, 3, 5, 0, 3, 5, 0, 3, 5]
    assert L["pairs"].tolist() == [[1, 2], [1, 4], [2, 4]] and L["colour_off"].tolist() == [0, 1, 2, 3]
    off = cr.contact_lists(t, 2)
    assert off["n_box_box"] == 0 and off["box_pairs"] == L["n_box_box"] == 5 and off["n_follow"] + off["n_pairs"] == L["n_follow"] + L["n_pairs"] - 5
    assert off["follow_idx"].tolist() == [0, 3, 5, 3, 3] and off["pairs"].tolist() == [[1, 2], [1, 4]]
    assert all(np.array_equal(off[k], L[k]) for k in ("radius", "half", "friction", "takes", "box", "ext", "boxes"))
    # two following boxes are no pair; a zero extent keeps a box out
    assert cr.contact_lists(pr.make_table([dict(fol, **bx), dict(fol, **bx)], []), 3)["n_box_box"] == 0
    assert cr.contact_lists(pr.make_table([dict(dyn, **bx), dict(fol, shape=1, size=[0.3, 0.0, 0.1])], []), 3)["n_box_box"] == 0
    t = bs.with_box_pair(apart=True)["table"]
    a, b = cr.contact_lists(t, 3), cr.contact_lists(t, 2)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_without_box_pairs_the_definition_is_contact_box_ref():
    """mode 2 on a table with pairs of two boxes, and mode 3 on a table without one: the runs are those of contact_box_scenes' Sim (mode
    2), bit for bit"""
    for sc, mode in ((bs.case("box pair")[0], 2), (bs.with_box_pair(apart=True), 3)):
        poses = [bs.pose(sc, k, 0.3) for k in range(3)]
        a = bs.run_reference(sc, poses, bs.SHORT, sim=xs.sim_of(sc, mode=mode))
        b = bs.run_reference(sc, poses, bs.SHORT, sim=bs.sim_of(sc))
        for (wa, sa), (wb, sb) in zip(a, b):
            assert np.array_equal(wa, wb) and np.array_equal(sa, sb)


def test_cases_are_well_conditioned_and_touch():
    """every GPU case, none left out: the float32 probe of the definition stays within 2.5e-5 x extent of its float64 run over the whole
    horizon (quaternions within 2.5e-5), a contact is active in at least a quarter of the substeps, contacts between two boxes are active
    and move the last state by more than 0.01 against the definition of mode 2; the cases take the launch forms, the roles and the kinds
    of contact they are there for; the pairs separated along one axis are that, and the box pair scene differs under mode 3"""
    rows, bad = [], {}
    for name in xs._CASES:
        c, act, turn = xs.conditioning(name)
        ref, sim = xs.reference(name)
        moved = float(np.abs(xs.reference(name, mode=2)[0][-1][1][:, :3] - ref[-1][1][:, :3]).max())
        rows.append("%s %.1e / %.2f / %.1e / %d / %.3f" % (name, c, act, turn, sim.n_boxbox, moved))
        if c > ILL or act < 0.25 or turn > ILL or sim.n_boxbox < 10 or moved <= 0.01:
            bad[name] = (c, act, turn, sim.n_boxbox, moved)
        sc, _, calls = xs.case(name)
        assert len(calls) <= 3 and sc["table"]["n_bodies"] <= 300 and sim.lists["n_box_box"] > 0, name
    print("float32 probe / extent, active fraction, quaternion probe, contacts between boxes, moved against mode 2: " + ", ".join(rows))
    assert not bad, "ill-conditioned or idle: %s" % bad
    for name, (block, own) in xs.FORMS.items():
        t = xs.case(name)[0]["table"]
        widest = max(np.bincount(pr.colouring(t)[0])) if t["n_joints"] else 0
        assert (64 if t["n_bodies"] <= 64 and widest <= 64 else 256) == block and int(t["n_joints"] <= block) == own, name
    for name, want in xs.KINDS.items():
        kinds = xs.reference(name)[1].kinds
        hits = sum(n for key, n in kinds.items() if want(key))
        assert hits >= 10 and hits >= 0.75 * sum(kinds.values()), (name, kinds)
    assert sum(n for key, n in xs.reference("edge on a face")[1].kinds.items()) > 0
    sim = xs.reference("near parallel")[1]
    assert sim.n_skipped >= 0.9 * sim.n_boxbox > 0
    for order, want in (("fd", [False, True]), ("df", [True, False]), ("dd", [True, True])):
        name = "box box " + order
        sc, sim = xs.case(name)[0], xs.reference(name)[1]
        t, dyn = sc["table"], pr.is_dynamic(sc["table"])
        pair = [b for b in range(1, t["n_bodies"]) if not (order == "dd" and b == 1)]
        assert [int(t["shape"][b]) for b in pair] == [1, 1] and [bool(dyn[b]) for b in pair] == want and (sim.lists["n_pairs"] == 1) == (order == "dd"), name
    for kind, axes in (("A", range(0, 3)), ("B", range(3, 6)), ("edge", range(6, 15))):
        sc = xs.single_axis(kind)
        sim = xs.sim_of(sc)
        xs.run_reference(sc, xs.single_axis_poses(sc), xs.SHORT, sim=sim)
        assert len(sim.apart) == 1 and sum(sim.apart.values()) == 84 and not sim.kinds, (kind, sim.apart, sim.kinds)
        (key,) = sim.apart
        assert len(key) == 1 and key[0] in axes and sum(a > 0 for a in sim.active) >= 10, (kind, key)
    sc, poses, calls = bs.case("box pair")
    a, b = bs.run_reference(sc, poses, calls, sim=xs.sim_of(sc)), bs.run_reference(sc, poses, calls, sim=xs.sim_of(sc, mode=2))
    assert np.abs(a[-1][1][:, :3] - b[-1][1][:, :3]).max() > 0.01
    # the Node end-to-end case: the PMX's table under one pose, the engine's substeps
    c, act, sim = xs.node_conditioning()
    print("node case: %.1e / %.2f / %d" % (c, act, sim.n_boxbox))
    assert c <= ILL and act >= 0.25 and sim.n_boxbox > 0


# ---- the host half: contact_table.h with pairs of two boxes kept against the definition's lists ----

@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    return cs.build_table_tool(tmp_path_factory.mktemp("contact_boxbox_table"))


run_tool, limit_table = cs.run_table_tool, xs.limit_table


def mixed_table():
    dyn = dict(type=1, mass=1.0, shape=0, size=[0.3, 0, 0])
    fol = dict(type=0, mass=0.0, shape=0, size=[0.3, 0, 0])
    bx = dict(shape=1, size=[0.3, 0.2, 0.1])
    return pr.make_table([dict(dyn, group=1), dict(dyn, group=1, **bx), dict(fol, shape=1, size=[1, 1, 1]), dict(fol, shape=1, size=[1, 1, 1], mask=0), dict(fol, shape=1, size=[1, 0, 1]),
                          dict(dyn, shape=2, size=[0.2, 0.5, 0]), dict(fol, group=3, mask=0xffff & ~2), dict(dyn, size=[0, 0, 0]), dict(fol, group=20), dict(fol, group=4),
                          dict(dyn, group=5, **bx), dict(dyn, shape=1, size=[0.3, 0.2, 0.0]), dict(dyn, group=6, mask=0xffff & ~(1 << 5), **bx), dict(fol, group=7, **bx)], [])


@pytest.mark.parametrize("name", ["own 64", "stride 256", "box box dd", "box pair", "mixed"])
def test_host_lists_equal_the_definition(tools, name):
    """shape records with the box bit, c_box, the follow CSR, the dynamic pairs in solve order, colour offsets and all counts, entry for
    entry, with pairs of two boxes kept; and with them left out, under mode 2"""
    tool = tools
    t = mixed_table() if name == "mixed" else bs.case("box pair")[0]["table"] if name == "box pair" else xs.case(name)[0]["table"]
    L = cr.contact_lists(t, 3)
    rows, _ = run_tool(tool, t, 3)
    cs.assert_host_lists(rows, L)
    assert L["box_pairs"] == 0 and L["n_box_box"] > 0
    # pairs of two boxes left out: the boxes mode
    L2 = cr.contact_lists(t, 2)
    rows, _ = run_tool(tool, t, 2)
    cs.assert_host_lists(rows, L2)
    assert L2["n_box_box"] == 0 and L2["box_pairs"] == L["n_box_box"]


def test_host_refuses_one_past_the_limit_with_box_pairs(tools):
    """256 dynamic boxes x 256 following boxes = 65 536 candidates, every one a pair of two boxes, are taken; 256 x 257 are refused with
    the counts in the message; a table of spheres, boxes and box pairs one past the limit is refused with its box pairs counted; with the
    pairs of two boxes left out both are taken"""
    tool = tools
    rows, _ = run_tool(tool, limit_table(256), 3)
    assert rows["counts"][:2] == ["65536", "0"] and rows["refused"][0] == "0" and len(rows["follow_idx"]) == 65536 and rows["box_box"] == ["65536"]
    rows, out = run_tool(tool, limit_table(257), 3)
    assert rows["counts"][:2] == ["65792", "0"] and rows["refused"][0] == "1" and rows.get("follow_idx", []) == [] and rows["box_box"] == ["65792"]
    assert cr.refusal(cr.contact_lists(limit_table(257), 3)) in out and "(65792 of them pairs of two boxes)" in out and "broad phase" in out
    assert not cr.refusal(cr.contact_lists(limit_table(256), 3)) and not cr.refusal(cr.contact_lists(limit_table(257), 2))
    rows, _ = run_tool(tool, limit_table(257), 2)
    assert rows["counts"][:2] == ["0", "0"] and rows["refused"][0] == "0" and rows["box_pairs"] == ["65792"] and rows["box_box"] == ["0"]
    # mixed: 255 dynamic spheres and one dynamic box against 257 following boxes: 65 535 sphere - box entries and 257 box - box ones
    t = limit_table(257)
    t["shape"][:255] = 0
    L = cr.contact_lists(t, 3)
    assert (L["n_follow"], L["n_box_box"]) == (65792, 257) and cr.refusal(L) == "65792 follow entries and 0 dynamic pairs (257 of them pairs of two boxes)"
    rows, out = run_tool(tool, t, 3)
    assert rows["refused"][0] == "1" and cr.refusal(L) in out
    rows, _ = run_tool(tool, t, 2)
    assert rows["counts"][:2] == ["65535", "0"] and rows["refused"][0] == "0" and rows["box_pairs"] == ["257"]


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_engine_all_option_with_a_recording_addon(tmp_path):
    """Engine { physicsContacts: 'all' } against a stand-in for the addon: physicsContacts(ctx, 3) follows uploadPhysics on every shard at
    loadModel; 'boxes' still passes 2 and true 1; any other string turns nothing on; 'all' without devicePhysics throws"""
    sc, data, _ = xs.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "contacts_engine_mock.js"), str(tmp_path / "s.pmx"), "all", "boxes", "true", "everything"], timeout=60).decode().strip().splitlines()[-1])
    assert r["needsDevicePhysics"] and r["shards"] >= 2 and len(r["all"]) == r["shards"]
    for tag, want in (("all", "physicsContacts:3"), ("boxes", "physicsContacts:2"), ("true", "physicsContacts:1")):
        for calls in r[tag]:
            assert [c for c in calls if c.startswith("physicsContacts")] == [want] and calls.index(want) == calls.index("uploadPhysics") + 1
    assert all("physicsContacts" not in " ".join(calls) for calls in r["everything"]) and all("uploadPhysics" in calls for calls in r["everything"])
