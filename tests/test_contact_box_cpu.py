"""Box contacts without a GPU: what the definition (tests/contact_box_ref.py) promises, its closest-point routine alone against a dense scan,
the host half of rz_physics_contacts(ctx, 2) (reze-engine_amd/csrc/contact_table.h, through tests/contact_table_main.cpp built with
-fsanitize=address,undefined) against the definition's lists, the conditioning and contact activity of every case
tests/test_gpu_contact_boxes.py runs, and the Engine option 'boxes' against a recording addon."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_box_ref as br
import contact_box_scenes as bs
import contact_ref as cr
import contact_scenes as cs
import physics_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILL = 2.5e-5                            # the conditioning bar of tests/test_contact_cpu.py
IDENT = np.eye(4).T.reshape(1, 16)


def one_bone(bodies, joints=(), dtype=np.float64, **kw):
    """a table on one bone at the origin; returns (Sim with boxes taking part, world, table)"""
    t = pr.make_table(list(bodies), list(joints), **kw)
    return cr.Sim(t, [-1], [[0, 0, 0]], dtype=dtype, mode=2), IDENT.copy(), t


def test_a_dropped_sphere_comes_to_rest_on_a_following_box():
    """A sphere of radius 0.5 released 0.3 above the top face of a following box: after 300 substeps it rests on it — the gap or
    penetration is below 2 % of its radius (the bar of the sphere-on-sphere test, for its reasons) — and it never passed through: its
    centre stays above the contact height minus 10 % of the radius in every substep."""
    E, r = 1.0, 0.5
    sim, W, _ = one_bone([dict(bone=0, type=0, shape=1, size=[1.5, E, 1.2], mass=0.0),
                          dict(bone=-1, type=1, shape=0, size=[r, 0, 0], mass=1.0, offset_pos=[0.2, E + r + 0.3, -0.1], linear_damping=0.9, angular_damping=0.9)])
    low = np.inf
    for _ in range(300):
        sim.step(W, 1)
        low = min(low, sim.x[1, 1])
    pen = (E + r) - sim.x[1, 1]
    print("rest: penetration %.2e (%.2f %% of the radius), lowest centre %.4f (contact at %.1f), speed %.2e" % (pen, 100 * abs(pen) / r, low, E + r, np.linalg.norm(sim.v[1])))
    assert abs(pen) < 0.02 * r and low > (E + r) - 0.1 * r
    assert sum(a > 0 for a in sim.active) > 100 and set(sim.regions) == {(1, False)}


def _slide(mu):
    """a capsule lying along the fall line of a following box's top face, the box tilted by 0.5 rad (under 45 degrees): its drift down the
    face over 30 substeps, its drift off the face, the substeps in contact and its final spin"""
    tilt = cs._quat([0, 0, 1], -0.5)
    down, normal = pr.qrot(tilt, np.array([1.0, 0.0, 0.0])), pr.qrot(tilt, np.array([0.0, 1.0, 0.0]))
    along = cs._quat([0, 0, 1], -(np.pi / 2 + 0.5))                   # the capsule's Y axis along `down`
    sim, W, _ = one_bone([dict(bone=0, type=0, shape=1, size=[12.0, 0.5, 2.0], mass=0.0, offset_rot=tilt, friction=1.0),
                          dict(bone=-1, type=1, shape=2, size=[0.3, 1.0, 0], mass=1.0, offset_pos=list(normal * 0.8), offset_rot=along, friction=mu)])
    sim.step(W, 0)
    x0 = sim.x[1].copy()
    sim.step(W, 30)
    return float(np.dot(sim.x[1] - x0, down)), float(np.dot(sim.x[1] - x0, normal)), sum(a > 0 for a in sim.active), float(np.linalg.norm(sim.w[1]))


def test_friction_holds_a_capsule_that_slides_without_it():
    """mu = 0 (the capsule's friction; the product is 0): the capsule slides down the tilted face by g sin(0.5) t^2 / 2 within 5 %.
    mu = 1 with tan(0.5) = 0.55 < 1: a capsule lying along the fall line cannot roll, so the contact sticks and it stays where it is —
    its drift is asserted below 5 % of the frictionless one (what is left is the slip friction removes one iteration late)."""
    free, off0, n0, w0 = _slide(0.0)
    held, off1, n1, w1 = _slide(1.0)
    t = 30 * pr.DEFAULT_H
    print("drift down the face over 30 substeps: %.4f without friction (g sin(0.5) t^2 / 2 = %.4f), %.4f with mu = 1 (ratio %.3f); spin %.2e / %.2e; off the face %.3f / %.3f; %d / %d substeps in contact"
          % (free, 0.5 * 98 * np.sin(0.5) * t * t, held, held / free, w0, w1, off0, off1, n0, n1))
    assert abs(free / (0.5 * 98 * np.sin(0.5) * t * t) - 1) < 0.05
    assert abs(held) < 0.05 * free and n0 >= 28 and n1 >= 28 and abs(off0) < 0.05 and abs(off1) < 0.05


def test_a_capsule_lying_flat_on_a_face_stays_finite():
    """the flat-derivative case (f(s) about 0 along the whole segment: the box's counterpart of the parallel capsules): CPU only, finite
    and not passed through, in both precisions"""
    for dt in (np.float64, np.float32):
        sim, W, _ = one_bone([dict(bone=0, type=0, shape=1, size=[3, 0.5, 3], mass=0.0),
                              dict(bone=-1, type=1, shape=2, size=[0.5, 2, 0], mass=1.0, offset_pos=[0.2, 0.98, 0], offset_rot=cs._quat([0, 0, 1], np.pi / 2),
                                   linear_damping=0.9, angular_damping=0.9)], dtype=dt)
        sim.step(W, 60)
        assert np.isfinite(sim.state13()).all() and sim.x[1, 1] > 0.9 and sum(a > 0 for a in sim.active) > 10


def test_a_centre_inside_the_box_leaves_through_the_nearest_face():
    """the deep case: a sphere whose centre starts inside a following box, nearest its -z face, is put outside that face in one solve
    (pen = r + the depth of the centre), whichever index order; a centre exactly in the middle of a cube takes +x (the first axis wins
    the tie, sign(0) = +)"""
    box = dict(bone=0, type=0, shape=1, size=[1.0, 0.8, 0.6], mass=0.0)
    ball = dict(bone=-1, type=1, shape=0, size=[0.25, 0, 0], mass=1.0)
    for bodies, k in (([box, dict(ball, offset_pos=[0.1, 0.2, -0.4])], 1), ([dict(ball, offset_pos=[0.1, 0.2, -0.4]), box], 0)):
        sim, W, _ = one_bone(bodies, gravity=(0, 0, 0), iterations=1)
        sim.step(W, 1)
        assert sim.regions == {(0, False): 1} and np.allclose(sim.x[k], [0.1, 0.2, -0.85], atol=1e-12), sim.x[k]
    sim, W, _ = one_bone([dict(box, size=[0.5, 0.5, 0.5]), dict(ball)], gravity=(0, 0, 0), iterations=1)
    sim.step(W, 1)
    assert np.allclose(sim.x[1], [0.75, 0, 0], atol=1e-12), sim.x[1]


def _lists(bodies, mode=2):
    return cr.contact_lists(pr.make_table(bodies, []), mode)


def test_what_is_a_candidate_with_boxes():
    """boxes against round shapes in either order and role; two boxes are counted, not paired; a zero extent or a zero mask keeps a box out;
    mode 1 leaves every box out"""
    dyn = dict(type=1, mass=1.0, shape=0, size=[0.3, 0, 0])
    fol = dict(type=0, mass=0.0, shape=0, size=[0.3, 0, 0])
    bx = dict(shape=1, size=[0.3, 0.2, 0.1])
    L = _lists([dict(fol, **bx), dict(dyn), dict(dyn, **bx), dict(fol, shape=2, size=[0.2, 0.5, 0])])
    assert (L["n_follow"], L["n_pairs"], L["box_pairs"], L["boxes"]) == (3, 1, 1, 0)
    assert L["follow_off"].tolist() == [0, 0, 2, 3, 3] and L["follow_idx"].tolist() == [0, 3, 3] and L["pairs"].tolist() == [[1, 2]]
    assert L["box"].tolist() == [True, False, True, False] and L["radius"].tolist() == [0, np.float32(0.3), 0, np.float32(0.2)]
    assert np.array_equal(L["ext"][0], np.float32([0.3, 0.2, 0.1])) and not L["ext"][1].any()
    # two following boxes are no pair at all; two boxes whose masks miss each other are not counted
    assert _lists([dict(fol, **bx), dict(fol, **bx)])["box_pairs"] == 0
    assert _lists([dict(dyn, group=1, mask=1, **bx), dict(dyn, group=2, mask=0xffff, **bx)])["box_pairs"] == 0
    # a zero extent: the box takes no part and is counted; a zero mask: neither
    L = _lists([dict(dyn), dict(fol, shape=1, size=[0.3, 0.0, 0.1]), dict(fol, mask=0, **bx), dict(dyn, **bx)])
    assert (L["boxes"], L["n_follow"], L["n_pairs"], L["box_pairs"]) == (1, 0, 1, 0) and L["takes"].tolist() == [True, False, False, True]
    # mode 1: the boxes are counted and leave no trace in the lists (those of the same table with the boxes' masks 0, but for the count)
    t = pr.make_table([dict(fol, **bx), dict(dyn), dict(dyn, **bx)], [])
    off, old = cr.contact_lists(t, 1), cr.contact_lists(bs.masked_boxes(dict(table=t))["table"], 1)
    assert off["box_pairs"] == 0 and off["boxes"] == 2 and old["boxes"] == 0 and not off["box"].any() and not off["ext"].any()
    assert all(np.array_equal(off[k], old[k]) for k in old if k != "boxes")


def test_without_boxes_the_definition_is_contact_ref():
    """a table without a box: the run under mode 2 is that under mode 1, bit for bit (pairs without a box go through the segment front end)"""
    sc = bs.no_boxes()
    poses = [bs.pose(sc, k) for k in range(3)]
    a = bs.run_reference(sc, poses, bs.SHORT, sim=bs.sim_of(sc))
    b = bs.run_reference(sc, poses, bs.SHORT, sim=bs.sim_of(sc, mode=1))
    for (wa, sa), (wb, sb) in zip(a, b):
        assert np.array_equal(wa, wb) and np.array_equal(sa, sb)


def _scan(P, d, e, n=2001):
    """the smallest distance between the segment and the box over n evenly spaced parameters"""
    s = np.linspace(0.0, 1.0, n)
    c = P[:, None, :] + d[:, None, :] * s[None, :, None]
    g = c - np.clip(c, -e[:, None, :], e[:, None, :])
    return np.sqrt((g * g).sum(axis=2)).min(axis=1)


def test_closest_point_against_a_dense_scan():
    """4000 seeded segment / box pairs (a quarter through the box, a quarter with one end inside, an eighth parallel to an axis, spheres):
    the distance to the box is 1-Lipschitz in the point, so the routine's distance is never above the 2001-point scan's best by more
    than the bisection's own resolution (s within 2^-25 of the minimiser: |d| 2^-25) and never below it by more than the scan can miss
    (a sample lies within |d| / 4000 of every point). The float32 routine's box point agrees with the float64 one to a median below
    1e-6 of the scale where the segment stays 0.05 and more outside the box. A sphere (d = 0) gives s = 0."""
    rng = np.random.default_rng(7)
    n = 4000
    e = rng.uniform(0.2, 1.5, size=(n, 3))
    P = rng.uniform(-2.5, 2.5, size=(n, 3))
    d = rng.uniform(-3, 3, size=(n, 3))
    P[: n // 4] = rng.uniform(-1, 1, size=(n // 4, 3)) * e[: n // 4]            # starts inside
    k = np.arange(n // 4, n // 4 + n // 8)
    d[k, rng.integers(0, 3, size=len(k))] = 0.0                                    # parallel to a face
    d[-n // 8:] = 0.0                                                              # spheres
    s, c, b = br.closest_on_segment(P, d, e)
    dist = np.linalg.norm(c - b, axis=1)
    best = _scan(P, d, e)
    res = np.linalg.norm(d, axis=1) / 4000
    print("closest point vs a 2001-point scan: routine - scan in [%.2e, %.2e], %d of %d decided by bisection, %d inside the box" % ((dist - best).min(), (dist - best).max(), int(((s > 0) & (s < 1)).sum()), n, int((dist == 0).sum())))
    assert (dist <= best + np.linalg.norm(d, axis=1) * 2.0 ** -25 + 1e-12).all() and (dist >= best - res - 1e-12).all()
    assert ((s > 0) & (s < 1)).sum() > n // 5 and (dist == 0).sum() > n // 8 and (s[-n // 8:] == 0).all()
    s32, c32, b32 = br.closest_on_segment(P.astype(np.float32), d.astype(np.float32), e.astype(np.float32), dt=np.float32)
    assert s32.dtype == np.float32 and c32.dtype == np.float32
    # where the minimiser is unique and well conditioned (outside the box by 0.05 and more) the float32 points agree with float64
    far = dist > 0.05
    scale = np.maximum(1.0, np.abs(P).max(axis=1) + np.abs(d).max(axis=1))
    err = np.abs(b32.astype(np.float64) - b).max(axis=1) / scale
    print("float32 box point vs float64: %.2e of the scale at the worst of %d pairs outside the box" % (err[far].max(), int(far.sum())))
    assert np.median(err[far]) < 1e-6


def test_cases_are_well_conditioned_and_touch():
    """every GPU case, none left out: the float32 probe of the definition stays within 2.5e-5 x extent of its float64 run over the whole
    horizon, and at least one contact is active in at least a quarter of the substeps; the probe's quaternions stay within 2.5e-5 as well
    (the GPU bar on quaternions and normals, 1e-4, does not scale with the extent: the same 4 x margin); the cases take the launch forms
    and meet the regions of the box they are there for"""
    rows, bad = [], {}
    for name in bs._CASES:
        c, act, turn = bs.conditioning(name)
        rows.append("%s %.1e / %.2f / %.1e" % (name, c, act, turn))
        if c > ILL or act < 0.25 or turn > ILL:
            bad[name] = (c, act, turn)
        sc, _, calls = bs.case(name)
        assert len(calls) <= 3 and sc["table"]["n_bodies"] <= 300, name
    print("float32 probe / extent, active fraction, quaternion probe: " + ", ".join(rows))
    assert not bad, "ill-conditioned or idle: %s" % bad
    for name, (block, own) in bs.FORMS.items():
        t = bs.case(name)[0]["table"]
        widest = max(np.bincount(pr.colouring(t)[0])) if t["n_joints"] else 0
        assert (64 if t["n_bodies"] <= 64 and widest <= 64 else 256) == block and int(t["n_joints"] <= block) == own, name
        L = bs.reference(name)[1].lists
        shape, dyn = t["shape"], pr.is_dynamic(t)
        assert shape[1] == 1 and not dyn[1] and (shape[dyn] == 1).sum() >= dyn.sum() // 2 - 1 and L["n_pairs"] == 0 and L["box_pairs"] > 0, name
    for name, (clamped, inside) in bs.REGIONS.items():
        reg = bs.reference(name)[1].regions
        hits = sum(n for (k, i), n in reg.items() if k == clamped and (i or not inside))
        assert hits >= (1 if name == "deep" else 10), (name, reg)
    # every pair case involves a box in every active contact, in the role its name gives
    for name in bs._CASES:
        if name.split()[-1] in ("fd", "df", "dd"):
            sc, sim = bs.case(name)[0], bs.reference(name)[1]
            t, L = sc["table"], sim.lists
            first, second, order = name.split()
            ids = {"sphere": 0, "box": 1, "capsule": 2}
            pair = [b for b in range(1, t["n_bodies"]) if not (order == "dd" and b == 1)]
            assert [int(t["shape"][b]) for b in pair] == [ids[first], ids[second]], name
            dyn = pr.is_dynamic(t)
            assert [bool(dyn[b]) for b in pair] == {"fd": [False, True], "df": [True, False], "dd": [True, True]}[order], name
            assert sum(sim.regions.values()) >= 10 and (L["n_pairs"] == 1) == (order == "dd"), name
    # the Node end-to-end case: the PMX's table under one pose, the engine's substeps
    c, act, sim = bs.node_conditioning()
    print("node case: %.1e / %.2f" % (c, act))
    assert c <= ILL and act >= 0.25 and sum(sim.regions.values()) > 0


# ---- the host half: contact_table.h in its boxes mode against the definition's lists ----

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return cs.build_table_tool(tmp_path_factory.mktemp("contact_box_table"))


run_tool, limit_table = cs.run_table_tool, bs.limit_table


def mixed_table():
    dyn = dict(type=1, mass=1.0, shape=0, size=[0.3, 0, 0])
    fol = dict(type=0, mass=0.0, shape=0, size=[0.3, 0, 0])
    bx = dict(shape=1, size=[0.3, 0.2, 0.1])
    return pr.make_table([dict(dyn, group=1), dict(dyn, group=1, **bx), dict(fol, shape=1, size=[1, 1, 1]), dict(fol, shape=1, size=[1, 1, 1], mask=0), dict(fol, shape=1, size=[1, 0, 1]),
                          dict(dyn, shape=2, size=[0.2, 0.5, 0]), dict(fol, group=3, mask=0xffff & ~2), dict(dyn, size=[0, 0, 0]), dict(fol, group=20), dict(fol, group=4),
                          dict(dyn, group=5, **bx), dict(dyn, shape=1, size=[0.3, 0.2, 0.0])], [])


@pytest.mark.parametrize("name", ["own 64", "stride 256", "capsule box dd", "box pair", "mixed"])
def test_host_lists_equal_the_definition(tool, name):
    """shape records with the box bit, c_box, the follow CSR, the dynamic pairs in solve order, colour offsets and all counts, entry for
    entry, with boxes taking part; and without, under mode 1"""
    t = mixed_table() if name == "mixed" else bs.case(name)[0]["table"]
    L = cr.contact_lists(t, 2)
    rows, _ = run_tool(tool, t, 2)
    cs.assert_host_lists(rows, L)
    assert L["box"].any()
    # boxes off
    rows, _ = run_tool(tool, t, 1)
    cs.assert_host_lists(rows, cr.contact_lists(t, 1))


def test_host_refuses_one_past_the_limit_with_boxes(tool):
    """256 dynamic spheres x 256 following boxes = 65 536 candidates are taken, 256 x 257 are refused with both counts in the message"""
    rows, _ = run_tool(tool, limit_table(256), 2)
    assert rows["counts"][:2] == ["65536", "0"] and rows["refused"][0] == "0" and len(rows["follow_idx"]) == 65536
    rows, out = run_tool(tool, limit_table(257), 2)
    assert rows["counts"][:2] == ["65792", "0"] and rows["refused"][0] == "1" and rows.get("follow_idx", []) == []
    assert "65792 follow entries and 0 dynamic pairs" in out and "broad phase" in out
    assert cr.refusal(cr.contact_lists(limit_table(257), 2)) and not cr.refusal(cr.contact_lists(limit_table(256), 2))
    assert cr.contact_lists(limit_table(257), 1)["n_follow"] == 0


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_engine_boxes_option_with_a_recording_addon(tmp_path):
    """Engine { physicsContacts: 'boxes' } against a stand-in for the addon: physicsContacts(ctx, 2) follows uploadPhysics on every shard at
    loadModel; true passes 1; any other string turns nothing on; 'boxes' without devicePhysics throws"""
    sc, data, _ = bs.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "contacts_engine_mock.js"), str(tmp_path / "s.pmx"), "boxes", "true", "everything"], timeout=60).decode().strip().splitlines()[-1])
    assert r["needsDevicePhysics"] and r["shards"] >= 2 and len(r["boxes"]) == r["shards"]
    for tag, want in (("boxes", "physicsContacts:2"), ("true", "physicsContacts:1")):
        for calls in r[tag]:
            assert [c for c in calls if c.startswith("physicsContacts")] == [want] and calls.index(want) == calls.index("uploadPhysics") + 1
    assert all("physicsContacts" not in " ".join(calls) for calls in r["everything"]) and all("uploadPhysics" in calls for calls in r["everything"])
