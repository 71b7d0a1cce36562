"""PMX type-2 bodies ("physics + bone position alignment") on the CPU: the definition tests/align_ref.py itself, the host half of
rz_physics_aligned (reze-engine_amd/csrc/physics_table.h through tests/align_table_main.cpp) against it, the refusals, the conditioning of
every scene and every sequence of calls tests/test_gpu_align.py runs, and the bindings."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import align_ref
import align_scenes as als
import physics_ref as pr
import physics_scenes as ps
import spring_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4                          # physics_gpu.BAR, the GPU tests' bar (x extent)
PROBE = BAR / 10                    # what the float32 run of the definition may leave its float64 run by: the margin the physics probes use


# ---- the definition itself ----

def swing_scene():
    """one strand of one body under a following base ("one joint" of physics_scenes), the joint a ball joint (rotation free, no spring),
    the body type 2, light damping so that it swings"""
    sc = ps.strands(1, 1, base=True, seed=6, n_verts=64)
    sc = als.with_first_links(sc)
    t = dict(sc["table"])
    for k, v in (("rotation_min", ps.FREE_MIN), ("rotation_max", ps.FREE_MAX), ("spring_rotation", (0, 0, 0))):
        t[k] = np.array([v], dtype=np.float32)
    t["linear_damping"], t["angular_damping"] = np.full_like(t["linear_damping"], 0.3), np.full_like(t["angular_damping"], 0.3)
    return dict(sc, table=t)


def moving_poses(sc, n):
    """the root translates further with every call and the base tips: (q, t) per call"""
    out = []
    for k in range(n):
        q = np.zeros((sc["B"], 4), dtype=np.float32); q[:, 3] = 1
        t = np.zeros((sc["B"], 3), dtype=np.float32)
        t[0] = [0.3 * k, 0.05 * k, -0.2 * k]
        a = 0.15 * np.sin(0.9 * k)
        q[2] = [np.sin(a / 2), 0, 0, np.cos(a / 2)]
        out.append((q, t))
    return out


def test_an_aligned_body_swings_and_its_bone_stays_on_the_animation():
    """a type-2 body hung by a ball joint from a following parent, under a root that translates: with the feature the body swings — its
    bone's rotation leaves the animated one — while the bone's origin is exactly the animated bone's after every call, and the body is on
    its bone at the start of every call; without it the bone is not overridden at all: it stays rigid"""
    sc = swing_scene()
    t = sc["table"]
    (body,) = np.nonzero(align_ref.aligned_bodies(t))[0]
    bone = int(t["bone"][body])
    calls = (1, 3, 2, 3, 3, 2)
    poses = moving_poses(sc, len(calls))
    on, sim = als.run(sc, poses, calls)
    off, sim_off = als.run(sc, poses, calls, aligned=False)
    assert sim.c["dyn"][body] and not sim_off.c["dyn"][body]
    turned = 0.0
    for (w, s, S), (w0, s0, S0) in zip(on, off):
        assert np.array_equal(w[bone, 12:15], S[bone, 12:15]), "the aligned bone left the animated position"
        assert np.array_equal(w0, S0), "without the feature nothing is overridden in this scene"
        turned = max(turned, float(np.abs(w[bone, :12] - S[bone, :12]).max()))
    print("the aligned bone's rotation leaves the animated one by up to %.3f" % turned)
    assert turned > 0.05
    # rule 1 at the start of a call: x = p_bone + R t_off with the state's q, before any substep
    sim = als.sim_of(sc)
    for (q, tr), n in zip(poses, calls):
        S = als.solved(sc, q, tr)
        before = sim.q[body].copy(), sim.v[body].copy(), sim.w[body].copy()
        first = sim.pending_reset
        sim.step(S, 0)
        R = pr.qmat(pr.qmul(sim.q[body], pr.qconj(sim.c["off_q"][body])))
        assert np.abs(sim.x[body] - (S[bone, 12:15] + R @ sim.c["off_p"][body])).max() <= 1e-12
        if not first:
            assert all(np.array_equal(a, b) for a, b in zip(before, (sim.q[body], sim.v[body], sim.w[body]))), "the re-pin keeps q, v and w"
        for _ in range(n):
            sim.substep()


def test_the_rest_of_type_2():
    """in the "own 64" scene: the type-2 base of mass 0 keeps following its bone; the type-2 first link of the strand without bones is a
    plain dynamic body — not aligned, and the run is the run of the same table with that body typed 1; the free type-2 body, held by no
    joint, falls during a call and is back on its bone at the next"""
    sc, poses, calls = als.case(als.CROWD)
    t = sc["table"]
    al = align_ref.aligned_bodies(t)
    two = np.nonzero(t["type"] == 2)[0]
    assert list(two) == [0, 1, 7, 13, 19, 24] and list(np.nonzero(al)[0]) == [1, 7, 13, 24]
    assert t["mass"][0] == 0 and t["bone"][19] == -1
    ref, sim = als.run(sc, poses, calls)
    assert not sim.c["dyn"][0] and sim.c["dyn"][19] and 19 not in sim.c["dyn_bodies"]
    for (w, s, S), (q, tr) in zip(ref, poses):
        place = align_ref.Sim(t, sc["parents"], sc["bind"])
        place.reset(S)
        assert np.array_equal(s[0, :7], place.state13()[0, :7]) and not s[0, 7:].any(), "the type-2 body of mass 0 left its bone"
    typed = als.retyped(sc, {19: 1})
    same_run, _ = als.run(typed, poses, calls)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(ref, same_run))
    assert float(np.abs(ref[-1][1][19, :3] - als.reference(als.CROWD, aligned=False)[-1][1][19, :3]).max()) > 0.01
    # the free body: after a call of 3 substeps it has fallen; a call without substeps puts it back
    free, bone = 24, int(t["bone"][24])
    sim = als.sim_of(sc)
    S = als.solved(sc, *poses[0])
    sim.step(S, 0)
    home = sim.x[free].copy()
    sim.step(S, 3)
    assert home[1] - sim.x[free][1] > 0.05
    ovr = sim.step(S, 0)
    assert np.abs(sim.x[free] - home).max() < 1e-3 and np.array_equal(ovr[bone][12:15], S[bone, 12:15])


def test_off_and_tables_without_type_2_step_as_ever():
    """aligned=False, and a table without a type-2 body with it on, give spring_ref.Sim's run on the table as it is, value for value;
    there physics_step(n) is n x physics_step(1). With aligned bodies it is not: the re-pin is per call"""
    sc, poses, calls = als.case(als.CROWD)
    plain = spring_ref.Sim(sc["table"], sc["parents"], sc["bind"], mode=0, springs=False)
    want = ps.run_reference(sc, poses, calls, sim=plain)
    got = als.run(sc, poses, calls, aligned=False)[0]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(want, got))
    psc, pposes = als.plain_scene()
    assert not (psc["table"]["type"] == 2).any()
    want = ps.run_reference(psc, pposes, als.SPLIT_CALLS, sim=spring_ref.Sim(psc["table"], psc["parents"], psc["bind"], mode=0, springs=False))
    got = als.run(psc, pposes, als.SPLIT_CALLS)[0]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(want, got))
    whole = als.run(psc, pposes, als.SPLIT_CALLS)[0][-1][1]
    parts = als.run(psc, *als.split(pposes, als.SPLIT_CALLS))[0][-1][1]
    assert np.array_equal(whole, parts)
    whole = als.run(sc, poses, als.SPLIT_CALLS)[0][-1][1]
    parts = als.run(sc, *als.split(poses, als.SPLIT_CALLS))[0][-1][1]
    diff = float(np.abs(whole[:, :3] - parts[:, :3]).max()) / sc["extent"]
    print("aligned table: whole calls and calls of one substep end %.3e x extent apart" % diff)
    assert diff >= 10 * BAR


# ---- conditioning: every scene and every sequence of calls the GPU tests run ----

def probe(sc, poses, calls, **kw):
    a = als.run(sc, poses, calls, **kw)[0]
    b = als.run(sc, poses, calls, dtype=np.float32, **kw)[0]
    return als.deviation(a, b) / sc["extent"]


@pytest.mark.parametrize("name", als.ORDER)
def test_cases_are_well_conditioned_and_the_feature_shows(name):
    """the float32 run of the definition stays within a tenth of the GPU bar of its float64 run over exactly the case's calls, and the
    feature moves the case by at least ten times the bar (the GPU run cannot pass with the feature missing)"""
    c = als.conditioning(name)
    effect = als.deviation(als.reference(name), als.reference(name, aligned=False)) / als.case(name)[0]["extent"]
    print("%s: float32 probe %.2e x extent, the feature moves the case by %.2e x extent" % (name, c, effect))
    assert c <= PROBE
    assert effect >= 10 * BAR
    mode = als.CASES[name][1]
    if mode:            # the contact cases touch: substeps with an active contact, an aligned body among the pairs' bodies
        sc, poses, calls = als.case(name)
        sim = als.run(sc, poses, calls, mode=mode)[1]
        print("%s: %d of %d substeps with an active contact" % (name, sum(1 for a in sim.active if a), len(sim.active)))
        assert sum(1 for a in sim.active if a) >= len(sim.active) // 2


def test_the_other_sequences_are_well_conditioned():
    """the crowd's three instances, the call without substeps, the reset between calls, whole and split calls, the table without type 2,
    the two-on-one-bone table with the feature off, and the Node engine's frames"""
    sc, poses, calls = als.case(als.CROWD)
    worst = {}
    for i in range(3):
        worst["crowd instance %d" % i] = probe(sc, als.crowd_poses(sc, i), calls)
    worst["zero substeps"] = probe(sc, poses, als.ZERO_CALLS)
    worst["reset"] = probe(sc, poses, als.RESET_CALLS)
    worst["whole calls"] = probe(sc, poses, als.SPLIT_CALLS)
    worst["split calls"] = probe(sc, *als.split(poses, als.SPLIT_CALLS))
    worst["off"] = probe(sc, poses, calls, aligned=False)
    psc, pposes = als.plain_scene()
    worst["no type 2"] = probe(psc, pposes, als.SPLIT_CALLS)
    worst["no type 2, split"] = probe(psc, *als.split(pposes, als.SPLIT_CALLS))
    two = als.two_on_one_bone(sc)[0]
    worst["two on one bone, off"] = probe(two, poses, calls, aligned=False)
    nsc, _, q = als.node_case()
    ncalls = ps.node_substeps()
    nposes = [(q, np.zeros((nsc["B"], 3), dtype=np.float32))] * len(ncalls)
    worst["node"] = probe(nsc, nposes, ncalls)
    worst["node, off"] = probe(nsc, nposes, ncalls, aligned=False)
    moved = float(np.abs(als.run(nsc, nposes, ncalls)[0][-1][1][:, :3] - als.run(nsc, nposes, ncalls, aligned=False)[0][-1][1][:, :3]).max()) / nsc["extent"]
    print("node case: the option moves the last frame's bodies by %.3e x extent" % moved)
    for k, v in worst.items():
        print("%s: float32 probe %.2e x extent" % (k, v))
    assert max(worst.values()) <= PROBE
    assert moved >= 10 * BAR


# ---- the host half against the definition ----

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_table") / "align_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "align_table_main.cpp")])
    return exe


def derive(tool, sc, on, B=None):
    t = sc["table"]
    out = subprocess.run([tool, "1" if on else "0"], input=ps.dump_table(t, sc["parents"], sc["bind"]), capture_output=True, text=True, check=True).stdout
    return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1].split() if " " in ln else [] for ln in out.strip().split("\n")}, out


def assert_derived(rows, sc, on):
    """the program's lines against the definition: the table as read, its colouring, the overridden bones and their slots, the flags, the
    body and joint records"""
    t = sc["table"]
    read = align_ref.read_table(t, on)
    al = align_ref.aligned_bodies(t, on)
    assert rows["refused"][0] == "0"
    colour, order, ncol = pr.colouring(read)
    c = pr.prepare(read, sc["parents"], sc["bind"])
    counts = [int(x) for x in rows["counts"]]
    assert counts[:4] == [t["n_bodies"], t["n_joints"], ncol, len(c["dyn_bodies"])] and counts[5] == int(al.sum())
    assert counts[4] == (int(np.diff(c["colour_off"]).max()) if t["n_joints"] else 0)
    assert [int(x) for x in rows["colour"]] == list(colour) and [int(x) for x in rows["order"]] == list(order)
    assert [int(x) for x in rows["colour_off"]] == list(c["colour_off"][:ncol + 1])
    assert [int(x) for x in rows["types"]] == list(read["type"]) and [int(x) for x in rows["kept_types"]] == list(t["type"])
    assert [int(x) for x in rows["dyn_bone"]] == [int(t["bone"][b]) for b in c["dyn_bodies"]]
    slot = np.full(t["n_bodies"], -1)
    slot[c["dyn_bodies"]] = np.arange(len(c["dyn_bodies"]))
    assert [int(x) for x in rows["slot"]] == list(slot)
    assert [float(x) for x in rows["flag"]] == [1.0 if a else 0.0 for a in al]
    body = np.array([float(x) for x in rows["body"]]).reshape(-1, 13)
    want = np.concatenate([c["off_p"], c["inv_mass"][:, None], c["off_q"], c["inv_inertia"], c["lin_keep"][:, None], c["ang_keep"][:, None]], axis=1)
    assert np.array_equal(body.astype(np.float32), want.astype(np.float32))
    if t["n_joints"]:
        ends = np.array([int(x) for x in rows["ends"]]).reshape(-1, 2)
        assert np.array_equal(ends[:, 0], c["ja"]) and np.array_equal(ends[:, 1], c["jb"])
        joint = np.array([float(x) for x in rows["joint"]]).reshape(-1, 29)
        a = c["alpha"]
        want = np.concatenate([c["r_a"], c["r_b"], c["j_a"], c["j_b"], c["pmin"], a[:, :1], c["pmax"], a[:, 1:2], c["rmin"], a[:, 2:3], c["rmax"]], axis=1)
        assert np.abs(joint - want).max() <= 4e-7 * max(1.0, np.abs(want[:, :6]).max())       # (tests/test_physics_cpu.py: float32 rounding of doubles on both sides)
    block = 64 if t["n_bodies"] <= 64 and counts[4] <= 64 else 256
    assert [int(x) for x in rows["form"]] == [block, int(t["n_joints"] <= block)]


@pytest.mark.parametrize("name", als.ORDER)
def test_host_tables_equal_the_definition(tool, name):
    """with the feature on: colours, order, nd / dyn_bone, the slots, the flag in the record's 16th float and every constant are those of
    the definition's table as read, and differ from the plain build; the launch form is the case's; with it off: the plain build byte for
    byte"""
    sc = als.case(name)[0]
    rows, _ = derive(tool, sc, True)
    assert_derived(rows, sc, True)
    assert rows["plain_equal"] == ["0"]
    assert tuple(int(x) for x in rows["form"]) == als.CASES[name][3]
    rows, _ = derive(tool, sc, False)
    assert_derived(rows, sc, False)
    assert rows["plain_equal"] == ["1"] and rows["form"] == rows["plain_form"] and int(rows["counts"][5]) == 0


def test_a_table_without_aligned_bodies_is_the_plain_build(tool):
    """on = 1 and a count of 0 — no type 2 at all; type 2 with mass 0 only — derive the plain build byte for byte; a type-2 body with a
    mass and no bone changes the build (it is dynamic) and is not flagged"""
    psc, _ = als.plain_scene()
    rows, _ = derive(tool, psc, True)
    assert rows["plain_equal"] == ["1"] and int(rows["counts"][5]) == 0
    massless = als.retyped(psc, {0: 2, 5: 2}, {0: 0.0, 5: 0.0})
    rows, _ = derive(tool, massless, True)
    assert_derived(rows, massless, True)
    assert rows["plain_equal"] == ["1"] and int(rows["counts"][5]) == 0
    sc = ps.strands(3, 2, base=True, seed=9, n_verts=64, boned=2)
    t = sc["table"]
    loose = [b for b in als.first_links(t) if t["bone"][b] < 0]
    assert len(loose) == 1
    types = {int(b): 0 for b in np.nonzero(t["type"] == 2)[0]}
    types[loose[0]] = 2
    sc = als.retyped(sc, types)
    rows, _ = derive(tool, sc, True)
    assert_derived(rows, sc, True)
    assert rows["plain_equal"] == ["0"] and int(rows["counts"][5]) == 0 and not any(float(x) for x in rows["flag"])


# ---- refusals ----

def test_two_dynamic_bodies_on_one_bone_are_refused(tool):
    """a table with a type-1 and a type-2 body on one bone is valid as uploaded and refused with the feature on, both bodies named"""
    sc, first, extra = als.two_on_one_bone(als.case(als.CROWD)[0])
    rows, out = derive(tool, sc, False)
    assert rows["refused"][0] == "0" and rows["plain_equal"] == ["1"]
    rows, out = derive(tool, sc, True)
    assert rows["refused"][0] == "-1" and list(rows) == ["refused"], out
    assert "rz_physics_aligned" in out and "dynamic bodies %d and %d both drive bone %d" % (first, extra, int(sc["table"]["bone"][first])) in out
    assert pr.validate(align_ref.read_table(sc["table"]), sc["B"]) == "two dynamic bodies on one bone" and pr.validate(sc["table"], sc["B"]) is None


def test_block_size_change_and_the_lds_limit(tool):
    """The feature can change the block size both ways: type-2 bodies that become dynamic split a colour that was wider than a wave (256
    lanes -> 64: the joints then outnumber the lanes and their multipliers move into LDS), and greedy colouring under more constraints can
    widen a later colour. derive runs the upload's own LDS check on the form the new colouring selects (RZ_ERR_UNSUPPORTED). With the
    present arithmetic — 96 B per body, + 12 B per joint once the joints outnumber the lanes, 160 KB — that refusal cannot be reached by
    a table the upload took: the block differs only with at most 64 bodies, and then the two forms differ by at most 12 B x 256 joints on
    top of 6 KB; with more joints than 256 both forms count them. The arithmetic is checked here over every count; the path is the
    upload's, which tests/test_physics_cpu.py and tests/test_gpu_physics.py hold to the limit."""
    # two type-2 bodies on two bones joined by 65 joints: off, both follow, one colour of 65 joints (256 lanes, joints in registers);
    # on, both are dynamic, every joint its own colour (64 lanes, striding, 12 B per joint of LDS)
    parents, bind = [-1, 0, 0], [[0, 0, 0], [0, 10, 0], [1, 10, 0]]
    bodies = [dict(bone=1, type=2, mass=1.0, shape=0, size=[0.3, 0, 0]), dict(bone=2, type=2, mass=1.0, shape=0, size=[0.3, 0, 0])]
    joints = [dict(body_a=0, body_b=1, position=[0.5, 10, 0], rotation=[0, 0, 0]) for _ in range(65)]
    sc = ps._scene(parents, bind, bodies, joints, np.random.default_rng(3), 16)
    off, _ = derive(tool, sc, False)
    on, _ = derive(tool, sc, True)
    assert (off["form"], off["lds"][0], off["counts"][2], off["counts"][4]) == (["256", "1"], "192", "1", "65")
    assert (on["form"], on["lds"][0], on["counts"][2], on["counts"][4]) == (["64", "0"], str(2 * 96 + 65 * 12), "65", "1")
    assert on["refused"][0] == "0" and on["plain_form"] == ["256", "1"] and int(on["counts"][5]) == 2
    assert_derived(on, sc, True)
    # the arithmetic: whenever one block's form fits, the other's does
    limit = ps.LDS_LIMIT
    lds = lambda nb, nj, block: nb * 96 + (nj * 12 if nj > block else 0)
    for nb in range(1, 65):
        for nj in (0, 64, 65, 256, 257, 4096, (limit - nb * 96) // 12, (limit - nb * 96) // 12 + 1):
            assert (lds(nb, nj, 64) <= limit) == (lds(nb, nj, 256) <= limit), (nb, nj)


# ---- the bindings ----

@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_engine_option_with_a_recording_addon(tmp_path):
    """Engine { physicsAligned } against a stand-in for the addon: on every shard uploadPhysics, physicsAligned(1), then physicsSprings and
    physicsContacts when those are asked for too; no call without the option; it throws without devicePhysics"""
    _, data, _ = als.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "align_engine_mock.js"), str(tmp_path / "s.pmx"), "aligned", "all", "off"],
                                           timeout=60).decode().strip().splitlines()[-1])
    assert r["needsDevicePhysics"] and r["needsDeviceFK"]
    assert r["shards"] >= 2 and len(r["aligned"]) == len(r["all"]) == r["shards"]
    for calls in r["aligned"]:
        at = calls.index("uploadPhysics")
        assert calls.count("physicsAligned:1") == 1 and calls[at + 1] == "physicsAligned:1"
        assert "physicsContacts" not in " ".join(calls) and "physicsSprings" not in " ".join(calls)
    for calls in r["all"]:
        at = calls.index("uploadPhysics")
        assert calls[at:at + 4] == ["uploadPhysics", "physicsAligned:1", "physicsSprings:1", "physicsContacts:1"] and calls.count("physicsAligned:1") == 1
    assert all("physicsAligned" not in " ".join(calls) for calls in r["off"]) and all("uploadPhysics" in calls for calls in r["off"])


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_pmx_round_trip_carries_the_type(tmp_path):
    """Model.physicsTables() on a PMX written with type-2 bodies passes the type through"""
    sc, data, _ = als.node_case()
    want = sc["table"]
    assert (want["type"] == 2).sum() == 4
    (tmp_path / "s.pmx").write_bytes(data)
    got = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "physics_tables.js"), str(tmp_path / "s.pmx")], timeout=60).decode().strip().splitlines()[-1])
    assert list(got["type"]) == [int(x) for x in want["type"]]


def test_python_binding_lists_the_symbol(rz):
    capi = rz.capi
    assert hasattr(capi.load(), "rz_physics_aligned")
    assert "rz_physics_aligned" in capi.SYMBOLS and "rz_physics_aligned" in capi.OPTIONAL_SYMBOLS
    assert hasattr(capi.DeformContext, "physics_aligned")
