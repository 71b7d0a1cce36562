"""tests/physics_ref.py, the definition the device physics is held to, is physics and not just self-consistent; the scenes the GPU tests
use are well-conditioned; and the GPU-free half of the upload (csrc/physics_table.h: validation, colouring, derived constants) is the same
function of a table as physics_ref's. No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import motion_ref
import physics_ref as pr
import physics_scenes as ps
from helpers import bone_morph_reference, sample_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILL = 2.5e-5
G = 98.0
FREE = dict(rotation_min=ps.FREE_MIN, rotation_max=ps.FREE_MAX)


def world_of(parents, bind, q=None):
    B = len(parents)
    q = np.tile([0.0, 0, 0, 1], (B, 1)) if q is None else q
    return ps.world_of(dict(parents=np.asarray(parents), bind=np.asarray(bind, dtype=np.float64)), q, np.zeros((B, 3)))


def test_free_fall_is_the_semi_implicit_euler_sum():
    t = pr.make_table([dict(bone=0, type=1, shape=0, size=[1, 0, 0], mass=1.0)], [])
    s = pr.Sim(t, [-1], [[0, 0, 0]])
    W = world_of([-1], [[0, 0, 0]])
    h = 1.0 / 75.0
    for n in (1, 7, 40):
        s.pending_reset = True
        s.step(W, n)
        want = -G * h * h * n * (n + 1) / 2
        print("free fall, %d substeps: y = %.17g, the sum %.17g" % (n, s.x[0][1], want))
        assert abs(s.x[0][1] - want) <= 4 * n * np.spacing(abs(want)) and s.x[0][0] == 0 and s.x[0][2] == 0


def pendulum(L, r, theta0, substeps):
    t = pr.make_table([dict(bone=0, type=0, mass=0), dict(bone=1, type=1, shape=0, size=[r, 0, 0], mass=1.0)],
                      [dict(body_a=0, body_b=1, position=[0, 0, 0], rotation=[0, 0, 0], **FREE)])
    parents, bind = [-1, 0], [[0, 0, 0], [0, -L, 0]]
    s = pr.Sim(t, parents, bind)
    W = world_of(parents, bind)
    s.reset(W)
    q = np.array([0, 0, math.sin(theta0 / 2), math.cos(theta0 / 2)])
    s.x[1], s.q[1] = pr.qrot(q, np.array([0, -L, 0.0])), q            # released at theta0 about z
    s.residuals = []
    ang = []
    for _ in range(substeps):
        s.step(W, 1)
        ang.append(math.atan2(s.x[1][0], -s.x[1][1]))
    return np.array(ang), np.array(s.residuals)


@pytest.mark.parametrize("L,r", [(2.0, 2.0), (2.0, 0.5)])
def test_pendulum_period_and_residual(L, r):
    """A sphere of radius r hanging L below a locked point joint with free rotation, released at 0.1 rad: the period over three swings
    (zero crossings interpolated) is the physical pendulum's within 1 %. Derivable at these parameters: the integrator's (w h)^2 / 24 =
    3.5e-4 and the amplitude's theta0^2 / 16 = 6.3e-4, under 0.2 % together; the rest is room for the projection's numerical damping.
    Measured: -0.08 % (L 2, r 2), -0.12 % (L 2, r 0.5: a body far smaller than its distance to the anchor)."""
    ang, res = pendulum(L, r, 0.1, 300)
    zc = [k - 1 + ang[k - 1] / (ang[k - 1] - ang[k]) for k in range(1, len(ang)) if ang[k - 1] > 0 >= ang[k]]
    T = (zc[3] - zc[0]) / 3 / 75.0
    want = 2 * math.pi * math.sqrt((L * L + 0.4 * r * r) / (G * L))
    print("pendulum L %.1f r %.1f: period %.6f s, physical pendulum %.6f s, off by %+.3f %%; residual per iteration in substep 2: %s"
          % (L, r, T, want, 100 * (T / want - 1), res[1]))
    assert abs(T / want - 1) <= 0.01
    grow = np.diff(res, axis=1)
    assert (grow <= 1e-12).all(), "the anchor residual grew from one iteration to the next: %s" % res[np.argmax(grow.max(axis=1))]


def welded_scene(off=(0.0, 0.0, 0.0)):
    parents, bind = [-1, 0, 1], [[0, 0, 0], [0, 16, 0], [1.0, -0.5, 0.3]]
    bodies = [dict(bone=1, type=0, mass=0, shape=1, size=[0.5, 0.5, 0.5], offset_pos=[0.1, 0.2, 0]),
              dict(bone=2, type=1, shape=1, size=[0.3, 0.5, 0.2], mass=1.5, linear_damping=0.9, angular_damping=0.9, offset_pos=list(off),
                   offset_rot=ps._quat([1, 1, 0], 0.4))]
    joints = [dict(body_a=0, body_b=1, position=[1.0, 15.5, 0.3], rotation=[0.2, -0.1, 0.3])]          # every limit 0 = 0: welded
    return parents, bind, pr.make_table(bodies, joints)


def test_welded_joint_follows_the_hierarchy():
    """All limits equal: the dynamic body's bone override is the hierarchy solve's matrix for that bone while the parent moves (the welded
    bone's own local rotation is identity). The bar is the float32 probe's deviation from the float64 run in the same scene. The joint sits
    at the body's centre, where the position and the rotation stage do not disturb each other and four passes converge to rounding; with
    the anchor 0.4 off the centre each stage undoes part of the other and the weld only converges linearly
    (test_welded_joint_off_the_centre_converges_with_the_iterations)."""
    parents, bind, t = welded_scene()
    worst, probe, _ = welded_run(parents, bind, t)
    print("welded joint: override off the hierarchy's matrix by %.3e; the float32 probe deviates by %.3e" % (worst, probe))
    assert worst <= probe


def test_welded_joint_off_the_centre_converges_with_the_iterations():
    """The weld with its anchor 0.4 off the body's centre, as PMX welds usually are, over the same moving parent. The position stage turns
    the body about its centre, the rotation stage turns it back about the centre and so moves the anchor again: the pair converges
    linearly, not in one pass. What holds, and is asserted:
      - at the default 4 iterations the override is off the hierarchy's matrix by no more than the step put in — the largest change of that
        matrix from one frame to the next plus one substep's fall g h^2 — because a pass never makes the residual larger;
      - more passes never make it worse (4, 8, 16, 32, 64), and at 64 it is back at the bar of the centred weld, the float32 probe's
        deviation.
    Measured: 1.6e-1, 4.0e-2, 1.9e-3, 4.0e-6, 1.6e-9 units against a step of 5.7e-1 + 1.7e-2; the probe deviates by 1.5e-6. A model whose welds
    must hold tighter at 4 iterations raises `iterations`; the header lists this under what the solver does not do."""
    errs = []
    for it in (4, 8, 16, 32, 64):
        parents, bind, t = welded_scene((0, -0.4, 0.1))
        t["iterations"] = it
        worst, probe, jump = welded_run(parents, bind, t)
        errs.append(worst)
    fall = G / 75.0 ** 2
    print("welded joint 0.4 off the centre: override off the hierarchy's matrix by %s at 4 .. 64 iterations; a step puts in %.3e + %.3e; the float32 probe deviates by %.3e"
          % (" ".join("%.2e" % e for e in errs), jump, fall, probe))
    assert errs[0] <= jump + fall
    assert all(b <= a for a, b in zip(errs, errs[1:]))
    assert errs[-1] <= probe


def welded_run(parents, bind, t):
    sims = {dt: pr.Sim(t, parents, bind, dtype=dt) for dt in (np.float64, np.float32)}
    rng = np.random.default_rng(3)
    worst, probe, jump, last = 0.0, 0.0, 0.0, None
    for k in range(12):
        a = rng.uniform(-0.1, 0.1, size=2)
        q = np.tile([0.0, 0, 0, 1], (3, 1))
        q[0] = ps._quat([0, 0, 1], a[0] * 0.2)
        q[1] = ps._quat(rng.normal(size=3), a[1])
        W = world_of(parents, bind, q)
        o64 = sims[np.float64].step(W, 1)[2]
        o32 = sims[np.float32].step(W.astype(np.float32), 1)[2].astype(np.float64)
        worst = max(worst, float(np.abs(o64 - W[2]).max()))
        probe = max(probe, float(np.abs(o32 - o64).max()))
        jump = max(jump, 0.0 if last is None else float(np.abs(W[2] - last).max()))
        last = W[2].copy()
    return worst, probe, jump


def test_nothing_moves_at_rest():
    for name in ("crowd", "63 bodies"):
        sc = ps.scene(name)
        t = dict(sc["table"])
        t["gravity"] = np.zeros(3, dtype=np.float32)
        s = pr.Sim(t, sc["parents"], sc["bind"])
        W = world_of(sc["parents"], sc["bind"])
        s.reset(W)
        x0, q0 = s.x.copy(), s.q.copy()
        s.step(W, 10)
        d = max(float(np.abs(s.x - x0).max()), float(np.abs(s.q - q0).max()), float(np.abs(s.v).max()), float(np.abs(s.w).max()))
        print("%s at the bind pose, g = 0, 10 substeps: largest change %.3e" % (name, d))
        assert d <= 1e-12


def limit_excess(iterations, a=0.3):
    """a pendulum swung hard against a limit of [-a, a] about x: the largest excess of the x angle after any substep"""
    t = pr.make_table([dict(bone=0, type=0, mass=0), dict(bone=1, type=1, shape=1, size=[0.3, 0.5, 0.3], mass=1.0, linear_damping=0.5, angular_damping=0.5)],
                      [dict(body_a=0, body_b=1, position=[0, 0, 0], rotation=[0, 0, 0], rotation_min=[-a, ps.FREE_MIN[1], ps.FREE_MIN[2]],
                            rotation_max=[a, ps.FREE_MAX[1], ps.FREE_MAX[2]])], gravity=[0, -98, 60], iterations=iterations)
    parents, bind = [-1, 0], [[0, 0, 0], [0, -1, 0]]
    s = pr.Sim(t, parents, bind)
    W = world_of(parents, bind)
    worst, reached, swing = 0.0, 0.0, 0.0
    for _ in range(60):
        s.step(W, 1)
        swing = max(swing, float(np.linalg.norm(s.w[1])) * s.c["h"])
        c = s.c
        e = pr.euler_xyz(pr.qmul(pr.qconj(pr.qmul(s.q[0], c["j_a"][0])), pr.qmul(s.q[1], c["j_b"][0])))
        worst, reached = max(worst, abs(e[0]) - a), max(reached, abs(e[0]))
    return worst, reached, swing


def test_rotation_limit_holds():
    """A limit of [-a, a] on one axis is not exceeded after a step by more than 1e-4 rad. Why 1e-4: the limit stage removes the whole
    violation v it meets, but its update q += 1/2 [d_phi, 0] q turns by 2 atan(v / 2) instead of v and leaves v^3 / 12 behind. The position
    stage in front of it (the anchor is off the body's centre) turns the body again in every pass, so the last pass still meets a violation
    of the order of the substep's swing |w| h, which stays under 0.1 rad here (asserted): 0.1^3 / 12 = 8e-5. The reference at 4 against 64
    iterations: 1.7e-5 against 1.2e-8 rad — at 64 the position stage has nothing left to do before the last limit pass."""
    e4, reached, swing = limit_excess(4)
    e64, _, _ = limit_excess(64)
    print("rotation limit 0.3 rad: excess %.3e at 4 iterations, %.3e at 64; the swing reached %.4f rad, at most %.3f rad per substep" % (e4, e64, reached, swing))
    assert reached >= 0.3 - 1e-9, "the limit was never reached"
    assert swing <= 0.1
    assert e4 <= 1e-4 and e64 <= 1e-4


PARAM_SCENES = ("params", "params h", "params iterations", "params gravity")
LOCAL_CROWD_SCENES = ("65 bodies 64 joints", "257 joints")          # tests/test_gpu_physics.py: test_256_lane_forms_in_a_crowd
NEW_CASES = PARAM_SCENES + tuple(ps.FORMS) + ("contents",) + tuple("%s, crowd instance %d" % (n, i) for n in LOCAL_CROWD_SCENES for i in range(3))


def test_every_parameter_moves_the_reference():
    """h, iterations and gravity, all three and one at a time, against the same table with the defaults (the "crowd" scene) over the same
    poses and calls: the float64 definition moves by more than 100 x the GPU tests' bar, so a kernel that ignored a parameter (or one
    component of gravity) cannot pass tests/test_gpu_physics.py: test_table_parameters. The variant that changes the iterations alone runs
    1 pass: 7 passes instead of the default 4 move these strands by 3.2e-3 x extent only (the solver has nearly converged by then), 1 pass
    by 2.1e-2. In "params" the 7 passes stand: a kernel with a fixed 4 would be 32 x the bar off the definition there."""
    base = ps.scene("crowd")
    poses = [ps.pose(base, k) for k in range(len(ps.CALLS))]
    ref = ps.run_reference(base, poses)
    for name in PARAM_SCENES:
        sc = ps.scene(name)
        assert all(np.array_equal(sc["table"][k], base["table"][k]) for k in pr.BODY_F + pr.JOINT_F), name
        got = ps.run_reference(sc, poses)
        moved = max(float(np.abs(a[1][:, :3] - b[1][:, :3]).max()) for a, b in zip(got, ref)) / sc["extent"]
        print("%s: the reference's bodies move by %.2e x extent against the default parameters" % (name, moved))
        assert moved > 100 * 1e-4, name
    # gravity: every component on its own, too (gx and gz are 0 by default)
    for ax in range(3):
        g = np.array(pr.DEFAULT_GRAVITY, dtype=np.float32)
        g[ax] = ps.PARAMS["gravity"][ax]
        got = ps.run_reference(dict(base, table=dict(base["table"], gravity=g)), poses)
        moved = max(float(np.abs(a[1][:, :3] - b[1][:, :3]).max()) for a, b in zip(got, ref)) / base["extent"]
        print("gravity component %d alone: %.2e x extent" % (ax, moved))
        assert moved > 100 * 1e-4


def gpu_cases():
    """every (scene, pose sequence, calls, chains) the GPU tests run"""
    for name in ("one body", "63 bodies", "65 bodies", "wide colour", "skirt", "one joint"):
        sc = ps.scene(name)
        yield name, sc, [ps.pose(sc, k) for k in range(len(ps.CALLS))], ps.CALLS, ()
    for name in PARAM_SCENES + tuple(n for n in ps.FORMS if not n.startswith("most")) + ("contents",):
        sc = ps.scene(name)
        yield name, sc, [ps.pose(sc, k) for k in range(len(ps.CALLS))], ps.CALLS, ()
    for name in ("most strands", "most bodies"):
        sc = ps.scene(name)
        yield name, sc, [ps.pose(sc, k) for k in range(len(ps.EDGE_CALLS))], ps.EDGE_CALLS, ()
    for name in LOCAL_CROWD_SCENES:
        sc = ps.scene(name)
        for i in range(3):
            yield "%s, crowd instance %d" % (name, i), sc, [ps.local_crowd_pose(sc, i, k) for k in range(len(ps.CROWD_CALLS))], ps.CROWD_CALLS, ()
    sc = ps.scene("crowd")
    a0, a1 = ps.motion(sc, 0), ps.motion(sc, 1)
    for i in range(3):
        yield "sampled %d" % i, sc, [sample_reference(a0, float(np.float32(ps.crowd_frames(i, k))), sc["B"], 0)[:2] for k in range(3)], ps.CROWD_CALLS, ()
    for i in range(5):
        st = [(i % 2, float(np.float32(ps.crowd_frames(i, k))), (i + 1) % 2, float(np.float32(ps.crowd_frames(i, k) + 0.5)), float(np.float32(0.25 * (i % 5)))) for k in range(3)]
        yield "blended %d" % i, sc, [motion_ref.blend_reference([a0, a1], s, sc["B"], 0)[:2] for s in st], ps.CROWD_CALLS, ()
    ik = ps.scene("ik")
    yield "ik", ik, [ps.ik_pose(ik, k) for k in range(len(ps.CALLS))], ps.CALLS, ik["chains"]
    _, bm, mw, plain = ps.bone_morph_case()
    yield "bone morph poses", sc, [bone_morph_reference(q, t, bm["morph"], bm["bone"], bm["t"], bm["q"], mw) for q, t in plain], ps.CROWD_CALLS, ()
    yield "replay poses", sc, [ps.pose(sc, 40 + k) for k in range(3)], (5, 5, 5), ()
    for k in (1, 2):
        yield "instance poses %d" % k, sc, [ps.pose(sc, 60 + k)], (4,), ()
    yield "reset poses", sc, [ps.pose(sc, 60)], (8,), ()           # (test_reset_and_instances: 8 substeps, a reset, then 6)
    yield "reset poses, after the reset", sc, [ps.pose(sc, 60)], (6,), ()
    node, _, q = ps.node_case()
    yield "node", node, [(q, np.zeros((node["B"], 3), dtype=np.float32))] * len(ps.NODE_TIMES), ps.node_substeps(), ()


def test_scenes_are_well_conditioned():
    """the float32 run of the definition stays within 2.5e-5 x extent of its float64 run over every GPU test's whole horizon"""
    worst, n, out = {}, 0, 0
    for name, sc, poses, calls, chains in gpu_cases():
        c = ps.conditioning(sc, poses, calls, chains)
        worst[name] = c
        n += 1
        out += c > ILL
    print("float32 probe / extent: " + ", ".join("%s %.1e" % kv for kv in worst.items()))
    assert out <= 0.02 * n, "%d of %d cases are ill-conditioned" % (out, n)
    # the launch-shape and table-content cases: none of them may be left to the 2 %
    assert all(k in worst for k in NEW_CASES)
    bad = {k: worst[k] for k in NEW_CASES if worst[k] > ILL}
    assert not bad, "ill-conditioned: %s" % bad


def test_node_physics_tables_equal_the_python_tables(tmp_path):
    """Model.physicsTables() on a synthetic PMX with rigid-body and joint sections: the flat arrays rz_upload_physics takes"""
    import json
    sc = ps.scene("crowd")
    data, want = ps.write_pmx(sc)
    (tmp_path / "s.pmx").write_bytes(data)
    got = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "physics_tables.js"), str(tmp_path / "s.pmx")], timeout=60).decode().strip().splitlines()[-1])
    assert got["nBodies"] == want["n_bodies"] and got["nJoints"] == want["n_joints"]
    names = dict(bone="bone", type="type", shape="shape", group="group", mask="mask", bodyA="body_a", bodyB="body_b", size="size", offsetPos="offset_pos",
                 offsetRot="offset_rot", mass="mass", linearDamping="linear_damping", angularDamping="angular_damping", restitution="restitution",
                 friction="friction", position="position", rotation="rotation", positionMin="position_min", positionMax="position_max",
                 rotationMin="rotation_min", rotationMax="rotation_max", springPosition="spring_position", springRotation="spring_rotation")
    worst = 0.0
    for js, py in names.items():
        a, b = np.array(got[js], dtype=np.float64), np.asarray(want[py], dtype=np.float64).reshape(-1)
        assert a.shape == b.shape, js
        worst = max(worst, float(np.abs(a - b).max()))
    print("Model.physicsTables() against the Python tables: largest difference %.2e" % worst)
    assert worst <= 2e-6            # (offsets: one float32 subtraction of values up to 17; quaternions: float32 of a double product)
    # and the table the loader derived runs: same colouring as the scene's
    t2 = dict(want)
    assert pr.colouring(t2)[2] == pr.colouring(sc["table"])[2]


def test_engine_device_physics_option_with_a_recording_addon(tmp_path):
    """Engine { devicePhysics } against a stand-in for the addon: the table goes to every shard after its topology; every frame is pose,
    physicsStep(min(10, floor(accumulated / h))), frame; resetPhysics() reaches every shard and drops the accumulated time; devicePhysics
    without deviceFK, with { physics } or with framesInFlight: 2 throws, and so does setBoneWorldOverrides beside a resident table."""
    import json
    sc, data, _ = ps.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    times = (0, 16.7, 33.4, 50.1, 66.8, 1000)
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "physics_engine_mock.js"), str(tmp_path / "s.pmx")] + ["%r" % t for t in times],
                                           timeout=60).decode().strip().splitlines()[-1])
    assert r["needsDeviceFK"] and r["exclusiveWithHook"] and r["noFramesInFlight"] and r["overridesRefused"] and r["plainRefusesReset"]
    nb, nj = sc["table"]["n_bodies"], sc["table"]["n_joints"]
    assert r["upload"] == [["topology", 0], ["uploadPhysics", 0, nb, nj, nb, nb * 4, True], ["topology", 1], ["uploadPhysics", 1, nb, nj, nb, nb * 4, True]]
    want = ps.node_substeps(times)
    assert want == (0, 1, 1, 1, 2, 10)                 # (the last frame owes 70 substeps: capped at 10, the rest dropped)
    frames = []
    for n in want:
        for shard in (0, 1):
            frames += [["setPoseLocal", shard], ["physicsStep", shard, n], ["deform", shard]]
    assert r["frames"] == frames
    # 10 ms in the accumulator, a reset, 10 ms more: without the drop the second frame would owe a substep
    assert r["reset"] == [["physicsStep", 0, 0], ["physicsStep", 1, 0], ["physicsReset", 0], ["physicsReset", 1], ["physicsStep", 0, 0], ["physicsStep", 1, 0]]
    assert r["plain"] == ["topology", "setPoseLocal", "deform", "setPoseLocal", "deform"]


@pytest.fixture(scope="module")
def table_tool(tmp_path_factory):
    return ps.build_table_tool(tmp_path_factory.mktemp("physics_table"))


@pytest.mark.parametrize("name", ["crowd", "63 bodies", "wide colour", "one body", "ik", "params", "params gravity", "contents", "gimbal", "64 joints", "65 joints",
                                  "256 joints", "257 joints", "most strands", "most bodies"])
def test_upload_colours_and_derives_what_the_reference_does(table_tool, name):
    """validation, colours, solve order, colour offsets, the widest colour, parameters and every derived constant of the body and joint
    records; with "contents": bone = -1, a zero inertia, dampings of 0 and 1 and limits given max first"""
    sc = ps.scene(name)
    t = sc["table"]
    out = subprocess.run([table_tool], input=ps.dump_table(t, sc["parents"], sc["bind"]), capture_output=True, text=True, check=True).stdout
    rows = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1].split() if " " in ln else [] for ln in out.strip().split("\n")}
    assert rows["valid"][0] == "1", out[:200]
    colour, order, ncol = pr.colouring(t)
    c = pr.prepare(t, sc["parents"], sc["bind"])
    counts = rows["counts"]
    assert [int(x) for x in counts[:4]] == [t["n_bodies"], t["n_joints"], ncol, len(c["dyn_bodies"])] and int(counts[5]) == c["iterations"]
    assert int(counts[4]) == (int(np.diff(c["colour_off"]).max()) if t["n_joints"] else 0)
    assert np.float32(counts[6]) == np.float32(c["h"]) and np.array_equal(np.array(rows["gravity"], dtype=np.float32), c["gravity"].astype(np.float32))
    assert [int(x) for x in rows["colour"]] == list(colour) and [int(x) for x in rows["order"]] == list(order)
    assert [int(x) for x in rows["colour_off"]] == list(c["colour_off"][:ncol + 1])
    body = np.array([float(x) for x in rows["body"]]).reshape(-1, 13)
    want = np.concatenate([c["off_p"], c["inv_mass"][:, None], c["off_q"], c["inv_inertia"], c["lin_keep"][:, None], c["ang_keep"][:, None]], axis=1)
    assert np.array_equal(body.astype(np.float32), want.astype(np.float32))
    if t["n_joints"]:
        joint = np.array([float(x) for x in rows["joint"]]).reshape(-1, 29)
        al = c["alpha"]
        want = np.concatenate([c["r_a"], c["r_b"], c["j_a"], c["j_b"], c["pmin"], al[:, :1], c["pmax"], al[:, 1:2], c["rmin"], al[:, 2:3], c["rmax"]], axis=1)
        # the spring compliances 1 / (k h^2) reach 288 once h is not the default (at 1 / 75 they are 112.5 and 28.125, exact in float32):
        # they are held to one float32 rounding of their size, every other constant to the absolute bound
        alpha = np.zeros(29, dtype=bool)
        alpha[[17, 21, 25]] = True
        err = np.abs(joint - want)[:, ~alpha].max()
        rel = (np.abs(joint - want)[:, alpha] / np.maximum(np.abs(want[:, alpha]), 1.0)).max()
        print("%s: joint constants differ from physics_ref.prepare by %.2e, the spring compliances by %.2e of their size" % (name, err, rel))
        assert err <= 4e-7 * max(1.0, np.abs(want[:, :6]).max())         # (float32 rounding of values computed in double on both sides)
        assert rel <= 2.0 ** -24
        if float(t["h"]) == 0:              # (the default h: the compliances are exact, and the one absolute bound covers them as it always did)
            assert np.abs(joint - want).max() <= 4e-7 * max(1.0, np.abs(want[:, :6]).max())


def test_upload_validation_messages(table_tool):
    sc = ps.scene("crowd")
    import copy
    for key, idx, val, word in (("bone", 2, 99, "names bone"), ("body_b", 1, 999, "names bodies"), ("mass", 3, -1.0, "negative mass"),
                                ("linear_damping", 3, 1.5, "damping"), ("bone", 2, int(sc["table"]["bone"][1]), "both drive bone"),
                                ("type", 3, 7, "has type"), ("shape", 3, 5, "has shape")):
        t = copy.deepcopy(sc["table"])
        t[key][idx] = val
        assert pr.validate(t, sc["B"]) is not None
        out = subprocess.run([table_tool], input=ps.dump_table(t, sc["parents"], sc["bind"]), capture_output=True, text=True, check=True).stdout
        assert out.startswith("valid 0") and word in out, out[:200]
