"""tests/spring_ref.py, the definition the device's linear joint springs are held to, is physics (a mass on a spring under backward Euler)
and is contact_ref.Sim when the stage is off; the scenes the GPU tests use (tests/spring_scenes.py) are well-conditioned and moved by the
springs; the GPU-free half of rz_physics_springs (csrc/physics_table.h) derives the definition's constants; the Engine option calls the
addon in order; the PMX loader carries spring positions through. No GPU."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_ref
import contact_scenes as cs
import physics_ref as pr
import physics_scenes as ps
import spring_ref
import spring_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILL = 2.5e-5                            # the conditioning bar of tests/test_physics_cpu.py
BAR = 1e-4                              # the GPU tests' bar
MASS = 2.0


def oscillator(k, iterations, substeps=400, x0=1.0):
    """a 2 kg sphere centred on the anchor of a joint to a body fixed at the origin: no gravity, no damping, rotation locked, 10 units of
    play and a spring of k along x; released x0 from the rest point. Returns its x after every substep."""
    t = pr.make_table([dict(bone=0, type=0, mass=0), dict(bone=0, type=1, shape=0, size=[0.5, 0, 0], mass=MASS)],
                      [dict(body_a=0, body_b=1, position=[0, 0, 0], rotation=[0, 0, 0], position_min=[-10, 0, 0], position_max=[10, 0, 0], spring_position=[k, 0, 0])],
                      gravity=[0, 0, 0], iterations=iterations)
    s = spring_ref.Sim(t, [-1], [[0, 0, 0]])
    W = np.eye(4).reshape(1, 16)
    s.reset(W)
    s.x[1, 0] = x0
    xs = []
    for _ in range(substeps):
        s.step(W, 1)
        xs.append(float(s.x[1, 0]))
        assert abs(s.x[1, 1]) <= 1e-12 and abs(s.x[1, 2]) <= 1e-12
    return np.array(xs), s.c["h"]


def period_of(x):
    """substeps per period, from the first and the last downward zero crossing (interpolated)"""
    zc = [n - 1 + x[n - 1] / (x[n - 1] - x[n]) for n in range(1, len(x)) if x[n - 1] > 0 >= x[n]]
    return (zc[-1] - zc[0]) / (len(zc) - 1)


def peaks_of(x):
    """(position, value) of the maxima, each from the parabola through the largest sample and its neighbours"""
    out = []
    for n in range(1, len(x) - 1):
        if x[n] > 0 and x[n - 1] < x[n] >= x[n + 1]:
            a, b, c = x[n - 1], x[n], x[n + 1]
            d = 0.5 * (a - c) / (a - 2 * b + c)
            out.append((n + d, b - 0.25 * (a - c) * d))
    return out


@pytest.mark.parametrize("k", [50.0, 200.0, 1000.0])
def test_mass_on_a_spring_is_backward_euler(k):
    """x'' = -omega^2 x stepped by backward Euler turns by atan(omega h) and shrinks by (1 + (omega h)^2)^(-1/2) per substep: the period is
    2 pi h / atan(omega h) within 0.1 % (room for the interpolated zero crossings), successive peaks stand in the ratio
    (1 + (omega h)^2)^(-steps / 2) within 1 %, the period is the same at 1, 4 and 16 iterations, and the amplitude never grows."""
    periods = {}
    for it in (1, 4, 16):
        x, h = oscillator(k, it)
        periods[it] = period_of(x) * h
    wh = math.sqrt(k / MASS) * h
    want = 2 * math.pi * h / math.atan(wh)
    print("k %g: period %.5f s at 1, %.5f at 4, %.5f at 16 iterations; backward Euler %.5f s" % (k, periods[1], periods[4], periods[16], want))
    for it in (1, 4, 16):
        assert abs(periods[it] / want - 1) <= 1e-3
    assert abs(periods[4] / periods[1] - 1) <= 1e-9 and abs(periods[16] / periods[1] - 1) <= 1e-9
    x, h = oscillator(k, 4)
    pk = peaks_of(x)
    assert len(pk) >= 3
    for (n0, a0), (n1, a1) in zip(pk, pk[1:]):
        ratio, decay = a1 / a0, (1 + wh * wh) ** (-(n1 - n0) / 2)
        assert abs(ratio / decay - 1) <= 0.01, (k, ratio, decay)
        assert a1 < a0
    print("k %g: first peaks %s, ratio %.5f against %.5f" % (k, " ".join("%.4f" % a for _, a in pk[:3]), pk[1][1] / pk[0][1], (1 + wh * wh) ** (-(pk[1][0] - pk[0][0]) / 2)))
    # never grows: every sample lies under the envelope that starts at the release
    n = np.arange(1, len(x) + 1)
    assert (np.abs(x) <= (1 + wh * wh) ** (-n / 2) * (1 + 1e-9)).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", [0, 1])
def test_off_is_off(dtype, mode):
    """springs=False, and springs=True on an all-zero column, step bit for bit as contact_ref.Sim does: over the standard calls, without
    contacts (the "crowd" strands with their play) and with them (contact_scenes' "own 64")"""
    if mode:
        base, poses, calls = cs.case("own 64")
        sc = ss.sprung(base, 77)
    else:
        sc = ss.sprung(ps.scene("crowd"), 77)
        poses, calls = [ps.pose(sc, k) for k in range(len(ps.CALLS))], ps.CALLS
    zero = ss.with_columns(sc, np.zeros((sc["table"]["n_joints"], 3)))
    args = (sc["parents"], sc["bind"])
    want = ps.run_reference(sc, poses, calls, dtype=dtype, sim=contact_ref.Sim(sc["table"], *args, dtype=dtype, mode=mode))
    off = ps.run_reference(sc, poses, calls, dtype=dtype, sim=spring_ref.Sim(sc["table"], *args, dtype=dtype, mode=mode, springs=False))
    none = ps.run_reference(zero, poses, calls, dtype=dtype, sim=spring_ref.Sim(zero["table"], *args, dtype=dtype, mode=mode))
    on = ps.run_reference(sc, poses, calls, dtype=dtype, sim=spring_ref.Sim(sc["table"], *args, dtype=dtype, mode=mode))
    for (w, s), (w1, s1), (w2, s2) in zip(want, off, none):
        assert np.array_equal(w, w1) and np.array_equal(s, s1) and np.array_equal(w, w2) and np.array_equal(s, s2)
    assert not np.array_equal(want[-1][1], on[-1][1])


def test_scenes_are_well_conditioned_and_moved_by_the_springs():
    """every case of the GPU file: the float32 run of the definition stays within ILL x extent of its float64 run, and the definition with
    the springs differs from the one without by at least 100 x the GPU bar — a kernel without the stage cannot pass"""
    bad = {}
    for name in ss.ORDER:
        c, e = ss.conditioning(name), ss.effect(name)
        print("%s: float32 probe %.1e x extent, the springs move the bodies by %.1e x extent" % (name, c, e))
        if c > ILL or e < 100 * BAR:
            bad[name] = (c, e)
    assert not bad, bad
    sc, _, q = ss.node_case()
    calls = ps.node_substeps()
    poses = [(q, np.zeros((sc["B"], 3), dtype=np.float32))] * len(calls)
    run = lambda **kw: ps.run_reference(sc, poses, calls, dtype=kw.pop("dtype", np.float64), sim=spring_ref.Sim(sc["table"], sc["parents"], sc["bind"], **kw))
    a, b, off = run(), run(dtype=np.float32), run(springs=False)
    c = max(max(float(np.abs(x[0] - y[0]).max()), float(np.abs(x[1][:, :3] - y[1][:, :3]).max())) for x, y in zip(a, b)) / sc["extent"]
    e = max(float(np.abs(x[1][:, :3] - y[1][:, :3]).max()) for x, y in zip(a, off)) / sc["extent"]
    print("node case: float32 probe %.1e x extent, the springs move the bodies by %.1e x extent" % (c, e))
    assert c <= ILL and e >= 100 * BAR


def test_roles_scene_holds_what_it_is_there_for():
    """the "roles" case: a joint between two followers with springs on every axis moves nothing, a k < 0 is no spring, and max-first limits
    are the same joint as min-first ones"""
    sc = ss.case("roles")[0]
    t = sc["table"]
    on, alpha = spring_ref.lin_constants(t, 1 / 75)
    order = list(pr.colouring(t)[1])
    assert not on[order.index(2), 1] and alpha[order.index(2), 1] == 0 and on[order.index(2), 0]
    dyn = pr.is_dynamic(t)
    assert not dyn[t["body_a"][3]] and not dyn[t["body_b"][3]] and (t["spring_position"][3] > 0).all()
    ref = ss.reference("roles")
    follow = ps.run_reference(sc, *ss.case("roles")[1:], sim=ss.sim_of("roles", springs=False))
    for (_, s), (_, s0) in zip(ref, follow):
        assert np.array_equal(s[~dyn], s0[~dyn])
    swapped = ss.with_columns(sc, t["spring_position"], np.minimum(t["position_min"], t["position_max"]), np.maximum(t["position_min"], t["position_max"]))
    assert (t["position_min"][1] > t["position_max"][1]).all()
    got = ps.run_reference(swapped, *ss.case("roles")[1:], sim=spring_ref.Sim(swapped["table"], sc["parents"], sc["bind"]))
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(ref, got))


# ---- the host half (tests/physics_table_main.cpp around reze-engine_amd/csrc/physics_table.h) ----

@pytest.fixture(scope="module")
def table_tool(tmp_path_factory):
    return ps.build_table_tool(tmp_path_factory.mktemp("spring_table"))


def run_tool(tool, sc, column=True):
    out = subprocess.run([tool], input=ps.dump_table(sc["table"], sc["parents"], sc["bind"], column), capture_output=True, text=True, check=True).stdout
    return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] if " " in ln else "" for ln in out.strip().split("\n")}


@pytest.mark.parametrize("name", ["own 64", "stride 64", "own 256", "stride 256", "roles", "h and iterations", "most strands", "contacts 1 stride 256"])
def test_host_records_equal_the_definition(table_tool, name):
    """the linear records in solve order: the axes' bits are the definition's lin_on, alpha~ its lin_alpha within one float32 rounding of
    their size; the count of spring axes; the form; the LDS of both forms by the stated arithmetic; no refusal"""
    sc = ss.case(name)[0]
    t = sc["table"]
    rows = run_tool(table_tool, sc)
    assert rows["valid"].split()[0] == "1" and rows["refused"].strip() == "0"
    h = float(t["h"]) if float(t["h"]) > 0 else pr.DEFAULT_H
    on, alpha = spring_ref.lin_constants(t, h)
    nb, nj = t["n_bodies"], t["n_joints"]
    assert [int(v) for v in rows["order"].split()] == list(pr.colouring(t)[1])
    bits = np.array([int(v) for v in rows["bits"].split()])
    assert np.array_equal(bits, (on * [1, 2, 4]).sum(axis=1))
    got = np.array([float(v) for v in rows["alpha"].split()]).reshape(nj, 3)
    rel = float((np.abs(got - alpha) / np.maximum(np.abs(alpha), 1.0)).max())
    print("%s: %d spring axes; alpha~ off the definition's by %.2e of their size" % (name, int(on.sum()), rel))
    assert rel <= 2.0 ** -24 and (got[~on] == 0).all()
    assert int(rows["axes"]) == int(on.sum()) == ss.axes_of(t)
    block, own = (int(v) for v in rows["form"].split())
    assert (block, own) == ss.CASES[name][2]
    stride = 0 if own else nj
    assert [int(v) for v in rows["lds"].split()] == [nb * 96 + stride * 12, nb * 96 + stride * 24]
    assert nb * 96 + stride * 24 <= ps.LDS_LIMIT


def test_host_refusals(table_tool):
    """a table uploaded without spring_position: RZ_ERR_INVALID naming the column; physics_scenes' "most strands" (1516 strands: it fits
    with 12 B per joint) with springs on it: RZ_ERR_UNSUPPORTED with the bodies, the joints, the bytes and the per-joint cost; the same
    table without any spring is taken (the old kernels at the old size); one strand more than spring_scenes' largest is refused"""
    sc = ss.case("own 64")[0]
    rows = run_tool(table_tool, sc, column=False)
    assert rows["refused"].startswith("-1 ") and "spring_position" in rows["refused"] and int(rows["axes"]) == 0
    big = ps.scene("most strands")
    nb, nj = big["table"]["n_bodies"], big["table"]["n_joints"]
    assert (nb, nj) == (ps.MOST_STRANDS + 1, ps.MOST_STRANDS) and nb * 96 + nj * 12 <= ps.LDS_LIMIT < nb * 96 + nj * 24
    rows = run_tool(table_tool, big)
    assert rows["refused"].strip() == "0" and int(rows["axes"]) == 0 and [int(v) for v in rows["lds"].split()] == [nb * 96 + nj * 12, nb * 96 + nj * 24]
    rows = run_tool(table_tool, ss.sprung(big, 28))
    msg = rows["refused"]
    print(msg)
    assert msg.startswith("-6 ") and all(w in msg for w in ("%d bodies" % nb, "%d joints" % nj, "%d B of LDS" % (nb * 96 + nj * 24), "24 B per joint", "160 KB"))
    over = ss.strands_table(ss.MOST_STRANDS + 1)
    assert ss.MOST_STRANDS == 1364 and run_tool(table_tool, over)["refused"].startswith("-6 ")


# ---- the bindings ----

@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_engine_option_with_a_recording_addon(tmp_path):
    """Engine { physicsSprings } against a stand-in for the addon: on every shard uploadPhysics, physicsSprings(1), then physicsContacts
    when that is asked for too; no call without the option; it throws without devicePhysics"""
    _, data, _ = ss.node_case()
    (tmp_path / "s.pmx").write_bytes(data)
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "springs_engine_mock.js"), str(tmp_path / "s.pmx"), "springs", "both", "off"],
                                           timeout=60).decode().strip().splitlines()[-1])
    assert r["needsDevicePhysics"] and r["needsDeviceFK"]
    assert r["shards"] >= 2 and len(r["springs"]) == len(r["both"]) == r["shards"]
    for calls in r["springs"]:
        at = calls.index("uploadPhysics")
        assert calls.count("physicsSprings:1") == 1 and calls[at + 1] == "physicsSprings:1" and "physicsContacts" not in " ".join(calls)
    for calls in r["both"]:
        at = calls.index("uploadPhysics")
        assert calls[at:at + 3] == ["uploadPhysics", "physicsSprings:1", "physicsContacts:1"] and calls.count("physicsSprings:1") == 1
    assert all("physicsSprings" not in " ".join(calls) for calls in r["off"]) and all("uploadPhysics" in calls for calls in r["off"])


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_pmx_round_trip_carries_spring_positions(tmp_path):
    """Model.physicsTables() on a PMX written with nonzero spring positions (and the widened position limits) carries them through"""
    sc, data, _ = ss.node_case()
    want = sc["table"]
    assert (want["spring_position"] > 0).sum() > 10
    (tmp_path / "s.pmx").write_bytes(data)
    got = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "physics_tables.js"), str(tmp_path / "s.pmx")], timeout=60).decode().strip().splitlines()[-1])
    for js, py in (("springPosition", "spring_position"), ("positionMin", "position_min"), ("positionMax", "position_max"), ("springRotation", "spring_rotation")):
        assert np.array_equal(np.array(got[js], dtype=np.float32), np.asarray(want[py], dtype=np.float32).reshape(-1)), js


def test_python_binding_lists_the_symbol(rz):
    capi = rz.capi
    assert hasattr(capi.load(), "rz_physics_springs")
    assert "rz_physics_springs" in capi.SYMBOLS and "rz_physics_springs" in capi.OPTIONAL_SYMBOLS
    assert hasattr(capi.DeformContext, "physics_springs")
