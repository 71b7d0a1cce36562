"""What rigid-body physics on the device (rz_upload_physics / rz_physics_step, kernels/physics.hip) adds to a device-animated live loop, and
how far the device solve is from the float64 definition (tests/physics_ref.py).
  python tools/physics_cost.py [rounds] [--parent LIB]        (writes profiles/physics_cost.txt)
Shapes: the demo-shaped 28 842-vertex character (sparse morphs, an uploaded local pose per frame) and C4 as a sampled crowd (256 characters,
each at its own frame of one motion), both with the strands of tests/physics_scenes.py grafted under bone 0: 6 strands of 5 dynamic bodies,
36 bodies in all. A live loop is pose call + rz_physics_step(2) + frame, `LOOPS` times by the host's clock around a drained stream; per shape
`rounds` (default 5) rounds alternate table off (pose call + frame) and on; the median round is printed with the spread. --parent LIB names a
build of the parent commit (same ABI, no rz_upload_physics): its loop is timed in the same process. No time target is set: a second
hierarchy solve per stepped frame and a latency-bound solve of substeps x iterations x colours phases are expected."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import physics_ref  # noqa: E402
import physics_scenes as ps  # noqa: E402
import reze_engine_amd as rz  # noqa: E402
from helpers import sample_reference  # noqa: E402
from reze_engine_amd import synth  # noqa: E402

LOOPS, SUBSTEPS = 200, 2


def graft(mesh, sc):
    """the mesh's skeleton with the scene's skeleton appended under bone 0; vertices keep their bones; the table's bones are shifted"""
    B0 = len(mesh["parents"])
    sp = sc["parents"].copy()
    sp[sp >= 0] += B0
    sp[0] = 0
    m = dict(mesh)
    m["parents"] = np.concatenate([mesh["parents"], sp]).astype(np.int32)
    m["bind"] = np.concatenate([mesh["bind"], sc["bind"]]).astype(np.float32)
    m["inv_bind"] = synth.inverse_bind_translation_only(m["parents"], m["bind"])
    t = dict(sc["table"])
    t["bone"] = np.where(t["bone"] >= 0, t["bone"] + B0, -1).astype(np.int32)
    offs = ps.ik_ref.bind_positions(m["parents"], m["bind"])[B0] - ps.ik_ref.bind_positions(sc["parents"], sc["bind"])[0]
    t["position"] = (t["position"] + offs).astype(np.float32)         # joint positions are in model space
    return m, B0, t


def build(name, lib):
    sc = ps.strands(6, 5, base=True, seed=11, n_verts=64)
    if name == "demo":
        mesh = synth.make_mesh(28842, 349)
        off, idx, d3, mw = synth.make_morphs_demo_shape(28842, 60)
    else:
        mesh = synth.make_mesh_range(30000, 200, 0, 30000)
    mesh, B0, table = graft(mesh, sc)
    B = len(mesh["parents"])
    c = rz.DeformContext(0) if lib is None else rz.DeformContext(0, lib=lib)
    c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
    c.upload_skeleton(mesh["inv_bind"])
    c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
    rng = np.random.default_rng(2)
    if name == "demo":
        c.upload_morphs_sparse(off, idx, d3)
        q = np.tile(np.array([0, 0, 0, 1], dtype=np.float32), (B, 1))
        poses = []
        for k in range(8):
            qk = q.copy()
            a = 0.05 * np.sin(0.7 * k)
            qk[B0 + 1] = [0, 0, np.sin(a / 2), np.cos(a / 2)]
            poses.append((qk, np.zeros((B, 3), dtype=np.float32)))
        pose_call = lambda k: c.set_pose_local(poses[k % 8][0], mw, poses[k % 8][1])      # noqa: E731
        ref_pose = lambda k, i: poses[k % 8]                                              # noqa: E731
    else:
        c.set_instances(256)
        anim = ps.motion(dict(sc, B=B, table=table), 0)
        c.upload_animation(anim["track_bone"], anim["key_off"], anim["key_frame"], anim["key_rot"], anim["key_pos"], anim["key_interp"])
        base = rng.uniform(0.0, 8.0, size=256).astype(np.float32)
        pose_call = lambda k: c.set_pose_sampled(base + np.float32(0.5 * (k % 8)))        # noqa: E731
        ref_pose = lambda k, i: sample_reference(anim, float(np.float32(base[i] + np.float32(0.5 * (k % 8)))), B, 0)[:2]      # noqa: E731
    return c, mesh, table, pose_call, ref_pose


def loop(c, pose_call, physics):
    pose_call(0)
    if physics:
        c.physics_reset()
    c.deform()
    c.sync()
    t0 = time.perf_counter()
    for k in range(LOOPS):
        pose_call(k)
        if physics:
            c.physics_step(SUBSTEPS)
        c.deform()
    c.sync()
    return (time.perf_counter() - t0) / LOOPS * 1e6


def errors(c, mesh, table, pose_call, ref_pose, instances):
    """body positions and world matrices after 8 stepped frames against the definition, in units of the skeleton's extent"""
    ext = ps.ik_ref.extent(ps.ik_ref.bind_positions(mesh["parents"], mesh["bind"]))
    sc = dict(parents=mesh["parents"], bind=mesh["bind"])
    c.physics_reset()
    sims = {i: physics_ref.Sim(table, mesh["parents"], mesh["bind"]) for i in instances}
    worst = 0.0
    for k in range(8):
        pose_call(k)
        c.physics_step(SUBSTEPS)
        c.deform()
        for i, sim in sims.items():
            w = ps.world_of(sc, *ref_pose(k, i))
            w = physics_ref.apply_overrides(w, sim.step(w, SUBSTEPS))
            worst = max(worst, float(np.abs(c.read_physics(i)[:, :3] - sim.x).max()) / ext, float(np.abs(c.read_world(i) - w).max()) / ext)
    return worst


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    if parent in args:
        args.remove(parent)
    rounds = int(args[0]) if args else 5
    plib = rz.capi.load(parent) if parent else None
    lines = ["live loop in us per frame (pose call + rz_physics_step(%d) + frame; host clock over %d frames; median of %d alternated rounds); device"
             " error of body positions and world matrices against tests/physics_ref.py in units of the skeleton's extent" % (SUBSTEPS, LOOPS, rounds),
             "shape  table off   on    added | parent build | error   rounds"]
    for name in ("demo", "c4"):
        c, mesh, table, pose_call, ref_pose = build(name, None)
        t = {0: [], 1: []}
        for r in range(rounds):
            for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                c.upload_physics(table if on else None)
                t[on].append(loop(c, pose_call, bool(on)))
        c.upload_physics(table)
        err = errors(c, mesh, table, pose_call, ref_pose, [0] if name == "demo" else [0, 100, 255])
        c.close()
        ptxt = "-"
        if plib is not None:
            pc, _, _, pcall, _ = build(name, plib)
            ptxt = "%.2f" % float(np.median([loop(pc, pcall, False) for _ in range(rounds)]))
            pc.close()
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        lines.append("%-5s %8.2f %8.2f %8.2f | %-12s | %.2e   off %s on %s" % (name, off, on, on - off, ptxt, err, " ".join("%.1f" % x for x in t[0]), " ".join("%.1f" % x for x in t[1])))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "physics_cost.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
