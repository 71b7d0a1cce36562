"""What PMX type-2 bodies simulated (rz_physics_aligned, the ALIGN instantiations of kernels/physics.hip) cost rz_physics_step(10) beside the
same table with the flag off, on the same build.
  python tools/align_cost.py [rounds]          (writes profiles/align_cost.txt)
Table: the "crowd" strands of tests/physics_scenes.py with the first link of every strand made type 2 (tests/align_scenes.py: cost_scene —
25 bodies, 20 joints: one wave, joints in registers). With the flag off those four bodies follow their bones and the strands hang from a
stiff root: 17 dynamic bodies; with it on 21 are dynamic, four of them re-pinned per call and emitted with the solved column. So the ratio
holds both what the flag adds to the kernel and what simulating four more bodies costs. Shapes: one character and a crowd of 256, all in ONE
process: per shape one context, the flag toggled on it between rounds (either value rebuilds the table's records and resets the simulation,
so every measurement starts from the same reset). One measurement: a few warm-up calls, then `CALLS` calls of rz_physics_step(10) by the
host's clock around a drained stream. `rounds` (default 7) rounds alternate off and on; the median is printed with every round beside it.
No target is set: the number to report is the ratio to the flag-off run."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CALLS, SUBSTEPS, WARM = 300, 10, 10
SHAPES = (("character", 1), ("crowd of 256", 256))


def timed(c):
    for _ in range(WARM):
        c.physics_step(SUBSTEPS)
    c.sync()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        c.physics_step(SUBSTEPS)
    c.sync()
    return (time.perf_counter() - t0) / CALLS * 1e6


def main():
    import align_ref
    import align_scenes as als
    import physics_ref
    import physics_scenes as ps
    import reze_engine_amd as rz
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    lines = ["rz_physics_step(%d) in us per call (host clock over %d calls around a drained stream, after %d warm-up calls; one process, the flag toggled"
             " between rounds; median of %d alternated rounds). Flag off = the kernels of a plain upload." % (SUBSTEPS, CALLS, WARM, rounds),
             "table          shape         bodies joints aligned  overridden off / on |     off      on   added  ratio | rounds"]
    sc = als.cost_scene()
    m = sc["mesh"]
    for shape, instances in SHAPES:
        with rz.DeformContext(0) as c:
            c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
            c.upload_skeleton(m["inv_bind"])
            c.upload_skeleton_topology(m["parents"], m["bind"])
            if instances > 1:
                c.set_instances(instances)
            c.upload_physics(sc["table"])
            q, t = ps.pose(sc, 1)
            c.set_pose_local(np.tile(q, (instances, 1, 1)), None, np.tile(t, (instances, 1, 1)))
            t_us, n_aligned = {0: [], 1: []}, 0
            nd = {on: len(physics_ref.prepare(align_ref.read_table(sc["table"], on), sc["parents"], sc["bind"])["dyn_bodies"]) for on in (0, 1)}
            for r in range(rounds):
                for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                    c.physics_aligned(bool(on))
                    assert c.get_tuning("physics_aligned") == on
                    n_aligned = max(n_aligned, c.get_tuning("physics_aligned_bodies"))
                    t_us[on].append(timed(c))
            off, on = float(np.median(t_us[0])), float(np.median(t_us[1]))
            lines.append("%-14s %-13s %6d %6d %7d %10d / %3d | %7.2f %7.2f %7.2f %6.3f | off %s on %s" % (
                "strands, type 2", shape, c.get_tuning("physics_bodies"), c.get_tuning("physics_joints"), n_aligned, nd[0], nd[1], off, on, on - off, on / off,
                " ".join("%.1f" % x for x in t_us[0]), " ".join("%.1f" % x for x in t_us[1])))
            print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "align_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
