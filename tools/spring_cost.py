"""What the linear joint springs (rz_physics_springs, the LSPRING instantiations of kernels/physics.hip) add to rz_physics_step(10) on the
same table.
  python tools/spring_cost.py [rounds]          (writes profiles/spring_cost.txt)
Tables: the sprung strands of tests/spring_scenes.py — "own 64" (25 bodies, 20 joints: one wave, joints in registers) and "stride 64" (40
bodies, 65 joints: one wave, lanes striding, multipliers in LDS) — with springs of 0 / 50 / 200 / 1000 per axis and 0.4 of play on two joints
in three. Shapes: one character and a crowd of 256, all in ONE process: per table and shape one context, the stage toggled on it between
rounds (the toggle does not touch the body state). One measurement: a few warm-up calls, then `CALLS` calls of rz_physics_step(10) by the
host's clock around a drained stream. `rounds` (default 7) rounds alternate off and on; the median is printed with every round beside it.
Springs off is the kernel from before the stage — the LSPRING = false instantiations are the code they were — so that column is the
baseline. No bar is set: this is a record."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CALLS, SUBSTEPS, WARM = 300, 10, 10
SHAPES = (("character", 1), ("crowd of 256", 256))
TABLES = ("own 64", "stride 64")


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
    import physics_scenes as ps
    import reze_engine_amd as rz
    import spring_scenes as ss
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    lines = ["rz_physics_step(%d) in us per call (host clock over %d calls around a drained stream, after %d warm-up calls; one process, the stage toggled"
             " between rounds; median of %d alternated rounds). Springs off = the parent commit's kernel." % (SUBSTEPS, CALLS, WARM, rounds),
             "table      shape         bodies joints axes  lds off / on |     off      on   added  ratio | rounds"]
    for name in TABLES:
        sc = ss.case(name)[0]
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
                t_us, lds, axes = {0: [], 1: []}, {}, 0
                for r in range(rounds):
                    for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                        c.physics_springs(bool(on))
                        assert c.get_tuning("physics_springs") == on
                        lds[on] = c.get_tuning("physics_lds")
                        axes = max(axes, c.get_tuning("physics_spring_axes"))
                        t_us[on].append(timed(c))
                off, on = float(np.median(t_us[0])), float(np.median(t_us[1]))
                lines.append("%-10s %-13s %6d %6d %4d %6d / %6d | %7.2f %7.2f %7.2f %6.2f | off %s on %s" % (
                    name, shape, c.get_tuning("physics_bodies"), c.get_tuning("physics_joints"), axes, lds[0], lds[1], off, on, on - off, on / off,
                    " ".join("%.1f" % x for x in t_us[0]), " ".join("%.1f" % x for x in t_us[1])))
                print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "spring_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
