"""What contacts between two boxes (rz_physics_contacts(ctx, 3), the CONTACT = 3 instantiations of kernels/physics.hip) add to
rz_physics_step(10) against box contacts without them (on = 2) on the same table.
  python tools/boxbox_contact_cost.py [rounds]        (writes profiles/boxbox_contact_cost.txt)
Shapes: one character and a crowd of 256, the strands of box plates, capsules and spheres around a following box torso of
tests/contact_box_scenes.py ("own 64": 21 bodies, 18 joints; 27 follow entries under on = 2, 36 under on = 3: the 9 plates against the
torso). One measurement is a FRESH
PROCESS: it uploads the table, enables contacts in the mode asked for, steps a few times under a pose that keeps the strands against the
torso, then times `CALLS` calls of rz_physics_step(10) by the host's clock around a drained stream. Per shape `rounds` (default 5) rounds
alternate the two modes; the median is printed with every round beside it. No bar is set: this is a record."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CALLS, SUBSTEPS, WARM = 100, 10, 5
SHAPES = {"character": 1, "crowd of 256": 256}


def child(instances, mode):
    import contact_box_scenes as bs
    import reze_engine_amd as rz
    sc = bs.case("own 64")[0]
    m = sc["mesh"]
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        if instances > 1:
            c.set_instances(instances)
        c.upload_physics(sc["table"])
        c.physics_contacts(True, boxes=True, box_pairs=mode == 3)
        q, t = bs.pose(sc, 1)
        c.set_pose_local(np.tile(q, (instances, 1, 1)), None, np.tile(t, (instances, 1, 1)))
        for _ in range(WARM):
            c.physics_step(SUBSTEPS)
        c.sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            c.physics_step(SUBSTEPS)
        c.sync()
        us = (time.perf_counter() - t0) / CALLS * 1e6
        keys = [c.get_tuning(k) for k in ("physics_bodies", "physics_joints", "physics_contact_follow", "physics_contact_pairs", "physics_contact_box_pairs", "physics_contact_box_box")]
    print("RESULT %.3f %s" % (us, " ".join(str(k) for k in keys)))


def measure(instances, mode):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(instances), str(mode)], capture_output=True, text=True, timeout=300, check=True).stdout
    row = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1].split()
    return float(row[1]), [int(v) for v in row[2:]]


def main():
    if "--child" in sys.argv:
        k = sys.argv.index("--child")
        return child(int(sys.argv[k + 1]), int(sys.argv[k + 2]))
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lines = ["rz_physics_step(%d) in us per call (host clock over %d calls around a drained stream, after %d warm-up calls; every figure from a fresh process;"
             " median of %d alternated rounds). on = 2: boxes against spheres and capsules, on = 3: and against each other." % (SUBSTEPS, CALLS, WARM, rounds),
             "shape          bodies joints | follow entries 2 / 3, pairs, pairs of two boxes left out under 2 / taking part under 3 |  on = 2  on = 3   added  ratio | rounds"]
    for name, instances in SHAPES.items():
        t, keys = {2: [], 3: []}, {}
        for r in range(rounds):
            for mode in ((2, 3) if r % 2 == 0 else (3, 2)):
                us, keys[mode] = measure(instances, mode)
                t[mode].append(us)
        one, two = float(np.median(t[2])), float(np.median(t[3]))
        lines.append("%-14s %6d %6d | %4d / %4d, %4d, %4d / %4d | %7.2f %7.2f %7.2f %6.2f | on = 2: %s on = 3: %s"
                     % (name, keys[3][0], keys[3][1], keys[2][2], keys[3][2], keys[3][3], keys[2][4], keys[3][5], one, two, two - one, two / one, " ".join("%.1f" % x for x in t[2]), " ".join("%.1f" % x for x in t[3])))
        print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "boxbox_contact_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
