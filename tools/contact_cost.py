"""What the contact stage (rz_physics_contacts, the CONTACT instantiations of kernels/physics.hip) adds to rz_physics_step(10) on the same table.
  python tools/contact_cost.py [rounds]        (writes profiles/contact_cost.txt)
Shapes: one character and a crowd of 256, both the strands-around-a-torso table of tests/contact_scenes.py ("own 64": 21 bodies, 18 joints,
36 follow entries) and the same strands unmasked against each other (follow entries and dynamic pairs in several colours). One measurement
is a FRESH PROCESS: it uploads the table, enables contacts or not, steps a few times under a pose that keeps the strands against the torso,
then times `CALLS` calls of rz_physics_step(10) by the host's clock around a drained stream. Per shape `rounds` (default 5) rounds alternate
contacts off and on; the median is printed with every round beside it. Contacts off is the parent commit's kernel — the CONTACT = false
instantiations are the code they were — so that column is the baseline. No bar is set: nobody has measured this yet."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CALLS, SUBSTEPS, WARM = 100, 10, 5
SHAPES = {"character follow": ("follow", 1), "character pairs": ("pairs", 1), "crowd follow": ("follow", 256), "crowd pairs": ("pairs", 256)}


def scene(kind):
    import contact_scenes as cs
    return cs.case("own 64")[0] if kind == "follow" else cs.strands(6, 3, 55, ring_radius=1.1, self_collide=True)


def child(kind, instances, on):
    import contact_scenes as cs
    import reze_engine_amd as rz
    sc = scene(kind)
    m = sc["mesh"]
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        if instances > 1:
            c.set_instances(instances)
        c.upload_physics(sc["table"])
        if on:
            c.physics_contacts(True)
        q, t = cs.pose(sc, 1)
        c.set_pose_local(np.tile(q, (instances, 1, 1)), None, np.tile(t, (instances, 1, 1)))
        for _ in range(WARM):
            c.physics_step(SUBSTEPS)
        c.sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            c.physics_step(SUBSTEPS)
        c.sync()
        us = (time.perf_counter() - t0) / CALLS * 1e6
        keys = [c.get_tuning(k) for k in ("physics_bodies", "physics_joints", "physics_contact_follow", "physics_contact_pairs", "physics_contact_colours")]
    print("RESULT %.3f %s" % (us, " ".join(str(k) for k in keys)))


def measure(kind, instances, on):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, str(instances), str(int(on))], capture_output=True, text=True, timeout=300, check=True).stdout
    row = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1].split()
    return float(row[1]), [int(v) for v in row[2:]]


def main():
    if "--child" in sys.argv:
        k = sys.argv.index("--child")
        return child(sys.argv[k + 1], int(sys.argv[k + 2]), sys.argv[k + 3] == "1")
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lines = ["rz_physics_step(%d) in us per call (host clock over %d calls around a drained stream, after %d warm-up calls; every figure from a fresh process;"
             " median of %d alternated rounds). Contacts off = the parent commit's kernel." % (SUBSTEPS, CALLS, WARM, rounds),
             "shape              bodies joints follow pairs colours |  off      on     added  ratio | rounds"]
    for name, (kind, instances) in SHAPES.items():
        t, keys = {0: [], 1: []}, None
        for r in range(rounds):
            for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                us, k = measure(kind, instances, on)
                t[on].append(us)
                if on:
                    keys = k
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        lines.append("%-18s %6d %6d %6d %5d %7d | %7.2f %7.2f %7.2f %6.2f | off %s on %s" % ((name,) + tuple(keys) + (off, on, on - off, on / off, " ".join("%.1f" % x for x in t[0]), " ".join("%.1f" % x for x in t[1]))))
        print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "contact_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
