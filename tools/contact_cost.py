"""What one mode of the contact stage (rz_physics_contacts(ctx, mode), the CONTACT instantiations of kernels/physics.hip) adds to
rz_physics_step(10) against the mode below it on the same table.
  python tools/contact_cost.py <mode a> <mode b> [rounds]
    0 1   contacts off and on                       (writes profiles/contact_cost.txt)
    1 2   without boxes and with them               (writes profiles/box_contact_cost.txt)
    2 3   without pairs of two boxes and with them  (writes profiles/boxbox_contact_cost.txt)
Shapes: one character and a crowd of 256. For 0 1 the strands-around-a-torso table of tests/contact_scenes.py ("own 64": 21 bodies,
18 joints, 36 follow entries) and the same strands unmasked against each other (follow entries and dynamic pairs in several colours); for
1 2 and 2 3 the strands of box plates, capsules and spheres around a following box torso of tests/contact_box_scenes.py ("own 64": 21
bodies, 18 joints; 9 follow entries under on = 1, 27 under on = 2, 36 under on = 3: the 9 plates against the torso). One measurement is a
FRESH PROCESS: it uploads the table, enables contacts in the mode asked for, steps a few times under a pose that keeps the strands against
the torso, then times `CALLS` calls of rz_physics_step(10) by the host's clock around a drained stream. Per shape `rounds` (default 5)
rounds alternate the two modes; the median is printed with every round beside it. Contacts off is the kernel from before the stage — the
CONTACT = 0 instantiations are the code they were — so that column is the baseline. No bar is set: this is a record."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CALLS, SUBSTEPS, WARM = 100, 10, 5
KEYS = ("physics_bodies", "physics_joints", "physics_contact_follow", "physics_contact_pairs", "physics_contact_colours", "physics_contact_box_pairs", "physics_contact_box_box")
BOX_SHAPES = {"character": ("boxes", 1), "crowd of 256": ("boxes", 256)}
# (mode a, mode b): the file, {shape: (scene, instances)}, the rest of the first line, the second line, a row's format and the keys in it
# as (mode, index into KEYS)
PAIRS = {
    (0, 1): ("contact_cost.txt", {"character follow": ("follow", 1), "character pairs": ("pairs", 1), "crowd follow": ("follow", 256), "crowd pairs": ("pairs", 256)},
             "Contacts off = the parent commit's kernel.",
             "shape              bodies joints follow pairs colours |  off      on     added  ratio | rounds",
             "%-18s %6d %6d %6d %5d %7d | %7.2f %7.2f %7.2f %6.2f | off %s on %s", ((1, 0), (1, 1), (1, 2), (1, 3), (1, 4))),
    (1, 2): ("box_contact_cost.txt", BOX_SHAPES, "on = 1: contacts without boxes, on = 2: boxes take part.",
             "shape          bodies joints | follow entries 1 / 2, pairs, pairs of two boxes left out |  on = 1  on = 2   added  ratio | rounds",
             "%-14s %6d %6d | %4d / %4d, %4d, %4d | %7.2f %7.2f %7.2f %6.2f | on = 1: %s on = 2: %s", ((2, 0), (2, 1), (1, 2), (2, 2), (2, 3), (2, 5))),
    (2, 3): ("boxbox_contact_cost.txt", BOX_SHAPES, "on = 2: boxes against spheres and capsules, on = 3: and against each other.",
             "shape          bodies joints | follow entries 2 / 3, pairs, pairs of two boxes left out under 2 / taking part under 3 |  on = 2  on = 3   added  ratio | rounds",
             "%-14s %6d %6d | %4d / %4d, %4d, %4d / %4d | %7.2f %7.2f %7.2f %6.2f | on = 2: %s on = 3: %s", ((3, 0), (3, 1), (2, 2), (3, 2), (3, 3), (2, 5), (3, 6))),
}


def child(kind, instances, mode):
    import contact_box_scenes as bs
    import contact_scenes as cs
    import reze_engine_amd as rz
    sc = {"follow": lambda: cs.case("own 64")[0], "pairs": lambda: cs.strands(6, 3, 55, ring_radius=1.1, self_collide=True), "boxes": lambda: bs.case("own 64")[0]}[kind]()
    m = sc["mesh"]
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        if instances > 1:
            c.set_instances(instances)
        c.upload_physics(sc["table"])
        if mode:
            c.physics_contacts(True, boxes=mode >= 2, box_pairs=mode == 3)
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
        keys = [c.get_tuning(k) for k in KEYS]
    print("RESULT %.3f %s" % (us, " ".join(str(k) for k in keys)))


def measure(kind, instances, mode):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, str(instances), str(mode)], capture_output=True, text=True, timeout=300, check=True).stdout
    row = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1].split()
    return float(row[1]), [int(v) for v in row[2:]]


def main():
    if "--child" in sys.argv:
        k = sys.argv.index("--child")
        return child(sys.argv[k + 1], int(sys.argv[k + 2]), int(sys.argv[k + 3]))
    if len(sys.argv) < 3 or (int(sys.argv[1]), int(sys.argv[2])) not in PAIRS:
        sys.exit(__doc__)
    a, b = int(sys.argv[1]), int(sys.argv[2])
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    name, shapes, legend, columns, fmt, cols = PAIRS[a, b]
    lines = ["rz_physics_step(%d) in us per call (host clock over %d calls around a drained stream, after %d warm-up calls; every figure from a fresh process;"
             " median of %d alternated rounds). %s" % (SUBSTEPS, CALLS, WARM, rounds, legend), columns]
    for shape, (kind, instances) in shapes.items():
        t, keys = {a: [], b: []}, {}
        for r in range(rounds):
            for mode in ((a, b) if r % 2 == 0 else (b, a)):
                us, keys[mode] = measure(kind, instances, mode)
                t[mode].append(us)
        one, two = float(np.median(t[a])), float(np.median(t[b]))
        lines.append(fmt % ((shape,) + tuple(keys[mode][k] for mode, k in cols) + (one, two, two - one, two / one, " ".join("%.1f" % x for x in t[a]), " ".join("%.1f" % x for x in t[b]))))
        print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
