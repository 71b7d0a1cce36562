"""What rz_override_follow (the FOLLOW stage of the hierarchy solve: rz_fk_kernel<RzFollowParams> instead of rz_fk_kernel<>) adds to a live frame.
  python tools/follow_cost.py [rounds]          (writes profiles/follow_cost.txt)
The loop a live application runs: a new local pose (rz_set_pose_local), rz_physics_step(1) and the frame (rz_deform), on the strands of
tests/follow_scenes.py's scene (j) — 21 bodies, 18 overridden bones, 5 follower bones per instance — for one character and for a crowd of
256. The flag off and on in the same tree: every measurement runs in a fresh process (this script starts itself with `--one`), `rounds`
(default 5) rounds alternate off and on, the median is printed with every round beside it. One measurement: warm-up frames, then FRAMES
frames by the host's clock around a drained stream. Flag off is the frame from before the stage — the old entry points are the code they
were (profiles/follow_identity.txt) — so that column is the baseline. No bar is set: this is a record."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

FRAMES, WARM = 400, 40
SHAPES = (("character", 1), ("crowd of 256", 256))
OUT = os.path.join(ROOT, "profiles", "follow_cost.txt")


def one(instances, on):
    """one fresh process: us per live frame, and what was resident"""
    import follow_scenes as fs
    import physics_scenes as ps
    import reze_engine_amd as rz
    sc = fs.scene("j")
    m = sc["mesh"]
    poses = [ps.pose(sc, 500 + k) for k in range(4)]
    q = [np.tile(p[0], (instances, 1, 1)) for p in poses]
    t = [np.tile(p[1], (instances, 1, 1)) for p in poses]
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        if instances > 1:
            c.set_instances(instances)
        if on:
            c.override_follow(True)
        c.upload_physics(sc["table"])

        def frames(n):
            for k in range(n):
                c.set_pose_local(q[k % 4], None, t[k % 4])
                c.physics_step(1)
                c.deform()
            c.sync()
        frames(WARM)
        t0 = time.perf_counter()
        frames(FRAMES)
        us = (time.perf_counter() - t0) / FRAMES * 1e6
        print(json.dumps(dict(us=us, followers=c.get_tuning("override_followers"), bones=sc["B"], bodies=c.get_tuning("physics_bodies"))))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(int(sys.argv[2]), int(sys.argv[3]))
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lines = ["live frame (rz_set_pose_local + rz_physics_step(1) + rz_deform) in us (host clock over %d frames around a drained stream, after %d warm-up"
             " frames; every measurement in a fresh process; median of %d alternated rounds). Flag off = the parent commit's frame." % (FRAMES, WARM, rounds),
             "scene      shape         bones bodies followers |     off      on   added  ratio | rounds"]
    for shape, instances in SHAPES:
        t_us, info = {0: [], 1: []}, {}
        for r in range(rounds):
            for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--one", str(instances), str(on)], timeout=300)
                d = json.loads(out.decode().strip().splitlines()[-1])
                assert (d["followers"] > 0) == bool(on), d
                t_us[on].append(d["us"])
                info[on] = d
        off, on = float(np.median(t_us[0])), float(np.median(t_us[1]))
        lines.append("%-10s %-13s %5d %6d %9d | %7.2f %7.2f %7.2f %6.3f | off %s on %s" % (
            "strands j", shape, info[1]["bones"], info[1]["bodies"], info[1]["followers"], off, on, on - off, on / off,
            " ".join("%.1f" % x for x in t_us[0]), " ".join("%.1f" % x for x in t_us[1])))
        print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
