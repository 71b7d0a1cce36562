"""What the per-instance IK chain switches (rz_set_ik_enabled; rz_fk_kernel<RzIkParams, RzIkSwitchParams> instead of rz_fk_kernel<RzIkParams>) cost and save in a live frame.
  python tools/ik_switch_cost.py [rounds]          (writes profiles/ik_switch_cost.txt)
The loop a live application runs: a new local pose (rz_set_pose_local) and the frame (rz_deform), on synth.make_leg_rig (14 bones, four
chains in two stages, 3000 vertices) for one character and for a crowd of 256, under three masks: all on (the parent commit's kernel: a mask
of all ones launches rz_fk_kernel<RzIkParams>), half the instances all off (one character: the two leg chains off, the toe chains on), every
instance all off. Every measurement runs in a fresh process (this script starts itself with `--one`), `rounds` (default 5) rounds alternate
the order of the three masks, the median is printed with every round beside it. One measurement: warm-up frames, then FRAMES frames by the
host's clock around a drained stream. No bar is set: this is a record of what a skipped chain and a skipped stage save."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FRAMES, WARM = 400, 40
SHAPES = (("character", 1), ("crowd of 256", 256))
MASKS = ("all on", "half off", "all off")
OUT = os.path.join(ROOT, "profiles", "ik_switch_cost.txt")


def one(instances, mask):
    """one fresh process: us per live frame, and the bits that were off"""
    import reze_engine_amd as rz
    from reze_engine_amd import synth
    m = synth.make_leg_rig(n_verts=3000)
    poses = [[synth.leg_rig_pose(m, 100 * k + i) for i in range(instances)] for k in range(4)]
    q = [np.stack([p[0] for p in ps]) for ps in poses]
    t = [np.stack([p[1] for p in ps]) for ps in poses]
    on = np.ones((instances, 4), dtype=np.uint8)
    if mask == 1:
        if instances == 1:
            on[0, [0, 2]] = 0           # the leg chains (chains ascend by goal: leg L, toe L, leg R, toe R)
        else:
            on[::2] = 0
    elif mask == 2:
        on[:] = 0
    with rz.DeformContext(0) as c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        if instances > 1:
            c.set_instances(instances)
        c.upload_ik(m["chains"])
        c.set_ik_enabled(on)

        def frames(n):
            for k in range(n):
                c.set_pose_local(q[k % 4], None, t[k % 4])
                c.deform()
            c.sync()
        frames(WARM)
        t0 = time.perf_counter()
        frames(FRAMES)
        us = (time.perf_counter() - t0) / FRAMES * 1e6
        print(json.dumps(dict(us=us, off=c.get_tuning("ik_switched"), chains=c.get_tuning("ik_chains"), stages=c.get_tuning("ik_stages"))))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(int(sys.argv[2]), int(sys.argv[3]))
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lines = ["live frame (rz_set_pose_local + rz_deform) in us (host clock over %d frames around a drained stream, after %d warm-up frames; every"
             " measurement in a fresh process; median of %d alternated rounds). All on = the solve without the switch stage (rz_fk_kernel<RzIkParams>)." % (FRAMES, WARM, rounds),
             "scene    shape         chains stages | all on  half off (bits)  all off (bits) | rounds"]
    for shape, instances in SHAPES:
        t_us, info = {k: [] for k in range(3)}, {}
        for r in range(rounds):
            for k in ((0, 1, 2) if r % 2 == 0 else (2, 1, 0)):
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--one", str(instances), str(k)], timeout=300)
                d = json.loads(out.decode().strip().splitlines()[-1])
                assert (d["off"] > 0) == (k > 0), d
                t_us[k].append(d["us"])
                info[k] = d
        med = [float(np.median(t_us[k])) for k in range(3)]
        lines.append("%-8s %-13s %6d %6d | %6.2f  %8.2f (%4d)  %7.2f (%4d) | %s" % (
            "leg rig", shape, info[0]["chains"], info[0]["stages"], med[0], med[1], info[1]["off"], med[2], info[2]["off"],
            "  ".join("%s %s" % (MASKS[k], " ".join("%.1f" % x for x in t_us[k])) for k in range(3))))
        print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
