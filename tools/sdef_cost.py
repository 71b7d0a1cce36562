"""What the SDEF pass (rz_upload_sdef, kernels/sdef.hip) adds to a frame, per workload shape.
  python tools/sdef_cost.py [rounds]     frame time with and without the table, alternated in one process (the tools/ab_inproc.py way):
                                         every round times `FRAMES` frames of each state by rz_time_span (events on the stream, 20 lead
                                         frames); the median round of each state and the difference are printed
  python tools/sdef_cost.py --prof       one rocprofv3 --kernel-trace --stats run of its own (a child process) over frames WITH the table;
                                         prints rz_sdef_kernel's average time per shape against its algorithmic bytes:
                                         SDEF vertices x instances x (36 + 24 + 12 x active dense morphs) B + 40 B per table entry
Shapes: the demo-shaped 28 842-vertex character (sparse morphs) with 10 % SDEF, C3 with 10 %, C4 (256 instances) with 10 %, C5 with 5 %
clustered in runs of 256 vertices as on real meshes."""
import csv
import glob
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import reze_engine_amd as rz  # noqa: E402
from reze_engine_amd import synth  # noqa: E402

FRAMES = 200
SHAPES = [("demo", 28842, 349, 60, 1, 0.10, 0), ("c3", 30000, 200, 64, 1, 0.10, 0), ("c4", 30000, 200, 0, 256, 0.10, 0),
          ("c5", 1000000, 256, 64, 1, 0.05, 256)]


def setup(name, V, B, M, I, frac, cluster):
    if name == "demo":
        mesh = synth.make_mesh(V, B)
        off, idx, d3, mw = synth.make_morphs_demo_shape(V, M)
        dense = None
    else:
        mesh = synth.make_mesh_range(max(V, 30000), B, 0, V)
        dense, mw = synth.make_morphs_dense_range(max(V, 30000), M, 0, V) if M else (None, None)
    table = synth.make_sdef(mesh, frac, cluster=cluster)
    c = rz.DeformContext(0)
    c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
    c.upload_skeleton(mesh["inv_bind"])
    if name == "demo":
        c.upload_morphs_sparse(off, idx, d3)
    elif dense is not None:
        c.upload_morphs_dense(dense)
    if I > 1:
        c.set_instances(I)
        c.set_pose(np.stack([synth.make_pose(mesh["parents"], mesh["bind"], B, seed=1000 + i) for i in range(I)]))
    else:
        c.set_pose(mesh["world"], mw)
    active = 0 if mw is None or name == "demo" else int(np.count_nonzero(mw))      # dense targets with a non-zero weight this frame
    return c, table, active


def put(c, table, on):
    if on:
        c.upload_sdef(table["idx"], table["c"], table["r0"], table["r1"])
    else:
        c.upload_sdef([], [], [], [])


def ab(rounds):
    print("shape   SDEF verts   without us   with us   added us   (median of %d alternated rounds of %d frames, rz_time_span)" % (rounds, FRAMES))
    for name, V, B, M, I, frac, cluster in SHAPES:
        c, table, _ = setup(name, V, B, M, I, frac, cluster)
        t = {0: [], 1: []}
        for r in range(rounds):
            for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                put(c, table, on)
                c.deform_n(4)
                t[on].append(c.time_span(FRAMES, lead=20) / FRAMES * 1e3)
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        print("%-6s %11d %12.2f %9.2f %10.2f   rounds off %s  on %s" % (name, len(table["idx"]), off, on, on - off,
              " ".join("%.2f" % x for x in t[0]), " ".join("%.2f" % x for x in t[1])))
        c.close()


def frames_only():
    for name, V, B, M, I, frac, cluster in SHAPES:
        c, table, _ = setup(name, V, B, M, I, frac, cluster)
        put(c, table, 1)
        c.deform_n(FRAMES)
        c.sync()
        c.close()


def prof():
    d = tempfile.mkdtemp(prefix="sdef_prof_")
    subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sdef", "--",
                           sys.executable, os.path.abspath(__file__), "--frames-only"], timeout=900)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        sys.exit("no kernel trace under %s" % d)
    rows = [r for r in csv.DictReader(open(trace[0])) if "rz_sdef_kernel" in r.get("Kernel_Name", "")]
    durs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    print("rz_sdef_kernel launches: %d (shapes in order %s, %d frames each)" % (len(durs), ",".join(s[0] for s in SHAPES), FRAMES))
    k = 0
    for name, V, B, M, I, frac, cluster in SHAPES:
        c, table, active = setup(name, V, B, M, I, frac, cluster)         # (the same data the child used: seeded)
        c.close()
        mesh_n = len(table["idx"])
        take = durs[k:k + FRAMES]
        k += FRAMES
        nbytes = mesh_n * I * (36 + 24 + 12 * active) + 40 * mesh_n
        if take:
            us = float(np.median(take)) / 1e3
            print("%-6s sdef verts %7d  active dense morphs %3d  kernel median %7.2f us  algorithmic %9.0f B  -> %6.1f GB/s"
                  % (name, mesh_n, active, us, nbytes, nbytes / us / 1e3))


if __name__ == "__main__":
    if "--frames-only" in sys.argv:
        frames_only()
    elif "--prof" in sys.argv:
        prof()
    else:
        ab(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
