"""What the QDEF pass (rz_upload_qdef, kernels/qdef.hip) adds to a frame, per workload shape.
  python tools/qdef_cost.py [rounds] [--parent LIB] [--out FILE]
      frame time with and without the table, alternated in one process (the tools/ab_inproc.py way): every round times `FRAMES` frames
      of each state by rz_time_span (events on the stream, 20 lead frames); the median round of each state and the difference are
      printed — the table "on" once per value of "qdef_chunks" (256-vertex chunks one workgroup takes behind one conversion of the
      skeleton). Then the largest device error against tests/qdef_ref.py per shape (the listed vertices, in units of the tests' bar; the
      vertices whose sign margin is under qdef_ref.AMBIGUOUS are counted apart). --parent LIB also times the frame WITHOUT a table with
      another build of the library (the parent commit's) in the same rounds: reported, not gated. --out FILE (default
      profiles/qdef_cost.txt) takes a copy of everything printed.
Shapes: the demo-shaped 28 842-vertex character (sparse morphs) with 10 % QDEF, C3 with 10 % scattered and 10 % clustered in runs of 256
vertices (as on real meshes: forearms, shoulders, thighs), C4 (256 instances) with 10 %, C5 with 5 % clustered."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import reze_engine_amd as rz  # noqa: E402
from reze_engine_amd import synth  # noqa: E402

FRAMES = 200
CHUNKS = (1, 2, 4)
SHAPES = [("demo", 28842, 349, 60, 1, 0.10, 0), ("c3", 30000, 200, 64, 1, 0.10, 0), ("c3-clu", 30000, 200, 64, 1, 0.10, 256),
          ("c4", 30000, 200, 0, 256, 0.10, 0), ("c5-clu", 1000000, 256, 64, 1, 0.05, 256)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def data(name, V, B, M, I, frac, cluster):
    d = dict(I=I, sparse=None, dense=None, mw=None)
    if name == "demo":
        d["mesh"] = synth.make_mesh(V, B)
        off, idx, d3, mw = synth.make_morphs_demo_shape(V, M)
        d["sparse"], d["mw"] = (off, idx, d3), mw
    else:
        d["mesh"] = synth.make_mesh_range(max(V, 30000), B, 0, V)
        if M:
            d["dense"], d["mw"] = synth.make_morphs_dense_range(max(V, 30000), M, 0, V)
    m = d["mesh"]
    d["table"] = synth.make_qdef(m, frac, cluster=cluster)
    d["world"] = np.stack([synth.make_pose(m["parents"], m["bind"], B, seed=1000 + i) for i in range(I)]) if I > 1 else m["world"]
    return d


def context(d, lib=None):
    m = d["mesh"]
    c = rz.DeformContext(0, lib=lib)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(m["inv_bind"])
    if d["sparse"] is not None:
        c.upload_morphs_sparse(*d["sparse"])
    elif d["dense"] is not None:
        c.upload_morphs_dense(d["dense"])
    if d["I"] > 1:
        c.set_instances(d["I"])
        c.set_pose(d["world"])
    else:
        c.set_pose(d["world"], d["mw"])
    return c


def device_error(c, d):
    """Largest position / normal error of the listed vertices against qdef_ref, in units of the tests' bar, over the sure vertices; and the
    count of ambiguous ones."""
    import qdef_ref
    from helpers import NRM_TOL, POS_TOL, parity_errors
    from oracle import rz_oracle_np as onp
    m, idx = d["mesh"], d["table"].astype(np.int64)
    worst_p = worst_n = 0.0
    amb = 0
    for inst in sorted({0, d["I"] - 1}):
        pos, nrm = c.read(inst)
        skin16 = onp.palette(c.read_world(inst), m["inv_bind"])
        pm = m["pos"][idx]
        if d["I"] == 1 and d["dense"] is not None:
            pm = onp.morph_dense(np.ascontiguousarray(d["dense"][:, idx]), d["mw"], pm)
        elif d["I"] == 1 and d["sparse"] is not None:
            off, vi, d3 = d["sparse"]
            pm = onp.morph_sparse(len(m["pos"]), off, vi, d3, d["mw"], m["pos"])[idx]
        sub = np.arange(len(idx))
        P, N = qdef_ref.qdef(pm, m["nrm"][idx], m["joints"][idx], m["weights"][idx], skin16, sub)
        sure = qdef_ref.margin(m["joints"][idx], m["weights"][idx], skin16, sub) >= qdef_ref.AMBIGUOUS
        ep, en = parity_errors(pos[idx], nrm[idx], P, N)
        worst_p, worst_n = max(worst_p, float(ep[sure].max()) / POS_TOL), max(worst_n, float(en[sure].max()) / NRM_TOL)
        amb = max(amb, int((~sure).sum()))
    return worst_p, worst_n, amb


def ab(rounds, parent):
    states = ["off"] + ["on/%d" % k for k in CHUNKS] + (["parent"] if parent is not None else [])
    say("shape    QDEF verts  " + "  ".join("%9s" % s for s in states) + "   added us per chunks %s   (us per frame: median of %d alternated rounds of %d frames, rz_time_span)"
        % ("/".join(str(k) for k in CHUNKS), rounds, FRAMES))
    errs = []
    for shape in SHAPES:
        d = data(*shape)
        c = context(d)
        cp = context(d, lib=parent) if parent is not None else None
        t = {s: [] for s in states}
        for r in range(rounds):
            for s in (states if r % 2 == 0 else states[::-1]):
                if s == "parent":
                    cp.deform_n(4)
                    t[s].append(cp.time_span(FRAMES, lead=20) / FRAMES * 1e3)
                    continue
                c.upload_qdef(d["table"] if s != "off" else [])
                c.set_tuning(qdef_chunks=int(s[3:]) if s != "off" else 0)
                c.deform_n(4)
                t[s].append(c.time_span(FRAMES, lead=20) / FRAMES * 1e3)
        med = {s: float(np.median(t[s])) for s in states}
        say("%-8s %10d  " % (shape[0], len(d["table"])) + "  ".join("%9.2f" % med[s] for s in states) + "   "
            + " / ".join("%.2f" % (med["on/%d" % k] - med["off"]) for k in CHUNKS)
            + "   rounds " + "  ".join("%s %s" % (s, " ".join("%.2f" % x for x in t[s])) for s in states))
        c.upload_qdef(d["table"])
        c.set_tuning(qdef_chunks=0)
        c.deform()
        errs.append((shape[0],) + device_error(c, d))
        c.close()
        if cp is not None:
            cp.close()
    say("")
    say("largest device error of the listed vertices against tests/qdef_ref.py, in units of the bar (helpers.POS_TOL / NRM_TOL = 1e-4):")
    for name, ep, en, amb in errs:
        say("%-8s position %.3f  normal %.3f   (%d ambiguous vertices, held apart)" % (name, ep, en, amb))


if __name__ == "__main__":
    args = sys.argv[1:]
    parent, out = None, os.path.join(ROOT, "profiles", "qdef_cost.txt")
    if "--parent" in args:
        k = args.index("--parent")
        parent = rz.capi.load(args[k + 1])
        del args[k:k + 2]
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    say("# tools/qdef_cost.py on one MI355X")
    say("")
    ab(int(args[0]) if args else 5, parent)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
