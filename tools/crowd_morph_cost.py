"""What a crowd with sparse morph targets costs on the crowd skin kernels ("inst_morphs" = 1: the MORPH instantiations of
kernels/crowd.hip, compiled in kernels/crowd_morph.hip) beside the frame it launches with the key off — rz_deform_small_kernel once per
instance, the frame of the parent commit — on the same build, in the same process.
  python tools/crowd_morph_cost.py [rounds] [--out FILE]
Shapes: the demo-shaped character (synth.make_morphs_demo_shape: 28 842 vertices, 349 bones, 60 sparse morphs, 36 397 entries on a
1 800-vertex face) at I = 256 and I = 32, and the C4 mesh (30 000 vertices, 200 bones) with the same targets at I = 256. Poses: a
resident world pose (rz_set_pose, every instance its own matrices and weights) and a blended device pose (rz_set_pose_blended out of a
three-clip library that keys morph tracks). One FRESH process per shape (this script starts itself again with --child); in it the key
goes 0 / 1 in alternated rounds (default 5), each round FRAMES replayed frames of the resident pose behind warmed-up shapes, timed by
rz_time_span's event pair on the stream; the median of the rounds with their spread. Beside the times: the launched form, and the
ALGORITHMIC bytes of both forms computed from the shapes — written once, I x V x 24 B, by both; read per pose (key off) or per pose
group (key on): V x 40 B of mesh and row pointers + E x 16 B of entries; and per pose B x 48 B of palette rows and M x 4 B of weights.
Writes profiles/crowd_morph_cost.txt (or --out). A measuring process that fails or runs past its time limit ends the run: the file is
still written, with that shape and every later one marked NOT MEASURED YET, nothing more is started on the GPU, and the exit status is 1."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FRAMES = 100
SHAPES = {"demo256": ("demo", 256), "demo32": ("demo", 32), "c4": ("c4", 256)}


def med(xs):
    return "%8.2f (%.2f .. %.2f)" % (float(np.median(xs)), min(xs), max(xs)) if xs else "       -"


def algorithmic_bytes(V, E, B, M, I, G):
    """(key off, key on) bytes of one frame, from the shapes alone"""
    written = I * V * 24
    per_pose = B * 48 + M * 4
    mesh = V * 40 + E * 16
    groups = (I + G - 1) // G if G else I
    return written + I * (mesh + per_pose), written + groups * mesh + I * per_pose


def child(name, rounds):
    import reze_engine_amd as rz
    from reze_engine_amd import synth
    kind, I = SHAPES[name]
    if kind == "demo":
        V, B, M = 28842, 349, 60
        mesh = synth.make_mesh(V, B)
    else:
        V, B, M = 30000, 200, 60
        mesh = synth.make_mesh_range(V, B, 0, V)
    off, idx, d3, _ = synth.make_morphs_demo_shape(V, M)
    c = rz.DeformContext(0)
    c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
    c.upload_skeleton(mesh["inv_bind"])
    c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
    c.upload_morphs_sparse(off, idx, d3)
    c.set_instances(I)
    base = synth.make_motion_base(B)
    clips = [synth.make_motion(B, M, seed=100 + k, base=base, n_keys=40, uneven=False, span=6) for k in range(3)]
    c.upload_motions(clips)
    rng = np.random.default_rng(1)
    poses = np.stack([synth.make_pose(mesh["parents"], mesh["bind"], B, 500 + k) for k in range(16)])       # 16 distinct poses, dealt round
    worlds = poses[np.arange(I) % 16]
    mw = rng.random((I, M), dtype=np.float32)
    mw[rng.random((I, M)) < 0.5] = 0.0                          # a face at rest half of the time
    frames = (rng.random((2, I)) * 200.0).astype(np.float32)
    ca, cb = rng.integers(0, 3, size=I), rng.integers(0, 3, size=I)

    def put(pose):
        if pose == "world":
            c.set_pose(worlds, mw)
        else:
            c.set_pose_blended(ca, frames[0], cb, frames[1], 0.5)
    out = {"V": V, "B": B, "M": M, "I": I, "E": int((idx < V).sum())}
    ref = {}
    for pose in ("world", "blended"):
        t = {0: [], 1: []}
        form = {}
        for r in range(rounds + 1):                             # round 0 warms both shapes up, untimed
            for key in ((0, 1) if r % 2 == 0 else (1, 0)):
                c.set_tuning(inst_morphs=key)
                put(pose)
                c.deform_n(8)
                ms = c.time_span(FRAMES, lead=20)
                if r:
                    t[key].append(ms / FRAMES * 1e3)
                if key not in form:
                    g = c.get_tuning
                    form[key] = dict(kernel=c.kernel_name(), morphs=g("effective_inst_morphs"), group=g("effective_inst_group"), block=g("effective_inst_block"),
                                     lds=g("effective_inst_lds"), grid=g("effective_grid"), one_launch=g("effective_fuse_fk"), front=g("effective_prep"))
                    p, n = c.read(I - 1)
                    if key == 0:
                        ref[pose] = (p, n)
                    else:
                        form[key]["same_bits"] = bool(np.array_equal(p, ref[pose][0]) and np.array_equal(n, ref[pose][1]))
        out[pose] = {"us": {str(k): v for k, v in t.items()}, "form": {str(k): v for k, v in form.items()}}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    argv = sys.argv[1:]
    opt = {}
    for flag in ("--out", "--child"):
        if flag in argv:
            k = argv.index(flag)
            opt[flag] = argv[k + 1]
            del argv[k:k + 2]
    rounds = int(argv[0]) if argv else 5
    if "--child" in opt:
        return child(opt["--child"], rounds)
    lines = ["tools/crowd_morph_cost.py [rounds] writes this file: a crowd with sparse morph targets on the crowd skin kernels (inst_morphs = 1) beside the",
             "frame it launches with the key off (rz_deform_small_kernel once per instance: the parent commit's frame), same build, same process.",
             "us per replayed frame of a resident pose, rz_time_span event spans of %d frames behind warmed-up shapes; median of %d alternated rounds" % (FRAMES, rounds),
             "(fastest .. slowest); one fresh process per shape. MB = algorithmic bytes of the form, computed from the shapes (nothing measured).", ""]
    failed = None
    for name in SHAPES:
        if failed:                  # a process that used the GPU ended badly: nothing more is started on it, the rest is only marked
            lines.append("%-8s NOT MEASURED YET: not started, the measuring process of %s failed" % (name, failed))
            continue
        cmd = [sys.executable, os.path.abspath(__file__), str(rounds), "--child", name]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
            code, so, se = p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:      # run() has killed and reaped the child
            code, so, se = "time limit", e.stdout or b"", b"ran past its time limit"
        res = [ln for ln in so.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
        if code != 0 or not res:
            failed = name
            lines.append("%-8s NOT MEASURED YET: the measuring process failed (exit %s: %s)"
                         % (name, code, (se.decode(errors="replace").strip().splitlines() or ["no output"])[-1][:160]))
            continue
        r = json.loads(res[-1][7:])
        lines.append("%-8s %d vertices, %d bones, %d morphs, %d entries, I = %d" % (name, r["V"], r["B"], r["M"], r["E"], r["I"]))
        for pose in ("world", "blended"):
            f0, f1 = r[pose]["form"]["0"], r[pose]["form"]["1"]
            b0, b1 = algorithmic_bytes(r["V"], r["E"], r["B"], r["M"], r["I"], f1["group"])
            m0, m1 = float(np.median(r[pose]["us"]["0"])), float(np.median(r[pose]["us"]["1"]))
            lines += ["  %-7s pose  key off  %s us  %6.1f MB  %s, grid %d x %d" % (pose, med(r[pose]["us"]["0"]), b0 / 1e6, f0["kernel"], f0["grid"], r["I"]),
                      "  %-7s pose  key on   %s us  %6.1f MB  %s, %d poses per group, %d B of LDS, %d runs; walks rows %d, one launch %d, front kernel %d, same bits %s"
                      % (pose, med(r[pose]["us"]["1"]), b1 / 1e6, f1["kernel"], f1["group"], f1["lds"], f1["grid"], f1["morphs"], f1["one_launch"], f1["front"], f1.get("same_bits")),
                      "  %-7s pose  key on / key off = %.2f" % (pose, m1 / m0)]
        lines.append("")
    text = "\n".join(lines).rstrip() + "\n"
    out = opt.get("--out", os.path.join(ROOT, "profiles", "crowd_morph_cost.txt"))
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
