"""What a pose blended out of the device motion library (rz_upload_motions / rz_set_pose_blended, kernels/motion.hip) costs beside a pose
sampled from the single resident motion (rz_upload_animation / rz_set_pose_sampled).
  python tools/motion_cost.py [rounds] [--parent LIB] [--out FILE]
Shapes: the demo-shaped character (28 842 vertices, 349 bones, 60 sparse morphs) and the C4 crowd (256 x 30 000 vertices, 200 bones).
Two measurements, each in a FRESH process per shape (this script starts itself again with --child), `rounds` (default 5) alternated rounds,
the median with the spread:
  replayed frame   rz_time_span over 200 frames of the RESIDENT pose: a blended pose is a local pose, a sampled pose is sampled again by
                   every frame — what the replayed frame costs, a local pose against a sampled one
  live loop        one pose call + one frame, 2000 times, by the host's clock (tools/live_loop.py): rz_set_pose_sampled (the yardstick; with
                   --parent LIB also on a build of the parent commit, which gives its spread), rz_set_pose_blended without a second clip,
                   with blend = 0.5 for every instance, and with half of the instances blending
Writes profiles/motion_cost.txt (or --out). A measuring process that fails or runs past its time limit ends the run: the file is still
written, with that shape and every later one marked NOT MEASURED YET, nothing more is started on the GPU, and the exit status is 1."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FRAMES, LIVE = 200, 2000


def build(rz, synth, name, lib):
    if name == "demo":
        V, B, M, I = 28842, 349, 60, 1
        mesh = synth.make_mesh(V, B)
    else:
        V, B, M, I = 30000, 200, 0, 256
        mesh = synth.make_mesh_range(V, B, 0, V)
    c = rz.DeformContext(0) if lib is None else rz.DeformContext(0, lib=lib)
    c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
    c.upload_skeleton(mesh["inv_bind"])
    c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
    if M:
        c.upload_morphs_sparse(*synth.make_morphs_demo_shape(V, M)[:3])
    if I > 1:
        c.set_instances(I)
    base = synth.make_motion_base(B)
    clips = [synth.make_motion(B, M, seed=100 + k, base=base, n_keys=40, uneven=False, span=6) for k in range(3)]      # baked motions: evenly spaced keys
    return c, clips, I


def live(c, call, check):
    for _ in range(200):
        call()
    c.sync()
    t0 = time.perf_counter()
    for _ in range(LIVE):
        call()
    c.sync()
    dt = (time.perf_counter() - t0) / LIVE * 1e6
    check()
    return dt


def child(name, rounds, parent):
    import reze_engine_amd as rz
    from reze_engine_amd import synth
    c, clips, I = build(rz, synth, name, None)
    c.upload_animation(**clips[0])
    c.upload_motions(clips)
    rng = np.random.default_rng(1)
    T = 16
    frames = (rng.random((T, I)) * 200.0).astype(np.float32)
    pack = rz.DeformContext.pack_motion_states

    def table(kind):
        rows = []
        for t in range(T):
            b = {"alone": None, "blend": rng.integers(0, 3, size=I), "half": np.where(np.arange(I) % 2 == 0, rng.integers(0, 3, size=I), -1)}[kind]
            rows.append(pack(I, rng.integers(0, 3, size=I), frames[t], b, frames[(t + 1) % T], 0.5))
        return np.stack(rows)
    out = {"replay_sampled": [], "replay_blended": [], "live_sampled": [], "live_alone": [], "live_blend": [], "live_half": [], "live_parent": []}
    calls = {"live_sampled": c.frame_call("sampled", frames)}
    for kind in ("alone", "blend", "half"):
        calls["live_" + kind] = c.frame_call("blended", table(kind))
    pc = None
    if parent:
        plib = rz.capi.load(parent)
        pc, pclips, _ = build(rz, synth, name, plib)
        pc.upload_animation(**pclips[0])
        calls["live_parent"] = pc.frame_call("sampled", frames)
    order = list(calls)
    for r in range(rounds):
        for key in (order if r % 2 == 0 else order[::-1]):
            call, check = calls[key]
            out[key].append(live(pc if key == "live_parent" else c, call, check))
        for key in (("replay_sampled", "replay_blended") if r % 2 == 0 else ("replay_blended", "replay_sampled")):
            if key == "replay_sampled":
                c.set_pose_sampled(frames[0])
            else:
                c.set_pose_blended(rng.integers(0, 3, size=I), frames[0], rng.integers(0, 3, size=I), frames[1], 0.5)
            c.deform_n(4)
            out[key].append(c.time_span(FRAMES, lead=20) / FRAMES * 1e3)
    out["kernel_blended"] = c.kernel_name()
    print("RESULT " + json.dumps(out), flush=True)


def med(xs):
    return "%7.2f (%.2f .. %.2f)" % (float(np.median(xs)), min(xs), max(xs)) if xs else "      -"


def main():
    argv = sys.argv[1:]
    opt = {}
    for flag in ("--parent", "--out", "--child"):
        if flag in argv:
            k = argv.index(flag)
            opt[flag] = argv[k + 1]
            del argv[k:k + 2]
    rounds = int(argv[0]) if argv else 5
    if "--child" in opt:
        return child(opt["--child"], rounds, opt.get("--parent"))
    lines = ["tools/motion_cost.py [rounds] [--parent LIB] writes this file: a pose blended out of the device motion library (rz_set_pose_blended)",
             "beside a pose sampled from the single resident motion (rz_set_pose_sampled). us per frame, median of %d alternated rounds (fastest .. slowest)," % rounds,
             "one fresh process per shape. replayed = %d frames of the resident pose by rz_time_span; live = one pose call + one frame, %d times, host clock." % (FRAMES, LIVE), ""]
    failed = None
    for name in ("demo", "c4"):
        if failed:                  # a process that used the GPU ended badly: nothing more is started on it, the rest is only marked
            lines.append("%-5s NOT MEASURED YET: not started, the measuring process of %s failed" % (name, failed))
            continue
        cmd = [sys.executable, os.path.abspath(__file__), str(rounds), "--child", name] + (["--parent", opt["--parent"]] if "--parent" in opt else [])
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            code, so, se = p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:      # run() has killed and reaped the child
            code, so, se = "time limit", e.stdout or b"", b"ran past its time limit"
        res = [ln for ln in so.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
        if code != 0 or not res:
            failed = name
            lines.append("%-5s NOT MEASURED YET: the measuring process failed (exit %s: %s)"
                         % (name, code, (se.decode(errors="replace").strip().splitlines() or ["no output"])[-1][:160]))
            continue
        r = json.loads(res[-1][7:])
        lines += ["%-5s replayed frame   sampled pose %s | blended pose (resident local pose) %s" % (name, med(r["replay_sampled"]), med(r["replay_blended"])),
                  "%-5s live loop        rz_set_pose_sampled %s | parent build %s" % (name, med(r["live_sampled"]), med(r["live_parent"])),
                  "%-5s live loop        rz_set_pose_blended: no second clip %s | blend 0.5 %s | half of the instances blending %s"
                  % (name, med(r["live_alone"]), med(r["live_blend"]), med(r["live_half"])),
                  "%-5s frame kernel behind a blended pose: %s" % (name, r["kernel_blended"]), ""]
    text = "\n".join(lines).rstrip() + "\n"
    out = opt.get("--out", os.path.join(ROOT, "profiles", "motion_cost.txt"))
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
