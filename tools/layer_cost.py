"""What a layered pose (rz_upload_motion_masks / rz_set_pose_layered) costs beside a blended one (rz_set_pose_blended) on the same build:
the two instantiations of rz_motion_kernel, kernels/motion.hip.
  python tools/layer_cost.py [rounds] [--out FILE]
Shapes: the demo-shaped character (28 842 vertices, 349 bones, 60 sparse morphs) and the C4 crowd (256 x 30 000 vertices, 200 bones).
One measurement, in a FRESH process per shape (this script starts itself again with --child), `rounds` (default 5) alternated rounds, the
median with the spread:
  live loop   one pose call + one frame, 2000 times, by the host's clock (tools/live_loop.py): rz_set_pose_blended (the yardstick, every
              instance cross-fading at 0.5), and rz_set_pose_layered on the same bases with 0, 1 and 4 layers per instance — an override
              layer under a mask of half the bones first, then additive and override layers alternating, weights 0.35 .. 1
Writes profiles/layer_cost.txt (or --out). A measuring process that fails or runs past its time limit ends the run: the file is still
written, with that shape and every later one marked NOT MEASURED YET, nothing more is started on the GPU, and the exit status is 1."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from motion_cost import build, live, med  # noqa: E402


def child(name, rounds):
    import reze_engine_amd as rz
    from reze_engine_amd import capi, synth
    c, clips, I = build(rz, synth, name, None)
    B, M = c.get_tuning("bones"), c.get_tuning("morphs")
    add = synth.make_motion(B, M, seed=104, max_angle=np.pi / 12, n_keys=40, uneven=False, span=6, trans=0.05)
    c.upload_motions(clips + [add])
    rng = np.random.default_rng(1)
    masks = (rng.random((2, B)) < 0.5).astype(np.uint8)
    c.upload_motion_masks(masks, (rng.random((2, M)) < 0.5).astype(np.uint8) if M else None)
    T = 16
    frames = (rng.random((T + 1, I)) * 200.0).astype(np.float32)
    states = np.stack([rz.DeformContext.pack_motion_states(I, rng.integers(0, 3, size=I), frames[t], rng.integers(0, 3, size=I), frames[t + 1], 0.5) for t in range(T)])

    def layers(n):
        ly = np.zeros((T, I, n), dtype=capi.MOTION_LAYER_DTYPE)
        for k in range(n):
            ly["clip"][:, :, k] = 3 if k % 2 else rng.integers(0, 3, size=(T, I))
            ly["mode"][:, :, k] = k % 2
            ly["mask"][:, :, k] = k % 2 if k < 2 else capi.NO_MASK
            ly["weight"][:, :, k] = rng.choice([0.35, 0.6, 1.0], size=(T, I))
            ly["frame"][:, :, k] = rng.random((T, I)) * 200.0
        return ly
    calls = {"blended": c.frame_call("blended", states)}
    for n in (0, 1, 4):
        calls["layers%d" % n] = c.frame_call("layered", (states, layers(n)))
    out = {k: [] for k in calls}
    order = list(calls)
    for r in range(rounds):
        for key in (order if r % 2 == 0 else order[::-1]):
            call, check = calls[key]
            out[key].append(live(c, call, check))
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
    lines = ["tools/layer_cost.py [rounds] writes this file: a layered pose (rz_set_pose_layered) beside a blended one (rz_set_pose_blended) on the same",
             "build and the same cross-fading bases. us per frame, live loop = one pose call + one frame, 2000 times, host clock; median of %d" % rounds,
             "alternated rounds (fastest .. slowest), one fresh process per shape.", ""]
    failed = None
    for name in ("demo", "c4"):
        if failed:                  # a process that used the GPU ended badly: nothing more is started on it, the rest is only marked
            lines.append("%-5s NOT MEASURED YET: not started, the measuring process of %s failed" % (name, failed))
            continue
        cmd = [sys.executable, os.path.abspath(__file__), str(rounds), "--child", name]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
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
        lines += ["%-5s live loop   rz_set_pose_blended %s" % (name, med(r["blended"])),
                  "%-5s live loop   rz_set_pose_layered: 0 layers %s | 1 layer %s | 4 layers %s" % (name, med(r["layers0"]), med(r["layers1"]), med(r["layers4"])), ""]
    text = "\n".join(lines).rstrip() + "\n"
    out = opt.get("--out", os.path.join(ROOT, "profiles", "layer_cost.txt"))
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
