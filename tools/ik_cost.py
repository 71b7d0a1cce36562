"""What the IK stage (rz_upload_ik, kernels/ik.hip.h: rz_fk_kernel<RzIkParams> instead of the fused / one-launch hierarchy solve) adds to a
device-animated frame, and how far the device solve is from the float64 restatement (tests/ik_ref.py).
  python tools/ik_cost.py [rounds] [--parent LIB]
Shapes: the demo-shaped 28 842-vertex character (sparse morphs, an uploaded local pose) and C4 as a sampled crowd (256 characters, each at
its own frame of one motion), both with the 14-bone leg rig of synth.make_leg_rig grafted under bone 0 and its four chains; each with the
goals in reach and out of reach (the worst case: every chain runs all its iterations). Per shape and state `rounds` (default 5) alternated
rounds of 200 frames are timed by rz_time_span (events on the stream, 20 lead frames); the median round is printed with the spread.
--parent LIB names a build of the parent commit (same ABI, no rz_upload_ik): its frame is timed twice in the same process, which gives the
no-table comparison and the run-to-run spread a no-table frame of this build has to stay within."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402

import ik_ref  # noqa: E402
import reze_engine_amd as rz  # noqa: E402
from helpers import sample_reference  # noqa: E402
from reze_engine_amd import synth  # noqa: E402

FRAMES = 200


def graft(mesh):
    """the mesh's skeleton with the leg rig appended under bone 0; vertices keep their bones. Returns (mesh', rig bone offset, chains)."""
    rig = synth.make_leg_rig()
    B0 = len(mesh["parents"])
    rp = rig["parents"].copy()
    rp[rp >= 0] += B0
    rp[0] = 0
    m = dict(mesh)
    m["parents"] = np.concatenate([mesh["parents"], rp]).astype(np.int32)
    m["bind"] = np.concatenate([mesh["bind"], rig["bind"]]).astype(np.float32)
    m["quats"] = np.concatenate([mesh["quats"], rig["quats"]]).astype(np.float32)
    m["inv_bind"] = synth.inverse_bind_translation_only(m["parents"], m["bind"])
    chains = [dict(goal=ch["goal"] + B0, effector=ch["effector"] + B0, loops=ch["loops"], limit_angle=ch["limit_angle"],
                   links=[dict(ln, bone=ln["bone"] + B0) for ln in ch["links"]]) for ch in rig["chains"]]
    return m, B0, chains, rig


def rig_pose(mesh, B0, rig, seed, reach):
    q = mesh["quats"].copy()
    t = np.zeros((len(q), 3), dtype=np.float32)
    rq, rt = synth.leg_rig_pose(rig, seed, reach=reach)
    q[B0:], t[B0:] = rq, rt
    return q, t


def motion(B0, rig, reach, nk=8, seed=4):
    """keys for the rig's centre and goals (positions from leg_rig_pose, so `reach` holds at the keys)"""
    bones = np.array([1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13], dtype=np.int32)
    kq = np.zeros((len(bones), nk, 4), dtype=np.float32)
    kp = np.zeros((len(bones), nk, 3), dtype=np.float32)
    for k in range(nk):
        q, t = synth.leg_rig_pose(rig, seed * 100 + k, reach=reach)
        kq[:, k], kp[:, k] = q[bones], t[bones]
    n = len(bones)
    return dict(track_bone=(bones + B0).astype(np.int32), key_off=(np.arange(n + 1) * nk).astype(np.uint32),
                key_frame=np.tile((np.arange(nk) * 6).astype(np.float32), n), key_rot=kq.reshape(-1, 4), key_pos=kp.reshape(-1, 3), key_interp=None)


def build(name, lib, reach):
    if name == "demo":
        mesh = synth.make_mesh(28842, 349)
        off, idx, d3, mw = synth.make_morphs_demo_shape(28842, 60)
    else:
        mesh = synth.make_mesh_range(30000, 200, 0, 30000)
    mesh, B0, chains, rig = graft(mesh)
    c = rz.DeformContext(0) if lib is None else rz.DeformContext(0, lib=lib)
    c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
    c.upload_skeleton(mesh["inv_bind"])
    c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
    if name == "demo":
        c.upload_morphs_sparse(off, idx, d3)
        q, t = rig_pose(mesh, B0, rig, 7, reach)
        c.set_pose_local(q, mw, t)
        poses = [(q, t)]
    else:
        I = 256
        c.set_instances(I)
        anim = motion(B0, rig, reach)
        c.upload_animation(anim["track_bone"], anim["key_off"], anim["key_frame"], anim["key_rot"], anim["key_pos"], None)
        frames = np.linspace(0.0, 42.0, I).astype(np.float32)
        c.set_pose_sampled(frames)
        poses = []
        for f in frames[::16]:
            q, t, _ = sample_reference(anim, float(f), len(mesh["parents"]), 0)
            poses.append((q, t))
    return c, mesh, chains, poses


def span(c):
    c.deform_n(4)
    return c.time_span(FRAMES, lead=20) / FRAMES * 1e3


def errors(c, mesh, chains, poses, stride):
    ext = ik_ref.extent(ik_ref.bind_positions(mesh["parents"], mesh["bind"]))
    e = []
    for k, (q, t) in enumerate(poses):
        w64, _ = ik_ref.solve(mesh["parents"], mesh["bind"], q, t, chains)
        e.append(np.abs(c.read_world(k * stride).astype(np.float64) - w64).reshape(-1) / ext)
    e = np.concatenate(e)
    return float(e.max()), float(np.percentile(e, 99.9))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    if parent in args:
        args.remove(parent)
    rounds = int(args[0]) if args else 5
    plib = rz.capi.load(parent) if parent else None
    print("frame time in us: median of %d alternated rounds of %d frames (rz_time_span); device error of the world matrices against the float64"
          " restatement in units of the skeleton's extent" % (rounds, FRAMES))
    print("shape goals        without   with    added   | parent build, two runs (spread)   | world error max / p99.9")
    for name in ("demo", "c4"):
        for reach, tag in (((0.3, 0.9), "in reach"), ((1.05, 1.4), "out of reach")):
            c, mesh, chains, poses = build(name, None, reach)
            t = {0: [], 1: []}
            for r in range(rounds):
                for on in ((0, 1) if r % 2 == 0 else (1, 0)):
                    c.upload_ik(chains if on else [])
                    t[on].append(span(c))
            c.upload_ik(chains)
            c.deform()
            emax, e999 = errors(c, mesh, chains, poses, 1 if name == "demo" else 16)
            c.close()
            ptxt = "-"
            if plib is not None:
                runs = []
                for _ in range(2):
                    pc, _, _, _ = build(name, plib, reach)
                    runs.append(float(np.median([span(pc) for _ in range(rounds)])))
                    pc.close()
                ptxt = "%.2f %.2f (%.2f)" % (runs[0], runs[1], abs(runs[0] - runs[1]))
            off, on = float(np.median(t[0])), float(np.median(t[1]))
            print("%-5s %-12s %7.2f %7.2f %7.2f   | %-32s | %.2e / %.2e   rounds off %s on %s"
                  % (name, tag, off, on, on - off, ptxt, emax, e999, " ".join("%.2f" % x for x in t[0]), " ".join("%.2f" % x for x in t[1])))


if __name__ == "__main__":
    main()
