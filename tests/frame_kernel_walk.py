"""Every arm of the frame kernel's launch switches that the product build carries (csrc/frame_kernel.h; kernels/deform_dense.hip,
deform_small.hip, crowd.hip), once each, on the smallest shapes that still separate the arms. walk(lib) sets one arm up after the other
and yields it BEFORE its frame is launched; the caller launches it (c.deform()). Shared by tests/test_gpu_frame_kernel.py and
tools/frame_kernel_trace.py, which compares a kernel trace of the same walk with the `symbol` column.

One mesh: V = 301 (one whole 256-vertex step, a partial step and a partial last quad), B = 5, I = 1. Crowds: the smallest scene of
tests/crowd_scenes.py and of tests/crowd_morph_scenes.py with I = 3 and inst_loop = 2, so the last pose group is partial.

An arm: name, c (the context, posed), kernel (what kernel_name() must say), symbol (the full demangled symbol: the dense kernel's eighth
argument spelled), family ("one" / "crowd"), and what a reference needs: mesh, worlds [I] (float32 world matrices of the posed
skeleton; float64 for device-solved poses), deltas / mw (dense restatement of the morph targets and the weights per instance, or None),
pose (callable(c, instance or None) that puts the arm's pose, or one instance of it alone, into a context)."""
import numpy as np

import crowd_morph_scenes as cms
import crowd_scenes as cs
from helpers import fk_reference, sample_reference
from reze_engine_amd import synth

V, B, I_CROWD, G_CROWD = 301, 5, 3, 2
RESET = dict(fast=-1, nt_store=-1, fuse_fk=-1, fuse_fk_plain=-1, inst_subsets=-1, inst_block=0, inst_morphs=-1, inst_loop=-1, grid_cap=0)


def _tf(b):
    return "true" if b else "false"


def small(mode, nts, fast, fkv):
    s = "rz_deform_small_kernel<4, %d, %s, false, %s, %d>" % (mode, _tf(nts), _tf(fast), fkv)
    return s, s


def dense(nts, fkv, q24):
    s = "rz_deform_dense_kernel<8, 8, true, %s, false, true, %d" % (_tf(nts), fkv)
    return s + ">", s + ", %s>" % _tf(q24)


def crowd(block, nts, sub, morph=False, fk=False):
    m = "_morph" if morph else ""
    s = "rz_skin_instances_fk%s_kernel<%d, %s>" % (m, block, _tf(nts)) if fk else "rz_skin_instances%s_kernel<%d, %s, %s>" % (m, block, _tf(nts), _tf(sub))
    return s, s


def _one_mesh(lib):
    mesh = synth.make_mesh(V, B, seed=301)
    off, idx, d3, mw3 = synth.make_morphs_sparse(V, 3, density=0.3, seed=302)
    d9, mw9 = synth.make_morphs_dense(V, 9, seed=303)
    edge = (np.random.default_rng(304).random(V, dtype=np.float32) * np.float32(1.5)).astype(np.float32)
    clip = synth.make_motion(B, 0, seed=305, keyed=1.0)
    frame = 7.25
    rng = np.random.default_rng(306)
    q = rng.normal(size=(1, B, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=2, keepdims=True)

    def ctx():
        c = lib.DeformContext(0)
        c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
        c.upload_skeleton(mesh["inv_bind"])
        return c

    def world_pose(mw):
        return lambda c, inst=None: c.set_pose(mesh["world"], mw)

    base = dict(family="one", mesh=mesh, worlds=[mesh["world"]], deltas=None, mw=None, edge=None)
    # world poses: no morphs / 3 sparse / 9 dense in fp32 and in 24-bit storage, each without (FKV 3) and with the outline hull (FKV 0)
    for what, mode, targets in (("no morphs", 0, None), ("3 sparse morphs", 2, "sparse"), ("9 dense morphs fp32", 1, "f32"), ("9 dense morphs 24-bit", 1, "q24")):
        with ctx() as c:
            deltas = mw = None
            if targets == "sparse":
                c.upload_morphs_sparse(off, idx, d3)
                deltas, mw = synth.sparse_to_dense(V, off, idx, d3), mw3
            elif targets:
                c.upload_morphs_dense(d9, storage=lib.capi.MORPH_F32 if targets == "f32" else None)
                assert c.get_tuning("effective_morph_storage") == (32 if targets == "f32" else 24)
                # (the reference reads the targets as they are resident: 24-bit storage is held to its own bar by tests/test_gpu_morph_storage.py)
                deltas, mw = np.ascontiguousarray(np.stack([c.read_morph_dense(m) for m in range(9)]).transpose(0, 2, 1)), mw9
            for hull in (False, True):
                if hull:
                    c.upload_edge_scale(edge)
                world_pose(mw)(c)
                k, s = dense(False, 0 if hull else 3, targets == "q24") if mode == 1 else small(mode, False, True, 0 if hull else 3)
                yield dict(base, name="one mesh, %s, hull %s" % (what, "on" if hull else "off"), c=c, kernel=k, symbol=s, deltas=deltas,
                           mw=None if mw is None else mw[None], edge=edge if hull else None, pose=world_pose(mw))
    # streaming stores on and off (no morphs, world pose)
    with ctx() as c:
        for nts in (0, 1):
            c.set_tuning(nt_store=nts)
            world_pose(None)(c)
            k, s = small(0, nts, True, 3)
            yield dict(base, name="one mesh, nt_store = %d" % nts, c=c, kernel=k, symbol=s, pose=world_pose(None))
    # device-solved poses (the frame is not the one-launch form): a local pose fused with the specialised solve (FKV 1) and with the generic
    # one ("fuse_fk_plain" = 0: FKV 3), a sampled pose (FKV 2)
    with ctx() as c:
        c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
        c.upload_animation(**clip)
        w_local = fk_reference(mesh["parents"], mesh["bind"], q[0])
        qs, ts, _ = sample_reference(clip, frame, B, 0)
        w_sampled = fk_reference(mesh["parents"], mesh["bind"], qs, ts)
        put_local = lambda c, inst=None: c.set_pose_local(q)            # noqa: E731
        put_sampled = lambda c, inst=None: c.set_pose_sampled(np.array([frame], dtype=np.float32))      # noqa: E731
        for what, put, plain, world, fkv in (("local pose, fused", put_local, -1, w_local, 1), ("sampled pose, fused", put_sampled, -1, w_sampled, 2),
                                             ("local pose, fuse_fk_plain = 0", put_local, 0, w_local, 3)):
            c.set_tuning(fuse_fk_plain=plain)
            put(c)
            k, s = small(0, False, False, fkv)
            yield dict(base, name="one mesh, " + what, c=c, kernel=k, symbol=s, worlds=[world], pose=put)


def _crowds(lib):
    # ---- no morphs: the smallest scene of tests/crowd_scenes.py, its first three poses ----
    sc = cs.scene(cs.NAMES[0])
    m, Bc = sc["mesh"], sc["B"]
    q, lt = sc["q"][:I_CROWD], sc["lt"][:I_CROWD]
    w64 = [fk_reference(sc["parents"], sc["bind"], q[i], lt[i], sc["ap"], sc["ratio"], sc["mv"]) for i in range(I_CROWD)]
    w32 = np.stack([w.reshape(Bc, 16).astype(np.float32) for w in w64])
    mesh = dict(m, inv_bind=sc["inv_bind"])
    base = dict(family="crowd", mesh=mesh, deltas=None, mw=None, edge=None)

    def put_world(c, inst=None):
        c.set_pose(w32 if inst is None else w32[inst])

    def put_local(c, inst=None):
        c.set_pose_local(q if inst is None else q[inst:inst + 1], None, lt if inst is None else lt[inst:inst + 1])

    c = lib.DeformContext(0)
    with c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(sc["inv_bind"])
        c.upload_skeleton_topology(sc["parents"], sc["bind"], sc["ap"], sc["ratio"], sc["mv"])
        c.set_instances(I_CROWD)
        shape = dict(inst_loop=G_CROWD, grid_cap=2 * ((I_CROWD + G_CROWD - 1) // G_CROWD))
        for block in (256, 512):
            for sub in (1, 0):
                for fast in (0, 1):
                    c.set_tuning(**dict(RESET, inst_block=block, inst_subsets=sub, fast=fast, **shape))
                    put_world(c)
                    k, s = crowd(block, False, sub)
                    yield dict(base, name="crowd, block %d, inst_subsets = %d, fast = %d" % (block, sub, fast), c=c, kernel=k, symbol=s, worlds=list(w32), pose=put_world)
            c.set_tuning(**dict(RESET, inst_block=block, **shape))
            put_local(c)
            k, s = crowd(block, False, True, fk=True)
            yield dict(base, name="crowd, block %d, the fk front" % block, c=c, kernel=k, symbol=s, worlds=w64, pose=put_local)
    # ---- sparse morphs in the crowd kernels: the smallest scene of tests/crowd_morph_scenes.py, its first three poses ----
    s_ = cms.scene(cms.NAMES[0])
    m = s_["mesh"]
    deltas = synth.sparse_to_dense(cms.V, s_["off"], s_["idx"], s_["d3"])
    mw = s_["mw"][:I_CROWD]
    base = dict(family="crowd", mesh=m, deltas=deltas, mw=mw, edge=None)
    wl64 = [fk_reference(m["parents"], m["bind"], m["q"][i]) for i in range(I_CROWD)]

    def put_world_m(c, inst=None):
        c.set_pose(m["worlds"][:I_CROWD], mw) if inst is None else c.set_pose(m["worlds"][inst], mw[inst:inst + 1])

    def put_local_m(c, inst=None):
        c.set_pose_local(m["q"][:I_CROWD], mw) if inst is None else c.set_pose_local(m["q"][inst:inst + 1], mw[inst:inst + 1])

    c = lib.DeformContext(0)
    with c:
        c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
        c.upload_skeleton(m["inv_bind"])
        c.upload_skeleton_topology(m["parents"], m["bind"])
        c.upload_morphs_sparse(s_["off"], s_["idx"], s_["d3"])
        c.set_instances(I_CROWD)
        shape = dict(inst_loop=G_CROWD, grid_cap=cms.RUNS * ((I_CROWD + G_CROWD - 1) // G_CROWD), inst_morphs=1)
        for block in (256, 512):
            for sub in (1, 0):
                c.set_tuning(**dict(RESET, inst_block=block, inst_subsets=sub, fast=1, **shape))
                put_world_m(c)
                k, s = crowd(block, False, sub, morph=True)
                yield dict(base, name="crowd with sparse morphs, block %d, inst_subsets = %d" % (block, sub), c=c, kernel=k, symbol=s,
                           worlds=list(m["worlds"][:I_CROWD]), pose=put_world_m)
            c.set_tuning(**dict(RESET, inst_block=block, **shape))
            put_local_m(c)
            k, s = crowd(block, False, True, morph=True, fk=True)
            yield dict(base, name="crowd with sparse morphs, block %d, the fk front" % block, c=c, kernel=k, symbol=s, worlds=wl64, pose=put_local_m)


def walk(lib):
    yield from _one_mesh(lib)
    yield from _crowds(lib)
