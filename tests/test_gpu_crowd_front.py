"""The crowd kernel's fused hierarchy front (kernels/crowd.hip: rz_skin_instances_fk_kernel, over the closure records of plan.cpp:
ensure_subfk) at the edges of its launch shape, on the scenes of tests/crowd_scenes.py: 0, 1, 2 and 3 doubling rounds and the chain of
65 bones that falls back; (pose, closure slot) items at, under and over two per thread for 256 and 512 threads; the LDS budget at 1024
threads; tail groups whose second items are all dead; padding records; a closure of 17 / 64 bones of which one has a palette slot; append
parents outside the closure, uploaded and sampled. Everything goes through the C ABI (ctypes).

Every scene, with "fuse_fk" = -1 and then 0: the launched form is the one tests/test_crowd_scenes_cpu.py works out from the scene's arrays;
the fused frame equals the two-launch frame (rz_fk_kernel + skin kernel) bit for bit on every instance, and so do three replays; and both
sit within the bars of the float64 definition — helpers.fk_reference (behind helpers.sample_reference for the sampled scene), then the
oracle's skin. Positions and normals are the only outputs that see the front: world matrices read back after a fused frame come from
rz_fk_kernel, run on demand.

Bars, none of them new. Positions 1e-4 x max(1, L // 8) relative to max(|ref|, 1), L = bones of the longest chain: the rule rz_fk_kernel is
held to at depth 64 (tests/test_gpu_round4.py: test_pointer_doubling_hierarchy_solve), and the front must reproduce its bits. Normals
2e-4 x max(1, L // 8): the bar of test_crowd_hierarchy_solved_in_the_skin_kernel. The sampled scene: helpers.POS_TOL / NRM_TOL, the bars
of tests/test_gpu_sampler.py. Every test prints the launched form and its worst errors before it asserts (profiles/crowd_front_edges_parity.txt)."""
import numpy as np
import pytest

import crowd_scenes as cs
from helpers import NRM_TOL, POS_TOL, fk_reference, parity_errors, sample_reference

pytestmark = pytest.mark.gpu
FK_KERNEL = "rz_skin_instances_fk_kernel"
_refs = {}


def bars(sc):
    if sc["clip"] is not None:
        return POS_TOL, NRM_TOL
    k = max(1, sc["expect"]["longest"] // 8)
    return 1e-4 * k, 2e-4 * k


def reference(sc, oracle):
    """[(positions, normals)] per instance from the float64 hierarchy, computed once per scene and left alone"""
    if sc["name"] not in _refs:
        m, out = sc["mesh"], []
        for i in range(sc["I"]):
            if sc["clip"] is not None:
                q, t, _ = sample_reference(sc["clip"], float(sc["frames"][i]), sc["B"], 0)
            else:
                q, t = sc["q"][i], sc["lt"][i]
            world = fk_reference(sc["parents"], sc["bind"], q, t, sc["ap"], sc["ratio"], sc["mv"])
            out.append(oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], world.reshape(sc["B"], 16).astype(np.float32), sc["inv_bind"]))
        _refs[sc["name"]] = out
    return _refs[sc["name"]]


def make_ctx(lib, sc):
    m = sc["mesh"]
    c = lib.DeformContext(0)
    c.upload_mesh(m["pos"], m["nrm"], m["joints"], m["weights"])
    c.upload_skeleton(sc["inv_bind"])
    c.upload_skeleton_topology(sc["parents"], sc["bind"], sc["ap"], sc["ratio"], sc["mv"])
    c.set_instances(sc["I"])
    if sc["clip"] is not None:
        c.upload_animation(**sc["clip"])
    c.set_tuning(**sc["tuning"])
    return c


def put_pose(c, sc):
    if sc["clip"] is not None:
        c.set_pose_sampled(sc["frames"])
    else:
        c.set_pose_local(sc["q"], None, sc["lt"])


def frame(c, sc, **tune):
    """one frame under these tuning values: [(positions, normals)] of every instance"""
    c.set_tuning(**tune)
    put_pose(c, sc)
    c.deform()
    return [c.read(i) for i in range(sc["I"])]


def same_bits(x, y):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for a, b in zip(x, y) for k in (0, 1))


def worst(outs, refs):
    e = np.zeros(2)
    for (pg, ng), (pr, nr) in zip(outs, refs):
        assert np.isfinite(pg).all() and np.isfinite(ng).all()
        ep, en = parity_errors(pg, ng, pr, nr)
        e = np.maximum(e, [ep.max(), en.max()])
    return e


def assert_form(c, sc, fuse):
    e = sc["expect"]
    fused = bool(fuse) and e["fused"]
    got = {k: c.get_tuning("effective_" + k) for k in ("fuse_fk", "subsets", "subset_bones", "inst_group", "inst_block", "grid", "closure_bones", "closure_rounds", "prep", "inst_lds")}
    want = dict(fuse_fk=int(fused), subsets=1, subset_bones=max(e["named"]), inst_group=e["G"], inst_block=e["block"], grid=e["runs"],
                closure_bones=e["stride"] if fused else 0, closure_rounds=e["rounds"] if fused else 0, prep=0 if fused else 1,
                inst_lds=e["lds"] if fused else e["G"] * max(e["named"]) * 48)
    assert got == want, (sc["name"], fuse, got, want)
    assert (FK_KERNEL in c.kernel_name()) == fused and "<%d," % e["block"] in c.kernel_name(), c.kernel_name()
    return got


@pytest.mark.parametrize("name", cs.NAMES)
def test_the_front_at_this_working_point(rz, oracle, name):
    sc = cs.scene(name)
    e, refs = sc["expect"], reference(sc, oracle)
    bar_p, bar_n = bars(sc)
    outs, errs = {}, {}
    with make_ctx(rz, sc) as c:
        for fuse in (-1, 0):
            c.set_tuning(fuse_fk=fuse)
            put_pose(c, sc)
            got = assert_form(c, sc, fuse)
            c.deform()
            outs[fuse] = [c.read(i) for i in range(sc["I"])]
            if fuse:
                print("crowd front | %s | %s: block %d, G %d, stride %d (named %s, closure %s), rounds %d, items per group %s, %d B of LDS"
                      % (sc["name"], "front" if e["fused"] else "refused (%s), rz_fk_kernel in front" % e["refused"], got["inst_block"], got["inst_group"],
                         e["stride"], e["named"], e["closure"], got["closure_rounds"], e["items"], got["inst_lds"]))
            c.deform_n(3)
            assert same_bits(outs[fuse], [c.read(i) for i in range(sc["I"])]), "%s fuse_fk = %d: a replay differs from the first frame" % (name, fuse)
            errs[fuse] = worst(outs[fuse], refs)
    print("crowd front | %s | %s: positions %.3e (bar %.0e) normals %.3e (bar %.0e) | two launches: positions %.3e normals %.3e"
          % (sc["name"], "one launch" if e["fused"] else "fuse_fk = -1", errs[-1][0], bar_p, errs[-1][1], bar_n, errs[0][0], errs[0][1]))
    for i in range(sc["I"]):
        assert same_bits(outs[-1][i:i + 1], outs[0][i:i + 1]), "%s instance %d: the fused front differs from rz_fk_kernel + skin kernel" % (name, i)
    assert errs[0][0] <= bar_p and errs[0][1] <= bar_n, ("two launches", name, errs[0])
    assert errs[-1][0] <= bar_p and errs[-1][1] <= bar_n, ("one launch", name, errs[-1])


@pytest.mark.parametrize("name", ["items256_tail3", "chain64"])
def test_workgroup_order_and_streaming_stores_leave_the_bits_alone(rz, name):
    """"inst_order" deals the (run, pose group) pairs to the workgroups the other way round, "nt_store" picks the kernel's other
    instantiation: on an item-limit scene and on a three-round one, the same bits"""
    sc = cs.scene(name)
    with make_ctx(rz, sc) as c:
        base = frame(c, sc, fuse_fk=-1, inst_order=1, nt_store=0)
        assert FK_KERNEL + "<%d, false>" % sc["expect"]["block"] in c.kernel_name()
        for order, nts in ((0, 0), (1, 1), (0, 1)):
            got = frame(c, sc, inst_order=order, nt_store=nts)
            assert FK_KERNEL + "<%d, %s>" % (sc["expect"]["block"], "true" if nts else "false") in c.kernel_name()
            assert c.get_tuning("effective_closure_bones") == sc["expect"]["stride"]
            assert same_bits(base, got), "%s: inst_order = %d nt_store = %d changes the frame" % (name, order, nts)


def test_variants_build_equals_the_product(rz, rzv):
    sc = cs.scene("append17")
    out = []
    for lib in (rz, rzv):
        with make_ctx(lib, sc) as c:
            out.append(frame(c, sc, fuse_fk=-1))
            assert FK_KERNEL in c.kernel_name() and c.get_tuning("effective_closure_rounds") == 3
    assert same_bits(out[0], out[1])
