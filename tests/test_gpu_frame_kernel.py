"""The frame kernel's launch switches on the device (csrc/frame_kernel.h; kernels/deform_dense.hip, deform_small.hip, crowd.hip): every arm
the product build carries, once each, over tests/frame_kernel_walk.py. Per arm one frame: kernel_name() is the string in the walk's table;
the output holds the parity bar of tests/helpers.py against the oracle (device-solved poses: behind helpers.fk_reference /
sample_reference in float64); and a crowd's instances are bit-equal to the same pose run alone through the single-mesh kernel, the
contract tests/test_gpu_round2.py states. A last test: the effective_* queries are read-only."""
import numpy as np
import pytest

import frame_kernel_walk as fkw
from helpers import assert_hull, assert_parity

pytestmark = pytest.mark.gpu

EFFECTIVE = ("variant", "nt", "nt_store", "geo", "split", "unroll", "fast", "inst_block", "subsets", "inst_morphs", "fuse_fk", "poses_per_wg", "inst_group",
             "fk_kind", "prep", "overlap", "closure_bones", "closure_rounds", "out_cap", "sparse_piece", "grid", "subset_bones", "inst_lds", "morph_storage")


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_every_arm_of_the_launch_switches(rz, oracle):
    seen = []
    for arm in fkw.walk(rz):
        c, m, what = arm["c"], arm["mesh"], arm["name"]
        assert c.kernel_name() == arm["kernel"], (what, c.kernel_name(), arm["kernel"])
        c.deform()
        n_inst = len(arm["worlds"])
        outs = [c.read(i) for i in range(n_inst)]
        worst = np.zeros(2)
        for i, (pg, ng) in enumerate(outs):
            world = np.asarray(arm["worlds"][i]).reshape(-1, 16).astype(np.float32)
            pr, nr = oracle.deform(m["pos"], m["nrm"], m["joints"], m["weights"], world, m["inv_bind"], arm["deltas"], None if arm["mw"] is None else arm["mw"][i])
            worst = np.maximum(worst, assert_parity(pg, ng, pr, nr, "%s, instance %d" % (what, i)))
            if arm["edge"] is not None:
                assert_hull(c.read_hull(i), oracle.hull(pr, nr, arm["edge"]), what)
        print("frame kernel | %s | %s | positions %.3e normals %.3e" % (what, arm["symbol"], worst[0], worst[1]))
        if arm["family"] == "crowd":
            # the same poses alone: one instance, the library's own plan for it (a single-mesh kernel)
            c.set_instances(1)
            for i in range(n_inst):
                arm["pose"](c, i)
                assert c.get_tuning("effective_inst_group") == 0 and "rz_deform_small_kernel" in c.kernel_name()
                c.deform()
                assert same_bits(outs[i], c.read(0)), "%s: instance %d differs from the same pose run alone (%s)" % (what, i, c.kernel_name())
            c.set_instances(fkw.I_CROWD)
        seen.append(arm["symbol"])
    # the walk reached every kernel template of the product, both MORPH halves included
    for stem in ("rz_deform_small_kernel<", "rz_deform_dense_kernel<", "rz_skin_instances_kernel<", "rz_skin_instances_fk_kernel<", "rz_skin_instances_morph_kernel<",
                 "rz_skin_instances_fk_morph_kernel<"):
        assert any(s.startswith(stem) for s in seen), stem


def test_queries_leave_the_next_frame_alone(rz):
    """kernel_name() on a dense and on a crowd context is the string it always was; reading every effective_* key moves neither
    effective_grid nor the frame's bits (a query that needs no run lists rebuilds none: the lists are built once, for the shape)."""
    arms = {}
    for arm in fkw.walk(rz):
        if arm["name"] not in ("one mesh, 9 dense morphs 24-bit, hull off", "crowd, block 512, inst_subsets = 1, fast = 1"):
            continue
        c = arm["c"]
        assert c.kernel_name() == arm["kernel"] == {"one": "rz_deform_dense_kernel<8, 8, true, false, false, true, 3>", "crowd": "rz_skin_instances_kernel<512, false, true>"}[arm["family"]]
        c.deform()
        n_inst = len(arm["worlds"])
        before, grid = [c.read(i) for i in range(n_inst)], c.get_tuning("effective_grid")
        values = {k: c.get_tuning("effective_" + k) for k in EFFECTIVE}
        assert values == {k: c.get_tuning("effective_" + k) for k in EFFECTIVE} and values["grid"] == grid
        assert c.kernel_name() == arm["kernel"]
        c.deform()
        for i in range(n_inst):
            assert same_bits(before[i], c.read(i)), (arm["name"], i)
        arms[arm["name"]] = values
    assert len(arms) == 2
