"""24-bit dense morph storage on the device (rz_upload_morphs_dense; kernels/common.hip.h, deform_dense.hip, pass_parts.hip.h, sdef.hip):
the device decode against the numpy model of the format (tests/morph24_ref.py), the kernels' arithmetic against an fp32-storage context fed
the decoded deltas (bit for bit, every consumer and every list-build site), the derived error bound against fp32 storage of the original
deltas, and the opt-out / fork / re-upload / fallback plumbing."""
import numpy as np
import pytest

import morph24_ref as ref
from helpers import assert_parity
from reze_engine_amd import synth

pytestmark = pytest.mark.gpu

B = 24


def small_deltas(M, V, seed):
    rng = np.random.default_rng(seed)
    d = ((rng.random((M, V, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)
    d *= (np.float32(2.0) ** rng.integers(-6, 7, size=M)).astype(np.float32)[:, None, None]     # another scale for every morph
    return d


def weights(M, seed, zeros=True):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, size=M).astype(np.float32)
    if zeros and M >= 4:
        w[rng.choice(M, size=M // 4, replace=False)] = 0.0        # the compaction skips them
    return w


def decoded_of(c, M):
    return np.ascontiguousarray(np.stack([c.read_morph_dense(m) for m in range(M)]).transpose(0, 2, 1))       # [M, V, 3]


@pytest.fixture(scope="module")
def pair(rz):
    """(q, f): a context with the default (24-bit) storage and one with fp32 planes; `load` gives both the same mesh, f the DECODED deltas"""
    q, f = rz.DeformContext(0), rz.DeformContext(0)

    def load(mesh, deltas, topology=False):
        for c in (q, f):
            c.set_instances(1)
            c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"])
            c.upload_skeleton(mesh["inv_bind"])
            c.upload_sdef([], [], [], []); c.upload_qdef([])
            if topology:
                c.upload_skeleton_topology(mesh["parents"], mesh["bind"])
            c.set_tuning(morph_split=0, grid_cap=0, fast=-1, out_cap=-1, fuse_fk=-1)
        q.upload_morphs_dense(deltas)
        assert q.get_tuning("effective_morph_storage") == 24
        dec = decoded_of(q, len(deltas))
        f.upload_morphs_dense(dec, storage=rz.capi.MORPH_F32)
        assert f.get_tuning("effective_morph_storage") == 32
        return dec

    yield q, f, load
    q.close(); f.close()


def frames_equal(q, f, pose, what):
    out = []
    for c in (q, f):
        pose(c)
        c.deform()
        out.append(c.read())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), what
    assert np.isfinite(out[0][0]).all()
    return out[0]


@pytest.mark.parametrize("V", [1, 3, 4, 5, 31, 33, 127, 129, 1021])
def test_device_decode_equals_the_model(pair, V):
    q, _f, _load = pair
    mesh = synth.make_mesh(V, B, seed=V)
    d = small_deltas(5, V, 300 + V)
    d[3] = 0                                            # an all-zero morph (s = 1)
    d[4, V // 2, 1] = np.nextafter(np.float32(0.125), np.float32(0)) * np.float32(8)      # a maximum that raises its exponent
    q.set_instances(1)
    q.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"]); q.upload_skeleton(mesh["inv_bind"])
    q.upload_morphs_dense(d)
    assert q.get_tuning("effective_morph_storage") == 24
    st, _s, _pk, dec = ref.encode(d)
    assert st == 24
    for m in range(5):
        assert np.array_equal(q.read_morph_dense(m), dec[m]), m


@pytest.mark.parametrize("M", [1, 7, 16, 17, 64, 129])
@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_one_launch_and_prep_frames_are_exact(pair, split, M):
    """the dense stream kernel: every slice count x remainder loop / full U*S groups / > 128 morphs (the prep kernel's list) x masked last
    step / run shorter than a step / several waves"""
    q, f, load = pair
    for V in (129, 1021, 4100):
        mesh = synth.make_mesh(V, B, seed=11)
        load(mesh, small_deltas(M, V, 1000 + M + V))
        w = weights(M, 7 * M + V)
        for fast in ((1, 0) if M <= 128 else (0,)):
            for c in (q, f):
                c.set_tuning(morph_split=split, fast=fast)
            frames_equal(q, f, lambda c: c.set_pose(mesh["world"], w), "S=%d M=%d V=%d fast=%d" % (split, M, V, fast))
            assert q.get_tuning("effective_fast") == fast and q.get_tuning("effective_split") == split


def test_crowd_of_three_with_dense_morphs_is_exact(pair):
    q, f, load = pair
    V, M = 1021, 17
    mesh = synth.make_mesh(V, B, seed=12)
    load(mesh, small_deltas(M, V, 77))
    worlds = np.stack([synth.make_pose(mesh["parents"], mesh["bind"], B, 50 + i) for i in range(3)])
    w = np.stack([weights(M, 60 + i) for i in range(3)])
    for c in (q, f):
        c.set_instances(3)
    for i in range(3):
        outs = []
        for c in (q, f):
            c.set_pose(worlds, w); c.deform()
            outs.append(c.read(i))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), i
    for c in (q, f):
        c.set_instances(1)


@pytest.mark.parametrize("fuse", [1, 0])
def test_device_fk_frame_is_exact(pair, fuse):
    """fuse 1: the list is compacted in the frame kernel's fused-hierarchy prologue; 0: rz_fk_kernel, then rz_prep_kernel's list"""
    q, f, load = pair
    V, M = 4100, 17
    mesh = synth.make_mesh(V, B, seed=13)
    load(mesh, small_deltas(M, V, 78), topology=True)
    w = weights(M, 61)
    for c in (q, f):
        c.set_tuning(fuse_fk=fuse)
    frames_equal(q, f, lambda c: c.set_pose_local(mesh["quats"], w), "device FK fuse=%d" % fuse)
    for c in (q, f):
        c.set_tuning(fuse_fk=-1)


@pytest.mark.parametrize("table", ["sdef", "qdef"])
@pytest.mark.parametrize("path", ["one_launch", "prep", "fused_fk"])
def test_sdef_and_qdef_passes_are_exact(pair, table, path):
    """the passes' per-vertex decode (add_dense) with the weights from each source: the kernel-argument list, the prep kernel's list, and
    the weights compacted in the pass itself (behind a fused-hierarchy frame)"""
    q, f, load = pair
    V, M = 1021, 17
    mesh = synth.make_mesh(V, B, seed=14)
    load(mesh, small_deltas(M, V, 79), topology=True)
    w = weights(M, 62)
    sd = synth.make_sdef(mesh, 0.05, seed=3)
    qd = synth.make_qdef(mesh, 0.05, seed=4)
    assert len(sd["idx"]) > 0 and len(qd) > 0
    for c in (q, f):
        if table == "sdef":
            c.upload_sdef(sd["idx"], sd["c"], sd["r0"], sd["r1"])
        else:
            c.upload_qdef(qd)
        c.set_tuning(fast=0 if path == "prep" else -1, fuse_fk=1 if path == "fused_fk" else -1)
    if path == "fused_fk":
        frames_equal(q, f, lambda c: c.set_pose_local(mesh["quats"], w), table + " " + path)
    else:
        frames_equal(q, f, lambda c: c.set_pose(mesh["world"], w), table + " " + path)
    for c in (q, f):
        c.upload_sdef([], [], [], []); c.upload_qdef([])
        c.set_tuning(fast=-1, fuse_fk=-1)


def test_error_bound_against_fp32_storage_of_the_original_deltas(pair):
    """identity pose, weights in [-1, 1], the ORIGINAL deltas in both contexts: per component
    |P_24 - P_f32| <= sum_m |w_m| * 2^(E_m - 23) + 2 ulp(|P|) — every stored delta is off by at most 2^(E_m - 23) (the format), and the two
    accumulations round at most once more each than the exact sums they follow (one ulp of the result apiece)."""
    q, f, _load = pair
    V, M = 4100, 64
    mesh = synth.make_mesh(V, B, seed=15)
    ident = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (B, 1))
    d, _ = synth.make_morphs_dense(V, M)
    w = weights(M, 63, zeros=False)
    out = []
    for c, st in ((q, None), (f, 1)):
        c.set_instances(1)
        c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"]); c.upload_skeleton(ident)
        c.upload_morphs_dense(d, storage=st)
        c.set_pose(ident, w); c.deform()
        out.append(c.read()[0].astype(np.float64))
    E = ref.exponents(d)
    bound = float((np.abs(w).astype(np.float64) * np.ldexp(1.0, E - 23)).sum()) + 2.0 * np.spacing(np.abs(out[1]).astype(np.float32)).astype(np.float64)
    diff = np.abs(out[0] - out[1])
    print("24-bit vs fp32 storage: max |diff| %.3e, max diff / bound %.3f" % (diff.max(), (diff / bound).max()))
    assert (diff <= bound).all()


def test_c3_parity_with_the_oracle_in_default_storage(rz, oracle):
    mesh = synth.make_mesh(30000, 200)
    deltas, mw = synth.make_morphs_dense(30000, 64)
    pr, nr = oracle.deform(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"], mesh["world"], mesh["inv_bind"], deltas, mw, threads=8)
    with rz.DeformContext(0) as c:
        c.upload_mesh(mesh["pos"], mesh["nrm"], mesh["joints"], mesh["weights"]); c.upload_skeleton(mesh["inv_bind"]); c.upload_morphs_dense(deltas)
        assert c.get_tuning("effective_morph_storage") == 24
        c.set_pose(mesh["world"], mw); c.deform()
        pg, ng = c.read()
    ep, en = assert_parity(pg, ng, pr, nr, "C3, 24-bit storage")
    print("C3 24-bit storage: max rel pos err %.3e, max nrm err %.3e" % (ep, en))


def test_opt_out_fork_reupload_and_fallback(rz, pair):
    q, f, load = pair
    V, M = 1021, 16
    mesh = synth.make_mesh(V, B, seed=16)
    d = small_deltas(M, V, 80)
    dec = load(mesh, d)
    w = weights(M, 64)
    base = frames_equal(q, f, lambda c: c.set_pose(mesh["world"], w), "base")
    # a fork borrows planes and scales and renders the same bits
    k = q.fork()
    assert k.get_tuning("effective_morph_storage") == 24
    k.set_pose(mesh["world"], w); k.deform()
    pk, nk = k.read()
    k.close()
    assert np.array_equal(pk, base[0]) and np.array_equal(nk, base[1])
    # the other storage on the live contexts: q takes fp32 planes of the decoded deltas, f takes 24-bit planes of them (they encode to themselves)
    q.upload_morphs_dense(dec, storage=rz.capi.MORPH_F32)
    f.upload_morphs_dense(dec)
    assert q.get_tuning("effective_morph_storage") == 32 and f.get_tuning("effective_morph_storage") == 24
    again = frames_equal(q, f, lambda c: c.set_pose(mesh["world"], w), "swapped storage")
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
    # a non-finite delta: the whole set stays fp32 and renders as the fp32 context renders it
    bad = d.copy(); bad[2, 5, 1] = np.inf
    q.upload_morphs_dense(bad); f.upload_morphs_dense(bad, storage=rz.capi.MORPH_F32)
    assert q.get_tuning("effective_morph_storage") == 32
    outs = []
    for c in (q, f):
        c.set_pose(mesh["world"], w); c.deform(); outs.append(c.read())
    assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True) and np.array_equal(outs[0][1], outs[1][1], equal_nan=True)
    # no morphs: the key reports nothing resident
    q.upload_morphs_dense(None)
    assert q.get_tuning("effective_morph_storage") == 0
