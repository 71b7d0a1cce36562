"""Scenes for crowds with sparse morph targets on the crowd skin kernels (kernels/crowd_morph.hip: the MORPH instantiations of
rz_skin_instances_kernel / rz_skin_instances_fk_kernel; tuning key "inst_morphs"), shared by tests/test_crowd_morph_cpu.py (which holds
every scene to the shape it claims, without a GPU) and tests/test_gpu_crowd_morphs.py (which runs them). Test infrastructure.

One mesh of 1 283 vertices (the last quad is padded) on a gentle skeleton of 24 bones, I = 11 instances at inst_loop = 4: pose groups of
4, 4 and 3. "grid_cap" = 2 x groups pins two vertex runs whatever the device's CU count (plan.cpp: inst_runs): 704 and 580 vertices, so a
run is more than one 256-vertex step. The runs' lengths and the workgroup sizes are multiples of 64, so a WAVE STEP — the 64 vertices one
wave decodes at a time, and the unit of the kernel's one ballot "does any of my vertices have a row" — is an aligned block of 64
vertices at every workgroup size: wave step j = vertices [64 j, 64 j + 64).

A scene = the targets in the PMX on-disk form (off, idx, d3: what upload_morphs_sparse takes) + per-instance weights mw [I, M]. Unless a
scene says otherwise a quarter of the weights are 0, some are negative, some above 1, one instance is all zero; all non-zero weights and
all deltas are distinct. Poses: per-instance local rotations q [I, B, 4] and the world matrices synth.fk_world makes of them."""
import numpy as np

import sparse_piece_scenes as sps
from reze_engine_amd import synth

V, B, I, G = 1283, 24, 11, 4
GROUPS = (I + G - 1) // G
GROUP_SIZES = (4, 4, 3)
RUNS = 2
PER = 704                               # vertices per run: round_up(ceil(V / 2), 64)
V4 = (V + 3) // 4 * 4                   # what the crowd kernels walk: whole quads
WAVE_STEPS = (V4 + 63) // 64
ZERO_INSTANCE = 5
TUNING = dict(inst_loop=G, grid_cap=RUNS * GROUPS)
BUDGET = {256: 80 * 1024, 512: 156 * 1024, 1024: 156 * 1024}      # plan.cpp: the crowd kernels' LDS per workgroup
FACE = (200, 130)                       # the face scene's vertices [200, 330): across the wave boundaries 256 and 320, and 256 is a workgroup-step boundary at 256 threads
FACE_LONG = 260                         # ... and the vertex listed 12 times in each of its 6 morphs: a row of 72 entries
EDGE_VERTS = (128, 191, 0, PER - 1, PER, V - 1)       # lane 0 and lane 63 of wave step 2; first / last vertex of run 0; first of run 1; vertex V - 1 (the last of run 1)
NAMES = ("scattered", "face", "edges", "empty", "many")
NOFIT = dict(I=64, inst_loop=64, M=600)               # the combination that must not fit: 64 x 608 x 4 B of weights alone are 152 KB
_memo = {}


def mpad(M):
    """upload.cpp: the stride of a pose's weights in LDS"""
    return (M + 8 + 3) // 4 * 4


def lds_bytes(G_, bones, per_bone, M):
    """rzlds::crowd (csrc/lds_layout.h) with the weight block, restated: G poses x (staged bones x 48 / 64 / 112 B + Mpad x 4 B)"""
    return G_ * bones * per_bone + G_ * mpad(M) * 4


def run_of(v):
    return v // PER


def wave_step_rows(rows):
    """per wave step: how many of its vertices have a row"""
    r = np.zeros(WAVE_STEPS * 64, dtype=np.int64)
    r[:len(rows)] = rows
    return (r.reshape(WAVE_STEPS, 64) > 0).sum(axis=1)


def _mesh():
    if "mesh" not in _memo:
        mesh = synth.make_mesh(V, B, seed=0xC0D)
        mesh["bind"] = (mesh["bind"] * np.float32(0.25)).astype(np.float32)
        mesh["inv_bind"] = synth.inverse_bind_translation_only(mesh["parents"], mesh["bind"])
        rng = np.random.default_rng(0xC0D + 1)
        mesh["pos"] = ((rng.random((V, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
        ax = rng.normal(size=(I, B, 3))
        ax /= np.linalg.norm(ax, axis=2, keepdims=True)
        ang = rng.uniform(-0.5, 0.5, size=(I, B, 1))
        q = np.concatenate([ax * np.sin(ang / 2), np.cos(ang / 2)], axis=2).astype(np.float32)
        mesh["q"] = q
        mesh["worlds"] = np.stack([synth.fk_world(mesh["parents"], mesh["bind"], q[i]) for i in range(I)]).astype(np.float32)
        mesh["world"] = mesh["worlds"][0]
        _memo["mesh"] = mesh
    return _memo["mesh"]


def run_bones(mesh=None):
    """per run: the bones its vertices name in any of the four slots, the padding vertices of the last quad naming bone 0
    (kernels/crowd.hip: rz_run_subsets_kernel)"""
    mesh = _mesh() if mesh is None else mesh
    j = np.zeros((V4, 4), dtype=np.int64)
    j[:V] = np.minimum(mesh["joints"].astype(np.int64), B - 1)
    return [sorted(set(j[r * PER:min(V4, (r + 1) * PER)].reshape(-1).tolist())) for r in range(RUNS)]


def _weights(rng, M, n_inst=I):
    n = n_inst * M
    mag = 0.25 + (rng.permutation(n) + 0.5) / n             # distinct, 0.25 .. 1.25: some above 1
    w = mag * np.where(rng.random(n) < 0.3, -1.0, 1.0)
    w[rng.permutation(n)[:n // 4]] = 0.0                    # a quarter of them off
    w = w.reshape(n_inst, M).astype(np.float32)
    w[min(ZERO_INSTANCE, n_inst - 1)] = 0.0
    return w


def _deltas(rng, E, lo=0.02, hi=0.05):
    d = rng.normal(size=(E, 3))
    d *= (rng.uniform(lo, hi, size=E) / np.linalg.norm(d, axis=1))[:, None]
    return d.astype(np.float32)


def _from_lists(lists, rng, **kw):
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([v for x in lists for v in x], dtype=np.uint32)
    return off, idx, _deltas(rng, len(idx), **kw)


def _targets(name, rng):
    if name == "scattered":
        off, idx, d3, _ = synth.make_morphs_sparse(V, 3, density=0.02, seed=0x5CA7)
        # ... and one hand-laid morph of three lone vertices, each the only row of its wave step
        rows = np.bincount(idx.astype(np.int64), minlength=V)
        lone = [64 * j + 17 for j in np.flatnonzero(wave_step_rows(rows) == 0)[:3]]
        off = np.concatenate([off, [off[-1] + len(lone)]]).astype(np.uint32)
        idx = np.concatenate([idx, np.array(lone, dtype=np.uint32)])
        d3 = np.concatenate([d3, _deltas(rng, len(lone))])
        return off, idx, d3
    if name == "face":
        face = list(range(FACE[0], FACE[0] + FACE[1]))
        lists = []
        for m in range(6):
            ls = list(face)
            for k in range(11):                              # eleven duplicates of one vertex, spread through the morph (file order is kept)
                ls.insert((k + 1) * len(face) // 12 + k, FACE_LONG)
            lists.append(ls)
        return _from_lists(lists, rng, lo=0.01, hi=0.02)
    if name == "edges":
        lists = [[] for _ in range(4)]
        for k, v in enumerate(EDGE_VERTS):
            lists[k % 4].append(v)
        return _from_lists([sorted(x) for x in lists], rng)
    if name == "empty":
        return _from_lists([[V, V + 5], [], [4000000]], rng)            # nothing inside the mesh (the first inside the vertex padding), one empty morph
    if name == "many":
        return _from_lists([sorted(int(v) for v in rng.choice(V, size=2, replace=False)) for _ in range(300)], rng)
    if name == "nofit":
        return _from_lists([[int(v)] for v in rng.choice(V, size=NOFIT["M"], replace=True)], rng)
    raise KeyError(name)


def build(name):
    rng = np.random.default_rng([0xC20D, ("scattered", "face", "edges", "empty", "many", "nofit").index(name)])
    mesh = _mesh()
    off, idx, d3 = _targets(name, rng)
    M = len(off) - 1
    n_inst = NOFIT["I"] if name == "nofit" else I
    mw = _weights(rng, M, n_inst)
    ptr, src, morph = sps.csr(V, off, idx)
    tuning = dict(TUNING)
    if name == "many":
        tuning = dict(inst_loop=8, grid_cap=RUNS * 2)           # groups of 8 and 3
    if name == "nofit":
        tuning = dict(inst_loop=NOFIT["inst_loop"], grid_cap=RUNS)
    return dict(name=name, V=V, B=B, I=n_inst, M=M, mesh=mesh, off=off, idx=idx, d3=d3, mw=mw, ptr=ptr, src=src, morph=morph,
                rows=np.diff(ptr), tuning=tuning)


def scene(name):
    """build(name), built once per process and never changed"""
    if name not in _memo:
        _memo[name] = build(name)
    return _memo[name]


# ---- the definition (ISSUE / DESIGN.md: the chain of kernels/deform_small.hip) ----
def chain32(s, mw):
    """float32 restatement: per vertex acc = fmaf(w[morph(e)], d(e), acc) over its row in row order from +0, then x += acc. (fmaf in
    numpy: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32 — a model of the chain's
    rounding, not of its last bit.)"""
    ptr, src, morph = s["ptr"], s["src"], s["morph"]
    w = np.asarray(mw, dtype=np.float32)
    out = s["mesh"]["pos"].astype(np.float32).copy()
    for v in np.flatnonzero(np.diff(ptr) > 0):
        acc = np.zeros(3, dtype=np.float32)
        for e in range(int(ptr[v]), int(ptr[v + 1])):
            acc = (np.float64(w[morph[e]]) * s["d3"][src[e]].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        out[v] = out[v] + acc
    return out


def reference64(s, inst, world=None):
    """(positions, normals) of one instance in float64: sps.morph64 + sps.skin64 with that instance's weights and world matrices"""
    world = s["mesh"]["worlds"][inst] if world is None else world
    p, n, _ = sps.skin64(s, sps.morph64(s, s["mw"][inst]), world)
    return p, n
