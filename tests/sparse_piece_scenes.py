"""Scenes for the sparse morph row walk at its LDS piece edges (kernels/deform_small.hip, MODE 2: sp_stage / sp_slot / the piece loop),
shared by tests/test_sparse_pieces_cpu.py (which holds every scene to the shape it claims, without a GPU) and
tests/test_gpu_sparse_pieces.py (which runs them). Test infrastructure.

A wave walks the per-vertex CSR one 64-vertex ROUND at a time: the round's entry range [E0, E1) — first entry of its first vertex to last
entry of its last live vertex — goes through LDS in pieces of `sparse_piece` entries counted from E0. A scene is a list of rounds, every
round a list of per-vertex row lengths; the last round is ragged (3 vertices). With V = 5 x 64 + 3 and the one-step-per-wave plan of so
small a mesh (step_quads below) the rounds are exactly the kernel's at morph_split = 4; at morph_split = 1 and under a grid cap the
steps start elsewhere, the same rows then meet the piece edges at other places (the GPU test's bars do not depend on where).

Rows longer than the morph count come from duplicates: PMX allows a vertex listed twice inside one morph, the upload keeps file order.
Every delta and every weight is distinct, a quarter of the morphs have weight 0, one morph is empty, three entries name vertices past the
mesh. The signs of the deltas are chosen entry by entry, in the row's accumulation order, against the running sum: the morphed position
stays within ~0.1 of the rest position however long the row, which keeps |P_ref| small (the per-entry bar of the CPU test is relative
to it) and the float32 chain's rounding far under the parity bar."""
import numpy as np

from reze_engine_amd import synth

LANES = 64
ROUNDS = 5                              # whole rounds in front of the ragged one
V = ROUNDS * LANES + 3
B = 12
M = 64
EMPTY_MORPH = 10
PIECES = (16, 32, 48, 64, 256, 0)       # what the GPU test sets "sparse_piece" to; 0 = the plan's own
AUTO_PIECE = 2048                       # ... which is min(2048, 64 x M) at 64-vertex steps here: a whole LDS budget, a 12-bone palette
TALL_ROUNDS = 17                        # the "tall" scene: enough rounds for 256-vertex steps of four, and for second steps


def step_quads(n_verts, split, grid_cap=0):
    """plan.cpp (make_plan / run_per_wave without the dense rules): (workgroups, quads per wave) of a sparse single-mesh frame on a
    device with more CUs than the mesh has steps — what lays a wave's steps over the mesh"""
    nq = (n_verts + 3) // 4
    qstep = 64 // split
    gx = max(1, (nq + 4 * qstep - 1) // (4 * qstep))
    if grid_cap:
        gx = min(gx, grid_cap)
    per = (nq + 4 * gx - 1) // (4 * gx)
    per = max(8, (per + 7) // 8 * 8)
    return (nq + 4 * per - 1) // (4 * per), per


def kernel_steps(n_verts, split, grid_cap=0):
    """the steps the waves of that frame take (kernels/deform_small.hip): [[(first vertex, live lanes) per round] per step], a wave's
    steps in the order it takes them, wave after wave. A round may end in up to three padding vertices (whole quads): their rows are empty."""
    nq = (n_verts + 3) // 4
    qstep = 64 // split
    gx, per = step_quads(n_verts, split, grid_cap)
    steps = []
    for w in range(4 * gx):
        q_end = min(nq, (w + 1) * per)
        for qw in range(w * per, q_end, qstep):
            v_live = min(4 * qstep, (q_end - qw) * 4)
            steps.append([(qw * 4 + 64 * r, min(64, v_live - 64 * r)) for r in range(qstep // 16) if v_live - 64 * r > 0])
    return steps


def _spread(rng, total, lanes=LANES, idle=0.25):
    """`total` entries over `lanes` rows, unevenly, about a quarter of the rows empty"""
    p = rng.random(lanes) * (rng.random(lanes) >= idle)
    if p.sum() == 0:
        p[:] = 1
    return [int(x) for x in rng.multinomial(total, p / p.sum())]


def _light(rng, total=90):
    return _spread(rng, total)


def rounds_of(name, P, rng):
    """the scene's rounds: ROUNDS lists of 64 row lengths and one of 3"""
    empty = [0] * LANES
    if name == "exact":
        return [_spread(rng, P - 1), _spread(rng, P), _spread(rng, P + 1), _spread(rng, 2 * P), empty, [1, 2, 1]]
    if name == "straddle":
        assert 4 * P <= 5 * LANES
        return [[5] * LANES, [5] * LANES, [2] + [5] * (LANES - 1), empty, [5] * LANES, [5, 5, 5]]
    if name == "long_row":
        a = [min(x, 2) for x in _light(rng, 40)]
        b = [min(x, 2) for x in _light(rng, 40)]
        a[0], a[1], a[2] = 3 * P + 5, 0, 1
        b[63], b[62], b[61] = 3 * P + 5, 0, 1
        return [a, _light(rng), b, empty, _light(rng), [2, 0, 3]]
    if name == "holes":
        return [empty, _light(rng, 100), empty, _light(rng, 150), empty, [33, 0, 45]]
    if name == "bursts":
        return [_spread(rng, 64 * 9 + 24, idle=0.0), [1 + x for x in _spread(rng, 640)], _light(rng), empty, _light(rng), [3, 1, 2]]
    if name == "tall":
        # for 256-vertex steps (morph_split = 1) and one workgroup: a wave's first step is four rounds, every one of several pieces, its
        # second a ragged round; at 64-vertex steps every wave takes five steps, four of them in the steady-state form
        out = []
        for i in range(TALL_ROUNDS):
            r = [[5] * LANES, [2] + [5] * (LANES - 1), _spread(rng, 4 * P + 3), [5] * LANES][i % 4]
            if i % 5 == 3:
                r = list(r)
                r[(17 * i) % LANES] = 3 * P + 5
            out.append(empty if i == 10 else r)        # (round 10: the second step of the third wave at one workgroup of 64-vertex steps)
        return out + [[5, 0, 7]]
    raise KeyError(name)


# (scene, the piece size it is designed around): every scene runs at every size of PIECES; the CPU test holds it to its claim at its own
DESIGNS = ([("exact", P) for P in (16, 32, 48, 64, 256, AUTO_PIECE)] + [("straddle", P) for P in (16, 32, 48, 64)] +
           [("long_row", P) for P in (16, 32, 48, 64, 256)] + [("holes", 16), ("bursts", 256)] + [("tall", P) for P in (16, 48)])


def csr(n_verts, off, idx):
    """rz_upload_morphs_sparse (csrc/upload.cpp) in numpy: the per-vertex CSR — a vertex's entries in ascending morph order, then file
    order; entries that name a vertex past the mesh dropped. Returns (ptr [V + 1], src [kept] = the file index of every kept entry,
    morph [kept])."""
    idx = np.asarray(idx, dtype=np.int64)
    keep = np.flatnonzero(idx < n_verts)
    order = keep[np.argsort(idx[keep], kind="stable")]          # file order is ascending morph already: stable by vertex keeps it
    ptr = np.zeros(n_verts + 1, dtype=np.int64)
    np.add.at(ptr, idx[keep] + 1, 1)
    morph = np.searchsorted(np.asarray(off, dtype=np.int64), order, side="right") - 1
    return np.cumsum(ptr), order, morph


def round_ranges(ptr, n_verts):
    """[(first vertex, live vertices, E0, E1)] of every 64-vertex round"""
    return [(v0, min(LANES, n_verts - v0), int(ptr[v0]), int(ptr[min(v0 + LANES, n_verts)])) for v0 in range(0, n_verts, LANES)]


def skin64(scene, pos, world=None):
    """vs() in float64: blended 3x4 per vertex from world * inv_bind, weights u8 / 255 normalised. Returns (positions, unit normals, the
    blended 3x3 of every vertex)."""
    m = scene["mesh"]
    W = np.asarray(m["world"] if world is None else world, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    IB = np.asarray(m["inv_bind"], dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    S = W @ IB
    w = m["weights"].astype(np.float64) / 255.0
    s = w.sum(axis=1, keepdims=True)
    w = np.where(s > 1e-4, w / np.where(s > 1e-4, s, 1), np.array([1.0, 0, 0, 0]))
    blend = np.einsum("vk,vkij->vij", w, S[m["joints"].astype(np.int64)])
    p = np.einsum("vij,vj->vi", blend[:, :3, :3], np.asarray(pos, dtype=np.float64)) + blend[:, :3, 3]
    n = np.einsum("vij,vj->vi", blend[:, :3, :3], m["nrm"].astype(np.float64))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p, n, blend[:, :3, :3]


def morph64(scene, mw, skip=None, twice=None):
    """rest positions + the weighted entries in float64; skip / twice: one CSR position left out / taken twice (the CPU test's mutants)"""
    ptr, src, morph = scene["ptr"], scene["src"], scene["morph"]
    contrib = np.asarray(mw, dtype=np.float64)[morph][:, None] * scene["d3"].astype(np.float64)[src]
    if skip is not None:
        contrib[skip] = 0
    if twice is not None:
        contrib[twice] *= 2
    vert = np.repeat(np.arange(scene["V"]), np.diff(ptr))
    out = scene["mesh"]["pos"].astype(np.float64).copy()
    np.add.at(out, vert, contrib)
    return out


def reference64(scene, mw=None, world=None, **mutant):
    p, n, _ = skin64(scene, morph64(scene, scene["mw"] if mw is None else mw, **mutant), world)
    return p, n


def build(name, P):
    """dict(name, P, V, rounds, rows [V], mesh, off, idx, d3 — the PMX on-disk form handed to upload_morphs_sparse —, mw, mw2 (a second
    instance's weights: three morphs active), and the upload's CSR: ptr, src, morph)"""
    rng = np.random.default_rng([0x5BA5E, ("exact", "straddle", "long_row", "holes", "bursts", "tall").index(name), P])
    rounds = rounds_of(name, P, rng)
    assert len(rounds) == (TALL_ROUNDS if name == "tall" else ROUNDS) + 1 and all(len(r) == LANES for r in rounds[:-1]) and len(rounds[-1]) == 3
    rows = np.array([x for r in rounds for x in r], dtype=np.int64)
    V = len(rows)                           # (the module's V, but for the tall scene)

    # a small gentle skeleton (bind offsets a quarter of synth's: |P_ref| stays near 1) and rest positions inside the unit ball's box
    mesh = synth.make_mesh(V, B, seed=int(rng.integers(1 << 30)))
    mesh["bind"] = (mesh["bind"] * np.float32(0.25)).astype(np.float32)
    mesh["inv_bind"] = synth.inverse_bind_translation_only(mesh["parents"], mesh["bind"])
    mesh["world"] = synth.fk_world(mesh["parents"], mesh["bind"], mesh["quats"])
    mesh["pos"] = ((rng.random((V, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)

    # weights: distinct, 0.5 <= |w| <= 1, both signs, every fourth morph off
    mag = 0.5 + 0.5 * (rng.permutation(M) + rng.random(M) * 0.5) / M
    mw = (mag * np.where(rng.random(M) < 0.5, -1.0, 1.0)).astype(np.float32)
    mw[1::4] = 0.0
    live = [m for m in range(M) if m != EMPTY_MORPH]
    # which morph an entry belongs to: entry k of vertex v goes to the (v x 7 + k)-th morph that is not the empty one, round and round —
    # written to the file k-major, so inside one morph the vertices come interleaved and a vertex's duplicates lie apart
    lists = [[] for _ in range(M)]
    for k in range(int(rows.max()) if len(rows) else 0):
        for v in np.flatnonzero(rows > k):
            lists[live[(int(v) * 7 + k) % len(live)]].append(int(v))
    stray = {3: V, 20: V + 5, 41: 4000000}                  # three entries past the mesh (the first inside the vertex padding), mid-morph
    for m, bad in stray.items():
        lists[m].insert(len(lists[m]) // 2, bad)
    off = np.zeros(M + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([v for x in lists for v in x], dtype=np.uint32)
    assert off[EMPTY_MORPH] == off[EMPTY_MORPH + 1]
    ptr, src, morph = csr(V, off, idx)
    assert np.array_equal(np.diff(ptr), rows)

    # deltas: |d| in [0.05, 0.1], a random direction, the sign against the row's running sum (in accumulation order)
    E = len(idx)
    d = rng.normal(size=(E, 3))
    d *= (rng.uniform(0.05, 0.1, size=E) / np.linalg.norm(d, axis=1))[:, None]
    w64 = mw.astype(np.float64)
    for v in range(V):
        acc = np.zeros(3)
        for e in range(int(ptr[v]), int(ptr[v + 1])):
            f, w = src[e], w64[morph[e]]
            if w != 0.0 and float(acc @ (w * d[f])) > 0.0:
                d[f] = -d[f]
            acc += w * d[f]
    active = [m for m in range(M) if mw[m] != 0 and m != EMPTY_MORPH][:3]
    mw2 = np.where(np.isin(np.arange(M), active), mw, 0).astype(np.float32)
    return dict(name=name, P=P, V=V, rounds=rounds, rows=rows, mesh=mesh, off=off, idx=idx, d3=d.astype(np.float32), mw=mw, mw2=mw2,
                ptr=ptr, src=src, morph=morph)


_CACHE = {}


def scene(name, P):
    """build(name, P), built once per process and never changed"""
    if (name, P) not in _CACHE:
        _CACHE[(name, P)] = build(name, P)
    return _CACHE[(name, P)]


def padded_skeleton(s, n_bones):
    """the scene's pose on a skeleton of n_bones: the bones behind its own are at rest at the origin, no vertex names them — the
    deformed mesh is the scene's. Returns (world [n_bones, 16], inv_bind [n_bones, 16])."""
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n_bones - B, 1))
    return np.concatenate([s["mesh"]["world"], eye]), np.concatenate([s["mesh"]["inv_bind"], eye])
