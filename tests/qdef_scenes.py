"""The scenes tests/test_gpu_qdef.py runs, built on the CPU so that tests/test_qdef_cpu.py can hold the reference's own condition (few
vertices with a sign s_i that float32 and float64 may choose differently) on every one of them.

2 049 vertices, 300 bones (a staging lane of the pass converts two bones), 9 dense and 9 sparse morphs (one batch of 8 plus a tail), a
table of about 600 vertices with two, three and four influences that includes vertex 0 and vertex V - 1 and is no multiple of 256,
3 instances for crowds; a pose that twists 40 bones by 60-120 degrees against their parents."""
import numpy as np

V, B, M, I = 2049, 300, 9, 3
BIG_B = 3242          # the largest skeleton the library accepts


def axis_angle(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]]).astype(np.float32)


def slerp(a, b, t):
    """math.ts Quat.slerp in float64: rows of a, b [N,4]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).copy()
    c = np.sum(a * b, axis=1)
    b[c < 0] *= -1
    c = np.abs(c)
    out = a + t * (b - a)
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    far = c <= 0.9995
    th0 = np.arccos(np.clip(c[far], -1, 1))
    out[far] = (np.sin(th0 - th0 * t) / np.sin(th0))[:, None] * a[far] + (np.sin(th0 * t) / np.sin(th0))[:, None] * b[far]
    return out.astype(np.float32)


def twisted(mesh, n_bones, seed, count=40, lo=60, hi=120):
    rng = np.random.default_rng(seed)
    quats = mesh["quats"].copy()
    for b in rng.choice(np.arange(1, n_bones), size=min(count, n_bones - 1), replace=False):
        quats[b] = axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(lo, hi)))
    return quats


def with_three_influences(mesh):
    """The synthetic mesh has two- and four-influence vertices; every third four-influence vertex loses its last weight, and vertex 0 and
    the last vertex get three and four influences (the last one with tied weights: the pivot is slot 0)."""
    w = mesh["weights"].copy()
    four = np.flatnonzero((w > 0).sum(axis=1) == 4)
    w[four[::3], 3] = 0
    w[0] = (100, 80, 75, 0)
    w[-1] = (64, 64, 64, 63)
    return dict(mesh, weights=w)


def table(synth, mesh, frac=0.29, seed=9):
    idx = np.union1d(synth.make_qdef(mesh, frac, seed=seed), [0, len(mesh["weights"]) - 1]).astype(np.uint32)
    assert len(idx) % 256 != 0
    return idx


def build(synth):
    mesh = with_three_influences(synth.make_mesh(V, B))
    idx = table(synth, mesh)
    quats = twisted(mesh, B, 21)
    world = synth.fk_world(mesh["parents"], mesh["bind"], quats).reshape(B, 16)
    dense, mw = synth.make_morphs_dense(V, M)
    sparse = synth.make_morphs_sparse(V, M, density=0.2)
    rng = np.random.default_rng(8)
    cq = np.stack([quats] * I).copy()                        # per-instance poses of the crowds
    for i in range(1, I):
        cq[i, rng.choice(np.arange(1, B), 10, replace=False)] = [axis_angle(rng.normal(size=3), 1.0 + 0.1 * i) for _ in range(10)]
    cworld = np.stack([synth.fk_world(mesh["parents"], mesh["bind"], q).reshape(B, 16) for q in cq])
    # the motion of the sampled poses: key 0 = the twisted pose, key 1 = another one, 10 frames apart
    rng = np.random.default_rng(5)
    key1 = np.stack([axis_angle(rng.normal(size=3), 1.5) for _ in range(B)])
    return dict(mesh=mesh, idx=idx, quats=quats, world=world, dense=dense, mw=mw, sparse=sparse, cq=cq, cworld=cworld, key1=key1,
                sample_t=7.5, crowd_t=np.linspace(0, 10, I), synth=synth)


def one_bone(synth):
    mesh = synth.make_mesh(300, 1)
    q = axis_angle([1, 2, 3], 1.0)[None]
    return dict(mesh=mesh, idx=np.arange(0, 300, 2, dtype=np.uint32), world=synth.fk_world(mesh["parents"], mesh["bind"], q).reshape(1, 16))


def big_skeleton(synth):
    mesh = with_three_influences(synth.make_mesh(1500, BIG_B))
    quats = twisted(mesh, BIG_B, 3, count=400)
    idx = table(synth, mesh, frac=0.05)
    return dict(mesh=mesh, idx=idx, world=synth.fk_world(mesh["parents"], mesh["bind"], quats).reshape(BIG_B, 16))


def poses(synth):
    """(name, mesh, table, world16 [B,16]) of every pose a GPU test deforms with a table (device-solved ones restated on the host)."""
    s = build(synth)
    m = s["mesh"]
    fk = lambda q: synth.fk_world(m["parents"], m["bind"], q).reshape(B, 16)     # noqa: E731
    out = [("twisted", m, s["idx"], s["world"]), ("all vertices", m, np.arange(V, dtype=np.uint32), s["world"])]
    out.append(("sampled", m, s["idx"], fk(slerp(s["quats"], s["key1"], s["sample_t"] / 10.0))))
    for i in range(I):
        out.append(("crowd %d" % i, m, s["idx"], s["cworld"][i]))
        out.append(("animated crowd %d" % i, m, s["idx"], fk(slerp(s["cq"][0], s["cq"][1], s["crowd_t"][i] / 10.0))))
    o, g = one_bone(synth), big_skeleton(synth)
    out.append(("one bone", o["mesh"], o["idx"], o["world"]))
    out.append(("3242 bones", g["mesh"], g["idx"], g["world"]))
    return out
