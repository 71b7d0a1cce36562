"""Small skeletons with IK tables at the edges of the device stage's launch shape (kernels/ik.hip.h), for tests/test_gpu_ik.py and the
conditioning check in tests/test_ik_cpu.py: a path of 64 bones (one bone per lane of the wave that solves the chain), a stage of nine
independent chains (a workgroup has four waves: a wave takes a second and a third chain), a chain whose outermost link is a root bone,
limits given max first, a per-step angle of 0 and a table of three stages. Every builder returns a mesh dict as synth.make_mesh does
(pos, nrm, joints, weights, parents, bind, inv_bind) with `chains` beside it."""
import numpy as np

import ik_ref

KNEE_LO, KNEE_HI = [float(np.float32(-np.pi)), 0.0, 0.0], [float(np.float32(-0.5 * np.pi / 180.0)), 0.0, 0.0]


def _mesh(parents, bind, chains, n_verts, seed):
    """n_verts vertices near the bones, BDEF1 / BDEF2 on a bone and its parent"""
    rng = np.random.default_rng(seed)
    parents = np.array(parents, dtype=np.int32)
    bind = np.array(bind, dtype=np.float32)
    B = len(parents)
    bp = ik_ref.bind_positions(parents, bind)
    vb = np.arange(n_verts) * B // n_verts if n_verts >= B else rng.integers(0, B, size=n_verts)
    pos = (bp[vb] + rng.uniform(-0.3, 0.3, size=(n_verts, 3))).astype(np.float32)
    nrm = rng.normal(size=(n_verts, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    jn = np.zeros((n_verts, 4), dtype=np.uint16)
    wt = np.zeros((n_verts, 4), dtype=np.uint8)
    jn[:, 0], jn[:, 1] = vb, np.maximum(parents[vb], 0)
    w0 = rng.integers(128, 256, size=n_verts)
    w0[::3] = 255
    wt[:, 0], wt[:, 1] = w0, 255 - w0
    inv_bind = np.zeros((B, 16), dtype=np.float32)
    inv_bind[:, 0] = inv_bind[:, 5] = inv_bind[:, 10] = inv_bind[:, 15] = 1
    inv_bind[:, 12:15] = -bp.astype(np.float32)
    return dict(pos=pos, nrm=nrm, joints=jn, weights=wt, parents=parents, bind=bind, inv_bind=inv_bind, chains=chains)


def free(bone):
    return dict(bone=int(bone), min=None, max=None)


def long_chain(n=64, links=(40, 20, 1), n_verts=260, seed=3):
    """Bone 0 is the root; bones 1 .. n hang from it in one line, 0.25 apart; bone n + 1, the goal, is a child of the root. One chain with
    its effector at bone n and links at `links` (outwards, the last one bone 1): the path is bones 1 .. n, so lane n - 1 holds the effector
    and every bone between two links stays rigid. The first link is limited."""
    parents = [-1] + list(range(n)) + [0]
    bind = [[0.0, 16.0, 0.0]] + [[0.0, -0.25, 0.0]] * n + [[4.0, -9.0, 2.0]]
    ll = [free(b) for b in links]
    if len(ll) > 1:
        ll[0] = dict(bone=int(links[0]), min=[-1.0, -0.8, -1.0], max=[1.0, 0.8, 1.0])
    chains = [dict(goal=n + 1, effector=n, loops=8, limit_angle=1.0, links=ll)]
    return _mesh(parents, bind, chains, n_verts, seed)


def nine_legs(n_legs=9, n_verts=300, seed=4):
    """A root with `n_legs` legs (hip, knee, ankle; thigh and shin 5 long, the knee limited to x as in synth.make_leg_rig) around it and one
    goal per leg under the root: no chain reads what another moves, so all of them form one stage."""
    parents, bind, chains = [-1], [[0.0, 12.0, 0.0]], []
    for k in range(n_legs):
        a = 2 * np.pi * k / n_legs
        hip = len(parents)
        parents += [0, hip, hip + 1]
        bind += [[2.0 * np.cos(a), -1.0, 2.0 * np.sin(a)], [0.0, -5.0, -0.1], [0.0, -5.0, 0.1]]
    for k in range(n_legs):
        a = 2 * np.pi * k / n_legs
        hip = 1 + 3 * k
        parents.append(0)
        bind.append([2.0 * np.cos(a), -9.0, 2.0 * np.sin(a) - 1.0])
        chains.append(dict(goal=len(parents) - 1, effector=hip + 2, loops=20, limit_angle=2.0, links=[dict(bone=hip + 1, min=KNEE_LO, max=KNEE_HI), free(hip)]))
    return _mesh(parents, bind, chains, n_verts, seed)


def root_link(n_verts=64, seed=5):
    """A leg whose thigh is a root bone (parent -1), the outermost link of its chain: the wave solves the path under identity parent rows.
    The goal is a root bone of its own; two more bones hang from the ankle and follow."""
    parents = [-1, 0, 1, -1, 2, 4]
    bind = [[0.0, 11.0, 0.0], [0.0, -5.0, -0.1], [0.0, -5.0, 0.1], [0.5, 2.5, -1.0], [0.0, -1.0, -1.5], [0.0, 0.0, -1.0]]
    chains = [dict(goal=3, effector=2, loops=20, limit_angle=2.0, links=[dict(bone=1, min=KNEE_LO, max=KNEE_HI), free(0)])]
    return _mesh(parents, bind, chains, n_verts, seed)


def three_stages(n_verts=96, seed=6):
    """The left leg of the leg rig with a tip chain below the toe: leg chain (knee, leg), toe chain (ankle), tip chain (a link below the toe).
    The toe chain's effector hangs below the leg chain's links and the tip chain's below the toe chain's: three stages, each on the pose
    the stage before left."""
    #          root centre leg knee ankle toe tip tip_end leg_ik toe_ik tip_ik
    parents = [-1, 0, 1, 2, 3, 4, 5, 6, 0, 8, 9]
    bind = [[0, 0, 0], [0, 12, 0], [1, -1, 0], [0, -5, -0.1], [0, -5, 0.1], [0, -1, -1.5], [0, 0, -1.0], [0, 0.2, -1.0], [1, 1, 0], [0, -1, -1.5], [0, 0.3, -1.8]]
    chains = [dict(goal=8, effector=4, loops=40, limit_angle=2.0, links=[dict(bone=3, min=KNEE_LO, max=KNEE_HI), free(2)]),
              dict(goal=9, effector=5, loops=3, limit_angle=4.0, links=[free(4)]),
              dict(goal=10, effector=7, loops=6, limit_angle=1.0, links=[dict(bone=6, min=[-0.6, -0.4, -0.6], max=[0.6, 0.4, 0.6])])]
    return _mesh(parents, bind, chains, n_verts, seed)


def pose(mesh, seed, angle=0.3, reach=1.0):
    """every bone turned by up to `angle` about a random axis, every goal moved by up to `reach` per axis"""
    rng = np.random.default_rng(4000 + seed)
    B = len(mesh["parents"])
    ax = rng.normal(size=(B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = rng.uniform(-angle, angle, size=B)
    q = np.concatenate([ax * np.sin(a / 2)[:, None], np.cos(a / 2)[:, None]], axis=1).astype(np.float32)
    t = np.zeros((B, 3), dtype=np.float32)
    for ch in mesh["chains"]:
        t[ch["goal"]] = rng.uniform(-reach, reach, size=3)
    return q, t


def poses(mesh, first, n=8):
    return [pose(mesh, first + k) for k in range(n)]


def swapped(chains, chain, link):
    """the same table with one link's limits given max first"""
    out = [dict(ch, links=[dict(ln) for ln in ch["links"]]) for ch in chains]
    ln = out[chain]["links"][link]
    ln["min"], ln["max"] = ln["max"], ln["min"]
    return out


def unlimited(chains, **kw):
    return [dict(ch, links=[free(ln["bone"]) for ln in ch["links"]], **kw) for ch in chains]
