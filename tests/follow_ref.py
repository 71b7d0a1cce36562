"""Bones below an overridden bone follow it (rz_override_follow; Model.followOverrides on the host): the one definition, in NumPy.

  S   the solved world matrices of an instance: hierarchy, bone morphs and IK, exactly what is solved without the stage
      (tests/ik_ref.py: solve)
  O   the set of that instance's overridden bones, with matrices O_a (hand-fed, or written by the physics step)
  for every bone b outside O that has an ancestor in O, with a = the NEAREST such ancestor along `parents`:
        W_b = O_a (S_a^-1 S_b)        S_a^-1 the rigid inverse (R^T, -R^T p): world matrices here carry no scale
  bones of O take O_a, all others keep S_b.

So an override below another override is absolute: the bones between the two follow the upper one, the bones below the lower one the
lower one. Nothing is evaluated again on the followed pose — NOT covered: append rotation / move whose append parent is overridden or
follows, IK chains below an overridden bone, following (type 0 / 2) bodies on follower bones (the physics step places its bodies on the
un-followed pose), PMX after-physics bones / transform levels.

The arithmetic is the device's (kernels/fk.hip.h: FOLLOW): R = R_a^T R_b, t = R_a^T (p_b - p_a), then the affine product with the upper
three rows of O_a. `dtype` switches every operation between float64 (the reference) and float32 (the conditioning probe), as in ik_ref.py.
Matrices travel as rz_read_world returns them: [B, 16] column-major 4 x 4."""
import numpy as np


def nearest_overridden(parents, bones):
    """per bone: the index INTO `bones` of the entry it takes its matrix from — its own when it is overridden (of several entries for one
    bone the last, as rz_override_world keeps them), else its nearest overridden ancestor's — or -1 when no bone above it is overridden"""
    B = len(parents)
    own = {}
    for k, b in enumerate(bones):
        own[int(b)] = k
    near = [None] * B
    for b in range(B):
        chain, cur = [], b
        while cur >= 0 and near[cur] is None and cur not in own:
            chain.append(cur)
            cur = int(parents[cur])
        found = -1 if cur < 0 else (own[cur] if cur in own else near[cur])
        if cur >= 0 and cur in own:
            near[cur] = own[cur]
        for x in chain:
            near[x] = found
    return near


def followers(parents, bones):
    """[(follower bone, index into `bones` of its nearest overridden ancestor)], ascending by bone: the list the host builds per instance"""
    own = set(int(b) for b in bones)
    near = nearest_overridden(parents, bones)
    return [(b, near[b]) for b in range(len(parents)) if b not in own and near[b] >= 0]


def _rows(m16, dt):
    """upper three rows (R [3,3], p [3]) of a column-major 4 x 4"""
    M = np.asarray(m16, dtype=dt).reshape(4, 4).T
    return M[:3, :3].copy(), M[:3, 3].copy()


def _m16(R, p, dt):
    M = np.zeros((4, 4), dtype=dt)
    M[:3, :3], M[:3, 3], M[3, 3] = R, p, 1
    return M.T.reshape(16)


def follow(parents, solved16, bones, mats16, dtype=np.float64):
    """W [B,16] of one instance: `solved16` = S [B,16], `bones` [n] with `mats16` [n,16] = the override set"""
    dt = np.dtype(dtype).type
    S = np.asarray(solved16, dtype=dt).reshape(-1, 16)
    B = len(parents)
    bones = [int(b) for b in bones]
    O = np.asarray(mats16, dtype=dt).reshape(len(bones), 16)
    near = nearest_overridden(parents, bones)
    own = set(bones)
    W = S.copy()
    for b in range(B):
        k = near[b]
        if k < 0:
            continue
        Ro, po = _rows(O[k], dt)
        if b in own:
            W[b] = _m16(Ro, po, dt)       # (the device writes the upper three rows over 0 0 0 1)
            continue
        Ra, pa = _rows(S[bones[k]], dt)
        Rb, pb = _rows(S[b], dt)
        R = (Ra.T @ Rb).astype(dt)
        t = (Ra.T @ (pb - pa)).astype(dt)
        W[b] = _m16((Ro @ R).astype(dt), (Ro @ t + po).astype(dt), dt)
    return W


def replaced(solved16, bones, mats16):
    """the seam without the stage: overridden bones take their matrices, every other bone keeps S"""
    W = np.array(solved16, dtype=np.float64).reshape(-1, 16).copy()
    for b, m in zip(bones, np.asarray(mats16, dtype=np.float64).reshape(len(bones), 16)):
        W[int(b)] = m
    return W
