"""Float64 restatement of QDEF skinning (PMX 2.1 weight type 4, dual-quaternion blending) — the definition kernels/qdef.hip and
include/reze_deform.h follow.

For a listed vertex:
  j0..j3          joints, clamped to B - 1
  w_i             u8_i / isum, as the linear path decodes them (isum == 0: (1, 0, 0, 0)); slots of weight zero contribute nothing
  p~, n           the morphed rest position (oracle morph_dense / morph_sparse) and the rest normal
Per bone j:
  S_j             palette rows (oracle palette: world x inverseBind, 3 x 4)
  q_j             the unit quaternion of the upper 3 x 3 (Shepperd, sdef_ref.quat_of); t_j the fourth column
  d_j             1/2 (t_j, 0) (x) q_j:  d.xyz = 1/2 (q.w t + t x q.xyz),  d.w = -1/2 t . q.xyz
                  (a palette that is not rigid loses its non-rigid part here; PMX poses are rigid)
Blend (Kavan et al., dual-quaternion linear blending):
  pivot           the slot with the largest u8 weight, the lowest slot on ties
  s_i             -1 if dot(q_pivot, q_ji) < 0 else +1
  b_r, b_d        sum_i w_i s_i q_ji, sum_i w_i s_i d_ji;  n_b = |b_r| (>= w_pivot >= 1/4);  c_r = b_r / n_b, c_d = b_d / n_b
  P'              R(c_r) p~ + 2 (c_r.w c_d.xyz - c_d.w c_r.xyz + c_r.xyz x c_d.xyz)
  N'              normalize(R(c_r) n) (zero or non-finite: the rest normal)

The one place where float32 and float64 may legitimately part is the sign s_i when |dot(q_pivot, q_ji)| is close to zero (influences
about 180 degrees apart): margin() returns the smallest such |dot| per vertex over its non-zero-weight slots, and `flip` evaluates the
definition with the other sign for chosen slots.
"""
import numpy as np

import sdef_ref
from oracle import rz_oracle_np as onp

AMBIGUOUS = 1e-2      # a vertex whose margin() is below this may take either sign for each slot under it


def dual_quats(skin16):
    """[B,16] column-major palette -> (q [B,4], d [B,4]) (x y z w), float64."""
    S = sdef_ref.rows(skin16)
    q = sdef_ref.quat_of(S[:, :, :3])
    t = S[:, :, 3]
    d = np.empty_like(q)
    d[:, :3] = 0.5 * (q[:, 3:4] * t + np.cross(t, q[:, :3]))
    d[:, 3] = -0.5 * np.sum(t * q[:, :3], axis=1)
    return q, d


def decode(joints4, weights4, idx, B):
    """(j [n,4] int64 clamped, w [n,4] float64, pivot [n] int64) of the rows idx."""
    j = np.minimum(np.asarray(joints4)[idx].astype(np.int64), B - 1)
    u = np.asarray(weights4)[idx].astype(np.int64)
    isum = u.sum(axis=1)
    w = u / np.where(isum > 0, isum, 1)[:, None].astype(np.float64)
    w[isum == 0] = (1.0, 0.0, 0.0, 0.0)
    pivot = np.argmax(u, axis=1)            # (numpy returns the first of equal maxima: the lowest slot)
    return j, w, pivot


def pivot_dots(joints4, weights4, skin16, idx):
    """dot(q_pivot, q_ji) [n,4] and the slots that count (w_i > 0) [n,4] bool."""
    idx = np.asarray(idx, dtype=np.int64)
    q, _ = dual_quats(skin16)
    j, w, pivot = decode(joints4, weights4, idx, len(q))
    qs = q[j]
    qp = qs[np.arange(len(idx)), pivot]
    return np.einsum("nk,nik->ni", qp, qs), w > 0


def margin(joints4, weights4, skin16, idx):
    """min over the non-zero-weight slots of |dot(q_pivot, q_ji)|, per listed vertex."""
    dots, on = pivot_dots(joints4, weights4, skin16, idx)
    return np.where(on, np.abs(dots), np.inf).min(axis=1)


def qdef(pos_morphed, nrm, joints4, weights4, skin16, idx, flip=None):
    """QDEF positions / normals [n,3] (float64) of the vertices `idx` (rows of the per-vertex arrays). flip [n,4] bool: take the other sign
    s_i for those slots."""
    idx = np.asarray(idx, dtype=np.int64)
    q, d = dual_quats(skin16)
    j, w, pivot = decode(joints4, weights4, idx, len(q))
    qs, ds = q[j], d[j]
    qp = qs[np.arange(len(idx)), pivot]
    s = np.where(np.einsum("nk,nik->ni", qp, qs) < 0, -1.0, 1.0)
    if flip is not None:
        s = np.where(np.asarray(flip, dtype=bool), -s, s)
    ws = w * s
    br = np.einsum("ni,nik->nk", ws, qs)
    bd = np.einsum("ni,nik->nk", ws, ds)
    nb = np.linalg.norm(br, axis=1, keepdims=True)
    cr, cd = br / nb, bd / nb
    R = sdef_ref.mat_of(cr)
    p = np.asarray(pos_morphed, dtype=np.float64)[idx]
    n = np.asarray(nrm, dtype=np.float64)[idx]
    t = 2.0 * (cr[:, 3:4] * cd[:, :3] - cd[:, 3:4] * cr[:, :3] + np.cross(cr[:, :3], cd[:, :3]))
    P = np.einsum("nij,nj->ni", R, p) + t
    N = np.einsum("nij,nj->ni", R, n)
    ln = np.linalg.norm(N, axis=1, keepdims=True)
    good = (ln[:, 0] > 0) & np.isfinite(ln[:, 0])
    N = np.where(good[:, None], N / np.where(ln > 0, ln, 1.0), n)
    return P, N


def frame(pos, nrm, joints4, weights4, world16, inv_bind16, idx, dense=None, sparse=None, weights=None, flip=None):
    """Whole reference frame: the oracle's LBS for every vertex, the listed rows replaced by qdef(). Returns float64 (pos, nrm)."""
    pm = sdef_ref.morphed(pos, dense, sparse, weights)
    skin16 = onp.palette(world16, inv_bind16)
    P, N = onp.skin(pm, nrm, joints4, weights4, skin16)
    P, N = np.asarray(P, dtype=np.float64).copy(), np.asarray(N, dtype=np.float64).copy()
    if len(idx):
        qp, qn = qdef(pm, nrm, joints4, weights4, skin16, idx, flip)
        P[np.asarray(idx, dtype=np.int64)] = qp
        N[np.asarray(idx, dtype=np.int64)] = qn
    return P, N
