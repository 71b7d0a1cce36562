"""Float64 restatement of SDEF skinning (PMX weight type 3) — the definition kernels/sdef.hip and include/reze_deform.h follow.

For an SDEF vertex (saba's PMXModel / MMD, PMX coordinates as they are, no z flip):
  j0, j1, w0, w1  joints of slots 0 / 1 (clamped to B - 1); unorm8 weights normalised over those two slots (sum <= 1e-4: w0 = 1, w1 = 0)
  p~, n           the morphed rest position (oracle morph_dense / morph_sparse) and the rest normal
  S0, S1          palette rows of j0 / j1 (oracle palette: world x inverseBind); Q0, Q1 the unit quaternions of their upper 3 x 3
                  (Shepperd); Q1 = -Q1 when dot(Q0, Q1) < 0; Q = slerp(Q0, Q1, w1) (normalised lerp above cos 0.9995); R = mat3(Q)
  rw = w0 R0 + w1 R1;  cr0 = (C + (C + R0 - rw)) / 2;  cr1 = (C + (C + R1 - rw)) / 2
  P' = R (p~ - C) + w0 S0 (cr0, 1) + w1 S1 (cr1, 1);  N' = normalize(R n) (zero length: the rest normal)
"""
import numpy as np

from oracle import rz_oracle_np as onp


def rows(skin16):
    """[B,16] column-major palette -> [B,3,4] rows (float64)."""
    s = np.asarray(skin16, dtype=np.float64).reshape(-1, 4, 4)     # s[b, col, row]
    return np.transpose(s, (0, 2, 1))[:, :3, :]


def quat_of(m):
    """[N,3,3] -> [N,4] (x y z w), Shepperd's method, normalised."""
    m = np.asarray(m, dtype=np.float64)
    q = np.zeros((len(m), 4))
    for i, a in enumerate(m):
        tr = a[0, 0] + a[1, 1] + a[2, 2]
        if tr > 0:
            s = np.sqrt(tr + 1.0) * 2
            q[i] = ((a[2, 1] - a[1, 2]) / s, (a[0, 2] - a[2, 0]) / s, (a[1, 0] - a[0, 1]) / s, 0.25 * s)
        elif a[0, 0] > a[1, 1] and a[0, 0] > a[2, 2]:
            s = np.sqrt(1.0 + a[0, 0] - a[1, 1] - a[2, 2]) * 2
            q[i] = (0.25 * s, (a[0, 1] + a[1, 0]) / s, (a[0, 2] + a[2, 0]) / s, (a[2, 1] - a[1, 2]) / s)
        elif a[1, 1] > a[2, 2]:
            s = np.sqrt(1.0 + a[1, 1] - a[0, 0] - a[2, 2]) * 2
            q[i] = ((a[0, 1] + a[1, 0]) / s, 0.25 * s, (a[1, 2] + a[2, 1]) / s, (a[0, 2] - a[2, 0]) / s)
        else:
            s = np.sqrt(1.0 + a[2, 2] - a[0, 0] - a[1, 1]) * 2
            q[i] = ((a[0, 2] + a[2, 0]) / s, (a[1, 2] + a[2, 1]) / s, 0.25 * s, (a[1, 0] - a[0, 1]) / s)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def slerp(a, b, t):
    """math.ts Quat.slerp (the hemisphere is chosen by the caller): rows of a, b [N,4], t [N]."""
    c = np.sum(a * b, axis=1)
    out = np.empty_like(a)
    lin = c > 0.9995
    x = a + t[:, None] * (b - a)
    out[lin] = x[lin] / np.linalg.norm(x[lin], axis=1, keepdims=True)
    th0 = np.arccos(np.clip(c[~lin], -1.0, 1.0))
    s = np.sin(th0)
    th = th0 * t[~lin]
    out[~lin] = (np.sin(th0 - th) / s)[:, None] * a[~lin] + (np.sin(th) / s)[:, None] * b[~lin]
    return out


def mat_of(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def sdef(pos_morphed, nrm, joints4, weights4, skin16, idx, c, r0, r1):
    """SDEF positions / normals [n,3] (float64) of the vertices `idx` (rows of the per-vertex arrays)."""
    idx = np.asarray(idx, dtype=np.int64)
    S = rows(skin16)
    bmax = len(S) - 1
    j = np.minimum(np.asarray(joints4)[idx, :2].astype(np.int64), bmax)
    q = np.asarray(weights4)[idx, :2].astype(np.float64) / 255.0
    s = q[:, 0] + q[:, 1]
    ok = s > 1e-4
    w0 = np.where(ok, q[:, 0] / np.where(ok, s, 1.0), 1.0)
    w1 = np.where(ok, q[:, 1] / np.where(ok, s, 1.0), 0.0)
    S0, S1 = S[j[:, 0]], S[j[:, 1]]
    Q0, Q1 = quat_of(S0[:, :, :3]), quat_of(S1[:, :, :3])
    Q1 = np.where((np.sum(Q0 * Q1, axis=1) < 0)[:, None], -Q1, Q1)
    R = mat_of(slerp(Q0, Q1, w1))
    C, A, B = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (c, r0, r1))
    rw = w0[:, None] * A + w1[:, None] * B
    cr0 = (C + (C + A - rw)) / 2
    cr1 = (C + (C + B - rw)) / 2
    p = np.asarray(pos_morphed, dtype=np.float64)[idx]
    n = np.asarray(nrm, dtype=np.float64)[idx]
    aff = lambda M, x: np.einsum("nij,nj->ni", M[:, :, :3], x) + M[:, :, 3]
    P = np.einsum("nij,nj->ni", R, p - C) + w0[:, None] * aff(S0, cr0) + w1[:, None] * aff(S1, cr1)
    N = np.einsum("nij,nj->ni", R, n)
    ln = np.linalg.norm(N, axis=1, keepdims=True)
    good = (ln[:, 0] > 0) & np.isfinite(ln[:, 0])
    N = np.where(good[:, None], N / np.where(ln > 0, ln, 1.0), n)
    return P, N


def morphed(pos, dense=None, sparse=None, weights=None):
    """p~ of the oracle: pos + dense deltas [M,V,3] or sparse (morph_off, vert_idx, delta3), with weights [M] (float32, as the frame)."""
    if dense is not None:
        return onp.morph_dense(dense, weights, pos)
    if sparse is not None:
        mo, vi, d = sparse
        return onp.morph_sparse(len(pos), mo, vi, d, weights, pos)
    return np.asarray(pos, dtype=np.float32)


def frame(pos, nrm, joints4, weights4, world16, inv_bind16, idx, c, r0, r1, dense=None, sparse=None, weights=None):
    """Whole reference frame: the oracle's LBS for every vertex, SDEF rows replaced by sdef(). Returns float64 (pos, nrm)."""
    pm = morphed(pos, dense, sparse, weights)
    skin16 = onp.palette(world16, inv_bind16)
    P, N = onp.skin(pm, nrm, joints4, weights4, skin16)
    P, N = np.asarray(P, dtype=np.float64).copy(), np.asarray(N, dtype=np.float64).copy()
    if len(idx):
        sp, sn = sdef(pm, nrm, joints4, weights4, skin16, idx, c, r0, r1)
        P[np.asarray(idx, dtype=np.int64)] = sp
        N[np.asarray(idx, dtype=np.int64)] = sn
    return P, N
