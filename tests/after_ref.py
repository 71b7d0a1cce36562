"""PMX after-physics bones solved again behind the overrides (rz_upload_after_physics; kernels/after.hip: rz_fk_after_kernel; on the host
Model.solveAfterPhysics): the one definition, in NumPy.

Inputs per instance
  F      the world matrices [B,16] as the frame leaves them without the stage: follow_ref.follow or follow_ref.replaced on ik_ref.solve
  O      the instance's override set (bones)
  q, t   the local pose AFTER bone morphs
  the topology: parents, bind translations, append parent / ratio / move
  A      the ordered list of after-physics bones (ascending transform level, then index: Model.afterPhysicsOrder)

Evaluation, for b in A, in list order:
  b in O: skipped — an overridden bone is never re-evaluated
  P = F[parent(b)], identity for a root
  with an append parent a: a's local transform AS FINALLY POSED, from the current F:
      R_a = rot(F[parent(a)])^T rot(F[a]),   t_a = rot(F[parent(a)])^T (pos(F[a]) - pos(F[parent(a)])) - bind_a   (a root a: F[a] itself)
      q_a = quat(R_a): the branch on the largest of trace, m00, m11, m22, then normalised (quat_of below)
    and on exactly as the first solve's local matrix (kernels/fk.hip.h: fk_local_matrix; ik_ref.Hierarchy.local) with q_a and t_a in the
    place of the append parent's pose quaternion and translation: ratio clamped to [-1, 1] for the rotation, conjugate for a negative
    ratio, slerp from the identity along the shorter arc, |ratio| <= 1e-6 = no append, the UNclamped ratio for append move:
      L = T(bind_b + t_b) R(A) R(q_b) T(add)
  F[b] = P L; later entries read the new F[b].

Consequences
  * a listed bone below an overridden bone follows it through its own local transform, not rigidly;
  * a helper that appends from an overridden bone, a follower, an IK link or an earlier listed bone sees where that bone really is;
  * where the append parent itself takes append, this stage sees its FULL local rotation, while the first solve, following the reference,
    leaves the parent's own append out: the one place where the two passes differ by more than rounding;
  * the stage runs only while the instance's context holds at least one override entry: without overrides the first solve is the answer
    already, and frames stay what they were.

NOT covered: non-listed bones below a listed bone keep their matrices (MMD does the same); IK chains whose bones are listed are not solved
again after physics; following bodies on listed bones are placed on the first solve; transform levels among before-physics bones (the
first solve reads pose quaternions, which adds no ordering dependency); an append parent whose final local rotation lies near 180
degrees — the shorter-arc choice flips there, exactly as it does in the first solve (test scenes keep at least 15 degrees away from it).

`dtype` switches every operation between float64 (the reference) and float32 (the conditioning probe), as in ik_ref.py and follow_ref.py.
Matrices travel as rz_read_world returns them: [B, 16] column-major 4 x 4."""
import numpy as np

from follow_ref import _m16, _rows
from ik_ref import _qmat, _slerp_id


def quat_of(R, dt):
    """x y z w of a rotation matrix: the branch on the largest of trace, m00, m11, m22, then normalised"""
    m = np.asarray(R, dtype=dt)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    one, two, quarter = dt(1), dt(2), dt(0.25)
    if tr >= m[0, 0] and tr >= m[1, 1] and tr >= m[2, 2]:
        s = np.sqrt(tr + one) * two
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, quarter * s]
    elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
        s = np.sqrt(one + m[0, 0] - m[1, 1] - m[2, 2]) * two
        q = [quarter * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] >= m[2, 2]:
        s = np.sqrt(one + m[1, 1] - m[0, 0] - m[2, 2]) * two
        q = [(m[0, 1] + m[1, 0]) / s, quarter * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = np.sqrt(one + m[2, 2] - m[0, 0] - m[1, 1]) * two
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, quarter * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q, dtype=dt)
    return (q / np.sqrt(q.dot(q))).astype(dt)


def effective_append(ap, ratio, b):
    """the append parent bone b's local matrix reads, or -1: none named, or a ratio that leaves none in effect"""
    if ap is None or int(ap[b]) < 0 or int(ap[b]) >= len(ap):
        return -1
    r = np.float32(1.0) if ratio is None else np.float32(ratio[b])
    return int(ap[b]) if abs(min(max(r, np.float32(-1)), np.float32(1))) > np.float32(1e-6) else -1


def levels(parents, ap, ratio, order):
    """per entry of `order` (list order) its dependency level: 1 + the largest level over EARLIER entries that are its parent, append
    parent or append parent's parent, 0 if there is none. Raises ValueError naming the bone when one of those three is listed LATER, on
    a bone listed twice and on an index out of range — the refusals of rz_upload_after_physics."""
    B = len(parents)
    pos = {}
    for k, b in enumerate(order):
        b = int(b)
        if b < 0 or b >= B:
            raise ValueError("entry %d names bone %d of %d" % (k, b, B))
        if b in pos:
            raise ValueError("bone %d is listed twice" % b)
        pos[b] = k
    lv = []
    for k, b in enumerate(order):
        b = int(b)
        a = effective_append(ap, ratio, b)
        reads = [int(parents[b]), a, int(parents[a]) if a >= 0 else -1]
        cur = 0
        for r in reads:
            if r < 0 or r == b or r not in pos:
                continue
            if pos[r] > k:
                raise ValueError("bone %d is evaluated before bone %d, which it reads" % (b, r))
            cur = max(cur, lv[pos[r]] + 1)
        lv.append(cur)
    return lv


def sorted_entries(parents, ap, ratio, order):
    """(bones sorted by (level, bone), level offsets): the order the device's records are kept in"""
    lv = levels(parents, ap, ratio, order)
    idx = sorted(range(len(order)), key=lambda k: (lv[k], int(order[k])))
    n_levels = max(lv) + 1 if lv else 0
    off = [0] * (n_levels + 1)
    for l in lv:
        off[l + 1] += 1
    for l in range(n_levels):
        off[l + 1] += off[l]
    return [int(order[k]) for k in idx], off


def solve(parents, bind, q, t, ap, ratio, move, F16, overridden, order, dtype=np.float64):
    """F [B,16] of one instance behind the stage. `q`, `t` the local pose after bone morphs (t None: zeros), `F16` the frame without the
    stage, `overridden` the instance's overridden bones, `order` the list A. Whether the stage runs at all is the CONTEXT's to say (one
    override entry in any instance of a crowd): an instance without overrides of its own is evaluated like every other."""
    dt = np.dtype(dtype).type
    B = len(parents)
    F = np.array(F16, dtype=dt).reshape(B, 16).copy()
    O = set(int(b) for b in overridden)
    bind = np.asarray(bind, dtype=dt).reshape(B, 3)
    q = np.asarray(q, dtype=dt).reshape(B, 4)
    t = np.zeros((B, 3), dtype=dt) if t is None else np.asarray(t, dtype=dt).reshape(B, 3)
    for b in order:
        b = int(b)
        if b in O:
            continue
        Rb = _qmat(q[b], dt)
        add = np.zeros(3, dtype=dt)
        a = effective_append(ap, ratio, b)
        if a >= 0:
            Ra, pa = _rows(F[a], dt)
            g = int(parents[a])
            if g >= 0:
                Rg, pg = _rows(F[g], dt)
                Ra, pa = (Rg.T @ Ra).astype(dt), (Rg.T @ (pa - pg)).astype(dt)
            ta = (pa - bind[a]).astype(dt)
            qa = quat_of(Ra, dt)
            raw = dt(ratio[b]) if ratio is not None else dt(1)
            r = min(max(raw, dt(-1)), dt(1))
            if move is not None and move[b]:
                add = (ta * raw).astype(dt)
            if r < 0:
                qa = qa.copy()
                qa[:3] = -qa[:3]
            Rb = (_qmat(_slerp_id(qa, abs(r), dt), dt) @ Rb).astype(dt)
        tl = (bind[b] + t[b] + Rb @ add).astype(dt)
        p = int(parents[b])
        if p >= 0:
            Rp, pp = _rows(F[p], dt)
            F[b] = _m16((Rp @ Rb).astype(dt), (Rp @ tl + pp).astype(dt), dt)
        else:
            F[b] = _m16(Rb, tl, dt)
    return F
