"""Contacts between two PMX box bodies restated in NumPy: the definition rz_physics_contacts(ctx, 3) (kernels/physics.hip, CONTACT = 3) is
held to. The front end contact_ref.Sim runs under mode 3 for a pair of two boxes (Sim._boxbox_contact); include/reze_deform.h states the
same in words. Everything contact_box_ref.py says holds; what changes:

Pairs     a pair of two boxes that the rule pairs is a candidate like any other: it enters the follow lists and the coloured dynamic pairs,
          counts toward the 65 536-candidate limit and is counted in `n_box_box`; `box_pairs`, the pairs left out, is 0.
One contact of two boxes, A the lower index, step 1. a_i = q_A axis_i, b_j = q_B axis_j (by qrot), half extents eA, eB, t = x_B - x_A,
C_ij = a_i.b_j, tA_i = a_i.t, tB_j = b_j.t:
  a. overlaps of the 15 axes (sums from the left):
       face A_i    o = (eA_i + (eB_0 |C_i0| + eB_1 |C_i1| + eB_2 |C_i2|)) - |tA_i|
       face B_j    o = ((eA_0 |C_0j| + eA_1 |C_1j| + eA_2 |C_2j|) + eB_j) - |tB_j|
       edge (i, j) i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1, j2 likewise, l2 = 1 - C_ij C_ij; considered only when l2 > 1e-6:
                   o = ((eA_i1 |C_i2,j| + eA_i2 |C_i1,j| + eB_j1 |C_i,j2| + eB_j2 |C_i,j1|) - |tA_i2 C_i1,j - tA_i1 C_i2,j|) / sqrt(l2)
     any considered o <= 0: no contact
  b. the face axis is the first smallest in the order A0 A1 A2 B0 B1 B2, the edge axis the first smallest in the order (0,0), (0,1) ..
     (2,2); the edge wins only when one is considered and o_edge < 0.95 o_face; pen is the chosen o
  c. face axis i of the reference box X (Y the other box, y_k its axes): s = tA_i when X is A, -tB_i when X is B (the component along the
     axis of the vector from x_X to x_Y); sg = +1 when s >= 0, else -1; N = axis sg;
       w_k = clamp((N.y_k) / 0.05, -1, 1) eY_k;  p = ((x_Y - y_0 w_0) - y_1 w_1) - y_2 w_2
       (a vertex of Y, sliding continuously to an edge midpoint or the face centre as Y's face becomes parallel to X's)
       p' = clamp(q_X^-1 (p - x_X), -eX, eX) with component i set to sg eX_i;  cX = x_X + q_X p';  cY = cX - N pen
     n = N when X is A, else -N; cA, cB = cX, cY when X is A, else cY, cX
  d. edge axis (i, j): c = a_i x b_j, L = c / |c|; n = L when t.L >= 0, else -L;
       A's edge: centre (x_A + a_i1 (s_i1 eA_i1)) + a_i2 (s_i2 eA_i2), s_k = +1 when a_k.n >= 0, else -1; u_A = a_i eA_i
       B's edge: centre (x_B - b_j1 (s'_j1 eB_j1)) - b_j2 (s'_j2 eB_j2), s'_k from b_k.n in the same way; u_B = b_j eB_j
       cA, cB: the closest points of the segments P = centre - u, d = u + u by the clamped solve of contact_ref.py's step 1
  then steps 3 - 7 of contact_ref.py with both radii 0 and this n and pen, without the dist > EPS test.
Pairs with fewer than two boxes run contact_ref.Sim._box_contact and Sim._contact themselves.
"""
import numpy as np

import contact_ref
from physics_ref import cross, dot, qconj, qrot

SLIDE = 0.05            # 1c: the width, in N.y_k, over which Y's point slides from a vertex to an edge midpoint or the face centre
EDGE_BIAS = 0.95        # 1b: an edge axis must beat the best face axis by this factor
PARALLEL = 1e-6         # 1a: an edge pair with 1 - C_ij^2 at or below this is skipped


def axes_of(q):
    """the three body axes of rows of rotations, by qrot: [3][n, 3]"""
    out = []
    for k in range(3):
        u = np.zeros((len(q), 3), dtype=q.dtype)
        u[:, k] = 1
        out.append(qrot(q, u))
    return out


def overlaps(xA, qA, eA, xB, qB, eB):
    """Step 1a for rows of box pairs: (face overlaps [n, 6] in the order A0 A1 A2 B0 B1 B2, edge overlaps [n, 9] in the order (0,0) ..
    (2,2), considered [n, 9], and what the later steps reuse)"""
    dt = xA.dtype.type
    one = dt(1)
    a, b = axes_of(qA), axes_of(qB)
    t = xB - xA
    C = [[dot(a[i], b[j]) for j in range(3)] for i in range(3)]
    AC = [[np.abs(C[i][j]) for j in range(3)] for i in range(3)]
    tA, tB = [dot(a[i], t) for i in range(3)], [dot(b[j], t) for j in range(3)]
    face = [(eA[:, i] + ((eB[:, 0] * AC[i][0] + eB[:, 1] * AC[i][1]) + eB[:, 2] * AC[i][2])) - np.abs(tA[i]) for i in range(3)]
    face += [(((eA[:, 0] * AC[0][j] + eA[:, 1] * AC[1][j]) + eA[:, 2] * AC[2][j]) + eB[:, j]) - np.abs(tB[j]) for j in range(3)]
    edge, considered = [], []
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            l2 = one - C[i][j] * C[i][j]
            ok = l2 > dt(PARALLEL)
            r = ((eA[:, i1] * AC[i2][j] + eA[:, i2] * AC[i1][j]) + eB[:, j1] * AC[i][j2]) + eB[:, j2] * AC[i][j1]
            edge.append((r - np.abs(tA[i2] * C[i1][j] - tA[i1] * C[i2][j])) / np.sqrt(np.where(ok, l2, one)))
            considered.append(ok)
    return np.stack(face, axis=1), np.stack(edge, axis=1), np.stack(considered, axis=1), (a, b, t, tA, tB)


def choose(face, edge, considered):
    """Steps 1a's verdict and 1b: (contact [n], the face axis 0 .. 5, the edge axis 0 .. 8 (0 when none is considered), whether the edge
    wins, pen)"""
    zero = face.dtype.type(0)
    sep = (face <= zero).any(axis=1) | (considered & (edge <= zero)).any(axis=1)
    kf = np.argmin(face, axis=1)                                                   # the first smallest
    of = face[np.arange(len(face)), kf]
    masked = np.where(considered, edge, np.inf)
    ke = np.argmin(masked, axis=1)
    oe = edge[np.arange(len(edge)), ke]
    wins = considered.any(axis=1) & (oe < face.dtype.type(EDGE_BIAS) * of)
    return ~sep, kf, ke, wins, np.where(wins, oe, of)


def front_end(xA, qA, eA, xB, qB, eB):
    """Step 1 for rows of box pairs, A the lower index: a dict with `ok` (in contact), the contact points `cA` and `cB`, the normal `n`
    from A to B and `pen`; and, for the tests: `edge` (the edge axis won), `axis` (0 .. 5 in the order A0 .. B2, or 0 .. 8 for an edge),
    `moved` (coordinates of p' that the clamp of 1c moved, 0 for an edge), `considered` [n, 9], `face` [n, 6] and `edges` [n, 9] (the
    overlaps)"""
    dt = xA.dtype.type
    one, zero = dt(1), dt(0)
    rows = np.arange(len(xA))
    # 1a, 1b
    face, edge, considered, (ax_a, ax_b, t, tA, tB) = overlaps(xA, qA, eA, xB, qB, eB)
    ok, kf, ke, wins, pen = choose(face, edge, considered)
    A3, B3 = np.stack(ax_a, axis=1), np.stack(ax_b, axis=1)                   # [n, 3 axes, 3]
    # 1c. the reference box X and the incident box Y
    isA = kf < 3
    i = np.where(isA, kf, kf - 3)
    sel = isA[:, None]
    xX, qX, eX, xY, eY = np.where(sel, xA, xB), np.where(sel, qA, qB), np.where(sel, eA, eB), np.where(sel, xB, xA), np.where(sel, eB, eA)
    X3, Y3 = np.where(isA[:, None, None], A3, B3), np.where(isA[:, None, None], B3, A3)
    s = np.where(isA, np.stack(tA, axis=1)[rows, i], -np.stack(tB, axis=1)[rows, i])
    sg = np.where(s >= zero, one, -one)
    N = X3[rows, i] * sg[:, None]
    p = xY
    for k in range(3):
        w = np.minimum(np.maximum(dot(N, Y3[:, k]) / dt(SLIDE), -one), one) * eY[:, k]
        p = p - Y3[:, k] * w[:, None]
    raw = qrot(qconj(qX), p - xX)
    pl = np.minimum(np.maximum(raw, -eX), eX)
    pl[rows, i] = sg * eX[rows, i]
    cX = xX + qrot(qX, pl)
    cY = cX - N * pen[:, None]
    n_f = np.where(sel, N, -N)
    cA_f, cB_f = np.where(sel, cX, cY), np.where(sel, cY, cX)
    moved = np.abs(raw) > eX
    moved[rows, i] = False
    # 1d. the edges
    ie, je = ke // 3, ke % 3
    ai, bj = A3[rows, ie], B3[rows, je]
    c = cross(ai, bj)
    ln = np.sqrt(dot(c, c))
    Lv = c / np.where(wins, ln, one)[:, None]
    n_e = np.where((dot(t, Lv) >= zero)[:, None], Lv, -Lv)
    ctr_a, ctr_b = xA, xB
    for d in (1, 2):
        ka, kb = (ie + d) % 3, (je + d) % 3
        ak, bk = A3[rows, ka], B3[rows, kb]
        sa = np.where(dot(ak, n_e) >= zero, one, -one)
        sb = np.where(dot(bk, n_e) >= zero, one, -one)
        ctr_a = ctr_a + ak * (sa * eA[rows, ka])[:, None]
        ctr_b = ctr_b - bk * (sb * eB[rows, kb])[:, None]
    ua, ub = ai * eA[rows, ie][:, None], bj * eB[rows, je][:, None]
    cA_e, cB_e = contact_ref.closest_on_segments(ctr_a - ua, ua + ua, ctr_b - ub, ub + ub)
    w3 = wins[:, None]
    return dict(ok=ok, cA=np.where(w3, cA_e, cA_f), cB=np.where(w3, cB_e, cB_f), n=np.where(w3, n_e, n_f), pen=pen, edge=wins,
                axis=np.where(wins, ke, kf), moved=np.where(wins, 0, moved.sum(axis=1)), considered=considered, face=face, edges=edge)
