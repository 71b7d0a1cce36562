"""Contacts between two PMX box bodies restated in NumPy: the definition rz_physics_contacts(ctx, 3) (kernels/physics.hip, CONTACT = 3) is
held to. A subclass of contact_box_ref.Sim; include/reze_deform.h states the same in words. Everything contact_box_ref.py says holds; what
changes:

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
Pairs with fewer than two boxes run contact_box_ref.Sim._contact itself.
"""
import numpy as np

import contact_box_ref
import physics_ref
from contact_box_ref import MAX_CANDIDATES  # noqa: F401
from physics_ref import EPS, cross, dot, qconj, qrot

SLIDE = 0.05            # 1c: the width, in N.y_k, over which Y's point slides from a vertex to an edge midpoint or the face centre
EDGE_BIAS = 0.95        # 1b: an edge axis must beat the best face axis by this factor
PARALLEL = 1e-6         # 1a: an edge pair with 1 - C_ij^2 at or below this is skipped


def contact_lists(t, box_pairs=True):
    """contact_box_ref.contact_lists(t, boxes=True) with `n_box_box`. box_pairs=True: the rule of contact_ref.contact_lists with boxes
    taking part and pairs of two boxes not removed — follow lists and colouring over the larger pair set, `box_pairs` 0."""
    L = contact_box_ref.contact_lists(t, boxes=True)
    if not box_pairs:
        return dict(L, n_box_box=0)
    nb = t["n_bodies"]
    dyn = physics_ref.is_dynamic(t)
    mask = np.asarray(t["mask"]).astype(np.int64)
    group = np.asarray(t["group"]).astype(np.int64)
    takes = L["takes"]
    takes_box = takes & L["box"]
    bit = np.where(group < 16, np.left_shift(1, np.minimum(group, 15)), 0)
    hit = (bit[:, None] & mask[None, :]) != 0                     # hit[a, b]: a's group is in b's mask
    cand = takes[:, None] & takes[None, :] & hit & hit.T & (dyn[:, None] | dyn[None, :])
    cand &= np.triu(np.ones((nb, nb), dtype=bool), 1)
    n_box_box = int((cand & takes_box[:, None] & takes_box[None, :]).sum())
    a, b = np.nonzero(cand)                                       # lexicographic (a, b)
    both = dyn[a] & dyn[b]
    follow_off = np.zeros(nb + 1, dtype=np.int64)
    fa, fb = a[~both], b[~both]
    owner = np.where(dyn[fa], fa, fb)
    partner = np.where(dyn[fa], fb, fa)
    o = np.lexsort((partner, owner))
    owner, partner = owner[o], partner[o]
    np.add.at(follow_off, owner + 1, 1)
    follow_off = np.cumsum(follow_off)
    pa, pb = a[both], b[both]
    used = [set() for _ in range(nb)]
    colour = np.zeros(len(pa), dtype=np.int64)
    for k in range(len(pa)):
        c = 0
        ua, ub = used[pa[k]], used[pb[k]]
        while c in ua or c in ub:
            c += 1
        ua.add(c); ub.add(c)
        colour[k] = c
    order = np.argsort(colour, kind="stable")
    ncol = int(colour.max()) + 1 if len(pa) else 0
    return dict(L, follow_off=follow_off, follow_idx=partner.astype(np.int64), pairs=np.stack([pa[order], pb[order]], axis=1).reshape(-1, 2),
                colour_off=np.searchsorted(colour[order], np.arange(ncol + 1)).astype(np.int64), n_colours=ncol,
                n_follow=int(len(partner)), n_pairs=int(len(pa)), box_pairs=0, n_box_box=n_box_box)


def refusal(lists):
    """What rz_physics_contacts refuses with RZ_ERR_UNSUPPORTED, or None: the counts as its message gives them"""
    if lists["n_follow"] + lists["n_pairs"] > MAX_CANDIDATES:
        of_boxes = " (%d of them pairs of two boxes)" % lists["n_box_box"] if lists.get("n_box_box") else ""
        return "%d follow entries and %d dynamic pairs%s" % (lists["n_follow"], lists["n_pairs"], of_boxes)
    return None


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


def closest_on_segments(p1, d1, p2, d2):
    """the clamped solve of contact_ref.Sim._contact's step 1: the closest points of rows of segments p1 + s d1 and p2 + t d2"""
    dt = p1.dtype.type
    eps, one, zero = dt(EPS), dt(1), dt(0)
    clamp01 = lambda v: np.minimum(np.maximum(v, zero), one)
    r = p1 - p2
    A, E, F, C, Bq = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
    dega, dege = A <= eps, E <= eps
    sa_, se_ = np.where(dega, one, A), np.where(dege, one, E)
    den = A * E - Bq * Bq
    s_gen = np.where(den > eps, clamp01((Bq * F - C * E) / np.where(den > eps, den, one)), zero)
    t_gen = (Bq * s_gen + F) / se_
    s_lo = clamp01(-C / sa_)
    s_hi = clamp01((Bq - C) / sa_)
    s_g = np.where(t_gen < zero, s_lo, np.where(t_gen > one, s_hi, s_gen))
    t_g = np.where(t_gen < zero, zero, np.where(t_gen > one, one, t_gen))
    s = np.where(dega, zero, np.where(dege, s_lo, s_g))
    t = np.where(dega, np.where(dege, zero, clamp01(F / se_)), np.where(dege, zero, t_g))
    return p1 + d1 * s[:, None], p2 + d2 * t[:, None]


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
    cA_e, cB_e = closest_on_segments(ctr_a - ua, ua + ua, ctr_b - ub, ub + ub)
    w3 = wins[:, None]
    return dict(ok=ok, cA=np.where(w3, cA_e, cA_f), cB=np.where(w3, cB_e, cB_f), n=np.where(w3, n_e, n_f), pen=pen, edge=wins,
                axis=np.where(wins, ke, kf), moved=np.where(wins, 0, moved.sum(axis=1)), considered=considered, face=face, edges=edge)


class Sim(contact_box_ref.Sim):
    """contact_box_ref.Sim with boxes taking part; box_pairs=True: pairs of two boxes are candidates too (rz_physics_contacts(ctx, 3)).
    `kinds` counts the active box - box contacts by ("A" | "B" | "edge", axis | (i, j), coordinates of p' that the clamp of 1c moved —
    0 for an edge); `n_boxbox` is their number, `n_skipped` that of those among them with an edge axis not considered (1a); `apart` counts
    the pairs found separated by the axes (0 .. 5 the faces, 6 .. 14 the edges) whose overlap was not positive."""

    def __init__(self, table, parents, bind, dtype=np.float64, contacts=True, box_pairs=True):
        super().__init__(table, parents, bind, dtype=dtype, contacts=contacts, boxes=True)
        self.box_pairs = box_pairs
        self.kinds, self.apart = {}, {}
        self.n_boxbox = self.n_skipped = 0
        self.lists = L = contact_lists(table, box_pairs=box_pairs)
        n = np.diff(L["follow_off"])
        self.ranks = []
        for k in range(int(n.max()) if len(n) else 0):
            me = np.nonzero(n > k)[0]
            other = L["follow_idx"][L["follow_off"][me] + k]
            self.ranks.append((np.minimum(me, other), np.maximum(me, other)))

    def _contact(self, a, b, xp, qp):
        a, b = np.asarray(a), np.asarray(b)
        two = self.cbox[a] & self.cbox[b]
        n = 0
        if (~two).any():
            n += super()._contact(a[~two], b[~two], xp, qp)
        if two.any():
            n += self._boxbox_contact(a[two], b[two], xp, qp)
        return n

    def _boxbox_contact(self, a, b, xp, qp):
        f = front_end(self.x[a], self.q[a], self.cext[a], self.x[b], self.q[b], self.cext[b])
        # 3 - 7
        ok = self._resolve(a, b, f["cA"], f["cB"], f["n"], f["pen"], f["ok"], xp, qp)
        for k in np.nonzero(ok)[0]:
            ax = int(f["axis"][k])
            key = ("edge", (ax // 3, ax % 3), 0) if f["edge"][k] else ("AB"[ax // 3], ax % 3, int(f["moved"][k]))
            self.kinds[key] = self.kinds.get(key, 0) + 1
        for k in np.nonzero(~f["ok"])[0]:
            key = tuple(np.nonzero(np.concatenate([f["face"][k] <= 0, f["considered"][k] & (f["edges"][k] <= 0)]))[0].tolist())
            self.apart[key] = self.apart.get(key, 0) + 1
        self.n_boxbox += int(ok.sum())
        self.n_skipped += int((ok & ~f["considered"].all(axis=1)).sum())
        return int(ok.sum())
