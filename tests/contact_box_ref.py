"""Contacts with PMX box bodies restated in NumPy: the definition rz_physics_contacts(ctx, 2) (kernels/physics.hip, CONTACT = 2) is held to.
A subclass of contact_ref.Sim; include/reze_deform.h states the same in words. Everything contact_ref.py says holds; what changes:

Shapes    a box is shape 1: the set |y_i| <= e_i in its own frame, e = size (three half extents, as the inertia reads them). It takes part
          when all three are > 0 and its mask is nonzero, and counts as a shape of radius 0 with no segment. A box with a nonzero mask that
          takes no part (an extent of 0) is counted in `boxes`.
Pairs     the same rule, now with sphere - box and capsule - box in either index order, the box following or dynamic. A pair of two boxes
          is no candidate: it is counted in `box_pairs` when it would have been one by every other condition.
One contact with a box X (half extents e) and a round shape R (segment P + s d, s in [0, 1], radius r; a sphere: d = 0), step 1:
  a. the segment in the box frame: P' = q_X^-1 (P - x_X), d' = q_X^-1 d
  b. c(s) = P' + s d', g(s) = c - clamp(c, -e, e), f(s) = g(s).d' (half the derivative of the squared distance, monotone):
       f(0) >= 0: s = 0;  else f(1) <= 0: s = 1;  else 24 bisection steps on [lo, hi] = [0, 1]: m = (lo + hi) / 2, f(m) > 0: hi = m, else
       lo = m;  s = (lo + hi) / 2
  c. b' = clamp(c(s), -e, e); the round shape's point is P + s d (in world space), the box's x_X + q_X b'
  d. shallow, |c(s) - b'| > EPS: steps 2 - 7 of contact_ref.py unchanged (A the lower index, n from cA to cB, the box's radius 0)
  e. deep, |c(s) - b'| <= EPS (the centre line is inside the box): the axis i with the smallest e_i - |c_i| (the first of x, y, z wins a tie),
     sg = +1 when c_i >= 0, else -1; outward normal N = sg q_X axis_i; the box's point is c with component i set to sg e_i (turned into
     world space as in c); pen = r + (e_i - |c_i|); n = N when the box is A, -N when it is B (from A to B); steps 3 - 7 with this n and pen,
     without the dist > EPS test.
Pairs without a box run contact_ref.Sim._contact itself.
"""
import numpy as np

import contact_ref
import physics_ref
from contact_ref import MAX_CANDIDATES, refusal  # noqa: F401
from physics_ref import EPS, cross, dot, qconj, qrot, rot_apply

BISECTIONS = 24


def contact_lists(t, boxes=False):
    """contact_ref.contact_lists with the keys `box` (the record's box bit), `ext` (half extents, zeros for non-boxes) and `box_pairs`;
    boxes=True: boxes take part"""
    nb = t["n_bodies"]
    if not boxes:
        L = contact_ref.contact_lists(t)
        return dict(L, box=np.zeros(nb, dtype=bool), ext=np.zeros((nb, 3), dtype=np.float32), box_pairs=0)
    dyn = physics_ref.is_dynamic(t)
    shape = np.asarray(t["shape"]).astype(np.int64)
    size = np.asarray(t["size"], dtype=np.float32).reshape(nb, 3)
    mask = np.asarray(t["mask"]).astype(np.int64)
    group = np.asarray(t["group"]).astype(np.int64)
    box = shape == 1
    radius = np.where(box, np.float32(0), size[:, 0]).astype(np.float32)
    half = np.where(shape == 2, size[:, 1].astype(np.float64) * 0.5, 0.0).astype(np.float32)
    ext = np.where(box[:, None], size, np.float32(0)).astype(np.float32)
    takes_round = ((shape == 0) | (shape == 2)) & (size[:, 0] > 0) & (mask != 0)
    takes_box = box & (size > 0).all(axis=1) & (mask != 0)
    takes = takes_round | takes_box
    bit = np.where(group < 16, np.left_shift(1, np.minimum(group, 15)), 0)
    hit = (bit[:, None] & mask[None, :]) != 0
    cand = takes[:, None] & takes[None, :] & hit & hit.T & (dyn[:, None] | dyn[None, :])
    cand &= np.triu(np.ones((nb, nb), dtype=bool), 1)
    two = takes_box[:, None] & takes_box[None, :]
    box_pairs = int((cand & two).sum())
    cand &= ~two
    a, b = np.nonzero(cand)
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
    return dict(radius=radius, half=half, friction=np.asarray(t["friction"], dtype=np.float32).reshape(nb), takes=takes, box=box, ext=ext,
                follow_off=follow_off, follow_idx=partner.astype(np.int64), pairs=np.stack([pa[order], pb[order]], axis=1).reshape(-1, 2),
                colour_off=np.searchsorted(colour[order], np.arange(ncol + 1)).astype(np.int64), n_colours=ncol,
                n_follow=int(len(partner)), n_pairs=int(len(pa)), boxes=int((box & (mask != 0) & ~takes_box).sum()), box_pairs=box_pairs)


def closest_on_segment(P, d, e, dt=np.float64):
    """Steps b and c in the box frame for rows of segments P + s d and half extents e: (s, c(s), b')"""
    P, d, e = np.asarray(P, dtype=dt), np.asarray(d, dtype=dt), np.asarray(e, dtype=dt)
    zero, one, half = dt(0), dt(1), dt(0.5)

    def f(s):
        c = P + d * s[:, None]
        g = c - np.minimum(np.maximum(c, -e), e)
        return dot(g, d)
    n = len(P)
    lo, hi = np.zeros(n, dtype=dt), np.ones(n, dtype=dt)
    f0, f1 = f(lo), f(hi)
    for _ in range(BISECTIONS):
        m = (lo + hi) * half
        up = f(m) > zero
        hi = np.where(up, m, hi)
        lo = np.where(up, lo, m)
    s = np.where(f0 >= zero, zero, np.where(f1 <= zero, one, (lo + hi) * half))
    c = P + d * s[:, None]
    return s, c, np.minimum(np.maximum(c, -e), e)


class Sim(contact_ref.Sim):
    """contact_ref.Sim; boxes=True: with boxes taking part (rz_physics_contacts(ctx, 2)). `regions` counts the active box contacts by
    (coordinates of the closest point that the clamp moved — 0 in the deep case —, whether s lies strictly inside (0, 1))."""

    def __init__(self, table, parents, bind, dtype=np.float64, contacts=True, boxes=True):
        super().__init__(table, parents, bind, dtype=dtype, contacts=contacts)
        self.boxes = boxes
        self.regions = {}
        self.lists = L = contact_lists(table, boxes=boxes)
        self.cr, self.chl, self.cmu = L["radius"].astype(self.dt), L["half"].astype(self.dt), L["friction"].astype(self.dt)
        self.cbox, self.cext = L["box"] & L["takes"], L["ext"].astype(self.dt)
        n = np.diff(L["follow_off"])
        self.ranks = []
        for k in range(int(n.max()) if len(n) else 0):
            me = np.nonzero(n > k)[0]
            other = L["follow_idx"][L["follow_off"][me] + k]
            self.ranks.append((np.minimum(me, other), np.maximum(me, other)))

    def _contact(self, a, b, xp, qp):
        a, b = np.asarray(a), np.asarray(b)
        wb = self.cbox[a] | self.cbox[b]
        n = 0
        if (~wb).any():
            n += super()._contact(a[~wb], b[~wb], xp, qp)
        if wb.any():
            n += self._box_contact(a[wb], b[wb], xp, qp)
        return n

    def _box_contact(self, a, b, xp, qp):
        c, dt = self.c, self.dt.type
        eps, one, zero = dt(EPS), dt(1), dt(0)
        xa, qa, xb, qb = self.x[a], self.q[a], self.x[b], self.q[b]
        ima, imb, iia, iib = c["inv_mass"][a], c["inv_mass"][b], c["inv_inertia"][a], c["inv_inertia"][b]
        da, db = c["dyn"][a], c["dyn"][b]
        rA, rB = self.cr[a], self.cr[b]
        # 1. the box X = A or B, the round shape R the other
        ax = self.cbox[a]
        X, R = np.where(ax, a, b), np.where(ax, b, a)
        xX, qX, xR, qR, e, r = self.x[X], self.q[X], self.x[R], self.q[R], self.cext[X], self.cr[R]
        u = np.zeros((len(a), 3), dtype=self.dt)
        u[:, 1] = self.chl[R]
        u = qrot(qR, u)
        P, d = xR - u, u + u
        qi = qconj(qX)
        Pl, dl_ = qrot(qi, P - xX), qrot(qi, d)
        s, cl, bl = closest_on_segment(Pl, dl_, e, dt=dt)
        cR = P + d * s[:, None]
        gap = cl - bl
        deep = ~(np.sqrt(dot(gap, gap)) > eps)
        m = e - np.abs(cl)
        i = np.argmin(m, axis=1)                                      # the first smallest
        rows = np.arange(len(a))
        sg = np.where(cl[rows, i] >= zero, one, -one)
        face = cl.copy()
        face[rows, i] = sg * e[rows, i]
        unit = np.zeros((len(a), 3), dtype=self.dt)
        unit[rows, i] = sg
        N = qrot(qX, unit)
        cX = xX + qrot(qX, np.where(deep[:, None], face, bl))
        cA, cB = np.where(ax[:, None], cX, cR), np.where(ax[:, None], cR, cX)
        # 2
        dv = cB - cA
        dist = np.sqrt(dot(dv, dv))
        pen_s = (rA + rB) - dist
        ok_s = (pen_s > zero) & (dist > eps)
        n_s = dv / np.where(ok_s, dist, one)[:, None]
        pen = np.where(deep, r + m[rows, i], pen_s)
        n = np.where(deep[:, None], np.where(ax[:, None], N, -N), n_s)
        ok = deep | ok_s
        # 3 - 7: contact_ref.Sim._contact from here on, operation by operation
        ra, rb = (cA + n * rA[:, None]) - xa, (cB - n * rB[:, None]) - xb
        can, cbn = cross(ra, n), cross(rb, n)
        w = (ima + dot(can, self._iinv(qa, iia, can))) + (imb + dot(cbn, self._iinv(qb, iib, cbn)))
        ok = ok & (w > zero)
        dl = pen / np.where(ok, w, one)
        p = n * dl[:, None]
        oa, ob = (ok & da)[:, None], (ok & db)[:, None]
        xa1 = np.where(oa, xa - p * ima[:, None], xa)
        qa1 = np.where(oa, rot_apply(qa, -self._iinv(qa, iia, cross(ra, p))), qa)
        xb1 = np.where(ob, xb + p * imb[:, None], xb)
        qb1 = np.where(ob, rot_apply(qb, self._iinv(qb, iib, cross(rb, p))), qb)
        mu = self.cmu[a] * self.cmu[b]
        la, lb = qrot(qconj(qa), ra), qrot(qconj(qb), rb)
        ra2, rb2 = qrot(qa1, la), qrot(qb1, lb)
        D = ((xa1 + ra2) - (xp[a] + qrot(qp[a], la))) - ((xb1 + rb2) - (xp[b] + qrot(qp[b], lb)))
        Dt = D - n * dot(D, n)[:, None]
        lt = np.sqrt(dot(Dt, Dt))
        okf = ok & (mu > zero) & (lt > eps)
        td = Dt / np.where(okf, lt, one)[:, None]
        cat, cbt = cross(ra2, td), cross(rb2, td)
        wt = (ima + dot(cat, self._iinv(qa1, iia, cat))) + (imb + dot(cbt, self._iinv(qb1, iib, cbt)))
        okf = okf & (wt > zero)
        sz = np.minimum(lt / np.where(okf, wt, one), mu * dl)
        pt = td * sz[:, None]
        oa, ob = (okf & da)[:, None], (okf & db)[:, None]
        xa2 = np.where(oa, xa1 - pt * ima[:, None], xa1)
        qa2 = np.where(oa, rot_apply(qa1, -self._iinv(qa1, iia, cross(ra2, pt))), qa1)
        xb2 = np.where(ob, xb1 + pt * imb[:, None], xb1)
        qb2 = np.where(ob, rot_apply(qb1, self._iinv(qb1, iib, cross(rb2, pt))), qb1)
        self.x[a[da]], self.q[a[da]] = xa2[da], qa2[da]
        self.x[b[db]], self.q[b[db]] = xb2[db], qb2[db]
        for k in np.nonzero(ok)[0]:
            key = (int((cl[k] != bl[k]).sum()), bool(zero < s[k] < one))
            self.regions[key] = self.regions.get(key, 0) + 1
        return int(ok.sum())
