"""Contacts between PMX rigid bodies restated in NumPy: the definition the device stage (kernels/physics.hip with CONTACT, rz_physics_contacts)
is held to. A subclass of physics_ref.Sim; include/reze_deform.h states the same stage in words. The mode is rz_physics_contacts': 0 off,
1 what this file states, 2 with boxes against round shapes (contact_box_ref.py states what changes), 3 with pairs of two boxes as well
(contact_boxbox_ref.py). One Sim for all of them: per batch of pairs, by the pairs' shapes, one of three front ends finds the contact
(steps 1 and 2) and the one _resolve applies it (steps 3 - 7).

Shapes    a sphere is the point x with radius size.x; a capsule the segment x +- q (0, size.y / 2, 0) with radius size.x (the axis is Y, as
          the inertia assumes). Boxes take no part (counted in `boxes`).
Pairs     fixed when contacts are enabled: all a < b with at least one dynamic, both sphere or capsule with radius > 0, both masks nonzero,
          (1 << group[a]) & mask[b] and (1 << group[b]) & mask[a] both nonzero (Bullet's rule). Bodies linked by a joint are not exempt.
          follow pairs (one dynamic body): per dynamic body the list of its following partners, ascending;
          dynamic pairs (both dynamic): coloured greedily in lexicographic (a, b) order so that no two pairs of a colour share a body,
          solved in (colour, a, b) order.
Where     in every iteration of a substep, after the last joint colour:
          pass F  every dynamic body, on itself alone, against its following partners in list order (Gauss-Seidel); a following body is only read
          pass D  the dynamic pairs, colour by colour
One contact, A the lower index:
  1. closest points cA, cB of the two segments P + s d, s in [0, 1], P = x - u, d = u + u, u = q (0, size.y / 2, 0) (a sphere: u = 0, d = 0):
       r = P_A - P_B; a = d_A.d_A; e = d_B.d_B; f = d_B.r; c = d_A.r; b = d_A.d_B
       a <= EPS and e <= EPS:  s = t = 0
       a <= EPS:               s = 0, t = clamp(f / e)
       e <= EPS:               t = 0, s = clamp(-c / a)
       else:                   s = clamp((b f - c e) / (a e - b b)) when a e - b b > EPS, else 0;  t = (b s + f) / e;
                               t < 0: t = 0, s = clamp(-c / a);  t > 1: t = 1, s = clamp((b - c) / a)
     (clamp to [0, 1]; Ericson, Real-Time Collision Detection 5.1.9)
  2. d = cB - cA, dist = |d|, pen = (rA + rB) - dist; skipped unless pen > 0 and dist > EPS
  3. n = d / dist; arms ra = (cA + n rA) - xA, rb = (cB - n rB) - xB
  4. w = wA + wB, wX = 1/mX + (rX x n)^T I_X^-1 (rX x n) (0 for a following body); skipped unless w > 0
  5. d_lambda = pen / w; p = n d_lambda;  x_A -= p / m_A, q_A = rot_apply(q_A, -I_A^-1 (ra x p));  x_B += p / m_B, q_B = rot_apply(q_B, +I_B^-1 (rb x p))
  6. friction, mu = friction[A] friction[B], when mu > 0: la = q_A^-1 ra, lb = q_B^-1 rb in the pose before 5; after 5 ra = q_A la, rb = q_B lb;
     slip D = [(x_A + ra) - (x_A,prev + q_A,prev la)] - [the same for B]; Dt = D - n (D.n); when |Dt| > EPS: along t = Dt / |Dt| an impulse of
     min(|Dt| / w_t, mu d_lambda), w_t the generalised inverse mass along t at the arms of the corrected pose (skipped unless w_t > 0), applied
     as in 5 (A -, B +). A following body's previous pose is its current pose.
  7. only dynamic bodies are written, and only they are corrected in 5 (a following body's pose is carried through unchanged).
No restitution and no velocity pass: a penetration removed in one substep arrives as velocity, as in plain XPBD.
"""
import numpy as np

import contact_box_ref
import contact_boxbox_ref
import physics_ref
from physics_ref import EPS, cross, dot, qconj, qrot, rot_apply

MAX_CANDIDATES = 65536


def contact_lists(t, mode=1):
    """What enabling contacts in `mode` (1, 2 or 3) derives from a table: per-body shape records, the follow CSR, the coloured dynamic
    pairs. From mode 2 boxes take part: `box` is the record's box bit, `ext` the half extents (zeros for non-boxes). A candidate pair of two
    boxes is left out and counted in `box_pairs` under mode 2, kept and counted in `n_box_box` under mode 3; all four are zeros where the
    mode has none."""
    nb = t["n_bodies"]
    dyn = physics_ref.is_dynamic(t)
    shape = np.asarray(t["shape"]).astype(np.int64)
    size = np.asarray(t["size"], dtype=np.float32).reshape(nb, 3)
    mask = np.asarray(t["mask"]).astype(np.int64)
    group = np.asarray(t["group"]).astype(np.int64)
    box = (shape == 1) & (mode >= 2)
    radius = np.where(box, np.float32(0), size[:, 0]).astype(np.float32)
    half = np.where(shape == 2, size[:, 1].astype(np.float64) * 0.5, 0.0).astype(np.float32)
    takes_box = box & (size > 0).all(axis=1) & (mask != 0)
    takes = (((shape == 0) | (shape == 2)) & (size[:, 0] > 0) & (mask != 0)) | takes_box
    bit = np.where(group < 16, np.left_shift(1, np.minimum(group, 15)), 0)
    hit = (bit[:, None] & mask[None, :]) != 0                     # hit[a, b]: a's group is in b's mask
    cand = takes[:, None] & takes[None, :] & hit & hit.T & (dyn[:, None] | dyn[None, :])
    cand &= np.triu(np.ones((nb, nb), dtype=bool), 1)
    two = takes_box[:, None] & takes_box[None, :]
    n_two = int((cand & two).sum())
    if mode < 3:
        cand &= ~two
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
    return {"radius": radius, "half": half, "friction": np.asarray(t["friction"], dtype=np.float32).reshape(nb), "takes": takes,
            "follow_off": follow_off, "follow_idx": partner.astype(np.int64), "pairs": np.stack([pa[order], pb[order]], axis=1).reshape(-1, 2),
            "colour_off": np.searchsorted(colour[order], np.arange(ncol + 1)).astype(np.int64), "n_colours": ncol,
            "n_follow": int(len(partner)), "n_pairs": int(len(pa)), "boxes": int(((shape == 1) & (mask != 0) & ~takes_box).sum()),
            "box": box, "ext": np.where(box[:, None], size, np.float32(0)).astype(np.float32),
            "box_pairs": n_two if mode == 2 else 0, "n_box_box": n_two if mode == 3 else 0}


def refusal(lists):
    """What rz_physics_contacts refuses with RZ_ERR_UNSUPPORTED, or None: the counts as its message gives them"""
    if lists["n_follow"] + lists["n_pairs"] > MAX_CANDIDATES:
        of_boxes = " (%d of them pairs of two boxes)" % lists["n_box_box"] if lists["n_box_box"] else ""
        return "%d follow entries and %d dynamic pairs%s" % (lists["n_follow"], lists["n_pairs"], of_boxes)
    return None


def closest_on_segments(p1, d1, p2, d2):
    """Step 1 on its own: the closest points of rows of segments p1 + s d1 and p2 + t d2, s and t in [0, 1]"""
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


def segment_of(x, q, hl):
    """a round shape's segment P + s d, s in [0, 1] (a sphere: d = 0): (P, d)"""
    u = np.zeros((len(hl), 3), dtype=x.dtype)
    u[:, 1] = hl
    u = qrot(q, u)
    return x - u, u + u


class Sim(physics_ref.Sim):
    """physics_ref.Sim with the contact stage in `mode`; mode=0 steps exactly as physics_ref.Sim does. `active` gets, per substep, the number
    of contact solves that passed steps 2 and 4.
    `regions` counts the active contacts of a box and a round shape by (coordinates of the closest point that the clamp moved — 0 in the
    deep case —, whether s lies strictly inside (0, 1)).
    `kinds` counts the active box - box contacts by ("A" | "B" | "edge", axis | (i, j), coordinates of p' that the clamp of 1c moved —
    0 for an edge); `n_boxbox` is their number, `n_skipped` that of those among them with an edge axis not considered (1a); `apart` counts
    the pairs found separated by the axes (0 .. 5 the faces, 6 .. 14 the edges) whose overlap was not positive."""

    def __init__(self, table, parents, bind, dtype=np.float64, mode=1):
        super().__init__(table, parents, bind, dtype=dtype)
        self.mode = mode
        self.lists = L = contact_lists(table, mode or 1)
        self.cr, self.chl, self.cmu = L["radius"].astype(self.dt), L["half"].astype(self.dt), L["friction"].astype(self.dt)
        self.cbox, self.cext = L["box"] & L["takes"], L["ext"].astype(self.dt)
        self.active = []
        self.regions, self.kinds, self.apart = {}, {}, {}
        self.n_boxbox = self.n_skipped = 0
        # pass F by partner rank: rank k = the k-th partner of every dynamic body that has one
        n = np.diff(L["follow_off"])
        self.ranks = []
        for k in range(int(n.max()) if len(n) else 0):
            me = np.nonzero(n > k)[0]
            other = L["follow_idx"][L["follow_off"][me] + k]
            self.ranks.append((np.minimum(me, other), np.maximum(me, other)))

    def _contacts(self, a, b, xp, qp):
        """the pairs (a, b) of one rank or colour, each through the front end of its shapes; returns the number of active contacts"""
        a, b = np.asarray(a), np.asarray(b)
        n_box = self.cbox[a].astype(int) + self.cbox[b]
        return sum(front(a[n_box == k], b[n_box == k], xp, qp)
                   for k, front in enumerate((self._contact, self._box_contact, self._boxbox_contact)) if (n_box == k).any())

    def _contact(self, a, b, xp, qp):
        """two segments: steps 1 and 2 above"""
        dt = self.dt.type
        eps, one, zero = dt(EPS), dt(1), dt(0)
        # 1. closest points
        cA, cB = closest_on_segments(*segment_of(self.x[a], self.q[a], self.chl[a]), *segment_of(self.x[b], self.q[b], self.chl[b]))
        # 2, and n of 3
        d = cB - cA
        dist = np.sqrt(dot(d, d))
        pen = (self.cr[a] + self.cr[b]) - dist
        ok = (pen > zero) & (dist > eps)
        n = d / np.where(ok, dist, one)[:, None]
        return int(self._resolve(a, b, cA, cB, n, pen, ok, xp, qp).sum())

    def _box_contact(self, a, b, xp, qp):
        """a box and a round shape: contact_box_ref.front_end"""
        ax = self.cbox[a]
        X, R = np.where(ax, a, b), np.where(ax, b, a)
        f = contact_box_ref.front_end(ax, self.x[X], self.q[X], self.cext[X], *segment_of(self.x[R], self.q[R], self.chl[R]), self.cr[R])
        ok = self._resolve(a, b, f["cA"], f["cB"], f["n"], f["pen"], f["ok"], xp, qp)
        for k in np.nonzero(ok)[0]:
            key = (int(f["moved"][k]), bool(f["inside"][k]))
            self.regions[key] = self.regions.get(key, 0) + 1
        return int(ok.sum())

    def _boxbox_contact(self, a, b, xp, qp):
        """two boxes: contact_boxbox_ref.front_end"""
        f = contact_boxbox_ref.front_end(self.x[a], self.q[a], self.cext[a], self.x[b], self.q[b], self.cext[b])
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

    def _resolve(self, a, b, cA, cB, n, pen, ok, xp, qp):
        """Steps 3 - 7 for the pairs (a, b) whose front end found the points cA and cB, the normal n from A to B and the penetration pen;
        `ok` marks the rows that passed step 2. Returns the rows that passed step 4 as well (the active contacts)."""
        c, dt = self.c, self.dt.type
        eps, one, zero = dt(EPS), dt(1), dt(0)
        xa, qa, xb, qb = self.x[a], self.q[a], self.x[b], self.q[b]
        ima, imb, iia, iib = c["inv_mass"][a], c["inv_mass"][b], c["inv_inertia"][a], c["inv_inertia"][b]
        da, db = c["dyn"][a], c["dyn"][b]
        rA, rB = self.cr[a], self.cr[b]
        # 3, 4
        ra, rb = (cA + n * rA[:, None]) - xa, (cB - n * rB[:, None]) - xb
        can, cbn = cross(ra, n), cross(rb, n)
        w = (ima + dot(can, self._iinv(qa, iia, can))) + (imb + dot(cbn, self._iinv(qb, iib, cbn)))
        ok = ok & (w > zero)
        # 5
        dl = pen / np.where(ok, w, one)
        p = n * dl[:, None]
        oa, ob = (ok & da)[:, None], (ok & db)[:, None]
        xa1 = np.where(oa, xa - p * ima[:, None], xa)
        qa1 = np.where(oa, rot_apply(qa, -self._iinv(qa, iia, cross(ra, p))), qa)
        xb1 = np.where(ob, xb + p * imb[:, None], xb)
        qb1 = np.where(ob, rot_apply(qb, self._iinv(qb, iib, cross(rb, p))), qb)
        # 6. friction
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
        # 7
        self.x[a[da]], self.q[a[da]] = xa2[da], qa2[da]
        self.x[b[db]], self.q[b[db]] = xb2[db], qb2[db]
        return ok

    def substep(self):
        if not self.mode:
            return super().substep()
        c, dt = self.c, self.dt.type
        L = self.lists
        h, dyn = dt(c["h"]), c["dyn"]
        d = dyn[:, None]
        self.v = np.where(d, self.v + h * c["gravity"], self.v)
        self.v = self.v * c["lin_keep"][:, None]
        self.w = self.w * c["ang_keep"][:, None]
        xp, qp = self.x.copy(), self.q.copy()
        self.x = np.where(d, self.x + h * self.v, self.x)
        wq = np.concatenate([self.w, np.zeros((c["nb"], 1), dtype=self.dt)], axis=1)
        self.q = np.where(d, physics_ref.qnormalize(self.q + (h * dt(0.5)) * physics_ref.qmul(wq, self.q)), self.q)
        lam = np.zeros((c["nj"], 3), dtype=self.dt)
        active = 0
        for it in range(c["iterations"]):
            res = [] if self.residuals is not None else None
            for k in range(c["n_colours"]):
                self._solve(np.arange(c["colour_off"][k], c["colour_off"][k + 1]), lam, res)
            if res is not None:
                self.residuals[-1].append(max(res) if res else 0.0)
            for a, b in self.ranks:                                                 # pass F
                active += self._contacts(a, b, xp, qp)
            for k in range(L["n_colours"]):                                         # pass D
                P = L["pairs"][L["colour_off"][k]:L["colour_off"][k + 1]]
                active += self._contacts(P[:, 0], P[:, 1], xp, qp)
        self.active.append(active)
        self.v = np.where(d, (self.x - xp) / h, self.v)
        dq = physics_ref.qmul(self.q, qconj(qp))
        om = (dt(2) * dq[:, :3]) / h
        self.w = np.where(d, np.where(dq[:, 3:4] < 0, -om, om), self.w)
