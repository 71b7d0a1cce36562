"""Contacts with PMX box bodies restated in NumPy: the definition rz_physics_contacts(ctx, 2) (kernels/physics.hip, CONTACT = 2) is held to.
The front end contact_ref.Sim runs under modes 2 and 3 for a pair of a box and a round shape (Sim._box_contact); include/reze_deform.h
states the same in words. Everything contact_ref.py says holds; what changes:

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

from physics_ref import EPS, dot, qconj, qrot

BISECTIONS = 24


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


def front_end(box_is_a, xX, qX, e, P, d, r):
    """Steps 1 and 2 for rows of pairs of a box X (half extents e) and a round shape R (segment P + s d in world space, radius r);
    box_is_a: the box has the lower index. A dict with `ok` (step 2 passed), the contact points `cA` and `cB`, the normal `n` from A to B
    and `pen`; and, for the tests: `moved` (coordinates of the closest point that the clamp moved, 0 in the deep case) and `inside` (s lies
    strictly inside (0, 1))"""
    dt = xX.dtype.type
    eps, one, zero = dt(EPS), dt(1), dt(0)
    ax = box_is_a[:, None]
    rows = np.arange(len(xX))
    # 1. a - c
    qi = qconj(qX)
    s, cl, bl = closest_on_segment(qrot(qi, P - xX), qrot(qi, d), e, dt=dt)
    cR = P + d * s[:, None]
    gap = cl - bl
    deep = ~(np.sqrt(dot(gap, gap)) > eps)
    # 1e
    m = e - np.abs(cl)
    i = np.argmin(m, axis=1)                                      # the first smallest
    sg = np.where(cl[rows, i] >= zero, one, -one)
    face = cl.copy()
    face[rows, i] = sg * e[rows, i]
    unit = np.zeros((len(xX), 3), dtype=xX.dtype)
    unit[rows, i] = sg
    N = qrot(qX, unit)
    cX = xX + qrot(qX, np.where(deep[:, None], face, bl))
    cA, cB = np.where(ax, cX, cR), np.where(ax, cR, cX)
    # 2 (the box's radius is 0)
    dv = cB - cA
    dist = np.sqrt(dot(dv, dv))
    pen_s = r - dist
    ok_s = (pen_s > zero) & (dist > eps)
    n_s = dv / np.where(ok_s, dist, one)[:, None]
    return dict(ok=deep | ok_s, cA=cA, cB=cB, n=np.where(deep[:, None], np.where(ax, N, -N), n_s), pen=np.where(deep, r + m[rows, i], pen_s),
                moved=(cl != bl).sum(axis=1), inside=(zero < s) & (s < one))
