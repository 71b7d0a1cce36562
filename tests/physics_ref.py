"""Rigid-body physics for PMX bodies and joints restated in NumPy: the definition the device stage (kernels/physics.hip, rz_upload_physics /
rz_physics_step) is held to. include/reze_deform.h states the same solver in words.

XPBD rigid bodies (Mueller et al. 2020, "Detailed Rigid Body Simulation with Extended Position Based Dynamics") in the smallest form that
covers what PMX joints express. A body is dynamic when its type is 1 and its mass > 0; every other body follows its bone. One step call:
  1. every following body is placed at boneWorld x offset with zero velocity (after a reset: every body);
  2. `substeps` fixed steps of h; per substep
       integrate the dynamic bodies:  v += h g;  v *= (1 - linear_damping)^h;  w *= (1 - angular_damping)^h;  keep x_prev, q_prev;
                                      x += h v;  q = normalize(q + (h/2) [w, 0] (x) q)            (no gyroscopic term)
       `iterations` passes over the joints in colour order (greedy in file order: no two joints of a colour share a dynamic body); per joint
         position        d = (Q_A)^-1 (p_B - p_A), p = x + q r the world anchors, Q_A = q_A j_A the joint frame carried by A; the excess
                         e = d - clamp(d, position_min, position_max), c = Q_A e, is removed as a rigid positional constraint with the
                         3 x 3 generalised inverse mass of the anchor pair:  K p = c,  K = (1/m_A + 1/m_B) 1 - [r_A]x I_A^-1 [r_A]x -
                         [r_B]x I_B^-1 [r_B]x;  A gets +p at r_A, B gets -p at r_B; skipped when |c| <= 1e-9 or det K <= 0. (The scalar
                         split 1/m + (r x n)^T I^-1 (r x n) along n = c / |c| was tried first: for a body that is not a ball around its
                         anchor the correction leaves n, the residual rose between iterations and strands jittered at the substep rate.)
         rotation limits the Euler angles ('XYZ', R = Rx Ry Rz) of q_rel = Q_A^-1 Q_B are clamped to [rotation_min, rotation_max]; when any
                         changed, the rotation Q_A q_clamped q_rel^-1 Q_A^-1 (angle theta = 2 atan2(|xyz|, w) about n) is removed as a rigid
                         angular constraint with the 3 x 3 inverse inertia of the pair:  K l = theta n,  K = I_A^-1 + I_B^-1 in world space;
                         A turns by -I_A^-1 l, B by +I_B^-1 l; skipped when |xyz| <= 1e-9 or det K <= 0. (Split by the scalar n^T I^-1 n a
                         body whose inertia is not a ball's turns about I^-1 n instead of n, and a welded joint only converges linearly.)
         angular springs Euler angles (ex, ey, ez), Q_A and Q_B are taken once, after the limits; per axis with spring_rotation k > 0 a compliant
                         constraint C = that angle about its gimbal axis n — x: Q_A e_x, y: Q_A (0, cos ex, sin ex), z: Q_B e_z, the axes a
                         rotation about which changes that angle alone (about Q_A e_y / Q_A e_z instead the z spring of a swung joint pumps
                         energy in) — alpha~ = 1 / (k h^2), d_lambda = (-C - alpha~ lambda) / (w_A + w_B + alpha~), lambda accumulated over
                         the iterations of a substep and zero at its start
       a rotation correction d_phi is applied as q = normalize(q + (1/2) [d_phi, 0] (x) q); a min > max pair of limits is swapped
       velocities from the pose change:  v = (x - x_prev) / h;  w = 2 (q (x) q_prev^-1).xyz / h, negated when .w < 0
  3. every dynamic body with a bone gives boneWorld = bodyWorld x offset^-1, that bone's override.
Inverse inertia is diagonal in the body frame: sphere 2/5 m r^2; box m/3 (b^2 + c^2) with half extents = size; capsule: the box of half
extents (r, r + height/2, r). The bind pose of a body is T(sum of the bind translations up its bone's parent chain) x offset (the hierarchy
solve at rest); joint anchors and joint frames are taken in it once (`prepare`), in float64, from the float32 values the ABI carries.
Not covered: collisions and friction of any kind, linear springs (spring_position), restitution. Shapes feed the inertia only.

`dtype` switches every per-step operation between float64 (the reference) and float32 (the conditioning probe).
"""
import numpy as np

EPS = 1e-9
DEFAULT_H = 1.0 / 75.0
DEFAULT_ITERATIONS = 4
DEFAULT_GRAVITY = (0.0, -98.0, 0.0)
MAX_SUBSTEPS = 10


# ---- quaternions (x y z w) on arrays [..., 4] ----
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def qconj(a):
    return a * np.array([-1, -1, -1, 1], dtype=a.dtype)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def qrot(q, v):
    """v turned by q:  v + w t + u x t,  t = 2 (u x v)"""
    u = q[..., :3]
    t = cross(u, v)
    t = t + t
    return v + q[..., 3:4] * t + cross(u, t)


def qnormalize(q):
    return q / np.sqrt(q[..., 0:1] * q[..., 0:1] + q[..., 1:2] * q[..., 1:2] + q[..., 2:3] * q[..., 2:3] + q[..., 3:4] * q[..., 3:4])


def rot_apply(q, dphi):
    """q = normalize(q + 1/2 [dphi, 0] (x) q)"""
    w = np.concatenate([dphi, np.zeros_like(dphi[..., :1])], axis=-1)
    return qnormalize(q + q.dtype.type(0.5) * qmul(w, q))


def qmat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    one = q.dtype.type(1)
    return np.stack([np.stack([one - (yy + zz), xy - wz, xz + wy], axis=-1),
                     np.stack([xy + wz, one - (xx + zz), yz - wx], axis=-1),
                     np.stack([xz - wy, yz + wx, one - (xx + yy)], axis=-1)], axis=-2)


def euler_xyz(q):
    """three.js Euler.setFromRotationMatrix, order 'XYZ', of the rotation q (tests/ik_ref.py: euler_xyz)"""
    R = qmat(q)
    one = q.dtype.type(1)
    m13 = np.minimum(np.maximum(R[..., 0, 2], -one), one)
    ey = np.arcsin(m13)
    reg = np.abs(R[..., 0, 2]) < q.dtype.type(0.9999999)
    ex = np.where(reg, np.arctan2(-R[..., 1, 2], R[..., 2, 2]), np.arctan2(R[..., 2, 1], R[..., 1, 1]))
    ez = np.where(reg, np.arctan2(-R[..., 0, 1], R[..., 0, 0]), np.zeros_like(ey))
    return np.stack([ex, ey, ez], axis=-1)


def from_euler_xyz(e):
    """three.js Quaternion.setFromEuler, order 'XYZ' (tests/ik_ref.py: from_euler_xyz)"""
    h = e * e.dtype.type(0.5)
    c1, c2, c3 = np.cos(h[..., 0]), np.cos(h[..., 1]), np.cos(h[..., 2])
    s1, s2, s3 = np.sin(h[..., 0]), np.sin(h[..., 1]), np.sin(h[..., 2])
    return np.stack([s1 * c2 * c3 + c1 * s2 * s3, c1 * s2 * c3 - s1 * c2 * s3,
                     c1 * c2 * s3 + s1 * s2 * c3, c1 * c2 * c3 - s1 * s2 * s3], axis=-1)


def quat_from_pmx_euler(r):
    """math.ts Quat.fromEuler(rotX, rotY, rotZ): how the loader's Euler angles (shape rotation, joint rotation) become quaternions"""
    r = np.asarray(r, dtype=np.float64)
    cx, sx = np.cos(r[..., 0] * 0.5), np.sin(r[..., 0] * 0.5)
    cy, sy = np.cos(r[..., 1] * 0.5), np.sin(r[..., 1] * 0.5)
    cz, sz = np.cos(r[..., 2] * 0.5), np.sin(r[..., 2] * 0.5)
    return qnormalize(np.stack([cy * sx * cz + sy * cx * sz, sy * cx * cz - cy * sx * sz,
                                cy * cx * sz - sy * sx * cz, cy * cx * cz + sy * sx * sz], axis=-1))


def quat_of_matrix(R):
    """unit quaternion of one 3x3 rotation (Shepperd; kernels/pass_parts.hip.h: quat_of_rows)"""
    dt = R.dtype.type
    m = R
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + dt(1)) * dt(2)
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, dt(0.25) * s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = np.sqrt(dt(1) + m[0, 0] - m[1, 1] - m[2, 2]) * dt(2)
        q = [dt(0.25) * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] > m[2, 2]:
        s = np.sqrt(dt(1) + m[1, 1] - m[0, 0] - m[2, 2]) * dt(2)
        q = [(m[0, 1] + m[1, 0]) / s, dt(0.25) * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = np.sqrt(dt(1) + m[2, 2] - m[0, 0] - m[1, 1]) * dt(2)
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, dt(0.25) * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q, dtype=R.dtype)
    return q / np.sqrt(q.dot(q))


# ---- the table ----
BODY_F = ("size", "offset_pos", "offset_rot", "mass", "linear_damping", "angular_damping", "restitution", "friction")
JOINT_F = ("position", "rotation", "position_min", "position_max", "rotation_min", "rotation_max", "spring_position", "spring_rotation")


def make_table(bodies, joints, gravity=None, h=0.0, iterations=0):
    """A table as rz_upload_physics takes it, from lists of dicts. Floats are rounded to float32 here: that is what the ABI carries."""
    nb, nj = len(bodies), len(joints)

    def col(rows, key, width, default):
        a = np.array([np.broadcast_to(np.asarray(r.get(key, default), dtype=np.float32), (width,)) for r in rows], dtype=np.float32)
        return a.reshape(len(rows), width) if width > 1 else a.reshape(len(rows))
    t = dict(n_bodies=nb, n_joints=nj)
    t["bone"] = np.array([int(b.get("bone", -1)) for b in bodies], dtype=np.int32)
    t["type"] = np.array([int(b.get("type", 0)) for b in bodies], dtype=np.uint8)
    t["shape"] = np.array([int(b.get("shape", 0)) for b in bodies], dtype=np.uint8)
    t["group"] = np.array([int(b.get("group", 0)) for b in bodies], dtype=np.uint8)
    t["mask"] = np.array([int(b.get("mask", 0xffff)) for b in bodies], dtype=np.uint16)
    t["size"] = col(bodies, "size", 3, 1.0)
    t["offset_pos"] = col(bodies, "offset_pos", 3, 0.0)
    t["offset_rot"] = col(bodies, "offset_rot", 4, (0.0, 0.0, 0.0, 1.0))
    for k, d in (("mass", 1.0), ("linear_damping", 0.0), ("angular_damping", 0.0), ("restitution", 0.0), ("friction", 0.5)):
        t[k] = col(bodies, k, 1, d)
    t["body_a"] = np.array([int(j["body_a"]) for j in joints], dtype=np.int32)
    t["body_b"] = np.array([int(j["body_b"]) for j in joints], dtype=np.int32)
    for k in JOINT_F:
        t[k] = col(joints, k, 3, 0.0) if nj else np.zeros((0, 3), dtype=np.float32)
    t["gravity"] = None if gravity is None else np.asarray(gravity, dtype=np.float32)
    t["h"] = np.float32(h)
    t["iterations"] = int(iterations)
    return t


def is_dynamic(t):
    return (t["type"] == 1) & (t["mass"] > 0)


def colouring(t):
    """Greedy, in file order: a joint takes the smallest colour in which no earlier joint shares a dynamic body with it. Returns
    (colour per joint, the joints sorted by (colour, file index), the number of colours)."""
    dyn = is_dynamic(t)
    used = [set() for _ in range(t["n_bodies"])]
    colour = np.zeros(t["n_joints"], dtype=np.int32)
    for j in range(t["n_joints"]):
        mine = [b for b in (int(t["body_a"][j]), int(t["body_b"][j])) if dyn[b]]
        c = 0
        while any(c in used[b] for b in mine):
            c += 1
        for b in mine:
            used[b].add(c)
        colour[j] = c
    order = np.array(sorted(range(t["n_joints"]), key=lambda j: (int(colour[j]), j)), dtype=np.int32)
    return colour, order, int(colour.max()) + 1 if t["n_joints"] else 0


def bind_positions(parents, bind):
    B = len(parents)
    out = np.zeros((B, 3))
    for b in range(B):
        p, acc = b, np.zeros(3)
        while p >= 0:
            acc = acc + np.asarray(bind[p], dtype=np.float64)
            p = int(parents[p])
        out[b] = acc
    return out


def inverse_inertia(shape, size, mass):
    if shape == 0:
        d = np.full(3, 0.4 * mass * size[0] * size[0])
    else:
        a, b, c = (size[0], size[1], size[2]) if shape == 1 else (size[0], size[0] + 0.5 * size[1], size[0])
        d = mass / 3.0 * np.array([b * b + c * c, a * a + c * c, a * a + b * b])
    return np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0)


def prepare(t, parents, bind):
    """The constants the solver runs on, in float64 from the table's float32 values (the upload does the same in double)."""
    f = {k: np.asarray(t[k], dtype=np.float64) for k in BODY_F + JOINT_F}
    nb, nj = t["n_bodies"], t["n_joints"]
    h = float(t["h"]) if float(t["h"]) > 0 else DEFAULT_H
    dyn = is_dynamic(t)
    bp = bind_positions(parents, bind)
    c = dict(nb=nb, nj=nj, h=h, dyn=dyn, iterations=t["iterations"] if t["iterations"] > 0 else DEFAULT_ITERATIONS,
             gravity=np.asarray(DEFAULT_GRAVITY if t["gravity"] is None else t["gravity"], dtype=np.float64),
             bone=t["bone"].astype(np.int64), off_p=f["offset_pos"], off_q=qnormalize(f["offset_rot"].reshape(nb, 4)))
    c["inv_mass"] = np.where(dyn, 1.0 / np.where(dyn, f["mass"], 1.0), 0.0)
    c["inv_inertia"] = np.array([inverse_inertia(int(t["shape"][b]), f["size"][b], f["mass"][b]) if dyn[b] else np.zeros(3) for b in range(nb)]).reshape(nb, 3)
    c["lin_keep"] = (1.0 - f["linear_damping"]) ** h
    c["ang_keep"] = (1.0 - f["angular_damping"]) ** h
    bx = np.array([f["offset_pos"][b] + (bp[t["bone"][b]] if t["bone"][b] >= 0 else 0.0) for b in range(nb)]).reshape(nb, 3)     # bind pose of the bodies
    bq = c["off_q"]
    colour, order, ncol = colouring(t)
    c["colour"], c["order"], c["n_colours"] = colour, order, ncol
    c["colour_off"] = np.searchsorted(colour[order], np.arange(ncol + 1)).astype(np.int64) if nj else np.zeros(1, dtype=np.int64)
    a, b = t["body_a"][order].astype(np.int64), t["body_b"][order].astype(np.int64)
    jq = quat_from_pmx_euler(f["rotation"][order]).reshape(nj, 4)
    jp = f["position"][order].reshape(nj, 3)
    c["ja"], c["jb"] = a, b                                           # (everything per joint is in solve order from here on)
    c["r_a"] = qrot(qconj(bq[a]), jp - bx[a]); c["r_b"] = qrot(qconj(bq[b]), jp - bx[b])
    c["j_a"] = qmul(qconj(bq[a]), jq); c["j_b"] = qmul(qconj(bq[b]), jq)
    for k in ("position", "rotation"):
        lo, hi = f[k + "_min"][order].reshape(nj, 3), f[k + "_max"][order].reshape(nj, 3)
        c[k[0] + "min"], c[k[0] + "max"] = np.minimum(lo, hi), np.maximum(lo, hi)
    ks = f["spring_rotation"][order].reshape(nj, 3)
    c["spring_on"] = ks > 0
    c["alpha"] = np.where(ks > 0, 1.0 / (np.where(ks > 0, ks, 1.0) * h * h), 0.0)
    c["dyn_bodies"] = np.array([b for b in range(nb) if dyn[b] and t["bone"][b] >= 0], dtype=np.int64)
    return c


FLOAT_KEYS = ("gravity", "off_p", "off_q", "inv_mass", "inv_inertia", "lin_keep", "ang_keep", "r_a", "r_b", "j_a", "j_b", "pmin", "pmax", "rmin", "rmax", "alpha")


class Sim:
    """One instance's simulation. world16 arguments are [B,16] column-major world matrices of the un-overridden hierarchy solve."""

    def __init__(self, table, parents, bind, dtype=np.float64):
        self.dt = np.dtype(dtype)
        self.c = prepare(table, parents, bind)
        for k in FLOAT_KEYS:
            self.c[k] = self.c[k].astype(self.dt)
        nb = self.c["nb"]
        self.x = np.zeros((nb, 3), dtype=self.dt); self.q = np.zeros((nb, 4), dtype=self.dt); self.q[:, 3] = 1
        self.v = np.zeros((nb, 3), dtype=self.dt); self.w = np.zeros((nb, 3), dtype=self.dt)
        self.pending_reset = True
        self.residuals = None         # a list: per substep, per iteration the largest anchor excess |c| met (diagnostics)

    def _place(self, world16, which):
        c, dt = self.c, self.dt
        W = np.asarray(world16, dtype=dt).reshape(-1, 4, 4).transpose(0, 2, 1)
        for b in np.nonzero(which)[0]:
            bone = int(c["bone"][b])
            if bone >= 0:
                R, P = W[bone, :3, :3], W[bone, :3, 3]
                self.x[b] = R @ c["off_p"][b] + P
                self.q[b] = qmul(quat_of_matrix(R), c["off_q"][b])
            else:
                self.x[b], self.q[b] = c["off_p"][b], c["off_q"][b]
            self.v[b] = 0
            self.w[b] = 0

    def reset(self, world16):
        self._place(world16, np.ones(self.c["nb"], dtype=bool))
        self.pending_reset = False

    def _iinv(self, q, ii, v):
        return qrot(q, ii * qrot(qconj(q), v))

    def _solve(self, J, lam, res):
        c, dt = self.c, self.dt.type
        a, b = c["ja"][J], c["jb"][J]
        xa, qa, xb, qb = self.x[a], self.q[a], self.x[b], self.q[b]
        ima, imb, iia, iib = c["inv_mass"][a][:, None], c["inv_mass"][b][:, None], c["inv_inertia"][a], c["inv_inertia"][b]
        # position
        ra, rb = qrot(qa, c["r_a"][J]), qrot(qb, c["r_b"][J])
        QA = qmul(qa, c["j_a"][J])
        d = qrot(qconj(QA), (xb + rb) - (xa + ra))
        e = d - np.minimum(np.maximum(d, c["pmin"][J]), c["pmax"][J])
        cv = qrot(QA, e)
        C = np.sqrt(dot(cv, cv))
        if res is not None and len(J):
            res.append(float(C.max()))
        ok = C > dt(EPS)
        # K p = c: the anchors' relative displacement for a correction p, K = (1/m_A + 1/m_B) 1 - [r_A]x I_A^-1 [r_A]x - [r_B]x I_B^-1 [r_B]x,
        # column by column, solved by Cramer's rule
        cols = []
        for ax in range(3):
            u = np.zeros_like(cv); u[:, ax] = 1
            cols.append((ima + imb) * u + cross(self._iinv(qa, iia, cross(ra, u)), ra) + cross(self._iinv(qb, iib, cross(rb, u)), rb))
        k0, k1, k2 = cols
        det = dot(k0, cross(k1, k2))
        ok = ok & (det > 0)
        det = np.where(ok, det, dt(1))
        p = np.stack([dot(cv, cross(k1, k2)), dot(k0, cross(cv, k2)), dot(k0, cross(k1, cv))], axis=-1) / det[:, None]
        o = ok[:, None]
        xa = np.where(o, xa + p * ima, xa)
        qa = np.where(o, rot_apply(qa, self._iinv(qa, iia, cross(ra, p))), qa)
        xb = np.where(o, xb - p * imb, xb)
        qb = np.where(o, rot_apply(qb, -self._iinv(qb, iib, cross(rb, p))), qb)
        # rotation limits
        QA, QB = qmul(qa, c["j_a"][J]), qmul(qb, c["j_b"][J])
        qrel = qmul(qconj(QA), QB)
        eu = euler_xyz(qrel)
        ec = np.minimum(np.maximum(eu, c["rmin"][J]), c["rmax"][J])
        viol = (ec != eu).any(axis=1)
        dq = qmul(qmul(QA, qmul(from_euler_xyz(ec), qconj(qrel))), qconj(QA))
        dq = np.where(dq[:, 3:4] < 0, -dq, dq)
        s = np.sqrt(dot(dq, dq))
        ok = viol & (s > dt(EPS))
        n = dq[:, :3] / np.where(ok, s, dt(1))[:, None]
        theta = dt(2) * np.arctan2(s, dq[:, 3])
        # K l = theta n with K = I_A^-1 + I_B^-1 (world), column by column, Cramer's rule; A turns by -I_A^-1 l, B by +I_B^-1 l
        cols = []
        for ax in range(3):
            u = np.zeros_like(n); u[:, ax] = 1
            cols.append(self._iinv(qa, iia, u) + self._iinv(qb, iib, u))
        k0, k1, k2 = cols
        det = dot(k0, cross(k1, k2))
        ok = ok & (det > 0)
        det = np.where(ok, det, dt(1))
        rhs = n * theta[:, None]
        lm = np.stack([dot(rhs, cross(k1, k2)), dot(k0, cross(rhs, k2)), dot(k0, cross(k1, rhs))], axis=-1) / det[:, None]
        o = ok[:, None]
        qa_new = rot_apply(qa, -self._iinv(qa, iia, lm))
        qb_new = rot_apply(qb, self._iinv(qb, iib, lm))
        qa, qb = np.where(o, qa_new, qa), np.where(o, qb_new, qb)
        # angular springs
        if c["spring_on"][J].any():
            QA, QB = qmul(qa, c["j_a"][J]), qmul(qb, c["j_b"][J])
            eu = euler_xyz(qmul(qconj(QA), QB))
            for ax in range(3):
                on = c["spring_on"][J, ax]
                unit = np.zeros((len(J), 3), dtype=self.dt)
                if ax == 1:
                    unit[:, 1], unit[:, 2] = np.cos(eu[:, 0]), np.sin(eu[:, 0])
                else:
                    unit[:, ax] = 1
                n = qrot(QB if ax == 2 else QA, unit)
                na, nb_ = self._iinv(qa, iia, n), self._iinv(qb, iib, n)
                al = c["alpha"][J, ax]
                dl = np.where(on, (-eu[:, ax] - al * lam[J, ax]) / np.where(on, dot(n, na) + dot(n, nb_) + al, dt(1)), dt(0))
                lam[J, ax] = lam[J, ax] + dl
                o = on[:, None]
                qa = np.where(o, rot_apply(qa, -(na * dl[:, None])), qa)
                qb = np.where(o, rot_apply(qb, nb_ * dl[:, None]), qb)
        # only dynamic bodies are written: a following body is shared freely inside a colour and never moves
        da, db = c["dyn"][a], c["dyn"][b]
        self.x[a[da]], self.q[a[da]] = xa[da], qa[da]
        self.x[b[db]], self.q[b[db]] = xb[db], qb[db]

    def substep(self):
        c, dt = self.c, self.dt.type
        h, dyn = dt(c["h"]), c["dyn"]
        d = dyn[:, None]
        self.v = np.where(d, self.v + h * c["gravity"], self.v)
        self.v = self.v * c["lin_keep"][:, None]
        self.w = self.w * c["ang_keep"][:, None]
        xp, qp = self.x.copy(), self.q.copy()
        self.x = np.where(d, self.x + h * self.v, self.x)
        wq = np.concatenate([self.w, np.zeros((c["nb"], 1), dtype=self.dt)], axis=1)
        self.q = np.where(d, qnormalize(self.q + (h * dt(0.5)) * qmul(wq, self.q)), self.q)
        lam = np.zeros((c["nj"], 3), dtype=self.dt)
        for it in range(c["iterations"]):
            res = [] if self.residuals is not None else None
            for k in range(c["n_colours"]):
                self._solve(np.arange(c["colour_off"][k], c["colour_off"][k + 1]), lam, res)
            if res is not None:
                self.residuals[-1].append(max(res) if res else 0.0)
        self.v = np.where(d, (self.x - xp) / h, self.v)
        dq = qmul(self.q, qconj(qp))
        om = (dt(2) * dq[:, :3]) / h
        self.w = np.where(d, np.where(dq[:, 3:4] < 0, -om, om), self.w)

    def step(self, world16, substeps):
        """One rz_physics_step: returns the overrides, {bone: float[16] column-major}."""
        if self.pending_reset:
            self.reset(world16)
        else:
            self._place(world16, ~self.c["dyn"])
        for _ in range(int(substeps)):
            if self.residuals is not None:
                self.residuals.append([])
            self.substep()
        return self.overrides()

    def overrides(self):
        c = self.c
        out = {}
        for b in c["dyn_bodies"]:
            qb = qmul(self.q[b], qconj(c["off_q"][b]))
            R = qmat(qb)
            M = np.zeros((4, 4), dtype=self.dt)
            M[:3, :3] = R
            M[:3, 3] = self.x[b] - R @ c["off_p"][b]
            M[3, 3] = 1
            out[int(c["bone"][b])] = M.T.reshape(16).copy()
        return out

    def state13(self):
        return np.concatenate([self.x, self.q, self.v, self.w], axis=1)


def apply_overrides(world16, ovr):
    w = np.array(world16, dtype=np.float64).reshape(-1, 16).copy()
    for b, m in ovr.items():
        w[b] = m
    return w


def validate(t, B):
    """What rz_upload_physics refuses with RZ_ERR_INVALID, as a message or None."""
    nb, nj = t["n_bodies"], t["n_joints"]
    for k in BODY_F + JOINT_F:
        if not np.isfinite(np.asarray(t[k], dtype=np.float64)).all():
            return "%s is not finite" % k
    if ((t["bone"] < -1) | (t["bone"] >= B)).any():
        return "bone out of range"
    if (t["type"] > 2).any() or (t["shape"] > 2).any():
        return "type or shape outside 0 .. 2"
    if (t["mass"] < 0).any():
        return "negative mass"
    for k in ("linear_damping", "angular_damping"):
        if ((t[k] < 0) | (t[k] > 1)).any():
            return "%s outside [0, 1]" % k
    for j in range(nj):
        a, b = int(t["body_a"][j]), int(t["body_b"][j])
        if not (0 <= a < nb and 0 <= b < nb):
            return "joint %d: body out of range" % j
        if a == b:
            return "joint %d joins body %d to itself" % (j, a)
    dyn = is_dynamic(t)
    bones = [int(t["bone"][b]) for b in range(nb) if dyn[b] and t["bone"][b] >= 0]
    if len(set(bones)) != len(bones):
        return "two dynamic bodies on one bone"
    return None
