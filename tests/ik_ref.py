"""PMX inverse kinematics restated in NumPy: the definition the host solver (host/model.js: Model.solveIK) and the device stage
(kernels/ik.hip.h) are both held to.

CCD in the simple clamp form: chains in ascending order of the IK (goal) bone; per iteration every link, in file order (effector
outwards), is turned so that the effector swings towards the goal, by at most the chain's per-step angle, then clamped to the
link's Euler limits ('XYZ' order, R = Rx * Ry * Rz); the hierarchy is re-solved after every link. The angle comes from
atan2(|a x b|, a . b): acos(a . b) near 1 loses half the digits in float32. World matrices are the hierarchy solve's,
W = W_parent * T(bind + t) * A * R(q) * T(add), A the append rotation and T(add) the append-move translation, exactly what the
device forms (kernels/fk.hip.h: fk_local_matrix). `dtype` switches every operation between float64 (the reference) and float32
(the conditioning probe: a pose whose float32 run strays from its float64 run is ill-conditioned, not mis-solved).
"""
import numpy as np


def _qmat(q, dt):
    x, y, z, w = q
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    one = dt(1)
    return np.array([[one - (yy + zz), xy - wz, xz + wy],
                     [xy + wz, one - (xx + zz), yz - wx],
                     [xz - wy, yz + wx, one - (xx + yy)]], dtype=dt)


def _qmul(a, b, dt):
    """Hamilton product a * b (math.ts Quat.multiply), x y z w."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=dt)


def _slerp_id(a, t, dt):
    """Quat.slerp(identity, a, t) (math.ts:156-189)."""
    a = np.array(a, dtype=dt)
    c = a[3]
    if c < 0:
        c = -c
        a = -a
    if c > dt(0.9995):
        s = np.array([t * a[0], t * a[1], t * a[2], dt(1) + t * (a[3] - dt(1))], dtype=dt)
        return s / np.sqrt(s.dot(s))
    th0 = np.arccos(c)
    sn = np.sin(th0)
    th = th0 * t
    s0, s1 = np.sin(th0 - th) / sn, np.sin(th) / sn
    return np.array([s1 * a[0], s1 * a[1], s1 * a[2], s0 + s1 * a[3]], dtype=dt)


def euler_xyz(R, dt):
    """three.js Euler.setFromRotationMatrix, order 'XYZ'."""
    m13 = min(max(R[0][2], dt(-1)), dt(1))
    ey = np.arcsin(m13)
    if abs(R[0][2]) < dt(0.9999999):
        ex = np.arctan2(-R[1][2], R[2][2])
        ez = np.arctan2(-R[0][1], R[0][0])
    else:
        ex = np.arctan2(R[2][1], R[1][1])
        ez = dt(0)
    return np.array([ex, ey, ez], dtype=dt)


def from_euler_xyz(e, dt):
    """three.js Quaternion.setFromEuler, order 'XYZ'."""
    h = np.asarray(e, dtype=dt) * dt(0.5)
    c1, c2, c3 = np.cos(h)
    s1, s2, s3 = np.sin(h)
    return np.array([s1 * c2 * c3 + c1 * s2 * s3, c1 * s2 * c3 - s1 * c2 * s3,
                     c1 * c2 * s3 + s1 * s2 * c3, c1 * c2 * c3 - s1 * s2 * s3], dtype=dt)


def link_limits(link, dt=np.float64):
    """(min[3], max[3]) of a link with an axis whose min > max swapped, or None."""
    if link.get("min") is None or link.get("max") is None:
        return None
    lo, hi = np.asarray(link["min"], dtype=dt), np.asarray(link["max"], dtype=dt)
    return np.minimum(lo, hi), np.maximum(lo, hi)


class Hierarchy:
    """The hierarchy solve on a mutable local pose; update(bones) re-solves a topologically ordered subset."""

    def __init__(self, parents, bind, q, t=None, append_parent=None, append_ratio=None, append_move=None, dtype=np.float64):
        self.dt = dt = np.dtype(dtype).type
        self.B = B = len(parents)
        self.parents = [int(p) for p in parents]
        self.bind = np.asarray(bind, dtype=dt).reshape(B, 3)
        self.q = np.array(q, dtype=dt).reshape(B, 4).copy()
        self.t = np.zeros((B, 3), dtype=dt) if t is None else np.array(t, dtype=dt).reshape(B, 3).copy()
        self.ap = [-1] * B if append_parent is None else [int(a) if 0 <= int(a) < B else -1 for a in append_parent]
        self.ratio = np.ones(B, dtype=dt) if append_ratio is None else np.asarray(append_ratio, dtype=dt)
        self.move = [False] * B if append_move is None else [bool(m) for m in append_move]
        depth = [0] * B
        for b in range(B):
            d, p = 0, self.parents[b]
            while p >= 0:
                d, p = d + 1, self.parents[p]
            depth[b] = d
        self.depth = depth
        self.order = sorted(range(B), key=lambda b: (depth[b], b))
        self.rank = {b: k for k, b in enumerate(self.order)}
        self.children = [[] for _ in range(B)]
        for b in range(B):
            if self.parents[b] >= 0:
                self.children[self.parents[b]].append(b)
        self.R = np.zeros((B, 3, 3), dtype=dt)
        self.P = np.zeros((B, 3), dtype=dt)
        self._dep = {}
        self.update(self.order)

    def local(self, b):
        dt = self.dt
        Rb = _qmat(self.q[b], dt)
        add = np.zeros(3, dtype=dt)
        ap = self.ap[b]
        if ap >= 0:
            raw = self.ratio[b]
            ratio = min(max(raw, dt(-1)), dt(1))
            if abs(ratio) > dt(1e-6):
                if self.move[b]:
                    add = self.t[ap] * raw
                a = self.q[ap].copy()
                if ratio < 0:
                    a[:3] = -a[:3]
                Rb = _qmat(_slerp_id(a, abs(ratio), dt), dt) @ Rb
        return Rb, self.bind[b] + self.t[b] + Rb @ add

    def update(self, bones):
        for b in bones:
            Rl, tl = self.local(b)
            p = self.parents[b]
            if p < 0:
                self.R[b], self.P[b] = Rl, tl
            else:
                self.R[b] = self.R[p] @ Rl
                self.P[b] = self.R[p] @ tl + self.P[p]

    def dependents(self, L):
        """every bone whose world matrix depends on q[L], parents first"""
        if L not in self._dep:
            seen = set()
            stack = [L] + [b for b in range(self.B) if self.ap[b] == L]
            while stack:
                b = stack.pop()
                if b in seen:
                    continue
                seen.add(b)
                stack.extend(self.children[b])
            self._dep[L] = sorted(seen, key=lambda b: self.rank[b])
        return self._dep[L]

    def world16(self):
        """[B,16] column-major 4x4, the layout rz_read_world returns"""
        W = np.zeros((self.B, 4, 4), dtype=self.dt)
        W[:, :3, :3] = self.R
        W[:, :3, 3] = self.P
        W[:, 3, 3] = 1
        return np.ascontiguousarray(W.transpose(0, 2, 1)).reshape(self.B, 16)


def solve_chain(h, chain, info=None):
    dt = h.dt
    G, E = int(chain["goal"]), int(chain["effector"])
    theta = dt(chain["limit_angle"])
    start = float(np.linalg.norm(h.P[G] - h.P[E]))
    its = 0
    for _ in range(int(chain["loops"])):
        its += 1
        rotated = False
        for link in chain["links"]:
            L = int(link["bone"])
            a = h.R[L].T @ (h.P[E] - h.P[L])
            b = h.R[L].T @ (h.P[G] - h.P[L])
            la, lb = np.sqrt(a.dot(a)), np.sqrt(b.dot(b))
            if la < dt(1e-6) or lb < dt(1e-6):
                continue
            a, b = a / la, b / lb
            c = np.cross(a, b).astype(dt)
            n = np.sqrt(c.dot(c))
            if n < dt(1e-7):
                continue
            ang = min(np.arctan2(n, a.dot(b)), theta)
            half = ang * dt(0.5)
            s = np.sin(half) / n
            dq = np.array([c[0] * s, c[1] * s, c[2] * s, np.cos(half)], dtype=dt)
            q = _qmul(h.q[L], dq, dt)
            lim = link_limits(link, dt)
            if lim is not None:
                e = euler_xyz(_qmat(q, dt), dt)
                e = np.minimum(np.maximum(e, lim[0]), lim[1])
                q = from_euler_xyz(e, dt)
            h.q[L] = q / np.sqrt(q.dot(q))
            rotated = True
            h.update(h.dependents(L))
        d = h.P[G] - h.P[E]
        if np.sqrt(d.dot(d)) < dt(1e-4) or not rotated:
            break
    if info is not None:
        info.append(dict(goal=G, start=start, end=float(np.linalg.norm(h.P[G] - h.P[E])), iterations=its))


def solve(parents, bind, q, t=None, chains=(), append_parent=None, append_ratio=None, append_move=None, dtype=np.float64, info=None):
    """The pose after IK: (world [B,16] column-major, solved local rotations [B,4]). `q` / `t` are the local pose AFTER bone morphs.
    `info`, a list, receives per chain dict(goal, start, end, iterations) in solve order."""
    h = Hierarchy(parents, bind, q, t, append_parent, append_ratio, append_move, dtype)
    for chain in sorted(chains, key=lambda ch: int(ch["goal"])):
        solve_chain(h, chain, info)
    h.update(h.order)          # the final pose: the hierarchy solve of the solved locals
    return h.world16(), h.q.copy()


def extent(bind_world):
    """the skeleton's extent: the largest side of the bind pose's bounding box (the unit of the parity bar)"""
    p = np.asarray(bind_world, dtype=np.float64).reshape(-1, 3)
    return float(max((p.max(axis=0) - p.min(axis=0)).max(), 1.0))


def bind_positions(parents, bind):
    B = len(parents)
    out = np.zeros((B, 3))
    done = [False] * B

    def go(b):
        if done[b]:
            return
        p = int(parents[b])
        if p >= 0:
            go(p)
            out[b] = out[p] + np.asarray(bind[b], dtype=np.float64)
        else:
            out[b] = np.asarray(bind[b], dtype=np.float64)
        done[b] = True
    for b in range(B):
        go(b)
    return out


def validate(B, parents, chains):
    """'A valid table' of the issue, as the library checks it. Returns None or a message."""
    def ancestors(b):
        out, p = [], int(parents[b])
        while p >= 0:
            out.append(p)
            p = int(parents[p])
        return out
    for k, ch in enumerate(chains):
        G, E = int(ch["goal"]), int(ch["effector"])
        if not (0 <= G < B and 0 <= E < B):
            return "chain %d: bone out of range" % k
        if G == E:
            return "chain %d: the effector is the goal" % k
        if int(ch["loops"]) < 0 or len(ch["links"]) > 255:
            return "chain %d: bad counts" % k
        prev = E
        for link in ch["links"]:
            L = int(link["bone"])
            if not 0 <= L < B:
                return "chain %d: link out of range" % k
            if L not in ancestors(prev):
                return "chain %d: link %d is not a proper ancestor of %d" % (k, L, prev)
            prev = L
    return None
