"""Linear joint springs (PMX spring_position) restated in NumPy: the definition the device stage (kernels/physics.hip with LSPRING,
rz_physics_springs) is held to. A subclass of contact_ref.Sim, so it composes with every contact mode, and mode 0 steps as physics_ref.Sim;
include/reze_deform.h states the same stage in words.

Where     the last stage of a joint's solve, behind the angular springs: _solve runs the joint as it always ran, then this stage for the
          same joints. The multipliers are three more per joint, zero at the start of every substep, accumulated over its iterations.
One joint, for axis ax = x, y, z in that order where spring_position[ax] = k > 0, each axis from the pose the previous one left:
  r_A = q_A r_a, r_B = q_B r_b, Q_A = q_A j_A, n = Q_A e_ax (taken as fixed for this correction)
  C = n . ((x_B + r_B) - (x_A + r_A))                   the component of d the position stage computes; the rest point is 0
  w = ((1/m_A + 1/m_B) + (r_A x n)^T I_A^-1 (r_A x n)) + (r_B x n)^T I_B^-1 (r_B x n)
  alpha~ = 1 / (k h^2);  d_lambda = (-C - alpha~ lambda) / (w + alpha~);  lambda += d_lambda;  p = n d_lambda
  x_A -= p / m_A, q_A = rot_apply(q_A, -(I_A^-1 (r_A x n)) d_lambda);  x_B += p / m_B, q_B = rot_apply(q_B, +(I_B^-1 (r_B x n)) d_lambda)
  only dynamic bodies are written. k <= 0: no spring on that axis. springs=False: no stage at all.
A spring on one body is backward Euler's mass on a spring: period 2 pi h / atan(omega h), omega^2 = k / m, and the amplitude falls by
(1 + (omega h)^2)^(-1/2) per substep, whatever `iterations` is (tests/test_spring_cpu.py).
"""
import numpy as np

import contact_ref
import physics_ref
from physics_ref import cross, dot, qmul, qrot, rot_apply


def lin_constants(table, h):
    """(lin_on [nj,3], lin_alpha [nj,3]) in joint solve order, in float64 from the table's float32 spring_position and its h"""
    nj = table["n_joints"]
    order = physics_ref.colouring(table)[1]
    k = np.asarray(table["spring_position"], dtype=np.float64).reshape(nj, 3)[order].reshape(nj, 3)
    on = k > 0
    return on, np.where(on, 1.0 / (np.where(on, k, 1.0) * h * h), 0.0)


class Sim(contact_ref.Sim):
    """contact_ref.Sim with the linear springs behind every joint's solve; springs=False steps exactly as contact_ref.Sim does"""

    def __init__(self, table, parents, bind, dtype=np.float64, mode=0, springs=True):
        super().__init__(table, parents, bind, dtype=dtype, mode=mode)
        self.springs = springs
        self.lin_on, alpha = lin_constants(table, self.c["h"])
        self.lin_alpha = alpha.astype(self.dt)
        self.llam, self._lam_of = None, None

    def _solve(self, J, lam, res):
        super()._solve(J, lam, res)
        if not self.springs:
            return
        if lam is not self._lam_of:                 # a new substep: its multipliers start at zero
            self._lam_of, self.llam = lam, np.zeros((self.c["nj"], 3), dtype=self.dt)
        if not self.lin_on[J].any():
            return
        c, dt = self.c, self.dt.type
        a, b = c["ja"][J], c["jb"][J]
        xa, qa, xb, qb = self.x[a], self.q[a], self.x[b], self.q[b]
        ima, imb, iia, iib = c["inv_mass"][a], c["inv_mass"][b], c["inv_inertia"][a], c["inv_inertia"][b]
        for ax in range(3):
            on = self.lin_on[J, ax]
            ra, rb = qrot(qa, c["r_a"][J]), qrot(qb, c["r_b"][J])
            unit = np.zeros((len(J), 3), dtype=self.dt)
            unit[:, ax] = 1
            n = qrot(qmul(qa, c["j_a"][J]), unit)
            C = dot(n, (xb + rb) - (xa + ra))
            can, cbn = cross(ra, n), cross(rb, n)
            na, nb_ = self._iinv(qa, iia, can), self._iinv(qb, iib, cbn)
            w = ((ima + imb) + dot(can, na)) + dot(cbn, nb_)
            al = self.lin_alpha[J, ax]
            dl = np.where(on, (-C - al * self.llam[J, ax]) / np.where(on, w + al, dt(1)), dt(0))
            self.llam[J, ax] = self.llam[J, ax] + dl
            p = n * dl[:, None]
            o = on[:, None]
            xa = np.where(o, xa - p * ima[:, None], xa)
            qa = np.where(o, rot_apply(qa, -(na * dl[:, None])), qa)
            xb = np.where(o, xb + p * imb[:, None], xb)
            qb = np.where(o, rot_apply(qb, nb_ * dl[:, None]), qb)
        da, db = c["dyn"][a], c["dyn"][b]
        self.x[a[da]], self.q[a[da]] = xa[da], qa[da]
        self.x[b[db]], self.q[b[db]] = xb[db], qb[db]
