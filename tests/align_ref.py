"""PMX type-2 rigid bodies ("physics + bone position alignment") restated in NumPy: the definition rz_physics_aligned and the ALIGN
instantiations of kernels/physics.hip are held to. A subclass of spring_ref.Sim, so it composes with the linear springs and every contact
mode; include/reze_deform.h states the same rules in words.

Without the feature a body of type 2 follows its bone, exactly as type 0 (physics_ref.is_dynamic). MMD simulates it like a dynamic body and
lets its bone take the rotation only: the bone's position stays where the animation put it. With the feature on a body is ALIGNED when its
type is 2, its mass is > 0 and it has a bone (bone >= 0). A type-2 body with a mass and no bone becomes a plain dynamic body; a type-2 body
of mass 0 keeps following its bone. The aligned table is the same table with those bodies' type read as 1 (read_table) — integration,
joints in colour order, angular and linear springs, every contact mode, velocities from the pose change: all unchanged — plus two rules:
  1. re-pin, at the start of every step call (once per call, not per substep: a call is what a frame is to MMD): an aligned body keeps q, v
     and w from the state and its position becomes x = p_bone + rot(q (x) conj(q_off)) t_off, p_bone the translation of the bone's matrix
     in the un-overridden solve the call was given, (t_off, q_off) the body's offset. On a reset, the implicit one of the first step
     included, every body is placed on its bone as ever; that placement already satisfies the pin.
  2. emit: the override of an aligned body's bone takes its rotation from the body, q (x) conj(q_off), as every override does, and its
     translation column is copied from the solved bone matrix (the same values as world[bone] column 3, not x - R t_off). The state keeps
     the simulated x.
There is no pin constraint inside the solve: as in MMD, joints hold the body. An aligned body without a joint drifts during a call and is
re-pinned at the next. Consequences: substeps = 0 re-pins the aligned bodies and re-emits with the new bone position; step(n) is NOT n x
step(1) for a table with aligned bodies, because the re-pin is per call (it remains so for a table without them).
"""
import numpy as np

import spring_ref
from physics_ref import qconj, qmat, qmul


def aligned_bodies(t, on=True):
    """bool [nb]: the aligned bodies of table t with the feature on (all False with it off)"""
    return (np.asarray(t["type"]) == 2) & (np.asarray(t["mass"]) > 0) & (np.asarray(t["bone"]) >= 0) & bool(on)


def read_table(t, on=True):
    """the table as the solver reads it: a copy with the type of every type-2 body of mass > 0 set to 1 (with or without a bone)"""
    r = dict(t)
    ty = np.array(t["type"], copy=True)
    if on:
        ty[(ty == 2) & (np.asarray(t["mass"]) > 0)] = 1
    r["type"] = ty
    return r


class Sim(spring_ref.Sim):
    """spring_ref.Sim on read_table(table) with the two rules; aligned=False, or a table without an aligned body, steps exactly as
    spring_ref.Sim does on the table it was given"""

    def __init__(self, table, parents, bind, dtype=np.float64, mode=0, springs=False, aligned=True):
        super().__init__(read_table(table, aligned), parents, bind, dtype=dtype, mode=mode, springs=springs)
        self.aligned = aligned_bodies(table, aligned)
        self.solved = None              # [B, 16] the un-overridden solve of the last call, in the Sim's precision

    def _place(self, world16, which):
        """placement as ever, and rule 1: an aligned body that is not being placed (no reset) is put back onto its bone"""
        super()._place(world16, which)
        c, dt = self.c, self.dt
        self.solved = np.asarray(world16, dtype=dt).reshape(-1, 16)
        for b in np.nonzero(self.aligned & ~np.asarray(which, dtype=bool))[0]:
            R = qmat(qmul(self.q[b], qconj(c["off_q"][b])))
            self.x[b] = self.solved[int(c["bone"][b]), 12:15] + R @ c["off_p"][b]

    def overrides(self):
        """rule 2: an aligned bone's override keeps the solved matrix's translation column"""
        out = super().overrides()
        for b in np.nonzero(self.aligned)[0]:
            bone = int(self.c["bone"][b])
            out[bone][12:15] = self.solved[bone, 12:15]
        return out
