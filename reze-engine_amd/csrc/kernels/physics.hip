// kernels/physics.hip — rz_physics_kernel: rigid-body physics for PMX bodies and joints on the device (rz_upload_physics / rz_physics_step).
// XPBD rigid bodies in the form tests/physics_ref.py defines and include/reze_deform.h states; this file spells the same operations in the
// same order in float32. One workgroup = one instance. Per call:
//   load      a following body (type != 1 or mass 0; after a reset: every body) is placed at boneWorld x offset with zero velocity, from the
//             world matrices the hierarchy solve (with IK) has just left in memory; a dynamic body's state x | q | v | w comes from its
//             64-byte record. All of it lives in LDS from here on: 96 B per body (state + the substep's previous pose).
//   substeps  integrate (lane per body) | barrier | iterations x colours x { joints of the colour, lane per joint | barrier } | velocities
//             (lane per body: the lane that integrates the body next, so no barrier behind it)
//   store     the state records, and per dynamic body with a bone boneWorld = bodyWorld x offset^-1 as four 16-byte stores into the
//             hierarchy solve's override table (slot inst * nd + k, written by nobody else).
// Joints of one colour share no dynamic body (the upload colours them), so their lanes read and write disjoint LDS records; a following body
// may be shared and is only ever read. OWN: the table has no more joints than the block has lanes — lane t keeps joint t's constants (eight
// float4) and its spring multipliers in registers for the whole kernel; otherwise lanes stride over a colour, reload the constants per
// visit (they stay in L1 / L2) and keep the multipliers in LDS. The block is 64 lanes when the bodies and the widest colour fit a wave, else
// 256. Every phase ends in __syncthreads() in the source of both; under __launch_bounds__(64) the workgroup is one wave and the compiler
// emits no barrier instruction for it, only the wait for the wave's own LDS accesses (the 64-lane code objects hold no s_barrier, the
// 256-lane ones three: DESIGN.md 9.7).
// CONTACT (rz_physics_contacts; tests/contact_ref.py is its definition): in every iteration, behind the last joint colour, pass F — lane per
// dynamic body (the integrate loop's mapping), the body in registers across its list of following partners, which are only read from LDS,
// written back once | barrier — then pass D, the dynamic pairs colour by colour in the joints' striding form, a barrier per colour. The
// lists and shape records stay in global memory (constants every workgroup reads); the stage adds no LDS. Without CONTACT the kernel is
// the code it was. One solver: a front end finds the contact points, the normal and the penetration (steps 1 and 2), resolve_contact
// corrects and applies friction (steps 3 - 7). solve_contact is the front end for two segments. CONTACT = 2 (tests/contact_box_ref.py):
// boxes take part against spheres and capsules — the body's record carries a box bit, its half extents come from c_box, and
// solve_contact_boxes is the box front end, a fixed 24-step bisection in the box frame, ahead of the same resolve_contact. CONTACT = 3
// (tests/contact_boxbox_ref.py): pairs of two boxes are candidates too — solve_contact_box_box is their front end, a separating-axis
// search over the 15 axes and one contact point on the axis of least overlap, ahead of the same resolve_contact.
// LSPRING (rz_physics_springs; tests/spring_ref.py is its definition): the linear springs of a joint, the tail of solve_joint behind the
// angular springs — per axis with spring_position > 0 a compliant constraint on that component of the anchors' offset in A's joint frame.
// A joint's linear constants are one more float4 (alpha~ x, y, z | bits(axes)) from p.lin and three more multipliers: in registers with
// the rest under OWN, loaded per visit and kept in LDS ([nj][6] then) otherwise. Without LSPRING the kernel is the code it was.
// ALIGN (rz_physics_aligned; tests/align_ref.py is its definition): the table has bodies of PMX type 2 that are simulated. Such a body's
// record carries a flag in word 3's w. load: it takes the state path and is then pinned, once per call — x = the translation of its bone's
// solved matrix + rot(q (x) offset_q^-1) offset_p, with q, v and w as the state has them. store: its override takes the rotation from the
// body as every other does, and its translation column is the solved matrix's, copied as one float4. Nothing between the two changes.
// Without ALIGN the kernel is the code it was. The instantiations are split over two translation units by ALIGN, so that the two halves
// compile side by side: this file is the ALIGN = false half and rz_launch_physics; kernels/physics_align.hip compiles it again with
// RZ_PHYSICS_ALIGN defined true and gives rz_launch_physics_aligned_half.
#include "pass_parts.hip.h"
#include "../physics_table.h"       // rzphys::lds_bytes: the LDS arithmetic, where the host half's own test program reaches it

#ifndef RZ_PHYSICS_ALIGN
#define RZ_PHYSICS_ALIGN false
#endif

namespace {

#pragma clang fp contract(off)      // tests/physics_ref.py restates this arithmetic in float64, operation by operation

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(const float x, const float y, const float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(const V3 a, const V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(const V3 a, const V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(const V3 a, const float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator*(const V3 a, const V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator/(const V3 a, const float s) { return v3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ V3 neg(const V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot3(const V3 a, const V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(const V3 a, const V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ V3 xyz(const float4 a) { return v3(a.x, a.y, a.z); }

__device__ __forceinline__ float4 qmul(const float4 a, const float4 b)
{
    return make_float4(a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                       a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
                       a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w,
                       a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z);
}
__device__ __forceinline__ float4 qconj(const float4 a) { return make_float4(-a.x, -a.y, -a.z, a.w); }
// v turned by q:  v + w t + u x t,  t = 2 (u x v)
__device__ __forceinline__ V3 qrot(const float4 q, const V3 v)
{
    const V3 u = xyz(q);
    V3 t = cross3(u, v);
    t = t + t;
    return v + t * q.w + cross3(u, t);
}
__device__ __forceinline__ float4 qnormalize(const float4 q)
{
    const float l = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return make_float4(q.x / l, q.y / l, q.z / l, q.w / l);
}
// q = normalize(q + 1/2 [dphi, 0] (x) q)
__device__ __forceinline__ float4 rot_apply(const float4 q, const V3 d)
{
    const float4 m = qmul(make_float4(d.x, d.y, d.z, 0.0f), q);
    return qnormalize(make_float4(q.x + 0.5f * m.x, q.y + 0.5f * m.y, q.z + 0.5f * m.z, q.w + 0.5f * m.w));
}
// I^-1 v in world space for a body at rotation q with the body-frame diagonal ii
__device__ __forceinline__ V3 iinv(const float4 q, const V3 ii, const V3 v) { return qrot(q, ii * qrot(qconj(q), v)); }

// Euler angles 'XYZ' (R = Rx Ry Rz) of the rotation q, through the matrix entries three.js reads (the convention of the IK limits)
__device__ __forceinline__ V3 euler_xyz(const float4 q)
{
    const float x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const float xx = q.x * x2, xy = q.x * y2, xz = q.x * z2, yy = q.y * y2, yz = q.y * z2, zz = q.z * z2;
    const float wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
    const float m00 = 1.0f - (yy + zz), m01 = xy - wz, m02 = xz + wy, m11 = 1.0f - (xx + zz), m12 = yz - wx, m21 = yz + wx, m22 = 1.0f - (xx + yy);
    V3 e;
    e.y = asinf(fminf(fmaxf(m02, -1.0f), 1.0f));
    if (fabsf(m02) < 0.9999999f) { e.x = atan2f(-m12, m22); e.z = atan2f(-m01, m00); }
    else { e.x = atan2f(m21, m11); e.z = 0.0f; }
    return e;
}
__device__ __forceinline__ float4 from_euler_xyz(const V3 e)
{
    const float c1 = cosf(e.x * 0.5f), c2 = cosf(e.y * 0.5f), c3 = cosf(e.z * 0.5f);
    const float s1 = sinf(e.x * 0.5f), s2 = sinf(e.y * 0.5f), s3 = sinf(e.z * 0.5f);
    return make_float4(s1 * c2 * c3 + c1 * s2 * s3, c1 * s2 * c3 - s1 * c2 * s3, c1 * c2 * s3 + s1 * s2 * c3, c1 * c2 * c3 - s1 * s2 * s3);
}
__device__ __forceinline__ V3 clamp3(const V3 v, const V3 lo, const V3 hi)
{
    return v3(fminf(fmaxf(v.x, lo.x), hi.x), fminf(fmaxf(v.y, lo.y), hi.y), fminf(fmaxf(v.z, lo.z), hi.z));
}

constexpr float kEps = 1e-9f;

// a joint's constants (deform_kernels.h: the eight float4 of a joint record)
struct JointC {
    V3 r_a, r_b, pmin, pmax, rmin, rmax, alpha;
    float4 j_a, j_b;
    int a, b;
    uint32_t springs;
};
__device__ __forceinline__ JointC load_joint(const float4 *rec)
{
    const float4 w0 = rec[0], w1 = rec[1], w4 = rec[4], w5 = rec[5], w6 = rec[6], w7 = rec[7];
    JointC c;
    c.r_a = xyz(w0); c.a = (int)__float_as_uint(w0.w);
    c.r_b = xyz(w1); c.b = (int)__float_as_uint(w1.w);
    c.j_a = rec[2]; c.j_b = rec[3];
    c.pmin = xyz(w4); c.pmax = xyz(w5); c.rmin = xyz(w6); c.rmax = xyz(w7);
    c.alpha = v3(w4.w, w5.w, w6.w);
    c.springs = __float_as_uint(w7.w);
    return c;
}

// One joint, once: position, rotation limits, angular springs (tests/physics_ref.py: Sim._solve). sx / sq are the workgroup's body positions
// and rotations in LDS, `body` the static body records (inverse mass in word 0's w, inverse inertia in word 2), lam the joint's three spring
// multipliers. LSPRING: then the linear springs (tests/spring_ref.py: Sim._solve) with the joint's linear record lin and their multipliers ll.
template <bool LSPRING>
__device__ __forceinline__ void solve_joint(const JointC &c, const float4 *body, float4 *sx, float4 *sq, float &lam0, float &lam1, float &lam2,
                                            const float4 lin, float &ll0, float &ll1, float &ll2)
{
    const float4 ba0 = body[4 * c.a], ba2 = body[4 * c.a + 2], bb0 = body[4 * c.b], bb2 = body[4 * c.b + 2];
    const float ima = ba0.w, imb = bb0.w;
    const V3 iia = xyz(ba2), iib = xyz(bb2);
    V3 xa = xyz(sx[c.a]), xb = xyz(sx[c.b]);
    float4 qa = sq[c.a], qb = sq[c.b];
    // position
    {
        const V3 ra = qrot(qa, c.r_a), rb = qrot(qb, c.r_b);
        const float4 QA = qmul(qa, c.j_a);
        const V3 d = qrot(qconj(QA), (xb + rb) - (xa + ra));
        const V3 e = d - clamp3(d, c.pmin, c.pmax);
        const V3 cv = qrot(QA, e);
        const float C = sqrtf(dot3(cv, cv));
        if (C > kEps) {
            // K p = c: the anchors' relative displacement for a correction p, K = (1/m_A + 1/m_B) 1 - [r_A]x I_A^-1 [r_A]x - [r_B]x I_B^-1 [r_B]x,
            // column by column, solved by Cramer's rule
            V3 k[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const V3 u = v3(ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f);
                k[ax] = u * (ima + imb) + cross3(iinv(qa, iia, cross3(ra, u)), ra) + cross3(iinv(qb, iib, cross3(rb, u)), rb);
            }
            const float det = dot3(k[0], cross3(k[1], k[2]));
            if (det > 0.0f) {
                const V3 p = v3(dot3(cv, cross3(k[1], k[2])), dot3(k[0], cross3(cv, k[2])), dot3(k[0], cross3(k[1], cv))) / det;
                const float4 qa_new = rot_apply(qa, iinv(qa, iia, cross3(ra, p)));
                const float4 qb_new = rot_apply(qb, neg(iinv(qb, iib, cross3(rb, p))));
                xa = xa + p * ima; xb = xb - p * imb;
                qa = qa_new; qb = qb_new;
            }
        }
    }
    // rotation limits
    {
        const float4 QA = qmul(qa, c.j_a), QB = qmul(qb, c.j_b);
        const float4 qrel = qmul(qconj(QA), QB);
        const V3 eu = euler_xyz(qrel);
        const V3 ec = clamp3(eu, c.rmin, c.rmax);
        if (ec.x != eu.x || ec.y != eu.y || ec.z != eu.z) {
            float4 dq = qmul(qmul(QA, qmul(from_euler_xyz(ec), qconj(qrel))), qconj(QA));
            if (dq.w < 0.0f) dq = make_float4(-dq.x, -dq.y, -dq.z, -dq.w);
            const float s = sqrtf(dot3(xyz(dq), xyz(dq)));
            if (s > kEps) {
                const V3 n = xyz(dq) / s;
                const float theta = 2.0f * atan2f(s, dq.w);
                // K l = theta n with K = I_A^-1 + I_B^-1 (world), column by column, Cramer's rule; A turns by -I_A^-1 l, B by +I_B^-1 l
                V3 k[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const V3 u = v3(ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f);
                    k[ax] = iinv(qa, iia, u) + iinv(qb, iib, u);
                }
                const float det = dot3(k[0], cross3(k[1], k[2]));
                if (det > 0.0f) {
                    const V3 rhs = n * theta;
                    const V3 lm = v3(dot3(rhs, cross3(k[1], k[2])), dot3(k[0], cross3(rhs, k[2])), dot3(k[0], cross3(k[1], rhs))) / det;
                    const float4 qa_new = rot_apply(qa, neg(iinv(qa, iia, lm)));
                    const float4 qb_new = rot_apply(qb, iinv(qb, iib, lm));
                    qa = qa_new; qb = qb_new;
                }
            }
        }
    }
    // angular springs
    if (c.springs) {
        const float4 QA = qmul(qa, c.j_a), QB = qmul(qb, c.j_b);
        const V3 eu = euler_xyz(qmul(qconj(QA), QB));
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!(c.springs >> ax & 1u)) continue;
            // the gimbal axis of that angle: x in A's joint frame, y turned by the x angle, z in B's joint frame
            const V3 n = ax == 0 ? qrot(QA, v3(1.0f, 0.0f, 0.0f)) : ax == 1 ? qrot(QA, v3(0.0f, cosf(eu.x), sinf(eu.x))) : qrot(QB, v3(0.0f, 0.0f, 1.0f));
            const V3 na = iinv(qa, iia, n), nb = iinv(qb, iib, n);
            const float al = ax == 0 ? c.alpha.x : ax == 1 ? c.alpha.y : c.alpha.z;
            const float ang = ax == 0 ? eu.x : ax == 1 ? eu.y : eu.z;
            float &lam = ax == 0 ? lam0 : ax == 1 ? lam1 : lam2;
            const float dl = (-ang - al * lam) / (dot3(n, na) + dot3(n, nb) + al);
            lam = lam + dl;
            qa = rot_apply(qa, neg(na * dl));
            qb = rot_apply(qb, nb * dl);
        }
    }
    // linear springs: per axis, from the pose the axis before left, the anchors' offset along that axis of A's joint frame
    if constexpr (LSPRING) {
        const uint32_t axes = __float_as_uint(lin.w);
        if (axes) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!(axes >> ax & 1u)) continue;
                const V3 ra = qrot(qa, c.r_a), rb = qrot(qb, c.r_b);
                const V3 n = qrot(qmul(qa, c.j_a), v3(ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f));
                const float C = dot3(n, (xb + rb) - (xa + ra));
                const V3 can = cross3(ra, n), cbn = cross3(rb, n);
                const V3 na = iinv(qa, iia, can), nb = iinv(qb, iib, cbn);
                const float w = ((ima + imb) + dot3(can, na)) + dot3(cbn, nb);
                const float al = ax == 0 ? lin.x : ax == 1 ? lin.y : lin.z;
                float &lam = ax == 0 ? ll0 : ax == 1 ? ll1 : ll2;
                const float dl = (-C - al * lam) / (w + al);
                lam = lam + dl;
                const V3 p = n * dl;
                xa = xa - p * ima; qa = rot_apply(qa, neg(na * dl));
                xb = xb + p * imb; qb = rot_apply(qb, nb * dl);
            }
        }
    }
    // only dynamic bodies are written: a following body may be shared inside a colour and never moves
    if (ima > 0.0f) { sx[c.a] = make_float4(xa.x, xa.y, xa.z, 0.0f); sq[c.a] = qa; }
    if (imb > 0.0f) { sx[c.b] = make_float4(xb.x, xb.y, xb.z, 0.0f); sq[c.b] = qb; }
}

// a body as the contact stage sees it. A following body: im = 0, ii = 0, previous pose = current pose (its sxp / sqp slots are never written)
struct CBody {
    V3 x, xp, ii;
    float4 q, qp;
    float im, r, hl, mu;
};
__device__ __forceinline__ CBody load_cbody(const int b, const float4 *body, const float4 *cshape, const float4 *sx, const float4 *sq, const float4 *sxp, const float4 *sqp)
{
    const float4 b0 = body[4 * b], b2 = body[4 * b + 2], sh = cshape[b];
    CBody c;
    c.im = b0.w; c.ii = xyz(b2);
    c.r = sh.x; c.hl = sh.y; c.mu = sh.z;
    c.x = xyz(sx[b]); c.q = sq[b];
    if (c.im > 0.0f) { c.xp = xyz(sxp[b]); c.qp = sqp[b]; }
    else { c.xp = c.x; c.qp = c.q; }
    return c;
}
__device__ __forceinline__ float clamp01(const float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// Steps 3 - 7 of one contact, whichever front end found it (tests/contact_ref.py: Sim._resolve, the same operations in the same order):
// from the contact points cA and cB, the normal n from A to B and the penetration pen, the arms, the generalised inverse mass, the
// correction and the friction. Only a dynamic body is corrected; the caller writes back what it owns.
__device__ __forceinline__ void resolve_contact(CBody &A, CBody &B, const V3 cA, const V3 cB, const V3 n, const float pen)
{
    // 3, 4
    const V3 ra = (cA + n * A.r) - A.x, rb = (cB - n * B.r) - B.x;
    const V3 can = cross3(ra, n), cbn = cross3(rb, n);
    const float w = (A.im + dot3(can, iinv(A.q, A.ii, can))) + (B.im + dot3(cbn, iinv(B.q, B.ii, cbn)));
    if (!(w > 0.0f)) return;
    // 5
    const float dl = pen / w;
    const V3 p = n * dl;
    const float4 qa0 = A.q, qb0 = B.q;
    if (A.im > 0.0f) { const float4 qn = rot_apply(A.q, neg(iinv(A.q, A.ii, cross3(ra, p)))); A.x = A.x - p * A.im; A.q = qn; }
    if (B.im > 0.0f) { const float4 qn = rot_apply(B.q, iinv(B.q, B.ii, cross3(rb, p))); B.x = B.x + p * B.im; B.q = qn; }
    // 6. friction
    const float mu = A.mu * B.mu;
    if (!(mu > 0.0f)) return;
    const V3 la = qrot(qconj(qa0), ra), lb = qrot(qconj(qb0), rb);
    const V3 ra2 = qrot(A.q, la), rb2 = qrot(B.q, lb);
    const V3 D = ((A.x + ra2) - (A.xp + qrot(A.qp, la))) - ((B.x + rb2) - (B.xp + qrot(B.qp, lb)));
    const V3 Dt = D - n * dot3(D, n);
    const float lt = sqrtf(dot3(Dt, Dt));
    if (!(lt > kEps)) return;
    const V3 td = Dt / lt;
    const V3 cat = cross3(ra2, td), cbt = cross3(rb2, td);
    const float wt = (A.im + dot3(cat, iinv(A.q, A.ii, cat))) + (B.im + dot3(cbt, iinv(B.q, B.ii, cbt)));
    if (!(wt > 0.0f)) return;
    const float sz = fminf(lt / wt, mu * dl);
    const V3 pt = td * sz;
    if (A.im > 0.0f) { const float4 qn = rot_apply(A.q, neg(iinv(A.q, A.ii, cross3(ra2, pt)))); A.x = A.x - pt * A.im; A.q = qn; }
    if (B.im > 0.0f) { const float4 qn = rot_apply(B.q, iinv(B.q, B.ii, cross3(rb2, pt))); B.x = B.x + pt * B.im; B.q = qn; }
}

// Step 1 of tests/contact_ref.py on its own, for the edges of two boxes: the closest points cA, cB of the segments p1 + s d1 and p2 + t d2,
// s and t in [0, 1]. solve_contact below keeps its own spelling of the same solve: calling this one from there changes the instruction
// streams of the CONTACT = 1 and 2 instantiations (four instructions fewer each), and those stay what they were.
__device__ __forceinline__ void closest_on_segments(const V3 p1, const V3 d1, const V3 p2, const V3 d2, V3 &cA, V3 &cB)
{
    const V3 r = p1 - p2;
    const float a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r), c = dot3(d1, r), b = dot3(d1, d2);
    float s, t;
    if (a <= kEps) {
        s = 0.0f;
        t = e <= kEps ? 0.0f : clamp01(f / e);
    } else if (e <= kEps) {
        t = 0.0f;
        s = clamp01(-c / a);
    } else {
        const float den = a * e - b * b;
        s = den > kEps ? clamp01((b * f - c * e) / den) : 0.0f;
        t = (b * s + f) / e;
        if (t < 0.0f) { t = 0.0f; s = clamp01(-c / a); }
        else if (t > 1.0f) { t = 1.0f; s = clamp01((b - c) / a); }
    }
    cA = p1 + d1 * s; cB = p2 + d2 * t;
}

// One contact, once, A the lower index: steps 1 and 2 for two segments (tests/contact_ref.py: Sim._contact, the same operations in the
// same order), then resolve_contact.
__device__ __forceinline__ void solve_contact(CBody &A, CBody &B)
{
    // 1. closest points of the two segments
    const V3 ua = qrot(A.q, v3(0.0f, A.hl, 0.0f)), ub = qrot(B.q, v3(0.0f, B.hl, 0.0f));
    const V3 p1 = A.x - ua, p2 = B.x - ub, d1 = ua + ua, d2 = ub + ub;
    const V3 r = p1 - p2;
    const float a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r), c = dot3(d1, r), b = dot3(d1, d2);
    float s, t;
    if (a <= kEps) {
        s = 0.0f;
        t = e <= kEps ? 0.0f : clamp01(f / e);
    } else if (e <= kEps) {
        t = 0.0f;
        s = clamp01(-c / a);
    } else {
        const float den = a * e - b * b;
        s = den > kEps ? clamp01((b * f - c * e) / den) : 0.0f;
        t = (b * s + f) / e;
        if (t < 0.0f) { t = 0.0f; s = clamp01(-c / a); }
        else if (t > 1.0f) { t = 1.0f; s = clamp01((b - c) / a); }
    }
    const V3 cA = p1 + d1 * s, cB = p2 + d2 * t;
    // 2
    const V3 d = cB - cA;
    const float dist = sqrtf(dot3(d, d));
    const float pen = (A.r + B.r) - dist;
    if (!(pen > 0.0f && dist > kEps)) return;
    resolve_contact(A, B, cA, cB, d / dist, pen);
}

// CONTACT = 2: a body with its half extents (a box: r = 0, hl = 0; every other body: box = false, e unread)
struct CBox : CBody {
    V3 e;
    bool box;
};
__device__ __forceinline__ CBox load_cbox(const int b, const float4 *body, const float4 *cshape, const float4 *cbox, const float4 *sx, const float4 *sq, const float4 *sxp, const float4 *sqp)
{
    CBox c;
    static_cast<CBody &>(c) = load_cbody(b, body, cshape, sx, sq, sxp, sqp);
    c.box = (__float_as_uint(cshape[b].w) & 4u) != 0;
    c.e = v3(0.0f, 0.0f, 0.0f);
    if (c.box) c.e = xyz(cbox[b]);
    return c;
}

// f(s) of the definition: half the derivative of the squared distance between P + s d and the box |y_i| <= e_i
__device__ __forceinline__ float box_slope(const V3 P, const V3 d, const V3 e, const float s)
{
    const V3 c = P + d * s;
    return dot3(c - clamp3(c, neg(e), e), d);
}
// the parameter s in [0, 1] at which the segment P + s d (box frame) is closest to the box: a fixed trip count with selects, so lanes
// that meet a box do not diverge among themselves whatever their geometry
__device__ __forceinline__ float box_closest(const V3 P, const V3 d, const V3 e)
{
    const float f0 = box_slope(P, d, e, 0.0f), f1 = box_slope(P, d, e, 1.0f);
    float lo = 0.0f, hi = 1.0f;
#pragma unroll 1
    for (int k = 0; k < 24; ++k) {
        const float m = (lo + hi) * 0.5f;
        const bool up = box_slope(P, d, e, m) > 0.0f;
        hi = up ? m : hi;
        lo = up ? lo : m;
    }
    return f0 >= 0.0f ? 0.0f : f1 <= 0.0f ? 1.0f : (lo + hi) * 0.5f;
}

// One contact under CONTACT = 2: the box front end (tests/contact_box_ref.py: Sim._box_contact, the same operations in the same order),
// then resolve_contact. A pair without a box is solve_contact's; a pair of two boxes does not occur (contact_table.h leaves them out).
__device__ __forceinline__ void solve_contact_boxes(CBox &A, CBox &B)
{
    if (!(A.box || B.box)) { solve_contact(A, B); return; }
    // 1. X the box, R the round shape
    const bool ax = A.box;
    const V3 xX = ax ? A.x : B.x, xR = ax ? B.x : A.x, e = ax ? A.e : B.e;
    const float4 qX = ax ? A.q : B.q, qR = ax ? B.q : A.q;
    const float r = ax ? B.r : A.r, hl = ax ? B.hl : A.hl;
    const V3 u = qrot(qR, v3(0.0f, hl, 0.0f));
    const V3 P = xR - u, d = u + u;
    const float4 qi = qconj(qX);
    const V3 Pl = qrot(qi, P - xX), dl_ = qrot(qi, d);
    const float s = box_closest(Pl, dl_, e);
    const V3 cl = Pl + dl_ * s;
    const V3 bl = clamp3(cl, neg(e), e);
    const V3 cR = P + d * s;
    const V3 gap = cl - bl;
    const bool deep = !(sqrtf(dot3(gap, gap)) > kEps);
    V3 n, cX;
    float pen;
    if (deep) {
        // the face the centre line is nearest to; the first of x, y, z wins a tie
        const float mx = e.x - fabsf(cl.x), my = e.y - fabsf(cl.y), mz = e.z - fabsf(cl.z);
        const int i = (mx <= my && mx <= mz) ? 0 : (my <= mz ? 1 : 2);
        const float ci = i == 0 ? cl.x : i == 1 ? cl.y : cl.z, ei = i == 0 ? e.x : i == 1 ? e.y : e.z, mi = i == 0 ? mx : i == 1 ? my : mz;
        const float sg = ci >= 0.0f ? 1.0f : -1.0f;
        const V3 face = v3(i == 0 ? sg * ei : cl.x, i == 1 ? sg * ei : cl.y, i == 2 ? sg * ei : cl.z);
        const V3 N = qrot(qX, v3(i == 0 ? sg : 0.0f, i == 1 ? sg : 0.0f, i == 2 ? sg : 0.0f));
        cX = xX + qrot(qX, face);
        pen = r + mi;
        n = ax ? N : neg(N);
    } else {
        cX = xX + qrot(qX, bl);
    }
    const V3 cA = ax ? cX : cR, cB = ax ? cR : cX;
    if (!deep) {
        // 2
        const V3 dv = cB - cA;
        const float dist = sqrtf(dot3(dv, dv));
        pen = (A.r + B.r) - dist;
        if (!(pen > 0.0f && dist > kEps)) return;
        n = dv / dist;
    }
    resolve_contact(A, B, cA, cB, n, pen);
}

// component i of v, and the members of a triple rotated by i — (v_i, v_i+1, v_i+2) —, by selects: the box - box front end indexes nothing at
// run time (a register array indexed by a variable would go to scratch)
__device__ __forceinline__ float pick(const V3 v, const int i) { return i == 0 ? v.x : i == 1 ? v.y : v.z; }
__device__ __forceinline__ float pick(const int i, const float a, const float b, const float c) { return i == 0 ? a : i == 1 ? b : c; }
__device__ __forceinline__ V3 pick(const int i, const V3 a, const V3 b, const V3 c)
{
    return v3(pick(i, a.x, b.x, c.x), pick(i, a.y, b.y, c.y), pick(i, a.z, b.z, c.z));
}
__device__ __forceinline__ float clamp11(const float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }
__device__ __forceinline__ float sign_of(const float v) { return v >= 0.0f ? 1.0f : -1.0f; }

// CONTACT = 3, one contact of two boxes, A the lower index: step 1 of tests/contact_boxbox_ref.py (Sim._boxbox_contact, the same operations
// in the same order) — the overlaps of the 15 axes, the choice between the best face and the best edge axis, the face's or the edges'
// contact points — then resolve_contact. The 15 axes are walked with compile-time indices; "the first smallest" is a chain of strict <.
__device__ __forceinline__ void solve_contact_box_box(CBox &A, CBox &B)
{
    const V3 a0 = qrot(A.q, v3(1.0f, 0.0f, 0.0f)), a1 = qrot(A.q, v3(0.0f, 1.0f, 0.0f)), a2 = qrot(A.q, v3(0.0f, 0.0f, 1.0f));
    const V3 b0 = qrot(B.q, v3(1.0f, 0.0f, 0.0f)), b1 = qrot(B.q, v3(0.0f, 1.0f, 0.0f)), b2 = qrot(B.q, v3(0.0f, 0.0f, 1.0f));
    const V3 t = B.x - A.x;
    const V3 c0 = v3(dot3(a0, b0), dot3(a0, b1), dot3(a0, b2)), c1 = v3(dot3(a1, b0), dot3(a1, b1), dot3(a1, b2)), c2 = v3(dot3(a2, b0), dot3(a2, b1), dot3(a2, b2));
    const V3 tA = v3(dot3(a0, t), dot3(a1, t), dot3(a2, t)), tB = v3(dot3(b0, t), dot3(b1, t), dot3(b2, t));
    const V3 eA = A.e, eB = B.e;
    // 1a, 1b: the faces in the order A0 A1 A2 B0 B1 B2
    float of = 0.0f, oe = 0.0f;
    int kf = 0, ke = -1;
    bool apart = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = k % 3;
        float o;
        if (k < 3) {
            const V3 c = pick(i, c0, c1, c2);
            o = (pick(eA, i) + ((eB.x * fabsf(c.x) + eB.y * fabsf(c.y)) + eB.z * fabsf(c.z))) - fabsf(pick(tA, i));
        } else {
            o = (((eA.x * fabsf(pick(c0, i)) + eA.y * fabsf(pick(c1, i))) + eA.z * fabsf(pick(c2, i))) + pick(eB, i)) - fabsf(pick(tB, i));
        }
        apart = apart || o <= 0.0f;
        if (k == 0 || o < of) { of = o; kf = k; }
    }
    // the edges in the order (0,0), (0,1) .. (2,2); a near-parallel pair is not considered
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int i = k / 3, j = k % 3, i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        const V3 ci = pick(i, c0, c1, c2), ci1 = pick(i1, c0, c1, c2), ci2 = pick(i2, c0, c1, c2);
        const float cij = pick(ci, j);
        const float l2 = 1.0f - cij * cij;
        const bool considered = l2 > 1e-6f;
        const float r = ((pick(eA, i1) * fabsf(pick(ci2, j)) + pick(eA, i2) * fabsf(pick(ci1, j))) + pick(eB, j1) * fabsf(pick(ci, j2))) + pick(eB, j2) * fabsf(pick(ci, j1));
        const float o = (r - fabsf(pick(tA, i2) * pick(ci1, j) - pick(tA, i1) * pick(ci2, j))) / sqrtf(considered ? l2 : 1.0f);
        apart = apart || (considered && o <= 0.0f);
        if (considered && (ke < 0 || o < oe)) { oe = o; ke = k; }
    }
    if (apart) return;
    const bool edge = ke >= 0 && oe < 0.95f * of;
    const float pen = edge ? oe : of;
    V3 cA, cB, n;
    if (!edge) {
        // 1c. X the reference box, Y the incident one
        const bool xa = kf < 3;
        const int i = xa ? kf : kf - 3;
        const V3 xX = xa ? A.x : B.x, xY = xa ? B.x : A.x, eX = xa ? eA : eB, eY = xa ? eB : eA;
        const float4 qX = xa ? A.q : B.q;
        const V3 y0 = xa ? b0 : a0, y1 = xa ? b1 : a1, y2 = xa ? b2 : a2;
        const V3 axis = xa ? pick(i, a0, a1, a2) : pick(i, b0, b1, b2);
        const float sg = sign_of(xa ? pick(tA, i) : -pick(tB, i));
        const V3 N = axis * sg;
        V3 p = xY - y0 * (clamp11(dot3(N, y0) / 0.05f) * eY.x);
        p = p - y1 * (clamp11(dot3(N, y1) / 0.05f) * eY.y);
        p = p - y2 * (clamp11(dot3(N, y2) / 0.05f) * eY.z);
        const V3 pl = clamp3(qrot(qconj(qX), p - xX), neg(eX), eX);
        const float on = sg * pick(eX, i);
        const V3 cX = xX + qrot(qX, v3(i == 0 ? on : pl.x, i == 1 ? on : pl.y, i == 2 ? on : pl.z));
        const V3 cY = cX - N * pen;
        n = xa ? N : neg(N);
        cA = xa ? cX : cY; cB = xa ? cY : cX;
    } else {
        // 1d. the two edges
        const int i = ke / 3, j = ke - 3 * i;
        const V3 ai = pick(i, a0, a1, a2), ai1 = pick(i, a1, a2, a0), ai2 = pick(i, a2, a0, a1);
        const V3 bj = pick(j, b0, b1, b2), bj1 = pick(j, b1, b2, b0), bj2 = pick(j, b2, b0, b1);
        const V3 c = cross3(ai, bj);
        const V3 L = c / sqrtf(dot3(c, c));
        n = dot3(t, L) >= 0.0f ? L : neg(L);
        const V3 ctrA = (A.x + ai1 * (sign_of(dot3(ai1, n)) * pick(i, eA.y, eA.z, eA.x))) + ai2 * (sign_of(dot3(ai2, n)) * pick(i, eA.z, eA.x, eA.y));
        const V3 ctrB = (B.x - bj1 * (sign_of(dot3(bj1, n)) * pick(j, eB.y, eB.z, eB.x))) - bj2 * (sign_of(dot3(bj2, n)) * pick(j, eB.z, eB.x, eB.y));
        const V3 ua = ai * pick(eA, i), ub = bj * pick(eB, j);
        closest_on_segments(ctrA - ua, ua + ua, ctrB - ub, ub + ub, cA, cB);
    }
    resolve_contact(A, B, cA, cB, n, pen);
}

// One contact under CONTACT = 3: no box — solve_contact; one box — the box front end; two boxes — solve_contact_box_box
__device__ __forceinline__ void solve_contact_all(CBox &A, CBox &B)
{
    if (A.box && B.box) solve_contact_box_box(A, B);
    else solve_contact_boxes(A, B);
}

// the contact stage's body and solve by mode. Two body types, not one with the box fields always there: CBody is small enough to come
// back from its loader in registers, and growing it changes the code of CONTACT = 1 (profiles/contact_fold_identity.txt)
template <int CONTACT> struct ContactOps {
    using Body = CBody;
    static __device__ __forceinline__ Body load(const int b, const float4 *body, const float4 *cshape, const float4 *, const float4 *sx, const float4 *sq, const float4 *sxp, const float4 *sqp)
    {
        return load_cbody(b, body, cshape, sx, sq, sxp, sqp);
    }
    static __device__ __forceinline__ void solve(Body &A, Body &B) { solve_contact(A, B); }
};
template <> struct ContactOps<2> {
    using Body = CBox;
    static __device__ __forceinline__ Body load(const int b, const float4 *body, const float4 *cshape, const float4 *cbox, const float4 *sx, const float4 *sq, const float4 *sxp, const float4 *sqp)
    {
        return load_cbox(b, body, cshape, cbox, sx, sq, sxp, sqp);
    }
    static __device__ __forceinline__ void solve(Body &A, Body &B) { solve_contact_boxes(A, B); }
};
template <> struct ContactOps<3> : ContactOps<2> {
    static __device__ __forceinline__ void solve(Body &A, Body &B) { solve_contact_all(A, B); }
};

// the rotation of the unit quaternion q, row by row: the arithmetic of the store loop's override, for the re-pin of ALIGN (the store loop keeps
// its own spelling, as solve_contact keeps its closest-point solve: the existing instantiations stay the instruction streams they were)
struct M3 { float m00, m01, m02, m10, m11, m12, m20, m21, m22; };
[[maybe_unused]] __device__ __forceinline__ M3 mat_of(const float4 qb)
{
    const float x2 = qb.x + qb.x, y2 = qb.y + qb.y, z2 = qb.z + qb.z;
    const float xx = qb.x * x2, xy = qb.x * y2, xz = qb.x * z2, yy = qb.y * y2, yz = qb.y * z2, zz = qb.z * z2;
    const float wx = qb.w * x2, wy = qb.w * y2, wz = qb.w * z2;
    M3 m;
    m.m00 = 1.0f - (yy + zz); m.m01 = xy - wz; m.m02 = xz + wy;
    m.m10 = xy + wz; m.m11 = 1.0f - (xx + zz); m.m12 = yz - wx;
    m.m20 = xz - wy; m.m21 = yz + wx; m.m22 = 1.0f - (xx + yy);
    return m;
}

template <int BLOCK, bool OWN, int CONTACT, bool LSPRING, bool ALIGN>
__global__ void __launch_bounds__(BLOCK) rz_physics_kernel(const RzPhysicsParams p)
{
    extern __shared__ float4 ph_lds[];
    const int tid = threadIdx.x, inst = blockIdx.x, nb = p.nb;
    float4 *sx = ph_lds, *sq = sx + nb, *sv = sq + nb, *sw = sv + nb, *sxp = sw + nb, *sqp = sxp + nb;
    constexpr int NLAM = LSPRING ? 6 : 3;
    float *slam = reinterpret_cast<float *>(sqp + nb);              // [nj][NLAM], the striding form only
    float4 *state = p.state + (size_t)inst * nb * 4;
    const float *world = p.world + (size_t)inst * p.B * 16;

    for (int b = tid; b < nb; b += BLOCK) {
        const float4 b0 = p.body[4 * b], b1 = p.body[4 * b + 1], b3 = p.body[4 * b + 3];
        const int bone = (int)__float_as_uint(b3.y);
        const bool dyn = b0.w > 0.0f;
        float4 x, q, v, w;
        if (!dyn || p.reset) {
            V3 px = xyz(b0);
            q = b1;
            if (bone >= 0) {
                const float4 *m = reinterpret_cast<const float4 *>(world + (size_t)bone * 16);
                const float4 c0 = m[0], c1 = m[1], c2 = m[2], c3 = m[3];
                const float4 r0 = make_float4(c0.x, c1.x, c2.x, c3.x), r1 = make_float4(c0.y, c1.y, c2.y, c3.y), r2 = make_float4(c0.z, c1.z, c2.z, c3.z);
                const Quatf qw = quat_of_rows(r0, r1, r2);
                q = qmul(make_float4(qw.x, qw.y, qw.z, qw.w), b1);
                const V3 o = px;
                px = v3((r0.x * o.x + r0.y * o.y + r0.z * o.z) + r0.w, (r1.x * o.x + r1.y * o.y + r1.z * o.z) + r1.w, (r2.x * o.x + r2.y * o.y + r2.z * o.z) + r2.w);
            }
            x = make_float4(px.x, px.y, px.z, 0.0f);
            v = w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            x = state[4 * b]; q = state[4 * b + 1]; v = state[4 * b + 2]; w = state[4 * b + 3];
            if constexpr (ALIGN) {
                // an aligned body (it has a bone: physics_table.h) goes back onto its bone, once per call: the solved bone position + R offset_p
                if (b3.w != 0.0f) {
                    const float4 c3 = reinterpret_cast<const float4 *>(world + (size_t)bone * 16)[3];
                    const M3 m = mat_of(qmul(q, qconj(b1)));
                    x = make_float4(c3.x + (m.m00 * b0.x + m.m01 * b0.y + m.m02 * b0.z), c3.y + (m.m10 * b0.x + m.m11 * b0.y + m.m12 * b0.z),
                                    c3.z + (m.m20 * b0.x + m.m21 * b0.y + m.m22 * b0.z), 0.0f);
                }
            }
        }
        sx[b] = x; sq[b] = q; sv[b] = v; sw[b] = w;
    }
    JointC own;
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
    float4 own_lin = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    if (OWN && tid < p.nj) own = load_joint(p.joint + (size_t)tid * 8);
    if constexpr (LSPRING && OWN) { if (tid < p.nj) own_lin = p.lin[tid]; }
    __syncthreads();

    const float h = p.h;
    for (int s = 0; s < p.substeps; ++s) {
        for (int b = tid; b < nb; b += BLOCK) {
            const float4 b0 = p.body[4 * b], b2 = p.body[4 * b + 2], b3 = p.body[4 * b + 3];
            if (b0.w > 0.0f) {
                V3 v = xyz(sv[b]), w = xyz(sw[b]);
                v = v + v3(h * p.gx, h * p.gy, h * p.gz);
                v = v * b2.w; w = w * b3.x;
                const float4 x = sx[b], q = sq[b];
                sxp[b] = x; sqp[b] = q;
                const V3 xn = xyz(x) + v * h;
                const float4 m = qmul(make_float4(w.x, w.y, w.z, 0.0f), q);
                const float hh = h * 0.5f;
                sx[b] = make_float4(xn.x, xn.y, xn.z, 0.0f);
                sq[b] = qnormalize(make_float4(q.x + hh * m.x, q.y + hh * m.y, q.z + hh * m.z, q.w + hh * m.w));
                sv[b] = make_float4(v.x, v.y, v.z, 0.0f); sw[b] = make_float4(w.x, w.y, w.z, 0.0f);
            }
        }
        if (OWN) { l0 = l1 = l2 = 0.0f; m0 = m1 = m2 = 0.0f; }
        else for (int k = tid; k < NLAM * p.nj; k += BLOCK) slam[k] = 0.0f;
        __syncthreads();
        for (int it = 0; it < p.iterations; ++it) {
            for (int col = 0; col < p.ncol; ++col) {
                const int j0 = p.colour_off[col], j1 = p.colour_off[col + 1];
                if (OWN) {
                    if (tid >= j0 && tid < j1) solve_joint<LSPRING>(own, p.body, sx, sq, l0, l1, l2, own_lin, m0, m1, m2);
                } else {
                    for (int j = j0 + tid; j < j1; j += BLOCK) {
                        const JointC c = load_joint(p.joint + (size_t)j * 8);
                        float *lj = slam + NLAM * j;
                        if constexpr (LSPRING) solve_joint<true>(c, p.body, sx, sq, lj[0], lj[1], lj[2], p.lin[j], lj[3], lj[4], lj[5]);
                        else solve_joint<false>(c, p.body, sx, sq, lj[0], lj[1], lj[2], own_lin, m0, m1, m2);
                    }
                }
                __syncthreads();
            }
            if (CONTACT) {
                using Ops = ContactOps<CONTACT>;
                // pass F: a dynamic body against its following partners, in list order
                for (int b = tid; b < nb; b += BLOCK) {
                    if (!(p.body[4 * b].w > 0.0f)) continue;
                    const int f0 = p.c_follow_off[b], f1 = p.c_follow_off[b + 1];
                    if (f0 == f1) continue;
                    typename Ops::Body me = Ops::load(b, p.body, p.c_shape, p.c_box, sx, sq, sxp, sqp);
                    for (int k = f0; k < f1; ++k) {
                        const int o = p.c_follow_idx[k];
                        typename Ops::Body other = Ops::load(o, p.body, p.c_shape, p.c_box, sx, sq, sxp, sqp);
                        if (b < o) Ops::solve(me, other); else Ops::solve(other, me);
                    }
                    sx[b] = make_float4(me.x.x, me.x.y, me.x.z, 0.0f); sq[b] = me.q;
                }
                __syncthreads();
                // pass D: the dynamic pairs of a colour share no body
                for (int col = 0; col < p.c_ncol; ++col) {
                    const int j0 = p.c_colour_off[col], j1 = p.c_colour_off[col + 1];
                    for (int j = j0 + tid; j < j1; j += BLOCK) {
                        const int2 ab = p.c_pair[j];
                        typename Ops::Body A = Ops::load(ab.x, p.body, p.c_shape, p.c_box, sx, sq, sxp, sqp), B = Ops::load(ab.y, p.body, p.c_shape, p.c_box, sx, sq, sxp, sqp);
                        Ops::solve(A, B);
                        sx[ab.x] = make_float4(A.x.x, A.x.y, A.x.z, 0.0f); sq[ab.x] = A.q;
                        sx[ab.y] = make_float4(B.x.x, B.x.y, B.x.z, 0.0f); sq[ab.y] = B.q;
                    }
                    __syncthreads();
                }
            }
        }
        for (int b = tid; b < nb; b += BLOCK) {
            if (p.body[4 * b].w > 0.0f) {
                const V3 v = (xyz(sx[b]) - xyz(sxp[b])) / h;
                const float4 dq = qmul(sq[b], qconj(sqp[b]));
                V3 om = (xyz(dq) * 2.0f) / h;
                if (dq.w < 0.0f) om = neg(om);
                sv[b] = make_float4(v.x, v.y, v.z, 0.0f); sw[b] = make_float4(om.x, om.y, om.z, 0.0f);
            }
        }
        // (no barrier: the lane that wrote body b's velocities is the lane that integrates body b)
    }

    for (int b = tid; b < nb; b += BLOCK) {
        const float4 x = sx[b], q = sq[b];
        state[4 * b] = x; state[4 * b + 1] = q; state[4 * b + 2] = sv[b]; state[4 * b + 3] = sw[b];
        const float4 b0 = p.body[4 * b], b1 = p.body[4 * b + 1], b3 = p.body[4 * b + 3];
        const int slot = (int)__float_as_uint(b3.z);
        if (slot >= 0) {
            // boneWorld = bodyWorld x offset^-1: rotation q (x) offset_q^-1, translation x - R offset_p
            const float4 qb = qmul(q, qconj(b1));
            const float x2 = qb.x + qb.x, y2 = qb.y + qb.y, z2 = qb.z + qb.z;
            const float xx = qb.x * x2, xy = qb.x * y2, xz = qb.x * z2, yy = qb.y * y2, yz = qb.y * z2, zz = qb.z * z2;
            const float wx = qb.w * x2, wy = qb.w * y2, wz = qb.w * z2;
            const float m00 = 1.0f - (yy + zz), m01 = xy - wz, m02 = xz + wy;
            const float m10 = xy + wz, m11 = 1.0f - (xx + zz), m12 = yz - wx;
            const float m20 = xz - wy, m21 = yz + wx, m22 = 1.0f - (xx + yy);
            const float tx = x.x - (m00 * b0.x + m01 * b0.y + m02 * b0.z);
            const float ty = x.y - (m10 * b0.x + m11 * b0.y + m12 * b0.z);
            const float tz = x.z - (m20 * b0.x + m21 * b0.y + m22 * b0.z);
            float4 *o = reinterpret_cast<float4 *>(p.ovr_world + ((size_t)inst * p.nd + slot) * 16);
            o[0] = make_float4(m00, m10, m20, 0.0f);
            o[1] = make_float4(m01, m11, m21, 0.0f);
            o[2] = make_float4(m02, m12, m22, 0.0f);
            if constexpr (ALIGN) {
                // an aligned body's bone stays where the hierarchy solve put it: that matrix's own translation column, bit for bit
                if (b3.w != 0.0f) o[3] = reinterpret_cast<const float4 *>(world + (size_t)__float_as_uint(b3.y) * 16)[3];
                else o[3] = make_float4(tx, ty, tz, 1.0f);
            } else {
                o[3] = make_float4(tx, ty, tz, 1.0f);
            }
        }
    }
}

#pragma clang fp contract(fast)

template <int BLOCK, bool OWN, int CONTACT, bool LSPRING, bool ALIGN>
hipError_t launch(const RzPhysicsParams &p, uint32_t instances, size_t lds, hipStream_t st)
{
    auto k = rz_physics_kernel<BLOCK, OWN, CONTACT, LSPRING, ALIGN>;
    if (hipError_t e = rz_opt_in_lds(k, lds)) return e;
    hipLaunchKernelGGL(k, dim3(instances), dim3(BLOCK), lds, st, p);
    return hipGetLastError();
}

// this unit's half of the launcher table: one instantiation per (LSPRING, block, OWN, CONTACT) with ALIGN = RZ_PHYSICS_ALIGN
hipError_t launch_half(const RzPhysicsParams &p, uint32_t instances, size_t lds, hipStream_t st)
{
    using Launch = hipError_t (*)(const RzPhysicsParams &, uint32_t, size_t, hipStream_t);
#define RZ_PH_ROW(B, O, L) { launch<B, O, 0, L, RZ_PHYSICS_ALIGN>, launch<B, O, 1, L, RZ_PHYSICS_ALIGN>, launch<B, O, 2, L, RZ_PHYSICS_ALIGN>, launch<B, O, 3, L, RZ_PHYSICS_ALIGN> }
    static const Launch table[2][2][2][4] = {
        {{RZ_PH_ROW(64, false, false), RZ_PH_ROW(64, true, false)}, {RZ_PH_ROW(256, false, false), RZ_PH_ROW(256, true, false)}},
        {{RZ_PH_ROW(64, false, true), RZ_PH_ROW(64, true, true)}, {RZ_PH_ROW(256, false, true), RZ_PH_ROW(256, true, true)}}};
#undef RZ_PH_ROW
    return table[p.lin != nullptr][p.block == 256][p.nj <= p.block][p.contacts](p, instances, lds, st);
}

}  // namespace

#if RZ_PHYSICS_ALIGN
// the ALIGN = true half, for rz_launch_physics in the other unit, which has checked p
hipError_t rz_launch_physics_aligned_half(const RzPhysicsParams &p, uint32_t instances, size_t lds, hipStream_t st) { return launch_half(p, instances, lds, st); }
#else
hipError_t rz_launch_physics_aligned_half(const RzPhysicsParams &p, uint32_t instances, size_t lds, hipStream_t st);      // kernels/physics_align.hip

hipError_t rz_launch_physics(const RzPhysicsParams &p, uint32_t instances, hipStream_t st, bool aligned)
{
    if (p.nb <= 0 || instances == 0 || (p.block != 64 && p.block != 256)) return hipErrorInvalidValue;
    const size_t lds = rzphys::lds_bytes(p.nb, p.nj, p.block, p.lin != nullptr);
    if (lds > rzphys::kLdsLimit) return hipErrorInvalidValue;
    if (p.contacts) {
        if (!p.c_shape || !p.c_follow_off || !p.c_follow_idx || !p.c_pair || !p.c_colour_off || p.c_ncol < 0) return hipErrorInvalidValue;
        if (p.contacts == 2 || p.contacts == 3 ? !p.c_box : p.contacts != 1) return hipErrorInvalidValue;
    }
    // aligned: the table has at least one aligned body
    if (aligned && !p.world) return hipErrorInvalidValue;
    return aligned ? rz_launch_physics_aligned_half(p, instances, lds, st) : launch_half(p, instances, lds, st);
}
#endif
