// kernels/after.hip — rz_fk_after_kernel: PMX after-physics bones (rz_upload_after_physics; defined by tests/after_ref.py). The listed bones
// are evaluated AGAIN behind the override write, on the world matrices F the hierarchy solve of this frame left in memory (hierarchy, bone
// morphs, IK, followers, overrides), so that a helper bone sees where the physics-driven bone it copies really is. Per listed bone b, in
// list order, unless b is overridden itself:
//   P = F[parent(b)] (identity for a root)
//   with an append parent a: its local transform AS FINALLY POSED, R_a = rot(F[parent(a)])^T rot(F[a]),
//   t_a = rot(F[parent(a)])^T (pos(F[a]) - pos(F[parent(a)])) - bind_a (a root a: F[a] itself), q_a = quat(R_a) by the branch on the largest
//   of trace, m00, m11, m22, normalised; then fk_local_matrix as the first solve runs it, on q_b, t_b (the local pose after bone morphs), q_a, t_a
//   F[b] = P * L; later entries read the new F[b].
// A kernel of its own behind whichever hierarchy kernel ran, launched only while the list and a non-empty override table are resident: the
// fk_solve template, its entry points and RzFkParams are untouched. One workgroup of kBlock threads per instance.
//   phase 1  the instance's world rows into LDS as 3 x float4 per bone (the output pass's layout; one coalesced 64-byte read per bone), and in
//            the same round trip a thread's first two entries: static record, the listed bone's inverse bind matrix and its local pose —
//            the resident local pose, or, for rz_set_pose_sampled, its keys (bone_issue / bone_finish from the bone's key record) — with
//            the bone morphs folded as the solve folds them, from the weights the hierarchy kernel left in memory
//   phase 2  lanes walk the instance's override entries and set the skip byte of after_index[bone]
//   phase 3  level by level out of LDS only: entries of a level are independent (after_table.h), lanes stride over them, each writes its row
//            back into F; one barrier per level. Rows are 48 B apart and entries ascend by bone inside a level: the follow stage's pattern.
//   phase 4  the listed, non-skipped bones write their world matrix and palette rows
// Lists of more than 2 x kBlock entries: the entries beyond a thread's two register slots are fetched where they are used (the solve treats
// skeletons beyond 512 bones the same way); up to 512 entries no global load sits inside the level loop.
#include "fk.hip.h"

namespace {

#pragma clang fp contract(off)

struct AfterEntry {
    uint4 r0, r1, r2;           // RzAfterParams::rec
    float4 q;                   // local pose of the bone after bone morphs
    float tx, ty, tz;
    float4 i0, i1, i2, i3;      // its inverse bind matrix
};

// q = quat(R), R row-major: the branch on the largest of trace, m00, m11, m22, then normalised (tests/after_ref.py: quat_of)
__device__ __forceinline__ float4 after_quat(const float (&m)[9])
{
    const float tr = m[0] + m[4] + m[8];
    float x, y, z, w;
    if (tr >= m[0] && tr >= m[4] && tr >= m[8]) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        w = 0.25f * s; x = (m[7] - m[5]) / s; y = (m[2] - m[6]) / s; z = (m[3] - m[1]) / s;
    } else if (m[0] >= m[4] && m[0] >= m[8]) {
        const float s = sqrtf(1.0f + m[0] - m[4] - m[8]) * 2.0f;
        w = (m[7] - m[5]) / s; x = 0.25f * s; y = (m[1] + m[3]) / s; z = (m[2] + m[6]) / s;
    } else if (m[4] >= m[8]) {
        const float s = sqrtf(1.0f + m[4] - m[0] - m[8]) * 2.0f;
        w = (m[2] - m[6]) / s; x = (m[1] + m[3]) / s; y = 0.25f * s; z = (m[5] + m[7]) / s;
    } else {
        const float s = sqrtf(1.0f + m[8] - m[0] - m[4]) * 2.0f;
        w = (m[3] - m[1]) / s; x = (m[2] + m[6]) / s; y = (m[5] + m[7]) / s; z = 0.25f * s;
    }
    const float il = 1.0f / sqrtf(x * x + y * y + z * z + w * w);
    return make_float4(x * il, y * il, z * il, w * il);
}

__global__ void __launch_bounds__(kBlock) rz_fk_after_kernel(const RzFkParams p, const RzAfterParams a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *F = reinterpret_cast<float4 *>(smem);                       // [B][3] world rows 0..2
    unsigned char *skip = smem + rzlds::after(p.B, a.n).skip_off;                     // [n] 1 = the entry's bone is overridden in this instance
    const int tid = threadIdx.x, inst = blockIdx.x;
    const float4 *lq = p.local_q + (size_t)inst * p.B;
    const float *glt = p.local_t ? p.local_t + (size_t)inst * p.B * 3 : nullptr;
    const bool sampled = p.sample.frames != nullptr || p.sample.frames_inline;
    const float frame = sampled ? (p.sample.frames_inline ? p.sample.frame0 : p.sample.frames[inst]) : 0.0f;
    // the morph weights of this pose where the hierarchy kernel left (sampled) or read (uploaded) them
    const float *mw = p.bm_off ? (sampled ? p.sample.morph_w + (size_t)inst * p.sample.M : p.bm_w + (size_t)inst * p.bm_M) : nullptr;
    float *world = p.world + (size_t)inst * p.B * 16;
    float4 *pal = p.palette + (size_t)inst * p.B * 3;

    auto fetch_static = [&](const int k, AfterEntry &e) {
        const uint4 *r = a.rec + (size_t)k * 3;
        e.r0 = r[0]; e.r1 = r[1]; e.r2 = r[2];
    };
    auto fetch_ib = [&](AfterEntry &e) {
        const float4 *Im = reinterpret_cast<const float4 *>(p.inv_bind + (size_t)e.r1.w * 16);
        e.i0 = Im[0]; e.i1 = Im[1]; e.i2 = Im[2]; e.i3 = Im[3];
    };
    auto uploaded = [&](AfterEntry &e) {
        const int b = (int)e.r1.w;
        e.q = lq[b];
        e.tx = e.ty = e.tz = 0.0f;
        if (glt) { e.tx = glt[b * 3]; e.ty = glt[b * 3 + 1]; e.tz = glt[b * 3 + 2]; }
    };
    // PMX bone morphs on the local pose: the solve's arithmetic (kernels/fk.hip.h), entries ascending by morph
    auto fold_morphs = [&](AfterEntry &e) {
        if (!mw) return;
        const int b = (int)e.r1.w;
        const uint32_t e0 = p.bm_off[b], e1 = p.bm_off[b + 1];
        float4 q = e.q;
        for (uint32_t i = e0; i < e1; ++i) {
            const float w = mw[p.bm_morph[i]];
            if (w == 0.0f) continue;
            const float4 t4 = p.bm_tr[i];
            e.tx += w * t4.x; e.ty += w * t4.y; e.tz += w * t4.z;
            const float4 r = slerp_from_identity(p.bm_rot[i], w);
            q = make_float4(q.w * r.x + q.x * r.w + q.y * r.z - q.z * r.y,
                            q.w * r.y - q.x * r.z + q.y * r.w + q.z * r.x,
                            q.w * r.z + q.x * r.y - q.y * r.x + q.z * r.w,
                            q.w * r.w - q.x * r.x - q.y * r.y - q.z * r.z);
        }
        e.q = q;
    };
    auto fetch = [&](const int k, AfterEntry &e) {             // everything of one entry (the entries beyond the register slots)
        fetch_static(k, e);
        fetch_ib(e);
        if (sampled) {
            BoneKeys bk = bone_issue(p.sample, frame, p.bone_rec[4 * (size_t)e.r1.w + 2]);
            bone_finish(p.sample, frame, bk, e.q, e.tx, e.ty, e.tz);
        } else uploaded(e);
        fold_morphs(e);
    };

    // ---- phase 1: F into LDS; the two register slots' records, inverse bind matrices and local poses in the same round trip ----
    constexpr int NS = 2;
    AfterEntry ent[NS];
    const bool h0 = tid < a.n, h1 = tid + kBlock < a.n;
    fetch_static(h0 ? tid : 0, ent[0]);
    fetch_static(h1 ? tid + kBlock : 0, ent[1]);
    for (int k = tid; k < a.n; k += kBlock) skip[k] = 0;
    for (int b = tid; b < p.B; b += kBlock) {
        const float4 *Wm = reinterpret_cast<const float4 *>(world + (size_t)b * 16);
        const float4 c0 = Wm[0], c1 = Wm[1], c2 = Wm[2], c3 = Wm[3];
        F[b * 3] = make_float4(c0.x, c1.x, c2.x, c3.x);
        F[b * 3 + 1] = make_float4(c0.y, c1.y, c2.y, c3.y);
        F[b * 3 + 2] = make_float4(c0.z, c1.z, c2.z, c3.z);
    }
    fetch_ib(ent[0]);
    fetch_ib(ent[1]);
    if (sampled) {
        BoneKeys k0 = bone_issue(p.sample, frame, h0 ? p.bone_rec[4 * (size_t)ent[0].r1.w + 2] : make_uint4(0, 0, 0, 0));
        BoneKeys k1 = bone_issue(p.sample, frame, h1 ? p.bone_rec[4 * (size_t)ent[1].r1.w + 2] : make_uint4(0, 0, 0, 0));
        bone_finish(p.sample, frame, k0, ent[0].q, ent[0].tx, ent[0].ty, ent[0].tz);
        bone_finish(p.sample, frame, k1, ent[1].q, ent[1].tx, ent[1].ty, ent[1].tz);
    } else {
        uploaded(ent[0]);
        uploaded(ent[1]);
    }
    if (h0) fold_morphs(ent[0]);
    if (h1) fold_morphs(ent[1]);
    __syncthreads();
    // ---- phase 2: the instance's overridden bones are never evaluated again ----
    for (int k = p.ovr_off[inst] + tid; k < p.ovr_off[inst + 1]; k += kBlock) {
        const int i = a.index[p.ovr_bone[k]];
        if (i >= 0) skip[i] = 1;
    }
    __syncthreads();
    // ---- phase 3: level by level ----
    auto evaluate = [&](const AfterEntry &e, float4 &w0, float4 &w1, float4 &w2) {
        const int b = (int)e.r1.w, par = (int)e.r0.x, ap = (int)e.r0.y, app = (int)e.r2.w;
        float4 qa = make_float4(0.f, 0.f, 0.f, 1.f);
        float ax = 0.0f, ay = 0.0f, az = 0.0f;
        if (ap >= 0) {
            const float4 a0 = F[ap * 3], a1 = F[ap * 3 + 1], a2 = F[ap * 3 + 2];
            float R[9];
            if (app >= 0) {
                const float4 g0 = F[app * 3], g1 = F[app * 3 + 1], g2 = F[app * 3 + 2];
                const float dx = a0.w - g0.w, dy = a1.w - g1.w, dz = a2.w - g2.w;
                // R_a = R_g^T R, t_a = R_g^T (p - p_g)
                R[0] = fmaf(g2.x, a2.x, fmaf(g1.x, a1.x, g0.x * a0.x)); R[1] = fmaf(g2.x, a2.y, fmaf(g1.x, a1.y, g0.x * a0.y)); R[2] = fmaf(g2.x, a2.z, fmaf(g1.x, a1.z, g0.x * a0.z));
                R[3] = fmaf(g2.y, a2.x, fmaf(g1.y, a1.x, g0.y * a0.x)); R[4] = fmaf(g2.y, a2.y, fmaf(g1.y, a1.y, g0.y * a0.y)); R[5] = fmaf(g2.y, a2.z, fmaf(g1.y, a1.z, g0.y * a0.z));
                R[6] = fmaf(g2.z, a2.x, fmaf(g1.z, a1.x, g0.z * a0.x)); R[7] = fmaf(g2.z, a2.y, fmaf(g1.z, a1.y, g0.z * a0.y)); R[8] = fmaf(g2.z, a2.z, fmaf(g1.z, a1.z, g0.z * a0.z));
                ax = fmaf(g2.x, dz, fmaf(g1.x, dy, g0.x * dx));
                ay = fmaf(g2.y, dz, fmaf(g1.y, dy, g0.y * dx));
                az = fmaf(g2.z, dz, fmaf(g1.z, dy, g0.z * dx));
            } else {
                R[0] = a0.x; R[1] = a0.y; R[2] = a0.z; R[3] = a1.x; R[4] = a1.y; R[5] = a1.z; R[6] = a2.x; R[7] = a2.y; R[8] = a2.z;
                ax = a0.w; ay = a1.w; az = a2.w;
            }
            ax -= __uint_as_float(e.r2.x); ay -= __uint_as_float(e.r2.y); az -= __uint_as_float(e.r2.z);
            qa = after_quat(R);
        }
        float4 l0, l1, l2;
        fk_local_matrix(e.q, e.r0, __uint_as_float(e.r1.x), __uint_as_float(e.r1.y), __uint_as_float(e.r1.z), true, e.tx, e.ty, e.tz, qa, ax, ay, az, l0, l1, l2);
        if (par >= 0) affine_mul(F[par * 3], F[par * 3 + 1], F[par * 3 + 2], l0, l1, l2, w0, w1, w2);
        else { w0 = l0; w1 = l1; w2 = l2; }
        F[b * 3] = w0; F[b * 3 + 1] = w1; F[b * 3 + 2] = w2;
    };
    for (int l = 0; l < a.n_levels; ++l) {
        // entry k belongs to thread k mod kBlock (its register slots hold entries tid and tid + kBlock): consecutive lanes, consecutive entries
        const int k0 = a.level_off[l], k1 = a.level_off[l + 1];
        for (int k = k0 + ((tid - k0) & (kBlock - 1)); k < k1; k += kBlock) {
            if (skip[k]) continue;
            float4 w0, w1, w2;
            AfterEntry e;
            if (k < kBlock) e = ent[0];
            else if (k < NS * kBlock) e = ent[1];
            else fetch(k, e);
            evaluate(e, w0, w1, w2);
        }
        __syncthreads();
    }
    // ---- phase 4: world matrices and palette rows of the listed, non-skipped bones ----
    auto emit = [&](const int b, const float4 i0, const float4 i1, const float4 i2, const float4 i3) {
        const float4 w0 = F[b * 3], w1 = F[b * 3 + 1], w2 = F[b * 3 + 2];
        float4 *wo = reinterpret_cast<float4 *>(world + (size_t)b * 16);
        wo[0] = make_float4(w0.x, w1.x, w2.x, 0.0f);
        wo[1] = make_float4(w0.y, w1.y, w2.y, 0.0f);
        wo[2] = make_float4(w0.z, w1.z, w2.z, 0.0f);
        wo[3] = make_float4(w0.w, w1.w, w2.w, 1.0f);
        float4 q0, q1, q2;
        fk_palette_rows(w0, w1, w2, i0, i1, i2, i3, q0, q1, q2);
        pal[b * 3] = q0; pal[b * 3 + 1] = q1; pal[b * 3 + 2] = q2;
    };
    if (h0 && !skip[tid]) emit((int)ent[0].r1.w, ent[0].i0, ent[0].i1, ent[0].i2, ent[0].i3);
    if (h1 && !skip[tid + kBlock]) emit((int)ent[1].r1.w, ent[1].i0, ent[1].i1, ent[1].i2, ent[1].i3);
    for (int k = tid + NS * kBlock; k < a.n; k += kBlock) {
        if (skip[k]) continue;
        const int b = (int)a.rec[(size_t)k * 3 + 1].w;
        const float4 *Im = reinterpret_cast<const float4 *>(p.inv_bind + (size_t)b * 16);
        emit(b, Im[0], Im[1], Im[2], Im[3]);
    }
}

#pragma clang fp contract(fast)

}  // namespace

hipError_t rz_launch_fk_after(const RzFkParams &p, const RzAfterParams &a, uint32_t instances, hipStream_t st)
{
    const size_t lds = rzlds::after(p.B, a.n).total();
    // (the host checks the LDS first and says why: launch_fk in frame.cpp; the stage walks the override table and reads the solve's output)
    if (lds > rzlds::kCuLds || !a.rec || !a.level_off || !a.index || a.n <= 0 || a.n_levels <= 0 || !p.ovr_off || !p.world || !p.palette) return hipErrorInvalidValue;
    if (hipError_t e = rz_opt_in_lds(rz_fk_after_kernel, lds)) return e;
    hipLaunchKernelGGL(rz_fk_after_kernel, dim3(instances), dim3(kBlock), lds, st, p, a);
    return hipGetLastError();
}
