// kernels/qdef.hip — QDEF skinning (PMX 2.1 weight type 4, dual-quaternion blending) of the vertices a context lists with rz_upload_qdef.
// Like the SDEF pass (kernels/sdef.hip) a pass of its own, launched on the frame's stream behind the deform / skin kernel: it re-skins
// only the listed vertices and overwrites what the frame kernel stored for them (their BDEF4 result). The frame kernels are not touched.
//
// For one listed vertex:
//   j0..j3 = the four joint slots (clamped to B - 1); w_i = u8_i / isum as the LBS path decodes them (common.hip.h skin_vertex;
//   isum == 0 gives (1, 0, 0, 0)); slots of weight zero contribute nothing.
//   p~ = the morphed rest position (this frame's weights, ascending morph order, zero weights skipped — what the SDEF pass forms), n = the rest normal
// Per bone j:
//   S_j = palette rows (world x inverseBind, 3 x 4); q_j = the unit quaternion of its upper 3 x 3 (Shepperd, quat_of_rows); t_j = its
//   fourth column; d_j = 1/2 (t_j, 0) (x) q_j:  d.xyz = 1/2 (q.w t + t x q.xyz),  d.w = -1/2 t . q.xyz.
//   (A palette that is not rigid loses its non-rigid part here: scale and shear do not survive the quaternion. PMX poses are rigid.)
// Blend (Kavan et al., dual-quaternion linear blending):
//   pivot = the slot with the largest u8 weight, the lowest slot on ties; s_i = -1 if dot(q_pivot, q_ji) < 0 else +1
//   b_r = sum_i w_i s_i q_ji, b_d = sum_i w_i s_i d_ji (slots ascending); n_b = |b_r| (>= w_pivot >= 1/4); c_r = b_r / n_b, c_d = b_d / n_b
//   P' = R(c_r) p~ + 2 (c_r.w c_d.xyz - c_d.w c_r.xyz + c_r.xyz x c_d.xyz);  N' = normalize(R(c_r) n) (zero or non-finite: the rest normal)
//   hull = P' + N' edge 0.01
// The float64 restatement the tests hold this to is tests/qdef_ref.py.
//
// CONVERSION IS PER BONE, NOT PER INFLUENCE: a workgroup first forms (q_j, d_j) of all B bones of its instance from the palette in memory
// into dynamic LDS (two float4 per bone), B / 256 conversions per lane, and every lane then gathers its four bones with ds_read_b128.
// Converting per lane would run Shepperd's branches, square roots and divides four times per (vertex, instance).
#include "pass_parts.hip.h"

namespace {

// everything of one table entry that does not depend on the pose: issued before the staging loop so that it arrives under it
struct QdefVertex {
    uint32_t v, j01, j23, wq;
    float x, y, z, nx, ny, nz;
};

__device__ __forceinline__ QdefVertex load_vertex(const RzQdefParams &p, const uint32_t t)
{
    QdefVertex o;
    o.v = t < p.n ? p.tab[t] : 0u;                  // (lanes past the table read vertex 0 and store nothing)
    const size_t Vp = p.Vp;
    o.x = p.geom[o.v]; o.y = p.geom[Vp + o.v]; o.z = p.geom[2 * Vp + o.v];
    o.nx = p.geom[3 * Vp + o.v]; o.ny = p.geom[4 * Vp + o.v]; o.nz = p.geom[5 * Vp + o.v];
    o.j01 = p.joints01[o.v]; o.j23 = p.joints23[o.v]; o.wq = p.weights[o.v];
    return o;
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }

// grid.x x p.chunks x kBlock covers the table, grid.y = instance. Dynamic LDS: float4 dq[B][2] = (q_j, d_j).
__global__ void __launch_bounds__(kBlock) rz_qdef_kernel(const RzQdefParams p, const RzMorphList ml)
{
    extern __shared__ float4 dq[];
    __shared__ uint32_t s_idx[kChunk];
    __shared__ float s_w[kChunk];
    __shared__ int wave_cnt[kBlock / 64];
    const int inst = blockIdx.y, tid = threadIdx.x;
    const size_t Vp = p.Vp;
    uint32_t t = blockIdx.x * (uint32_t)p.chunks * kBlock + tid;
    QdefVertex o = load_vertex(p, t);

    // stage: bone -> dual quaternion
    const float4 *pal = p.palette + (size_t)inst * p.B * 3;
    for (int b = tid; b < p.B; b += kBlock) {
        const float4 r0 = pal[b * 3], r1 = pal[b * 3 + 1], r2 = pal[b * 3 + 2];
        const Quatf q = quat_of_rows(r0, r1, r2);
        const float tx = r0.w, ty = r1.w, tz = r2.w;
        float4 d;
        d.x = 0.5f * fmaf(q.w, tx, fmaf(ty, q.z, -(tz * q.y)));
        d.y = 0.5f * fmaf(q.w, ty, fmaf(tz, q.x, -(tx * q.z)));
        d.z = 0.5f * fmaf(q.w, tz, fmaf(tx, q.y, -(ty * q.x)));
        d.w = -0.5f * fmaf(tz, q.z, fmaf(ty, q.y, tx * q.x));
        dq[b * 2] = make_float4(q.x, q.y, q.z, q.w);
        dq[b * 2 + 1] = d;
    }

    float bb[6] = { __builtin_inff(), __builtin_inff(), __builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
    bool any_live = false;
    for (int c = 0;;) {                                // (workgroup-uniform: add_morphs may synchronise the workgroup)
        const bool live = t < p.n;
        any_live |= live;
        float x = o.x, y = o.y, z = o.z;
        add_morphs(p, ml, inst, live, o.v, Vp, s_idx, s_w, wave_cnt, x, y, z);
        if (c == 0) __syncthreads();                   // the dual quaternions are staged
        if (live) {
            const uint32_t u[4] = { o.wq & 255u, (o.wq >> 8) & 255u, (o.wq >> 16) & 255u, o.wq >> 24 };
            const uint32_t isum = u[0] + u[1] + u[2] + u[3];
            const bool ok = isum != 0u;
            const float inv = __builtin_amdgcn_rcpf((float)(ok ? isum : 1u));
            const float w[4] = { ok ? (float)u[0] * inv : 1.0f, (float)u[1] * inv, (float)u[2] * inv, (float)u[3] * inv };
            const uint32_t bmax = (uint32_t)p.B - 1u;
            const uint32_t j[4] = { min(o.j01 & 0xffffu, bmax), min(o.j01 >> 16, bmax), min(o.j23 & 0xffffu, bmax), min(o.j23 >> 16, bmax) };
            float4 q[4], d[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { q[i] = dq[j[i] * 2]; d[i] = dq[j[i] * 2 + 1]; }
            // pivot: largest u8 weight, lowest slot on ties (integer comparison)
            float4 qp = q[0];
            uint32_t um = u[0];
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if (u[i] > um) { um = u[i]; qp = q[i]; }
            float4 br = make_float4(0.f, 0.f, 0.f, 0.f), bd = br;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = dot4(qp, q[i]) < 0.0f ? -w[i] : w[i];
                if (w[i] != 0.0f) {
                    br.x = fmaf(s, q[i].x, br.x); br.y = fmaf(s, q[i].y, br.y); br.z = fmaf(s, q[i].z, br.z); br.w = fmaf(s, q[i].w, br.w);
                    bd.x = fmaf(s, d[i].x, bd.x); bd.y = fmaf(s, d[i].y, bd.y); bd.z = fmaf(s, d[i].z, bd.z); bd.w = fmaf(s, d[i].w, bd.w);
                }
            }
            const float rn = 1.0f / sqrtf(dot4(br, br));
            const float qx = br.x * rn, qy = br.y * rn, qz = br.z * rn, qw = br.w * rn;
            const float dx = bd.x * rn, dy = bd.y * rn, dz = bd.z * rn, dw = bd.w * rn;
            // R = mat3(c_r), rows
            const float xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
            const float wx = qw * qx, wy = qw * qy, wz = qw * qz;
            const float r00 = 1.0f - 2.0f * (yy + zz), r01 = 2.0f * (xy - wz), r02 = 2.0f * (xz + wy);
            const float r10 = 2.0f * (xy + wz), r11 = 1.0f - 2.0f * (xx + zz), r12 = 2.0f * (yz - wx);
            const float r20 = 2.0f * (xz - wy), r21 = 2.0f * (yz + wx), r22 = 1.0f - 2.0f * (xx + yy);
            const float tx = 2.0f * fmaf(qw, dx, fmaf(-dw, qx, fmaf(qy, dz, -(qz * dy))));
            const float ty = 2.0f * fmaf(qw, dy, fmaf(-dw, qy, fmaf(qz, dx, -(qx * dz))));
            const float tz = 2.0f * fmaf(qw, dz, fmaf(-dw, qz, fmaf(qx, dy, -(qy * dx))));
            const float px = fmaf(r02, z, fmaf(r01, y, fmaf(r00, x, tx)));
            const float py = fmaf(r12, z, fmaf(r11, y, fmaf(r10, x, ty)));
            const float pz = fmaf(r22, z, fmaf(r21, y, fmaf(r20, x, tz)));
            const float ax = fmaf(r02, o.nz, fmaf(r01, o.ny, r00 * o.nx));
            const float ay = fmaf(r12, o.nz, fmaf(r11, o.ny, r10 * o.nx));
            const float az = fmaf(r22, o.nz, fmaf(r21, o.ny, r20 * o.nx));
            const float l2 = fmaf(az, az, fmaf(ay, ay, ax * ax));
            const bool good = (l2 > 0.0f) && (l2 < __builtin_inff());
            const float rl = good ? 1.0f / sqrtf(l2) : 1.0f;
            const float ox = good ? ax * rl : o.nx, oy = good ? ay * rl : o.ny, oz = good ? az * rl : o.nz;

            const size_t at = ((size_t)inst * Vp + o.v) * 3;
            p.out_pos[at] = px; p.out_pos[at + 1] = py; p.out_pos[at + 2] = pz;
            p.out_nrm[at] = ox; p.out_nrm[at + 1] = oy; p.out_nrm[at + 2] = oz;
            if (p.edge) {
                const float e = p.edge[o.v];
                p.out_hull[at] = px + (ox * e) * 0.01f; p.out_hull[at + 1] = py + (oy * e) * 0.01f; p.out_hull[at + 2] = pz + (oz * e) * 0.01f;
            }
            bb[0] = fminf(bb[0], px); bb[1] = fminf(bb[1], py); bb[2] = fminf(bb[2], pz);
            bb[3] = fmaxf(bb[3], px); bb[4] = fmaxf(bb[4], py); bb[5] = fmaxf(bb[5], pz);
        }
        if (++c >= p.chunks) break;
        t += kBlock;
        if (t - tid >= p.n) break;                     // (the workgroup's next chunk starts past the table)
        o = load_vertex(p, t);
    }

    if (p.aabb) extend_aabb(p.aabb, inst, p.aabb_slot, bb, any_live);
}

}  // namespace

hipError_t rz_launch_qdef(const RzQdefParams &p, const RzMorphList &ml, uint32_t instances, hipStream_t st)
{
    if (p.n == 0 || instances == 0) return hipSuccess;
    if (p.chunks < 1 || p.B < 1) return hipErrorInvalidValue;
    const size_t lds = rzlds::qdef(p.B).total();
    if (hipError_t e = rz_opt_in_lds(rz_qdef_kernel, lds)) return e;
    const uint32_t per = (uint32_t)p.chunks * kBlock;
    hipLaunchKernelGGL(rz_qdef_kernel, dim3((p.n + per - 1) / per, instances), dim3(kBlock), lds, st, p, ml);
    return hipGetLastError();
}
