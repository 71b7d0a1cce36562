// kernels/sdef.hip — SDEF skinning (PMX weight type 3, "spherical deformation") of the vertices a context lists with rz_upload_sdef.
// A pass of its own, launched on the frame's stream right behind the deform / skin kernel: it re-skins only the listed vertices and
// overwrites what the frame kernel stored for them (which is their BDEF2 result). The frame kernels are not touched: SDEF vertices are a
// small, clustered minority of a mesh, and a branch for them in the dense one-launch kernels would cost every vertex registers.
//
// For one SDEF vertex (saba's PMXModel / MMD, without the z flip — the project keeps PMX coordinates):
//   j0, j1 = joint slots 0 / 1 (clamped to B - 1, as the LBS path does); w0, w1 = their unorm8 weights normalised over slots 0 and 1 only
//   (a sum <= 1e-4 gives w0 = 1, w1 = 0); slots 2 and 3 are ignored.
//   p~ = the morphed rest position (the morph deltas of this frame's weights, ascending morph order over the non-zero weights), n = the rest normal
//   S0, S1 = palette rows of j0, j1 (world x inverseBind, 3 x 4); Q0, Q1 = unit quaternions of their upper 3 x 3 (Shepperd's method)
//   Q1 = -Q1 when dot(Q0, Q1) < 0; Q = slerp(Q0, Q1, w1) (normalised lerp above cos 0.9995, math.ts Quat.slerp); R = mat3(Q)
//   rw = w0 R0 + w1 R1; cr0 = (C + (C + R0 - rw)) / 2; cr1 = (C + (C + R1 - rw)) / 2
//   P' = R (p~ - C) + w0 S0 (cr0, 1) + w1 S1 (cr1, 1);   N' = normalize(R n) (a zero-length result keeps the rest normal)
// The float64 restatement the tests hold this to is tests/sdef_ref.py.
#include "pass_parts.hip.h"

namespace {

// math.ts slerpInto, with the hemisphere already chosen by the caller
__device__ __forceinline__ Quatf slerp_q(const Quatf a, const Quatf b, const float t)
{
    const float c = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    Quatf o;
    if (c > 0.9995f) {
        o.x = a.x + t * (b.x - a.x); o.y = a.y + t * (b.y - a.y); o.z = a.z + t * (b.z - a.z); o.w = a.w + t * (b.w - a.w);
        const float k = 1.0f / sqrtf(o.x * o.x + o.y * o.y + o.z * o.z + o.w * o.w);
        o.x *= k; o.y *= k; o.z *= k; o.w *= k;
        return o;
    }
    const float th0 = acosf(fminf(c, 1.0f));
    const float s = sinf(th0);
    const float ka = sinf(th0 - th0 * t) / s, kb = sinf(th0 * t) / s;
    o.x = ka * a.x + kb * b.x; o.y = ka * a.y + kb * b.y; o.z = ka * a.z + kb * b.z; o.w = ka * a.w + kb * b.w;
    return o;
}

__device__ __forceinline__ float3 affine(const float4 r0, const float4 r1, const float4 r2, const float x, const float y, const float z)
{
    return make_float3(fmaf(r0.z, z, fmaf(r0.y, y, fmaf(r0.x, x, r0.w))), fmaf(r1.z, z, fmaf(r1.y, y, fmaf(r1.x, x, r1.w))),
                       fmaf(r2.z, z, fmaf(r2.y, y, fmaf(r2.x, x, r2.w))));
}

// One lane per (SDEF vertex, instance): grid.x covers the table, grid.y = instance. The dense morph weights come from where the frame left
// them (RzSdefParams::wsrc): the kernel-argument list of a one-launch frame, the ring slot's active list rz_prep_kernel wrote, or, for a
// frame without either, the weights themselves, compacted here kChunk at a time through LDS.
__global__ void __launch_bounds__(kBlock) rz_sdef_kernel(const RzSdefParams p, const RzMorphList ml)
{
    __shared__ uint32_t s_idx[kChunk];
    __shared__ float s_w[kChunk];
    __shared__ int wave_cnt[kBlock / 64];
    const int inst = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const uint32_t t = blockIdx.x * kBlock + tid;
    const bool live = t < p.n;
    const uint32_t v = live ? p.tab[t] : 0u;         // (lanes past the table read vertex 0 and store nothing)
    const size_t Vp = p.Vp;
    float x = p.geom[v], y = p.geom[Vp + v], z = p.geom[2 * Vp + v];

    if (p.mode == 1 && p.M > 0) {
        const bool q24 = p.dense_fold != nullptr;       // 24-bit planes: the listed weights carry the morphs' scales (common.hip.h)
        if (p.wsrc == 0) {
            if (live) add_dense(ml.idx, ml.w, ml.count, 0u, p.dense, Vp, v, x, y, z, q24);
        } else if (p.wsrc == 1) {
            if (live) add_dense(p.act_idx + (size_t)inst * p.Mpad, p.act_w + (size_t)inst * p.Mpad, p.act_count[inst], 0u, p.dense, Vp, v, x, y, z, q24);
        } else {
            const float *mw = p.morph_w + (size_t)inst * p.M;
            for (int m0 = 0; m0 < p.M; m0 += kChunk) {          // (workgroup-uniform: compact_active synchronises the workgroup)
                const int cnt = compact_active(mw + m0, min(kChunk, p.M - m0), kChunk, s_idx, s_w, wave_cnt, p.dense_fold, m0);
                if (live) add_dense(s_idx, s_w, cnt, (uint32_t)m0, p.dense, Vp, v, x, y, z, q24);
                __syncthreads();
            }
        }
    } else if (p.mode == 2 && p.M > 0 && live) {
        const float *mw = p.morph_w + (size_t)inst * p.M;
        constexpr uint32_t U = 4;
        for (uint32_t e = p.sp_ptr[v], e1 = p.sp_ptr[v + 1]; e < e1; e += U) {
            float4 d[U];
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) d[u] = e + u < e1 ? p.sp_entries[e + u] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const float w = e + u < e1 ? mw[__float_as_uint(d[u].w)] : 0.0f;
                if (w != 0.0f) { x = fmaf(w, d[u].x, x); y = fmaf(w, d[u].y, y); z = fmaf(w, d[u].z, z); }
            }
        }
    }

    float bb[6] = { __builtin_inff(), __builtin_inff(), __builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
    if (live) {
        const uint32_t n = p.n;
        const float *tf = reinterpret_cast<const float *>(p.tab);
        const float cx = tf[n + t], cy = tf[2 * n + t], cz = tf[3 * n + t];
        const float r0x = tf[4 * n + t], r0y = tf[5 * n + t], r0z = tf[6 * n + t];
        const float r1x = tf[7 * n + t], r1y = tf[8 * n + t], r1z = tf[9 * n + t];
        const float nx = p.geom[3 * Vp + v], ny = p.geom[4 * Vp + v], nz = p.geom[5 * Vp + v];
        const uint32_t j01 = p.joints01[v], wq = p.weights[v];
        const uint32_t bmax = (uint32_t)p.B - 1u;
        const uint32_t j0 = min(j01 & 0xffffu, bmax), j1 = min(j01 >> 16, bmax);
        const float a0 = (float)(wq & 255u) / 255.0f, a1 = (float)((wq >> 8) & 255u) / 255.0f;
        const float s = a0 + a1;
        const float w0 = s > 1e-4f ? a0 / s : 1.0f, w1 = s > 1e-4f ? a1 / s : 0.0f;

        const float4 *pal = p.palette + (size_t)inst * p.B * 3;
        const float4 s00 = pal[j0 * 3], s01 = pal[j0 * 3 + 1], s02 = pal[j0 * 3 + 2];
        const float4 s10 = pal[j1 * 3], s11 = pal[j1 * 3 + 1], s12 = pal[j1 * 3 + 2];
        const Quatf q0 = quat_of_rows(s00, s01, s02);
        Quatf q1 = quat_of_rows(s10, s11, s12);
        if (q0.x * q1.x + q0.y * q1.y + q0.z * q1.z + q0.w * q1.w < 0.0f) { q1.x = -q1.x; q1.y = -q1.y; q1.z = -q1.z; q1.w = -q1.w; }
        const Quatf q = slerp_q(q0, q1, w1);
        // R = mat3(q), rows
        const float xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z;
        const float wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
        const float4 R0 = make_float4(1.0f - 2.0f * (yy + zz), 2.0f * (xy - wz), 2.0f * (xz + wy), 0.0f);
        const float4 R1 = make_float4(2.0f * (xy + wz), 1.0f - 2.0f * (xx + zz), 2.0f * (yz - wx), 0.0f);
        const float4 R2 = make_float4(2.0f * (xz - wy), 2.0f * (yz + wx), 1.0f - 2.0f * (xx + yy), 0.0f);

        const float rwx = w0 * r0x + w1 * r1x, rwy = w0 * r0y + w1 * r1y, rwz = w0 * r0z + w1 * r1z;
        const float c0x = (cx + (cx + r0x - rwx)) * 0.5f, c0y = (cy + (cy + r0y - rwy)) * 0.5f, c0z = (cz + (cz + r0z - rwz)) * 0.5f;
        const float c1x = (cx + (cx + r1x - rwx)) * 0.5f, c1y = (cy + (cy + r1y - rwy)) * 0.5f, c1z = (cz + (cz + r1z - rwz)) * 0.5f;
        const float3 rp = affine(R0, R1, R2, x - cx, y - cy, z - cz);
        const float3 t0 = affine(s00, s01, s02, c0x, c0y, c0z), t1 = affine(s10, s11, s12, c1x, c1y, c1z);
        const float px = rp.x + w0 * t0.x + w1 * t1.x, py = rp.y + w0 * t0.y + w1 * t1.y, pz = rp.z + w0 * t0.z + w1 * t1.z;
        const float3 tn = affine(R0, R1, R2, nx, ny, nz);
        const float l2 = fmaf(tn.z, tn.z, fmaf(tn.y, tn.y, tn.x * tn.x));
        const bool good = (l2 > 0.0f) && (l2 < __builtin_inff());
        const float rl = good ? 1.0f / sqrtf(l2) : 1.0f;
        const float ox = good ? tn.x * rl : nx, oy = good ? tn.y * rl : ny, oz = good ? tn.z * rl : nz;

        const size_t o = ((size_t)inst * Vp + v) * 3;
        p.out_pos[o] = px; p.out_pos[o + 1] = py; p.out_pos[o + 2] = pz;
        p.out_nrm[o] = ox; p.out_nrm[o + 1] = oy; p.out_nrm[o + 2] = oz;
        if (p.edge) {
            const float e = p.edge[v];
            p.out_hull[o] = px + (ox * e) * 0.01f; p.out_hull[o + 1] = py + (oy * e) * 0.01f; p.out_hull[o + 2] = pz + (oz * e) * 0.01f;
        }
        bb[0] = px; bb[1] = py; bb[2] = pz; bb[3] = px; bb[4] = py; bb[5] = pz;
    }

    // bounding box: extend the slot the frame kernel just accumulated into (same order-preserving keys; one atomic per wave and component)
    if (p.aabb) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bb[k] = fminf(bb[k], __shfl_xor(bb[k], off));
                bb[3 + k] = fmaxf(bb[3 + k], __shfl_xor(bb[3 + k], off));
            }
        }
        const bool any = __ballot(live) != 0ull;
        if (any && lane < 6) {
            uint32_t *slot = p.aabb + ((size_t)inst * 2 + (p.aabb_slot & 1)) * 6;
            const float sel = lane == 0 ? bb[0] : lane == 1 ? bb[1] : lane == 2 ? bb[2] : lane == 3 ? bb[3] : lane == 4 ? bb[4] : bb[5];
            const uint32_t bits = __float_as_uint(sel);
            const uint32_t key = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
            if (lane < 3) atomicMin(slot + lane, key); else atomicMax(slot + lane, key);
        }
    }
}

}  // namespace

hipError_t rz_launch_sdef(const RzSdefParams &p, const RzMorphList &ml, uint32_t instances, hipStream_t st)
{
    if (p.n == 0 || instances == 0) return hipSuccess;
    hipLaunchKernelGGL(rz_sdef_kernel, dim3((p.n + kBlock - 1) / kBlock, instances), dim3(kBlock), 0, st, p, ml);
    return hipGetLastError();
}
