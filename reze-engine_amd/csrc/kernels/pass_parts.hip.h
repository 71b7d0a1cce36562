// kernels/pass_parts.hip.h — what the passes behind the frame kernel (kernels/sdef.hip, kernels/qdef.hip) share: the unit quaternion of
// a palette rotation (quat_of_rows), the batched dense-morph gather (add_dense, kChunk), and, as functions, the morph gather by weight
// source (add_morphs) and the bounding-box epilogue (extend_aabb).
// rz_sdef_kernel calls the first group only and keeps the last two written out in its body, as it was written first: routing them
// through these functions changes how the compiler vectorises and contracts that kernel's arithmetic (measured: its outputs differ in the
// last bit), and its results are held bit-identical to what they were. add_morphs / extend_aabb are those bodies as functions, for
// rz_qdef_kernel and whatever pass comes next.
#pragma once
#include "common.hip.h"

namespace {

struct Quatf { float x, y, z, w; };

// unit quaternion of a rotation given as three matrix rows (Shepperd: branch on the trace, then on the largest diagonal)
__device__ __forceinline__ Quatf quat_of_rows(const float4 r0, const float4 r1, const float4 r2)
{
    const float m00 = r0.x, m01 = r0.y, m02 = r0.z, m10 = r1.x, m11 = r1.y, m12 = r1.z, m20 = r2.x, m21 = r2.y, m22 = r2.z;
    const float tr = m00 + m11 + m22;
    Quatf q;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        q.w = 0.25f * s; q.x = (m21 - m12) / s; q.y = (m02 - m20) / s; q.z = (m10 - m01) / s;
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(1.0f + m00 - m11 - m22) * 2.0f;
        q.w = (m21 - m12) / s; q.x = 0.25f * s; q.y = (m01 + m10) / s; q.z = (m02 + m20) / s;
    } else if (m11 > m22) {
        const float s = sqrtf(1.0f + m11 - m00 - m22) * 2.0f;
        q.w = (m02 - m20) / s; q.x = (m01 + m10) / s; q.y = 0.25f * s; q.z = (m12 + m21) / s;
    } else {
        const float s = sqrtf(1.0f + m22 - m00 - m11) * 2.0f;
        q.w = (m10 - m01) / s; q.x = (m02 + m20) / s; q.y = (m12 + m21) / s; q.z = 0.25f * s;
    }
    const float l = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const float k = l > 0.0f ? 1.0f / l : 0.0f;
    q.x *= k; q.y *= k; q.z *= k; q.w *= k;
    if (l == 0.0f) q.w = 1.0f;
    return q;
}

constexpr int kChunk = 512;        // morph weights compacted into LDS at a time (frames whose active list is not in memory already)

// this frame's deltas of vertex v for an ordered active list (idx[k] + base, w[k]), k < n. A lane's reads are gathers from scattered
// vertices: a batch of them is issued before the first is used (the accumulation keeps ascending morph order), else the pass waits out one
// memory latency per morph. `q24`: the planes are 24-bit integers and the weights carry the morphs' scales (common.hip.h).
__device__ __forceinline__ void add_dense(const uint32_t *idx, const float *w, const int n, const uint32_t base, const float *dense, const size_t Vp,
                                          const uint32_t v, float &x, float &y, float &z, const bool q24 = false)
{
    constexpr int U = 8;
    int k = 0;
    if (q24) {
        const uint32_t *dq = reinterpret_cast<const uint32_t *>(dense);
        const size_t pd = Vp / 4 * 3;                   // dwords per plane
        for (; k + U <= n; k += U) {
            float ww[U], dx[U], dy[U], dz[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ww[u] = w[k + u];
                const uint32_t *d = dq + (size_t)(idx[k + u] + base) * 3 * pd;
                dx[u] = decode24_at(d, v); dy[u] = decode24_at(d + pd, v); dz[u] = decode24_at(d + 2 * pd, v);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { x = fmaf(ww[u], dx[u], x); y = fmaf(ww[u], dy[u], y); z = fmaf(ww[u], dz[u], z); }
        }
        for (; k < n; ++k) {
            const uint32_t *d = dq + (size_t)(idx[k] + base) * 3 * pd;
            x = fmaf(w[k], decode24_at(d, v), x); y = fmaf(w[k], decode24_at(d + pd, v), y); z = fmaf(w[k], decode24_at(d + 2 * pd, v), z);
        }
        return;
    }
    for (; k + U <= n; k += U) {
        float ww[U], dx[U], dy[U], dz[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ww[u] = w[k + u];
            const float *d = dense + (size_t)(idx[k + u] + base) * 3 * Vp + v;
            dx[u] = d[0]; dy[u] = d[Vp]; dz[u] = d[2 * Vp];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { x = fmaf(ww[u], dx[u], x); y = fmaf(ww[u], dy[u], y); z = fmaf(ww[u], dz[u], z); }
    }
    for (; k < n; ++k) {
        const float *d = dense + (size_t)(idx[k] + base) * 3 * Vp + v;
        x = fmaf(w[k], d[0], x); y = fmaf(w[k], d[Vp], y); z = fmaf(w[k], d[2 * Vp], z);
    }
}

// The morphed rest position of vertex v: x / y / z come in as the rest position and leave with this frame's deltas added (ascending morph
// order, zero weights skipped). P is RzSdefParams or RzQdefParams — the same fields under the same names. The dense weights come from
// where the frame left them (wsrc): the kernel-argument list of a one-launch frame, the ring slot's active list rz_prep_kernel wrote, or,
// for a frame without either, the weights themselves, compacted here kChunk at a time through LDS (s_idx / s_w of kChunk entries,
// wave_cnt of kBlock / 64). Workgroup-uniform control flow: every lane of the workgroup calls it, `live` or not.
template <typename P>
__device__ __forceinline__ void add_morphs(const P &p, const RzMorphList &ml, const int inst, const bool live, const uint32_t v, const size_t Vp,
                                           uint32_t *s_idx, float *s_w, int *wave_cnt, float &x, float &y, float &z)
{
    if (p.mode == 1 && p.M > 0) {
        const bool q24 = p.dense_fold != nullptr;
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
}

// bounding box: extend the slot the frame kernel just accumulated into by this wave's box bb[6] (min xyz, max xyz; lanes that are not
// `live` carry +-inf) — same order-preserving keys as the frame kernels, one atomic per wave and component
__device__ __forceinline__ void extend_aabb(uint32_t *aabb, const int inst, const int aabb_slot, float (&bb)[6], const bool live)
{
    const int lane = threadIdx.x & 63;
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
        uint32_t *slot = aabb + ((size_t)inst * 2 + (aabb_slot & 1)) * 6;
        const float sel = lane == 0 ? bb[0] : lane == 1 ? bb[1] : lane == 2 ? bb[2] : lane == 3 ? bb[3] : lane == 4 ? bb[4] : bb[5];
        const uint32_t bits = __float_as_uint(sel);
        const uint32_t key = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
        if (lane < 3) atomicMin(slot + lane, key); else atomicMax(slot + lane, key);
    }
}

}  // namespace
