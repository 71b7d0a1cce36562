// kernels/motion.hip — rz_motion_kernel<P>: the local pose of every instance from a LIBRARY of resident motions (rz_upload_motions), in its
// two instantiations: RzMotionParams (rz_set_pose_blended) and RzLayerParams (rz_upload_motion_masks / rz_set_pose_layered). Instance i is
// posed from a state (clip_a, frame_a, clip_b, frame_b, blend): both clips are sampled with the sampler of kernels/fk.hip.h (bone_issue /
// bone_finish / morph_issue / morph_finish / sample_feeds: the GPU twin of host/vmd-sampler.js) and cross-faded — rotations by Quat.slerp
// (math.ts:156-189), translations and effective morph weights linearly. Then, with RzLayerParams, up to kRzMaxLayers layers are applied in
// order: one clip each, sampled at its own frame, with a weight, an optional bone / morph mask and a mode (override: slerp / lerp towards
// the layer; additive: the forms bone morphs use, q * slerp(identity, qL, weight) and t + tL * weight). A layer acts on a bone only where
// its clip keys the bone and its mask includes it, on a vertex morph only where one of the morph's feeds in that clip holds a key and the
// mask includes it. tests/motion_ref.py and tests/layer_ref.py are the definition in float64. RzMotionParams carries no layers: what is left
// is the cross-fade — the same operations in the same order, so no live layer gives the blended pose bit for bit (tests/test_gpu_layers.py).
// The result is written as a device-resident local pose [weights | rotations | translations] into a pose block; everything behind it (bone
// morphs, the hierarchy solve in all its forms, IK, overrides, the SDEF / QDEF passes) runs on it exactly as on a pose rz_set_pose_local
// copied there. It runs once per pose call, in front of the frame, never inside one: replays read the resident pose.
#include "fk.hip.h"

namespace {

#pragma clang fp contract(off)      // the arithmetic of fk.hip.h's sampler, spelled the same way (tests/motion_ref.py restates it in float64)

// Quat.slerp(a, b, t) (math.ts:156-189) — the form bone_finish ends with: b is negated when the dot product is negative, the normalised
// lerp above 0.9995, the sine form otherwise
__device__ __forceinline__ float4 quat_slerp(const float4 a, float4 b, const float t)
{
    float c = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    if (c < 0.0f) { c = -c; b.x = -b.x; b.y = -b.y; b.z = -b.z; b.w = -b.w; }
    float4 q;
    if (c > 0.9995f) {
        q = make_float4(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z), a.w + t * (b.w - a.w));
        const float il = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        q.x *= il; q.y *= il; q.z *= il; q.w *= il;
    } else {
        const float th0 = acosf(c), sn = sinf(th0), th = th0 * t;
        const float ka = sinf(th0 - th) / sn, kb = sinf(th) / sn;
        q = make_float4(ka * a.x + kb * b.x, ka * a.y + kb * b.y, ka * a.z + kb * b.z, ka * a.w + kb * b.w);
    }
    return q;
}

// bit i of mask `mask` in a table of `words` 32-bit words per mask; kRzNoMask, or no table, includes everything
__device__ __forceinline__ bool mask_has(const uint32_t *bits, int words, uint32_t mask, int i)
{
    if (mask == kRzNoMask || !bits) return true;
    return (bits[(size_t)mask * words + (i >> 5)] >> (i & 31)) & 1u;
}

// of either parameter block: the library, base states and output; and the layers, which RzMotionParams has none of (nothing reads the null)
__host__ __device__ __forceinline__ const RzMotionParams &base_of(const RzMotionParams &p) { return p; }
__host__ __device__ __forceinline__ const RzMotionParams &base_of(const RzLayerParams &p) { return p.m; }
__device__ __forceinline__ const RzLayerParams *layers_of(const RzMotionParams &) { return nullptr; }
__device__ __forceinline__ const RzLayerParams *layers_of(const RzLayerParams &p) { return &p; }

// One workgroup = one instance (blockIdx.x) and one chunk of 256 bones and of 256 vertex morphs (blockIdx.y), no LDS. The state AND the layer
// list are the same for the whole workgroup — read through a uniform address (scalar loads), or from the kernel arguments for one
// character — so every branch on them is workgroup-uniform: blend 0 / 1 or no second clip samples ONE clip and stores what its sampler
// returned, bit for bit, and "is this layer skipped", its mode and "is its weight 1" are uniform too. What differs per lane is two tests:
// the mask's bit and the clip's track record of the lane's bone (a lane the mask leaves out is handed an empty record, which the sampler
// answers without a load). The track records of the base clips and of every live layer are loaded, and all their bone_issue() calls made,
// before the first bone_finish(): the key loads of up to six clips are REQUESTED before any is used. That is the order the source issues
// them in, not an observed overlap — the default bone_issue() loads inside divergent branches, which the compiler ends with a wait
// (fk.hip.h) — and nobody has measured how much of it the hardware overlaps. Stores: one float4 (rotation), three floats (translation),
// one float (weight) per lane.
template <class P> __global__ void __launch_bounds__(kBlock) rz_motion_kernel(const P p)
{
    constexpr int NL = std::is_same<P, RzLayerParams>::value ? kRzMaxLayers : 0;
    constexpr int NA = NL ? NL : 1;     // (no array of no elements)
    const int inst = blockIdx.x;
    const int i = (int)blockIdx.y * kBlock + (int)threadIdx.x;
    const RzMotionParams &m = base_of(p);
    const RzLayerParams *const lp = layers_of(p);
    RzMotionState st = m.state0;
    if (m.states) st = m.states[inst];
    const bool has_b = st.clip_b != kRzNoClip && st.blend != 0.0f;
    const bool only_b = has_b && st.blend == 1.0f;
    const bool both = has_b && !only_b;
    // the clip that is sampled alone (or first), and the one that is blended in
    const uint32_t c0 = only_b ? st.clip_b : st.clip_a, c1 = st.clip_b;
    const float f0 = only_b ? st.frame_b : st.frame_a, f1 = st.frame_b;
    RzMotionLayer ly[NA];
    bool live[NA];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        ly[l] = lp->layers0[l];
        if (lp->layers && l < lp->n_layers) ly[l] = lp->layers[(size_t)inst * lp->n_layers + l];
        live[l] = l < lp->n_layers && ly[l].clip != kRzNoClip && ly[l].weight != 0.0f;
    }
    const RzSampleParams &s = m.sample;
    if (i < m.B) {
        const uint4 r0 = m.bone_rec[(size_t)c0 * m.B + i];
        uint4 rl[NA];
        BoneKeys kl[NA];
        float4 q;
        float tx, ty, tz;
        if constexpr (NL == 0) {
            // Two copies of issue / finish, one per case: the spelling below would do (same operations, 1 200 instructions fewer) and
            // measured 1 % slower on the live loop of one character (NOTEBOOK.md)
            if (both) {
                const uint4 r1 = m.bone_rec[(size_t)c1 * m.B + i];
                BoneKeys k0 = bone_issue(s, f0, r0), k1 = bone_issue(s, f1, r1);
                float4 qb;
                float bx, by, bz;
                bone_finish(s, f0, k0, q, tx, ty, tz);
                bone_finish(s, f1, k1, qb, bx, by, bz);
                q = quat_slerp(q, qb, st.blend);
                tx = tx + (bx - tx) * st.blend; ty = ty + (by - ty) * st.blend; tz = tz + (bz - tz) * st.blend;
            } else {
                BoneKeys k0 = bone_issue(s, f0, r0);
                bone_finish(s, f0, k0, q, tx, ty, tz);
            }
        } else {
            uint4 r1 = make_uint4(0u, 0u, 0u, 0u);           // (first key == end: a track without keys)
            if (both) r1 = m.bone_rec[(size_t)c1 * m.B + i];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                rl[l] = make_uint4(0u, 0u, 0u, 0u);
                if (live[l]) {
                    rl[l] = m.bone_rec[(size_t)ly[l].clip * m.B + i];
                    if (!mask_has(lp->bone_bits, lp->bone_words, ly[l].mask, i)) rl[l].y = rl[l].x;      // left out: end = first key
                }
            }
            BoneKeys k0 = bone_issue(s, f0, r0), k1;
            k1.mode = 0;
            if (both) k1 = bone_issue(s, f1, r1);
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                kl[l].mode = 0;
                if (live[l]) kl[l] = bone_issue(s, ly[l].frame, rl[l]);
            }
            bone_finish(s, f0, k0, q, tx, ty, tz);
            if (both) {
                float4 qb;
                float bx, by, bz;
                bone_finish(s, f1, k1, qb, bx, by, bz);
                q = quat_slerp(q, qb, st.blend);
                tx = tx + (bx - tx) * st.blend; ty = ty + (by - ty) * st.blend; tz = tz + (bz - tz) * st.blend;
            }
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (!live[l]) continue;
            const bool acts = kl[l].mode != 0;          // the clip keys this bone and the mask includes it
            const float wt = ly[l].weight;
            float4 ql;
            float lx, ly_, lz;
            bone_finish(s, ly[l].frame, kl[l], ql, lx, ly_, lz);
            if (!acts) continue;
            if (ly[l].mode != 0u) {
                const float4 r = slerp_from_identity(ql, wt);
                q = make_float4(q.w * r.x + q.x * r.w + q.y * r.z - q.z * r.y,          // Hamilton product q * r (math.ts Quat.multiply)
                                q.w * r.y - q.x * r.z + q.y * r.w + q.z * r.x,
                                q.w * r.z + q.x * r.y - q.y * r.x + q.z * r.w,
                                q.w * r.w - q.x * r.x - q.y * r.y - q.z * r.z);
                tx = tx + lx * wt; ty = ty + ly_ * wt; tz = tz + lz * wt;
            } else if (wt == 1.0f) {
                q = ql; tx = lx; ty = ly_; tz = lz;     // exactly what the sampler returned
            } else {
                q = quat_slerp(q, ql, wt);
                tx = tx + (lx - tx) * wt; ty = ty + (ly_ - ty) * wt; tz = tz + (lz - tz) * wt;
            }
        }
        const size_t o = (size_t)inst * m.B + i;
        m.local_q[o] = q;
        float *t = m.local_t + o * 3;
        t[0] = tx; t[1] = ty; t[2] = tz;
    }
    if (i < m.M) {
        const uint32_t *o0 = m.feed_off + (size_t)c0 * (m.M + 1) + i;
        float w = sample_feeds(s, f0, o0[0], o0[1], 0.0f);
        if (both) {
            const uint32_t *o1 = m.feed_off + (size_t)c1 * (m.M + 1) + i;
            const float wb = sample_feeds(s, f1, o1[0], o1[1], 0.0f);
            w = w + (wb - w) * st.blend;
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (!live[l]) continue;
            // sample_feeds() does not say whether any feed held a key: the same loop, with the flag
            const uint32_t *ol = m.feed_off + (size_t)ly[l].clip * (m.M + 1) + i;
            const uint32_t fa = ol[0], fb = mask_has(lp->morph_bits, lp->morph_words, ly[l].mask, i) ? ol[1] : fa;
            const float wt = ly[l].weight;
            float wl = 0.0f;
            bool driven = false;
            for (uint32_t f = fa; f < fb; ++f) {
                const MorphKeys k = morph_issue(s, ly[l].frame, s.feed_range[f]);
                bool keyed;
                const float wk = morph_finish(s, ly[l].frame, k, keyed);
                if (keyed) { wl += wk * s.feed_ratio[f]; driven = true; }
            }
            if (!driven) continue;
            if (ly[l].mode != 0u) w = w + wl * wt;
            else if (wt == 1.0f) w = wl;
            else w = w + (wl - w) * wt;
        }
        m.morph_w[(size_t)inst * m.M + i] = w;
    }
}

#pragma clang fp contract(fast)

template <class P> hipError_t launch(const P &p, uint32_t instances, hipStream_t st)
{
    const RzMotionParams &m = base_of(p);
    if (m.B <= 0 || instances == 0) return hipErrorInvalidValue;
    const uint32_t chunks = ((uint32_t)std::max(m.B, m.M) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(rz_motion_kernel<P>, dim3(instances, chunks), dim3(kBlock), 0, st, p);
    return hipGetLastError();
}

}  // namespace

hipError_t rz_launch_motion(const RzMotionParams &p, uint32_t instances, hipStream_t st) { return launch(p, instances, st); }
hipError_t rz_launch_motion(const RzLayerParams &p, uint32_t instances, hipStream_t st)
{
    return p.n_layers < 0 || p.n_layers > kRzMaxLayers ? hipErrorInvalidValue : launch(p, instances, st);
}
