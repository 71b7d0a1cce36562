// kernels/motion.hip — rz_motion_blend_kernel: the local pose of every instance from a LIBRARY of resident motions (rz_upload_motions /
// rz_set_pose_blended). Instance i is posed from a state (clip_a, frame_a, clip_b, frame_b, blend): both clips are sampled with the
// sampler of kernels/fk.hip.h (bone_issue / bone_finish / morph_issue / morph_finish / sample_feeds: the GPU twin of host/vmd-sampler.js)
// and cross-faded — rotations by Quat.slerp (math.ts:156-189), translations and effective morph weights linearly. The result is written
// as a device-resident local pose [weights | rotations | translations] into a pose block; everything behind it (bone morphs, the
// hierarchy solve in all its forms, IK, overrides, the SDEF / QDEF passes) runs on it exactly as on a pose rz_set_pose_local copied
// there. It runs once per pose call, in front of the frame, never inside one: replays read the resident pose.
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

// One workgroup = one instance (blockIdx.x) and one chunk of 256 bones and of 256 vertex morphs (blockIdx.y). The state is the same for the
// whole workgroup: it is read through a uniform address (scalar loads) or rides in the kernel arguments (one character), and every
// branch on it is workgroup-uniform — blend 0 / 1 or no second clip samples ONE clip and stores what its sampler returned, bit for bit.
// With two clips both records are loaded and both bone_issue() calls go before either bone_finish(): the key loads of both clips are
// REQUESTED before either is used. That is the order the source issues them in, not an observed overlap — the default bone_issue() loads
// inside divergent branches, which the compiler ends with a wait (fk.hip.h) — and nobody has measured how much of it the hardware
// overlaps. Stores: one float4 (rotation), three floats (translation), one float (weight) per lane; no LDS.
__global__ void __launch_bounds__(kBlock) rz_motion_blend_kernel(const RzMotionParams p)
{
    const int inst = blockIdx.x;
    const int i = (int)blockIdx.y * kBlock + (int)threadIdx.x;
    RzMotionState st = p.state0;
    if (p.states) st = p.states[inst];
    const bool has_b = st.clip_b != kRzNoClip && st.blend != 0.0f;
    const bool only_b = has_b && st.blend == 1.0f;
    const bool both = has_b && !only_b;
    // the clip that is sampled alone (or first), and the one that is blended in
    const uint32_t c0 = only_b ? st.clip_b : st.clip_a, c1 = st.clip_b;
    const float f0 = only_b ? st.frame_b : st.frame_a, f1 = st.frame_b;
    const RzSampleParams &s = p.sample;
    if (i < p.B) {
        const uint4 r0 = p.bone_rec[(size_t)c0 * p.B + i];
        float4 q;
        float tx, ty, tz;
        if (both) {
            const uint4 r1 = p.bone_rec[(size_t)c1 * p.B + i];
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
        const size_t o = (size_t)inst * p.B + i;
        p.local_q[o] = q;
        float *t = p.local_t + o * 3;
        t[0] = tx; t[1] = ty; t[2] = tz;
    }
    if (i < p.M) {
        const uint32_t *o0 = p.feed_off + (size_t)c0 * (p.M + 1) + i;
        float w = sample_feeds(s, f0, o0[0], o0[1], 0.0f);
        if (both) {
            const uint32_t *o1 = p.feed_off + (size_t)c1 * (p.M + 1) + i;
            const float wb = sample_feeds(s, f1, o1[0], o1[1], 0.0f);
            w = w + (wb - w) * st.blend;
        }
        p.morph_w[(size_t)inst * p.M + i] = w;
    }
}

#pragma clang fp contract(fast)

}  // namespace

hipError_t rz_launch_motion_blend(const RzMotionParams &p, uint32_t instances, hipStream_t st)
{
    if (p.B <= 0 || instances == 0) return hipErrorInvalidValue;
    const uint32_t chunks = ((uint32_t)std::max(p.B, p.M) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(rz_motion_blend_kernel, dim3(instances, chunks), dim3(kBlock), 0, st, p);
    return hipGetLastError();
}
