// kernels/ik.hip.h — PMX inverse kinematics on the device: the IK stage of rz_fk_kernel (front.hip: the instantiations that receive RzIkParams) between the doubling rounds and the
// override pass of fk_solve. Included by fk.hip.h in front of fk_solve (inside its namespace and under its contraction pragma: every
// FMA is spelled out); tests/ik_ref.py is the definition of what it computes.
//
// CCD, clamp form: per iteration every link of a chain, in file order, is turned about (effector x goal) in its own frame by
// min(atan2(|a x b|, a . b), theta), clamped to its Euler limits ('XYZ'), and the chain's path is re-solved. Shape:
//   * a chain is solved by ONE WAVE with the path (outermost link ... effector, rigid bones between links included, at most 64 bones)
//     one bone per lane: local rotation, local matrix and world rows of a path bone live in its lane's registers for the whole
//     solve. A step broadcasts the link's world rows and the effector's position by v_readlane, every lane forms the same new
//     rotation, and the path below the link is re-solved serially, parent first, one affine product per bone with the parent's
//     rows read from the lane above. LDS is read at the start of a chain and written at its end (the solved link rotations).
//   * chains are grouped into stages at upload (upload.cpp: rz_upload_ik): the chains of a stage read nothing another chain of it
//     writes, so they run on different waves at once (left and right leg; the toe chains follow in the next stage). After each
//     stage the whole skeleton is solved again from the local rotations (ik_resolve: local matrices + doubling rounds), so append
//     children of a link follow and the next stage sees the world matrices all earlier chains left.
//   * every exit (degenerate link, per-step clamp, stall, 1e-4 convergence) is decided on broadcast values: wave-uniform.
// sincosf / atan2f / asinf are the accurate library forms.
#pragma once

__device__ __forceinline__ float ik_lane(const float v, const int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ float4 ik_lane4(const float4 v, const int lane) { return make_float4(ik_lane(v.x, lane), ik_lane(v.y, lane), ik_lane(v.z, lane), ik_lane(v.w, lane)); }

// the local matrix of bone b from the staged pose in LDS (what fk_solve's pass A forms)
__device__ __forceinline__ void ik_local_of(const int b, const float4 *sq, const uint4 *s_rec, const float4 *s_bind, const float *s_lt, const bool has_t,
                                            const float4 q, float4 &l0, float4 &l1, float4 &l2)
{
    const uint4 rec = s_rec[b];
    const float4 bind = s_bind[b];
    const int ap = (int)rec.y;
    const float4 a = ap >= 0 ? sq[ap] : make_float4(0.f, 0.f, 0.f, 1.f);
    float apx = 0.0f, apy = 0.0f, apz = 0.0f, ltx = 0.0f, lty = 0.0f, ltz = 0.0f;
    if (has_t) {
        ltx = s_lt[b * 3]; lty = s_lt[b * 3 + 1]; ltz = s_lt[b * 3 + 2];
        if (ap >= 0 && (rec.w & 1u)) { apx = s_lt[ap * 3]; apy = s_lt[ap * 3 + 1]; apz = s_lt[ap * 3 + 2]; }
    }
    fk_local_matrix(q, rec, bind.x, bind.y, bind.z, has_t, ltx, lty, ltz, a, apx, apy, apz, l0, l1, l2);
}

// One chain, one wave (all 64 lanes arrive; `c` is wave-uniform). `src` = every bone's world rows after the last whole-skeleton solve.
__device__ __forceinline__ void ik_solve_chain(const RzIkParams &ik, const uint32_t c, const float4 *src, float4 *sq, const uint4 *s_rec,
                                               const float4 *s_bind, const float *s_lt, const bool has_t, const int lane)
{
    const uint4 r0 = ik.chain[2 * c], r1 = ik.chain[2 * c + 1];
    const int G = (int)r0.x, P = (int)r0.z, par = (int)r0.w;
    const uint32_t loops = r1.x, loff = r1.z, nl = r1.w;
    const float theta = __uint_as_float(r1.y);
    if (loops == 0u || nl == 0u || P <= 0 || P > 64) return;
    const uint32_t pe = ik.path[r0.y + (uint32_t)min(lane, P - 1)];
    const int b = (int)(pe & 0x7fffffffu);
    float4 q = sq[b];
    float4 w0 = src[b * 3], w1 = src[b * 3 + 1], w2 = src[b * 3 + 2];
    float4 l0, l1, l2;
    ik_local_of(b, sq, s_rec, s_bind, s_lt, has_t, q, l0, l1, l2);
    float4 pw0 = make_float4(1.f, 0.f, 0.f, 0.f), pw1 = make_float4(0.f, 1.f, 0.f, 0.f), pw2 = make_float4(0.f, 0.f, 1.f, 0.f);
    if (par >= 0) { pw0 = src[par * 3]; pw1 = src[par * 3 + 1]; pw2 = src[par * 3 + 2]; }
    const float gx = src[G * 3].w, gy = src[G * 3 + 1].w, gz = src[G * 3 + 2].w;
    for (uint32_t it = 0; it < loops; ++it) {
        bool rotated = false;
        for (uint32_t k = 0; k < nl; ++k) {
            const float4 lmin = ik.link[2 * (loff + k)], lmax = ik.link[2 * (loff + k) + 1];
            const int j = (int)__float_as_uint(lmin.w);
            const bool limited = __float_as_uint(lmax.w) != 0u;
            const float4 a0 = ik_lane4(w0, j), a1 = ik_lane4(w1, j), a2 = ik_lane4(w2, j);      // the link's world rows
            const float ex = ik_lane(w0.w, P - 1) - a0.w, ey = ik_lane(w1.w, P - 1) - a1.w, ez = ik_lane(w2.w, P - 1) - a2.w;
            const float hx = gx - a0.w, hy = gy - a1.w, hz = gz - a2.w;
            // a = Rw^T * (effector - link), b = Rw^T * (goal - link)
            float ax = fmaf(a2.x, ez, fmaf(a1.x, ey, a0.x * ex)), ay = fmaf(a2.y, ez, fmaf(a1.y, ey, a0.y * ex)), az = fmaf(a2.z, ez, fmaf(a1.z, ey, a0.z * ex));
            float bx = fmaf(a2.x, hz, fmaf(a1.x, hy, a0.x * hx)), by = fmaf(a2.y, hz, fmaf(a1.y, hy, a0.y * hx)), bz = fmaf(a2.z, hz, fmaf(a1.z, hy, a0.z * hx));
            const float la = sqrtf(fmaf(az, az, fmaf(ay, ay, ax * ax))), lb = sqrtf(fmaf(bz, bz, fmaf(by, by, bx * bx)));
            if (__builtin_amdgcn_readfirstlane((la < 1e-6f || lb < 1e-6f) ? 1 : 0)) continue;
            ax /= la; ay /= la; az /= la; bx /= lb; by /= lb; bz /= lb;
            const float cx = fmaf(ay, bz, -(az * by)), cy = fmaf(az, bx, -(ax * bz)), cz = fmaf(ax, by, -(ay * bx));
            const float n = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
            if (__builtin_amdgcn_readfirstlane(n < 1e-7f ? 1 : 0)) continue;
            const float ang = fminf(atan2f(n, fmaf(az, bz, fmaf(ay, by, ax * bx))), theta);
            float sn, cs;
            sincosf(0.5f * ang, &sn, &cs);
            const float s = sn / n;
            const float4 r = make_float4(cx * s, cy * s, cz * s, cs);
            const float4 o = ik_lane4(q, j);
            float4 t = make_float4(o.w * r.x + o.x * r.w + o.y * r.z - o.z * r.y,          // Hamilton product o * r (math.ts Quat.multiply)
                                   o.w * r.y - o.x * r.z + o.y * r.w + o.z * r.x,
                                   o.w * r.z + o.x * r.y - o.y * r.x + o.z * r.w,
                                   o.w * r.w - o.x * r.x - o.y * r.y - o.z * r.z);
            if (limited) {
                // three.js 'XYZ': R = Rx * Ry * Rz
                float R[9];
                quat_to_rows(t.x, t.y, t.z, t.w, R);
                float e1 = asinf(fminf(1.0f, fmaxf(-1.0f, R[2]))), e0, e2;
                if (fabsf(R[2]) < 0.9999999f) { e0 = atan2f(-R[5], R[8]); e2 = atan2f(-R[1], R[0]); }
                else { e0 = atan2f(R[7], R[4]); e2 = 0.0f; }
                const float lo0 = fminf(lmin.x, lmax.x), hi0 = fmaxf(lmin.x, lmax.x), lo1 = fminf(lmin.y, lmax.y), hi1 = fmaxf(lmin.y, lmax.y);
                const float lo2 = fminf(lmin.z, lmax.z), hi2 = fmaxf(lmin.z, lmax.z);
                e0 = fminf(fmaxf(e0, lo0), hi0); e1 = fminf(fmaxf(e1, lo1), hi1); e2 = fminf(fmaxf(e2, lo2), hi2);
                float s1, c1, s2, c2, s3, c3;
                sincosf(0.5f * e0, &s1, &c1); sincosf(0.5f * e1, &s2, &c2); sincosf(0.5f * e2, &s3, &c3);
                t = make_float4(s1 * c2 * c3 + c1 * s2 * s3, c1 * s2 * c3 - s1 * c2 * s3, c1 * c2 * s3 + s1 * s2 * c3, c1 * c2 * c3 - s1 * s2 * s3);
            }
            const float il = 1.0f / sqrtf(t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w);
            t.x *= il; t.y *= il; t.z *= il; t.w *= il;
            rotated = true;
            if (lane == j) {
                q = t;
                ik_local_of(b, sq, s_rec, s_bind, s_lt, has_t, q, l0, l1, l2);
            }
            // the path from the link down, parent first: W_i = W_(i-1) * L_i
            for (int i = j; i < P; ++i) {
                float4 p0 = pw0, p1 = pw1, p2 = pw2;
                if (i > 0) { p0 = ik_lane4(w0, i - 1); p1 = ik_lane4(w1, i - 1); p2 = ik_lane4(w2, i - 1); }
                float4 n0, n1, n2;
                affine_mul(p0, p1, p2, l0, l1, l2, n0, n1, n2);
                if (lane == i) { w0 = n0; w1 = n1; w2 = n2; }
            }
        }
        const float dx = gx - ik_lane(w0.w, P - 1), dy = gy - ik_lane(w1.w, P - 1), dz = gz - ik_lane(w2.w, P - 1);
        const bool close = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) < 1e-4f;
        if (__builtin_amdgcn_readfirstlane((close || !rotated) ? 1 : 0)) break;
    }
    if (lane < P && (pe >> 31)) sq[b] = q;          // the solved local rotations of the links: what the next whole-skeleton solve reads
}

// The whole skeleton again from the staged local pose: local matrices into `wl`, then the doubling rounds between `wl` and `m2` (the IK
// instantiation's own second buffer: region X stays alive). Every bone through LDS; ends with a barrier. Returns the buffer that holds
// the world rows.
__device__ __forceinline__ float4 *ik_resolve(const RzFkParams &p, float4 *wl, float4 *m2, const float4 *sq, const uint4 *s_rec, const float4 *s_bind,
                                              const float *s_lt, const bool has_t, const int tid)
{
    for (int b = tid; b < p.B; b += kBlock) {
        float4 l0, l1, l2;
        ik_local_of(b, sq, s_rec, s_bind, s_lt, has_t, sq[b], l0, l1, l2);
        wl[b * 3] = l0; wl[b * 3 + 1] = l1; wl[b * 3 + 2] = l2;
    }
    __syncthreads();
    float4 *src = wl, *dst = m2;
    for (int r = 0; r < p.n_rounds; ++r) {
        for (int b = tid; b < p.B; b += kBlock) {
            uint32_t lo, hi;
            if (r < 2) { const uint4 w3 = p.bone_rec[4 * b + 3]; lo = r == 0 ? w3.x : w3.z; hi = r == 0 ? w3.y : w3.w; }
            else { const uint2 am = p.anc_more[(size_t)(r - 2) * p.B + b]; lo = am.x; hi = am.y; }
            float4 w0 = src[b * 3], w1 = src[b * 3 + 1], w2 = src[b * 3 + 2];
            fk_round(src, lo & 0xffffu, lo >> 16, hi & 0xffffu, w0, w1, w2);
            dst[b * 3] = w0; dst[b * 3 + 1] = w1; dst[b * 3 + 2] = w2;
        }
        __syncthreads();
        float4 *t4 = src; src = dst; dst = t4;
    }
    return src;
}

// Word `i` of an instance's chain switches (RzIkSwitchParams): wave-uniform, so a scalar load or a select between kernel arguments
__device__ __forceinline__ uint32_t ik_sw_word(const RzIkSwitchParams &sw, const int inst, const uint32_t i)
{
    if (sw.mask) return sw.mask[(size_t)inst * (size_t)sw.words + i];
    return i == 0u ? sw.w0[0] : i == 1u ? sw.w0[1] : i == 2u ? sw.w0[2] : sw.w0[3];
}

// is any chain of [c0, c1) switched on?
__device__ __forceinline__ bool ik_sw_any(const RzIkSwitchParams &sw, const int inst, const uint32_t c0, const uint32_t c1)
{
    if (c0 >= c1) return false;
    const uint32_t wa = c0 >> 5, wb = (c1 - 1u) >> 5;
    for (uint32_t i = wa; i <= wb; ++i) {
        uint32_t m = ik_sw_word(sw, inst, i);
        if (i == wa) m &= 0xffffffffu << (c0 & 31u);
        if (i == wb) m &= 0xffffffffu >> (31u - ((c1 - 1u) & 31u));
        if (m) return true;
    }
    return false;
}

// The IK stage of one pose (its workgroup): `src` holds the world rows of the plain solve; returns the buffer with the solved ones.
// SW (the instantiations that receive RzIkSwitchParams; tests/ik_switch_ref.py): the instance's chain switches. A wave skips a chain whose bit is clear (its
// links keep the staged rotations, as a chain with no loops does); a stage none of whose chains is on changes no rotation, so its
// whole-skeleton solve is skipped as well and `src` stays what the last live stage left; an instance with every bit clear does not enter
// the loop. The bits are read through wave-uniform addresses and the two stage-level decisions depend on the instance alone: every
// barrier is reached by the whole workgroup or by none of it.
template <bool SW = false>
__device__ __forceinline__ float4 *ik_stage(const RzFkParams &p, const RzIkParams &ik, float4 *src, float4 *wl, float4 *m2, float4 *sq, const uint4 *s_rec,
                                            const float4 *s_bind, const float *s_lt, const bool has_t, const int tid, const RzIkSwitchParams *sw = nullptr,
                                            const int inst = 0)
{
    const int lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    if constexpr (SW) {
        if (!ik_sw_any(*sw, inst, 0u, (uint32_t)ik.n_chains)) return src;
    }
    for (int s = 0; s < ik.n_stages; ++s) {
        const uint32_t c1 = ik.stage_off[s + 1];
        if constexpr (SW) {
            if (!ik_sw_any(*sw, inst, ik.stage_off[s], c1)) continue;
        }
        for (uint32_t c = ik.stage_off[s] + wave; c < c1; c += kBlock / 64) {
            if constexpr (SW) {
                if (!((ik_sw_word(*sw, inst, c >> 5) >> (c & 31u)) & 1u)) continue;
            }
            ik_solve_chain(ik, c, src, sq, s_rec, s_bind, s_lt, has_t, lane);
        }
        __syncthreads();            // every chain of the stage has left its rotations; nobody reads `src` any more
        src = ik_resolve(p, wl, m2, sq, s_rec, s_bind, s_lt, has_t, tid);
    }
    return src;
}
