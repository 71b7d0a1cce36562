// upload.cpp — static data of a context: mesh shard, skeleton, topology, morph targets, bone morphs, motion, edge scale (ctx.h).
#include "ctx.h"

using namespace rzi;

namespace rzi {

// The device block behind fk_rec: the bone records with the CURRENT motion's tracks filled in, then the motion's vertex-morph records.
// Called when either side changes (the caller has drained the stream); a context without a topology has no block.
int rebuild_fk_static(rz_ctx *c)
{
    if (!c->fk.has_topology || c->fk.host.size() != (size_t)c->skel.B * 4) return RZ_OK;
    const bool motion = c->has_animation && c->an_host_range.size() == c->skel.B;
    const size_t nm = motion ? c->an_host_mrec.size() / 2 : 0;
    std::vector<uint4> blk(c->fk.host);
    blk.resize((size_t)c->skel.B * 4 + nm * 2);
    for (uint32_t b = 0; b < c->skel.B; ++b) blk[4 * (size_t)b + 2] = motion ? c->an_host_range[b] : make_uint4(0u, 0u, 0u, 0u);
    for (size_t k = 0; k < nm * 2; ++k) blk[(size_t)c->skel.B * 4 + k] = c->an_host_mrec[k];
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    c->fk.rec = {};
    c->fk_gen++;                        // (the closure records of crowd frames carry copies of these: plan.cpp ensure_subfk)
    if (int r = to_device(c->fk.rec, blk.data(), blk.size())) { c->fk = {}; return r; }      // (no block, no topology: nothing solves on the device until the next one)
    return RZ_OK;
}

}  // namespace rzi

namespace {

int upload_skinning(rz_ctx *c, uint32_t V, const uint16_t *joints4, const uint8_t *weights4)
{
    Scratch<uint16_t> dj;
    Scratch<uint8_t> dw;
    HIP_TRY(dj.alloc((size_t)V * 4));
    HIP_TRY(dw.alloc((size_t)V * 4));
    HIP_TRY(hipMemcpy(dj.p, joints4, (size_t)V * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dw.p, weights4, (size_t)V * 4, hipMemcpyHostToDevice));
    HIP_TRY(rz_launch_pack_skinning(dj.p, dw.p, V, c->mesh.j01, c->mesh.j23, c->mesh.wq, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RZ_OK;
}

int alloc_mesh(rz_ctx *c, uint32_t V)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_direct_gather(c);                // shard sizes are about to change: back to private output buffers
    c->mesh = {}; c->edge = {};
    c->rj01 = {}; c->rj23 = {}; c->sub_valid = false;      // the run lists name this mesh's joints
    free_morphs(c);                       // morph targets are per-vertex: a new mesh invalidates them
    free_sdef(c);                         // ... and so does the SDEF table: its indices name the old mesh's vertices
    free_qdef(c);                         // ... and the QDEF table
    RzStatic::Mesh m;                     // (takes its place whole: a failure leaves no vertex count over a missing plane)
    m.V = V;
    m.Vp = round_up(V, kVertPad);
    const size_t Vp = m.Vp;
    HIP_TRY(m.geom.alloc(6 * Vp));
    HIP_TRY(m.j01.alloc(Vp));
    HIP_TRY(m.j23.alloc(Vp));
    HIP_TRY(m.wq.alloc(Vp));
    c->mesh = std::move(m);
    // padding vertices: zero position/normal, joint 0, weights 0 (takes the (1,0,0,0) branch)
    HIP_TRY(hipMemsetAsync(c->mesh.geom, 0, 6 * Vp * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->mesh.j01, 0, Vp * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->mesh.j23, 0, Vp * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->mesh.wq, 0, Vp * 4, c->stream));
    return RZ_OK;
}

}  // namespace

extern "C" {

int rz_shard_range(uint32_t v_total, int nranks, int rank, uint32_t *begin, uint32_t *count)
{
    if (nranks < 1 || rank < 0 || rank >= nranks || !begin || !count)
        return fail(RZ_ERR_INVALID, "bad shard query (nranks=%d rank=%d)", nranks, rank);
    const uint64_t per = ((uint64_t)v_total + nranks - 1) / nranks;
    const uint64_t chunk = (per + kShardGrain - 1) / kShardGrain * kShardGrain;
    uint64_t b = std::min<uint64_t>(v_total, chunk * (uint64_t)rank);
    uint64_t n = std::min<uint64_t>(chunk, v_total - b);
    *begin = (uint32_t)b;
    *count = (uint32_t)n;
    return RZ_OK;
}

int rz_gather_chunk(uint32_t v_total, int nranks, uint32_t *chunk)
{
    if (!chunk) return fail(RZ_ERR_INVALID, "null chunk");
    uint32_t b0 = 0, n0 = 0;
    if (int r = rz_shard_range(v_total, nranks, 0, &b0, &n0)) return r;
    const uint64_t ch = ((uint64_t)n0 + kShardGrain - 1) / kShardGrain * kShardGrain;
    if (ch > 0xffffffffull) return fail(RZ_ERR_INVALID, "a shard of %u vertices rounds up past 2^32: no gathered buffer for this mesh", n0);
    *chunk = (uint32_t)ch;
    return RZ_OK;
}

int rz_instance_range(uint32_t instances, int nranks, int rank, uint32_t *begin, uint32_t *count)
{
    if (nranks < 1 || rank < 0 || rank >= nranks || !begin || !count)
        return fail(RZ_ERR_INVALID, "bad instance-shard query (nranks=%d rank=%d)", nranks, rank);
    const uint64_t per = ((uint64_t)instances + nranks - 1) / nranks;
    const uint64_t b = std::min<uint64_t>(instances, per * (uint64_t)rank);
    *begin = (uint32_t)b;
    *count = (uint32_t)std::min<uint64_t>(per, instances - b);
    return RZ_OK;
}

int rz_upload_mesh(rz_ctx *c, uint32_t V, const float *interleaved8, const uint16_t *joints4, const uint8_t *weights4)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_mesh")) return r;
    if (V == 0 || !interleaved8 || !joints4 || !weights4) return fail(RZ_ERR_INVALID, "rz_upload_mesh: empty mesh or null array");
    if (int r = alloc_mesh(c, V)) return r;
    Scratch<float> scratch;
    HIP_TRY(scratch.alloc((size_t)V * 8));
    float *tmp = scratch.p;
    HIP_TRY(hipMemcpy(tmp, interleaved8, (size_t)V * 8 * sizeof(float), hipMemcpyHostToDevice));
    const size_t Vp = c->mesh.Vp;
    HIP_TRY(rz_launch_deinterleave(tmp, 8, 0, V, c->mesh.geom, c->mesh.geom + Vp, c->mesh.geom + 2 * Vp, c->stream));
    HIP_TRY(rz_launch_deinterleave(tmp, 8, 3, V, c->mesh.geom + 3 * Vp, c->mesh.geom + 4 * Vp, c->mesh.geom + 5 * Vp, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int r = upload_skinning(c, V, joints4, weights4)) return r;
    return ensure_outputs(c);
}

int rz_upload_mesh_soa(rz_ctx *c, uint32_t V, const float *pos3, const float *nrm3, const uint16_t *joints4,
                       const uint8_t *weights4)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_mesh_soa")) return r;
    if (V == 0 || !pos3 || !nrm3 || !joints4 || !weights4) return fail(RZ_ERR_INVALID, "rz_upload_mesh_soa: empty mesh or null array");
    if (int r = alloc_mesh(c, V)) return r;
    Scratch<float> scratch;
    HIP_TRY(scratch.alloc((size_t)V * 3));
    float *tmp = scratch.p;
    const size_t Vp = c->mesh.Vp;
    HIP_TRY(hipMemcpy(tmp, pos3, (size_t)V * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rz_launch_deinterleave(tmp, 3, 0, V, c->mesh.geom, c->mesh.geom + Vp, c->mesh.geom + 2 * Vp, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(tmp, nrm3, (size_t)V * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rz_launch_deinterleave(tmp, 3, 0, V, c->mesh.geom + 3 * Vp, c->mesh.geom + 4 * Vp, c->mesh.geom + 5 * Vp, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int r = upload_skinning(c, V, joints4, weights4)) return r;
    return ensure_outputs(c);
}

int rz_upload_skeleton(rz_ctx *c, uint32_t B, const float *inverse_bind16)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_skeleton")) return r;
    if (B == 0 || !inverse_bind16) return fail(RZ_ERR_INVALID, "rz_upload_skeleton: model has no bones");
    if ((size_t)B * 48 + rzlds::kSkeletonReserve > rzlds::kCuLds) return fail(RZ_ERR_UNSUPPORTED, "more than %d bones do not fit the LDS palette", (int)((rzlds::kCuLds - rzlds::kSkeletonReserve) / 48));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    c->ovr_count = 0;
    c->ovr_follow = 0; c->fol_count = 0;        // rz_override_follow goes with the hierarchy it was set for
    c->skel = {};
    if (int r = to_device(c->skel.inv_bind, inverse_bind16, (size_t)B * 16)) { c->skel = {}; return r; }
    c->skel.B = B;
    retire_pose_tags(c);                // a pose staged for the old skeleton must never match
    c->sub_valid = false;               // joints are clamped to the bone count when the run lists are built
    c->palette_stale = false;
    c->pl.cur.set = false;
    c->fk = {}; c->fk_gen++;            // the topology belongs to the previous skeleton, and so do its records (sized for the old bone count: nothing may read them for the new one)
    c->fk_stale = false; c->subfk_valid = false;
    free_bone_morphs(c);                // ... as do bone morphs (their entries name its bones)
    free_ik(c);                         // ... and the IK table (its chains name its bones)
    free_after(c);                      // ... and the after-physics list (it names its bones)
    free_physics(c);                    // ... and the physics table (its bodies name its bones)
    free_animation(c);                  // ... and so does an uploaded motion (its tracks name bones of that skeleton)
    free_motions(c);                    // ... and the motion library
    free_motion_masks(c);               // ... and the masks of layered poses (one bit per bone of that skeleton)
    return ensure_pose_buffers(c);
}

// ---- 24-bit dense morph storage: the encoder (kernels/common.hip.h reads what it writes; DESIGN.md "Dense morph storage") ----
// Per morph: E = the binary exponent of its largest finite |delta| over the three planes, s = 2^(E - 22), q = rint(d / s); a maximum
// that rounds to 2^23 takes E + 1. An all-zero morph gets s = 1. |q * s - d| <= s / 2 = 2^(E - 23), about max|d| * 2^-23.
// The whole SET stays fp32 (returns false) when a delta is not finite or an exponent leaves [-64, 64], which keeps weight * scale away
// from underflow and overflow.
static bool morph_scales24(uint32_t M, uint32_t V, const float *deltas, float *scales)
{
    for (uint32_t m = 0; m < M; ++m) {
        const uint32_t *bits = reinterpret_cast<const uint32_t *>(deltas + (size_t)m * V * 3);
        uint32_t top = 0;
        for (size_t i = 0, n = (size_t)V * 3; i < n; ++i) top = std::max(top, bits[i] & 0x7fffffffu);
        if (top >= 0x7f800000u) return false;                   // Inf / NaN
        if (top == 0) { scales[m] = 1.0f; continue; }
        float mx;
        memcpy(&mx, &top, 4);
        int e;
        (void)frexpf(mx, &e);                                   // mx = f * 2^e, 0.5 <= f < 1: the binary exponent is e - 1
        int E = e - 1;
        if (E < -126 || lrintf(ldexpf(mx, 22 - E)) >= (1 << 23)) E += 1;
        if (E < -64 || E > 64) return false;
        scales[m] = ldexpf(1.0f, E - 22);
    }
    return true;
}

// one plane (component `comp` of one morph's [V][3] deltas) as 12-byte quads; dst holds ceil(V / 4) * 12 bytes, the last quad zero-padded
static void encode_plane24(const float *d3, uint32_t V, int comp, float inv_scale, uint32_t *dst)
{
    for (uint32_t v0 = 0; v0 < V; v0 += 4) {
        uint32_t q[4] = { 0u, 0u, 0u, 0u };
        for (uint32_t k = 0; k < 4 && v0 + k < V; ++k) q[k] = (uint32_t)(int32_t)lrintf(d3[(size_t)(v0 + k) * 3 + comp] * inv_scale) & 0xffffffu;
        uint32_t *o = dst + (size_t)(v0 / 4) * 3;
        o[0] = q[0] | q[1] << 24;
        o[1] = q[1] >> 8 | q[2] << 16;
        o[2] = q[2] >> 16 | q[3] << 8;
    }
}

int rz_morph_encode24(const float *deltas, uint32_t M, uint32_t V, uint8_t *packed, float *scales, int *storage)
{
    if (!deltas || !scales || !storage || M == 0 || V == 0) return fail(RZ_ERR_INVALID, "rz_morph_encode24: null array or empty set");
    *storage = 32;
    if (!morph_scales24(M, V, deltas, scales)) return RZ_OK;
    *storage = 24;
    if (!packed) return RZ_OK;
    const size_t plane = (size_t)(V + 3) / 4 * 12;
    for (uint32_t m = 0; m < M; ++m)
        for (int comp = 0; comp < 3; ++comp)
            encode_plane24(deltas + (size_t)m * V * 3, V, comp, 1.0f / scales[m], reinterpret_cast<uint32_t *>(packed + ((size_t)m * 3 + comp) * plane));
    return RZ_OK;
}

// the two forms of a dense set, built into `t` (a local of the upload: it takes the context's place only when it is whole)
static int upload_dense_f32(rz_ctx *c, RzStatic::Morphs &t, uint32_t M, const float *deltas)
{
    const size_t Vp = c->mesh.Vp, V = c->mesh.V;
    size_t dense_off = 0;
#ifdef RZ_ALL_VARIANTS
    // tools-only build: place the morph planes `RZ_DENSE_OFFSET` bytes into a larger allocation (tools/archive/placement.py: how much of the C5
    // frame's box-to-box spread is WHERE the 768 MB land). The owner keeps the allocation's base; frames read the shifted pointer.
    if (const char *e = getenv("RZ_DENSE_OFFSET")) dense_off = (size_t)strtoull(e, nullptr, 0) / 256 * 256;
#endif
    HIP_TRY(t.dense_base.alloc((size_t)M * 3 * Vp + dense_off / sizeof(float)));
    t.dense = t.dense_base + dense_off / sizeof(float);
    if (Vp != V) HIP_TRY(hipMemsetAsync(t.dense, 0, (size_t)M * 3 * Vp * sizeof(float), c->stream));
    // stream the host array through a bounded device staging buffer, re-laying each morph into planes
    const uint32_t batch = (uint32_t)std::max<size_t>(1, std::min<size_t>(M, (64u << 20) / (V * 12)));
    Scratch<float> scratch;
    HIP_TRY(scratch.alloc((size_t)batch * V * 3));
    float *tmp = scratch.p;
    for (uint32_t m0 = 0; m0 < M; m0 += batch) {
        const uint32_t nb = std::min(batch, M - m0);
        HIP_TRY(hipMemcpy(tmp, deltas + (size_t)m0 * V * 3, (size_t)nb * V * 3 * sizeof(float), hipMemcpyHostToDevice));
        for (uint32_t k = 0; k < nb; ++k) {
            float *pl = t.dense + (size_t)(m0 + k) * 3 * Vp;
            HIP_TRY(rz_launch_deinterleave(tmp + (size_t)k * V * 3, 3, 0, (uint32_t)V, pl, pl + Vp, pl + 2 * Vp, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    t.storage = 32;
    return RZ_OK;
}

// 24-bit planes: encoded on the host a batch of morphs at a time (at most 64 MB of packed planes), each batch one copy
static int upload_dense_q24(rz_ctx *c, RzStatic::Morphs &t, uint32_t M, const float *deltas, const std::vector<float> &scales)
{
    const size_t Vp = c->mesh.Vp, V = c->mesh.V, plane = Vp * 3, per_morph = plane * 3;      // bytes
    HIP_TRY(t.dense_base.alloc((size_t)M * per_morph / sizeof(float)));       // (Vp is a multiple of 1024: whole floats)
    t.dense = t.dense_base;
    HIP_TRY(t.dense_fold.alloc(M));
    const uint32_t batch = (uint32_t)std::max<size_t>(1, std::min<size_t>(M, (64u << 20) / per_morph));
    std::vector<uint32_t> stage((size_t)batch * per_morph / 4, 0u);               // (the pad past V stays zero: every batch writes the same quads)
    char *dst = reinterpret_cast<char *>(t.dense);
    for (uint32_t m0 = 0; m0 < M; m0 += batch) {
        const uint32_t nb = std::min(batch, M - m0);
        for (uint32_t k = 0; k < nb; ++k)
            for (int comp = 0; comp < 3; ++comp)
                encode_plane24(deltas + (size_t)(m0 + k) * V * 3, (uint32_t)V, comp, 1.0f / scales[m0 + k], stage.data() + ((size_t)k * 3 + comp) * (plane / 4));
        HIP_TRY(hipMemcpy(dst + (size_t)m0 * per_morph, stage.data(), (size_t)nb * per_morph, hipMemcpyHostToDevice));
    }
    t.dense_fold_host.resize(M);
    for (uint32_t m = 0; m < M; ++m) t.dense_fold_host[m] = scales[m] * (1.0f / 256.0f);
    HIP_TRY(hipMemcpy(t.dense_fold, t.dense_fold_host.data(), (size_t)M * sizeof(float), hipMemcpyHostToDevice));
    t.storage = 24;
    return RZ_OK;
}

int rz_upload_morphs_dense_ex(rz_ctx *c, uint32_t M, const float *deltas, uint32_t flags)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_morphs_dense")) return r;
    if (flags & ~(uint32_t)RZ_MORPH_F32) return fail(RZ_ERR_INVALID, "rz_upload_morphs_dense_ex: unknown flags 0x%x", flags);
    if (c->mesh.V == 0) return fail(RZ_ERR_INVALID, "upload the mesh before its morph targets");
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_morphs(c);
    if (M == 0) return ensure_pose_buffers(c);
    if (!deltas) return fail(RZ_ERR_INVALID, "null morph deltas");
    std::vector<float> scales(M);
    bool q24 = !(flags & RZ_MORPH_F32);
    if (q24) q24 = morph_scales24(M, c->mesh.V, deltas, scales.data());
    RzStatic::Morphs t;
    if (int r = q24 ? upload_dense_q24(c, t, M, deltas, scales) : upload_dense_f32(c, t, M, deltas)) return r;
    t.mode = 1;
    t.M = M;
    t.Mpad = round_up(M + 8, 4);
    c->morphs = std::move(t);
    return ensure_pose_buffers(c);
}

int rz_upload_morphs_dense(rz_ctx *c, uint32_t M, const float *deltas) { return rz_upload_morphs_dense_ex(c, M, deltas, 0u); }

int rz_read_morph_dense(rz_ctx *c, uint32_t m, float *planes3)
{
    if (int r = use(c)) return r;
    if (c->morphs.mode != 1 || !c->morphs.dense) return fail(RZ_ERR_INVALID, "rz_read_morph_dense: no dense morph targets resident");
    if (m >= c->morphs.M || !planes3) return fail(RZ_ERR_INVALID, "rz_read_morph_dense: morph %u of %u, or null output", m, c->morphs.M);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t Vp = c->mesh.Vp, V = c->mesh.V;
    if (c->morphs.storage != 24) {
        for (int comp = 0; comp < 3; ++comp)
            HIP_TRY(hipMemcpy(planes3 + comp * V, c->morphs.dense + ((size_t)m * 3 + comp) * Vp, V * sizeof(float), hipMemcpyDeviceToHost));
        return RZ_OK;
    }
    std::vector<uint8_t> raw(Vp * 9);
    HIP_TRY(hipMemcpy(raw.data(), reinterpret_cast<const char *>(c->morphs.dense) + (size_t)m * Vp * 9, raw.size(), hipMemcpyDeviceToHost));
    const float fold = c->morphs.dense_fold_host[m];
    for (int comp = 0; comp < 3; ++comp)
        for (size_t v = 0; v < V; ++v) {
            const uint8_t *b = raw.data() + (size_t)comp * Vp * 3 + v * 3;
            const int32_t q8 = (int32_t)((uint32_t)b[0] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 24);       // q << 8, as the kernels decode it
            planes3[comp * V + v] = (float)q8 * fold;
        }
    return RZ_OK;
}

int rz_upload_morphs_sparse(rz_ctx *c, uint32_t M, const uint32_t *morph_off, const uint32_t *vert_idx, const float *delta3)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_morphs_sparse")) return r;
    if (c->mesh.V == 0) return fail(RZ_ERR_INVALID, "upload the mesh before its morph targets");
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_morphs(c);
    if (M == 0) return ensure_pose_buffers(c);
    if (!morph_off) return fail(RZ_ERR_INVALID, "null morph offsets");
    const uint32_t E = morph_off[M];
    if (E > 0 && (!vert_idx || !delta3)) return fail(RZ_ERR_INVALID, "null morph entries");
    for (uint32_t m = 0; m < M; ++m)
        if (morph_off[m] > morph_off[m + 1]) return fail(RZ_ERR_INVALID, "morph offsets must be non-decreasing");
    // transpose morph-major (PMX file order) into a per-vertex CSR; a vertex's entries keep
    // ascending morph order (then file order), which is the oracle's accumulation order
    const size_t Vp = c->mesh.Vp;
    std::vector<uint32_t> ptr(Vp + 1, 0);
    for (uint32_t e = 0; e < E; ++e)
        if (vert_idx[e] < c->mesh.V) ptr[vert_idx[e] + 1]++;
    for (size_t v = 0; v < Vp; ++v) ptr[v + 1] += ptr[v];
    const uint32_t kept = ptr[Vp];
    std::vector<float4> ent(std::max<uint32_t>(kept, 1));
    std::vector<uint32_t> cur(ptr.begin(), ptr.end() - 1);
    for (uint32_t m = 0; m < M; ++m)
        for (uint32_t e = morph_off[m]; e < morph_off[m + 1]; ++e) {
            const uint32_t v = vert_idx[e];
            if (v >= c->mesh.V) continue;
            float4 x;
            x.x = delta3[(size_t)e * 3]; x.y = delta3[(size_t)e * 3 + 1]; x.z = delta3[(size_t)e * 3 + 2];
            memcpy(&x.w, &m, 4);
            ent[cur[v]++] = x;
        }
    RzStatic::Morphs t;
    HIP_TRY(t.sp_ptr.alloc(Vp + 1));
    HIP_TRY(t.sp_entries.alloc(ent.size()));
    HIP_TRY(hipMemcpy(t.sp_ptr, ptr.data(), (Vp + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.sp_entries, ent.data(), ent.size() * sizeof(float4), hipMemcpyHostToDevice));
    t.sp_count = kept;
    t.mode = 2;
    t.M = M;
    t.Mpad = round_up(M + 8, 4);
    c->morphs = std::move(t);
    return ensure_pose_buffers(c);
}

int rz_set_instances(rz_ctx *c, uint32_t I)
{
    if (int r = use(c)) return r;
    if (I == 0 || I > 65535) return fail(RZ_ERR_INVALID, "instance count must be 1..65535");
    if (I > 1 && (c->comm || c->gather_root)) return fail(RZ_ERR_UNSUPPORTED, "instancing and vertex sharding are exclusive");
    // the chain switches follow the count: planned under the old count (nothing is changed if that fails), committed with the new one before
    // anything else can fail, so the mirror is never sized for another count than c->I
    IkWordsPlan sw;
    if (int r = plan_ik_resize(c, I, &sw)) return r;
    if (I != c->I) {
        forget_search(c);
        drop_graph(c);
        c->aabb_rearm = true;
        c->ovr_count = 0;                 // overrides name (instance, bone) pairs of the old crowd
        c->ph.reset = true;               // (a physics table rebuilds its per-instance state and the overrides at its next step)
        // The host-compacted active-morph list is only maintained while I == 1 (upload_pose). Coming back to one instance
        // from a crowd it is stale (zeroed): let the prep kernel compact instance 0's weights, which are still on the device.
        if (c->morphs.M > 0 && c->morphs.mode == 1) c->pl.cur.ml.count = -1;
        // A crowd larger than the one the resident pose was uploaded for has no pose for its new members (and a
        // single-character pose may still sit in its pinned slot, which holds exactly one instance): ask for a new one.
        if (I > c->pl.cur.I) c->pl.cur.set = false;
        retire_pose_tags(c);
    }
    c->I = I;
    if (int r = commit_ik_words(c, sw)) return r;
    if (int r = ensure_pose_buffers(c)) return r;
    return ensure_outputs(c);
}

int rz_upload_skeleton_topology(rz_ctx *c, uint32_t B, const int32_t *parents, const float *bind_translation3,
                                const int32_t *append_parent, const float *append_ratio, const uint8_t *append_move)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_skeleton_topology")) return r;
    if (B == 0 || B != c->skel.B) return fail(RZ_ERR_INVALID, "topology has %u bones but the uploaded skeleton has %u", B, c->skel.B);
    if (!parents || !bind_translation3) return fail(RZ_ERR_INVALID, "null topology arrays");
    // hierarchy levels (parents may come in any order, like the reference's recursive solve; cycles are an error)
    std::vector<int> level(B, -1);
    for (uint32_t b = 0; b < B; ++b) {
        if (parents[b] >= (int32_t)B) return fail(RZ_ERR_INVALID, "bone %u parent %d out of range", b, parents[b]);
        std::vector<uint32_t> chain;
        uint32_t cur = b;
        while (level[cur] < 0) {
            chain.push_back(cur);
            if (chain.size() > B) return fail(RZ_ERR_INVALID, "bone hierarchy has a cycle through bone %u", b);
            if (parents[cur] < 0) { level[cur] = 0; chain.pop_back(); break; }
            cur = (uint32_t)parents[cur];
        }
        for (size_t k = chain.size(); k-- > 0;) level[chain[k]] = level[(uint32_t)parents[chain[k]]] + 1;
    }
    int n_levels = 0;
    for (uint32_t b = 0; b < B; ++b) n_levels = std::max(n_levels, level[b] + 1);
    // ancestors by level: up[b][d] for d = 1, 2, ... (parents may come in any order)
    auto ancestor = [&](uint32_t b, uint32_t d) -> uint32_t {
        int32_t cur = (int32_t)b;
        for (uint32_t k = 0; k < d && cur >= 0; ++k) cur = parents[cur];
        return cur < 0 ? 0xffffu : (uint32_t)cur;
    };
    int n_rounds = 0;
    for (int span = 1; span < n_levels; span *= 4) ++n_rounds;          // radix-4 pointer doubling: ceil(log4(depth)) rounds
    // 64-byte bone records (kernels/fk.hip.h): topology | bind translation | the motion's track (rebuild_fk_static) | ancestors of rounds 0, 1
    std::vector<uint4> rec((size_t)B * 4);
    std::vector<uint2> more((size_t)std::max(0, n_rounds - 2) * B);
    for (uint32_t b = 0; b < B; ++b) {
        const int32_t ap = (append_parent && append_parent[b] >= 0 && append_parent[b] < (int32_t)B) ? append_parent[b] : -1;
        const float ratio = append_ratio ? append_ratio[b] : 1.0f;
        uint32_t rb, bx, by, bz;
        memcpy(&rb, &ratio, 4);
        memcpy(&bx, bind_translation3 + (size_t)b * 3, 4); memcpy(&by, bind_translation3 + (size_t)b * 3 + 1, 4); memcpy(&bz, bind_translation3 + (size_t)b * 3 + 2, 4);
        rec[4 * b] = make_uint4((uint32_t)(parents[b] < 0 ? -1 : parents[b]), (uint32_t)ap, rb, (append_move && append_move[b]) ? 1u : 0u);
        rec[4 * b + 1] = make_uint4(bx, by, bz, 0u);
        rec[4 * b + 2] = make_uint4(0u, 0u, 0u, 0u);
        uint32_t span = 1, w[4] = { 0xffffffffu, 0xffffu, 0xffffffffu, 0xffffu };
        for (int r = 0; r < n_rounds; ++r, span *= 4) {
            const uint32_t a1 = ancestor(b, span), a2 = ancestor(b, 2 * span), a3 = ancestor(b, 3 * span);
            if (r < 2) { w[2 * r] = a1 | (a2 << 16); w[2 * r + 1] = a3; }
            else more[(size_t)(r - 2) * B + b] = make_uint2(a1 | (a2 << 16), a3);
        }
        rec[4 * b + 3] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    free_ik(c);                         // its chains were checked against the old parents
    free_after(c);                      // rz_upload_after_physics: its levels were derived from the old parents and append parents
    free_physics(c);                    // its bind pose was taken from the old hierarchy
    c->ovr_count = 0;
    c->ovr_follow = 0; c->fol_count = 0;        // rz_override_follow: the follower lists were built from the old parents
    c->fk_stale = false;                // (a crowd frame solved under the old topology: nothing of it can be formed on demand any more)
    c->fk = {}; c->fk_gen++;
    RzStatic::Hierarchy t;
    if (!more.empty())
        if (int r = to_device(t.anc_more, more.data(), more.size())) return r;
    t.host = std::move(rec);
    t.rounds = n_rounds;
    t.has_topology = true;
    c->fk = std::move(t);
    return rebuild_fk_static(c);
}

int rz_upload_bone_morphs(rz_ctx *c, uint32_t n, const uint32_t *morph, const uint32_t *bone, const float *translation3, const float *rotation4)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_bone_morphs")) return r;
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        free_bone_morphs(c);
        return RZ_OK;
    }
    if (!c->fk.has_topology) return fail(RZ_ERR_INVALID, "bone morphs act on device-solved poses: call rz_upload_skeleton_topology first");
    if (c->morphs.M == 0) return fail(RZ_ERR_INVALID, "upload the morph set first (rz_upload_morphs_*): bone-morph entries name its morphs");
    if (!morph || !bone || !translation3 || !rotation4) return fail(RZ_ERR_INVALID, "null bone-morph arrays");
    for (uint32_t k = 0; k < n; ++k) {
        if (morph[k] >= c->morphs.M) return fail(RZ_ERR_INVALID, "bone-morph entry %u names morph %u of %u", k, morph[k], c->morphs.M);
        if (bone[k] >= c->skel.B) return fail(RZ_ERR_INVALID, "bone-morph entry %u names bone %u of %u", k, bone[k], c->skel.B);
        for (int j = 0; j < 7; ++j) {
            const float x = j < 3 ? translation3[(size_t)k * 3 + j] : rotation4[(size_t)k * 4 + j - 3];
            if (!(x == x) || x - x != 0.0f) return fail(RZ_ERR_INVALID, "bone-morph entry %u is not finite", k);
        }
    }
    // group by bone; inside a bone ascending morph index, file order among equal morphs (a stable sort of the entry list)
    std::vector<uint32_t> idx(n);
    for (uint32_t k = 0; k < n; ++k) idx[k] = k;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return bone[a] != bone[b] ? bone[a] < bone[b] : morph[a] < morph[b]; });
    std::vector<uint32_t> off(c->skel.B + 1, 0), mo(n);
    std::vector<float4> rot(n), tr(n);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t e = idx[k];
        off[bone[e] + 1]++;
        mo[k] = morph[e];
        rot[k] = make_float4(rotation4[(size_t)e * 4], rotation4[(size_t)e * 4 + 1], rotation4[(size_t)e * 4 + 2], rotation4[(size_t)e * 4 + 3]);
        tr[k] = make_float4(translation3[(size_t)e * 3], translation3[(size_t)e * 3 + 1], translation3[(size_t)e * 3 + 2], 0.0f);
    }
    for (uint32_t b = 0; b < c->skel.B; ++b) off[b + 1] += off[b];
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_bone_morphs(c);
    drop_graph(c);
    RzStatic::BoneMorphs t;
    if (int r = to_device(t.off, off.data(), off.size())) return r;
    if (int r = to_device(t.morph, mo.data(), n)) return r;
    if (int r = to_device(t.rot, rot.data(), n)) return r;
    if (int r = to_device(t.tr, tr.data(), n)) return r;
    t.count = n;
    c->bm = std::move(t);
    return RZ_OK;
}

// One motion store from motion_table.h's arrays, into an empty store (a local of the upload). Every pointer is allocated, of four
// elements at least (to_device), but the interpolation bytes: null when no clip carries any.
static int upload_keys(RzStatic::RzKeys &k, const rzmotion::Flat &f, uint32_t M)
{
    if (int r = to_device(k.key_frame, f.key_frame.data(), f.key_frame.size())) return r;
    if (int r = to_device(k.key_rot, f.key_rot.data(), f.key_rot.size() / 4)) return r;
    if (int r = to_device(k.key_pos, f.key_pos.data(), f.key_pos.size())) return r;
    if (!f.key_interp.empty())
        if (int r = to_device(k.key_interp, f.key_interp.data(), f.key_interp.size() / 16)) return r;
    if (int r = to_device(k.mkey_frame, f.mkey_frame.data(), f.mkey_frame.size())) return r;
    if (int r = to_device(k.mkey_weight, f.mkey_weight.data(), f.mkey_weight.size())) return r;
    if (int r = to_device(k.feed_off, f.feed_off.data(), f.feed_off.size())) return r;
    if (int r = to_device(k.feed_range, f.feed_range.data(), f.feed_range.size() / 4)) return r;
    if (int r = to_device(k.feed_ratio, f.feed_ratio.data(), f.feed_ratio.size())) return r;
    k.M = M;
    return RZ_OK;
}

int rz_upload_animation(rz_ctx *c, const rz_animation *a)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_animation")) return r;
    rzmotion::Flat f;
    std::string why;
    if (!rzmotion::flatten(c->skel.B, c->morphs.M, 1, a, nullptr, f, why)) return fail(RZ_ERR_INVALID, "%s", why.c_str());
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_animation(c);
    RzStatic::RzKeys keys;
    if (int r = upload_keys(keys, f, c->morphs.M)) return r;
    c->an = std::move(keys);
    // host copies for the hierarchy's static block. Per bone: the key range itself, so the sampler's chain of dependent loads starts one
    // level lower. Per vertex morph: the key range of its FIRST feed and (first feed, end of feeds, bits(its ratio)) — the sampler's one record per morph
    auto rec = [](const std::vector<uint32_t> &v, size_t k) { return make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]); };
    c->an_host_range.resize(c->skel.B);
    for (uint32_t b = 0; b < c->skel.B; ++b) c->an_host_range[b] = rec(f.bone_rec, b);
    c->an_host_mrec.assign((size_t)c->morphs.M * 2, make_uint4(0u, 0u, 0u, 0u));
    for (uint32_t m = 0; m < c->morphs.M; ++m) {
        const uint32_t f0 = f.feed_off[m], f1 = f.feed_off[m + 1];
        if (f1 > f0) {
            uint32_t rb;
            memcpy(&rb, &f.feed_ratio[f0], 4);
            c->an_host_mrec[2 * m] = rec(f.feed_range, f0);
            c->an_host_mrec[2 * m + 1] = make_uint4(f0, f1, rb, 0u);
        }
    }
    c->has_animation = true;
    return rebuild_fk_static(c);
}

int rz_upload_motions(rz_ctx *c, uint32_t n_clips, const rz_animation *clips)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_motions")) return r;
    if (n_clips == 0) {
        free_motions(c);
        return RZ_OK;
    }
    if (!clips) return fail(RZ_ERR_INVALID, "rz_upload_motions: null clips");
    if (n_clips == 0xffffffffu) return fail(RZ_ERR_INVALID, "rz_upload_motions: too many clips");
    rzmotion::Flat f;                   // every clip is checked before anything is replaced
    std::string why;
    if (!rzmotion::flatten(c->skel.B, c->morphs.M, n_clips, clips, "rz_upload_motions", f, why)) return fail(RZ_ERR_INVALID, "%s", why.c_str());
    free_motions(c);                    // (drains both streams first: a pose kernel may still be reading the old library)
    RzStatic::Library lib;
    RzStatic::RzKeys keys;
    if (int r = to_device(lib.bone_rec, f.bone_rec.data(), f.bone_rec.size() / 4)) return r;
    if (int r = upload_keys(keys, f, c->morphs.M)) return r;
    lib.clips = n_clips;
    c->mo = std::move(keys);
    c->lib = std::move(lib);
    return RZ_OK;
}

// The masks of layered poses, packed into bit sets on the way to the device: one 32-bit word per 32 bones (vertex morphs), whole words per
// mask, so a wave reads two words of a mask where it would read 64 bytes.
int rz_upload_motion_masks(rz_ctx *c, uint32_t n_masks, const uint8_t *bone_mask, const uint8_t *morph_mask)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_motion_masks")) return r;
    if (n_masks == 0) {
        free_motion_masks(c);
        return RZ_OK;
    }
    if (c->skel.B == 0) return fail(RZ_ERR_INVALID, "upload the skeleton before the motion masks");
    if (!bone_mask) return fail(RZ_ERR_INVALID, "rz_upload_motion_masks: null bone masks");
    if (n_masks == 0xffffffffu) return fail(RZ_ERR_INVALID, "rz_upload_motion_masks: too many masks");
    const uint32_t B = c->skel.B, M = c->morphs.M, wb = (B + 31) / 32, wm = (M + 31) / 32;
    auto pack = [n_masks](const uint8_t *bytes, uint32_t n, uint32_t words) {
        std::vector<uint32_t> bits((size_t)n_masks * words, 0u);
        for (uint32_t k = 0; k < n_masks; ++k)
            for (uint32_t i = 0; i < n; ++i)
                if (bytes[(size_t)k * n + i]) bits[(size_t)k * words + (i >> 5)] |= 1u << (i & 31);
        return bits;
    };
    const std::vector<uint32_t> bone_bits = pack(bone_mask, B, wb);
    const bool morphs = morph_mask != nullptr && M > 0;
    const std::vector<uint32_t> morph_bits = morphs ? pack(morph_mask, M, wm) : std::vector<uint32_t>();
    free_motion_masks(c);               // (drains both streams first: a layer kernel may still be reading the old masks)
    RzStatic::Masks t;
    if (int r = to_device(t.bone_bits, bone_bits.data(), bone_bits.size())) return r;
    if (morphs)
        if (int r = to_device(t.morph_bits, morph_bits.data(), morph_bits.size())) return r;
    t.bone_words = wb;
    t.morph_words = morphs ? wm : 0;
    t.M = M;
    t.count = n_masks;
    c->mk = std::move(t);
    return RZ_OK;
}

int rz_upload_edge_scale(rz_ctx *c, uint32_t V, const float *edge_size)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_edge_scale")) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    if (!edge_size) { c->edge = {}; return RZ_OK; }
    if (V != c->mesh.V || V == 0) return fail(RZ_ERR_INVALID, "edge scale has %u entries but the mesh has %u vertices", V, c->mesh.V);
    c->edge = {};
    rzi::Lent<float> edge;
    HIP_TRY(edge.alloc(c->mesh.Vp));
    HIP_TRY(hipMemsetAsync(edge, 0, (size_t)c->mesh.Vp * sizeof(float), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(edge, edge_size, (size_t)V * sizeof(float), hipMemcpyHostToDevice));
    c->edge = std::move(edge);
    return ensure_outputs(c);
}

// the first vertex two strictly ascending lists share, or -1 (a PMX vertex has one weight type: the SDEF and QDEF tables are disjoint)
static int64_t first_shared(const uint32_t *a, size_t na, const std::vector<uint32_t> &b)
{
    size_t i = 0, k = 0;
    while (i < na && k < b.size()) {
        if (a[i] == b[k]) return (int64_t)a[i];
        if (a[i] < b[k]) ++i; else ++k;
    }
    return -1;
}

int rz_upload_sdef(rz_ctx *c, uint32_t n, const uint32_t *vert_idx, const float *c3, const float *r0_3, const float *r1_3)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_sdef")) return r;
    if (n > 0) {
        if (!vert_idx || !c3 || !r0_3 || !r1_3) return fail(RZ_ERR_INVALID, "rz_upload_sdef: null arrays for %u entries", n);
        if (c->mesh.V == 0) return fail(RZ_ERR_INVALID, "upload the mesh before its SDEF table");
        for (uint32_t k = 0; k < n; ++k) {
            if (vert_idx[k] >= c->mesh.V) return fail(RZ_ERR_INVALID, "rz_upload_sdef: vertex index %u (entry %u) is outside the shard's %u vertices", vert_idx[k], k, c->mesh.V);
            if (k > 0 && vert_idx[k] <= vert_idx[k - 1])
                return fail(RZ_ERR_INVALID, "rz_upload_sdef: vertex indices must be strictly ascending (entry %u: %u after %u)", k, vert_idx[k], vert_idx[k - 1]);
        }
        const int64_t both = first_shared(vert_idx, n, c->qdef.idx_host);
        if (both >= 0) return fail(RZ_ERR_INVALID, "rz_upload_sdef: vertex %lld is in the QDEF table already (a vertex has one weight type)", (long long)both);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    free_sdef(c);
    if (n == 0) return RZ_OK;
    // [10][n] planes: index | C xyz | R0 xyz | R1 xyz
    std::vector<uint32_t> tab((size_t)n * 10);
    memcpy(tab.data(), vert_idx, (size_t)n * 4);
    const float *src[3] = { c3, r0_3, r1_3 };
    for (int a = 0; a < 3; ++a)
        for (int d = 0; d < 3; ++d)
            for (uint32_t k = 0; k < n; ++k) memcpy(&tab[(size_t)(1 + 3 * a + d) * n + k], &src[a][(size_t)k * 3 + d], 4);
    RzStatic::VertexTable t;
    if (int r = to_device(t.tab, tab.data(), tab.size())) return r;
    t.n = n;
    t.idx_host.assign(vert_idx, vert_idx + n);
    c->sdef = std::move(t);
    return RZ_OK;
}

int rz_upload_qdef(rz_ctx *c, uint32_t n, const uint32_t *vert_idx)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_qdef")) return r;
    if (n > 0) {
        if (!vert_idx) return fail(RZ_ERR_INVALID, "rz_upload_qdef: null array for %u entries", n);
        if (c->mesh.V == 0) return fail(RZ_ERR_INVALID, "upload the mesh before its QDEF table");
        for (uint32_t k = 0; k < n; ++k) {
            if (vert_idx[k] >= c->mesh.V) return fail(RZ_ERR_INVALID, "rz_upload_qdef: vertex index %u (entry %u) is outside the shard's %u vertices", vert_idx[k], k, c->mesh.V);
            if (k > 0 && vert_idx[k] <= vert_idx[k - 1])
                return fail(RZ_ERR_INVALID, "rz_upload_qdef: vertex indices must be strictly ascending (entry %u: %u after %u)", k, vert_idx[k], vert_idx[k - 1]);
        }
        const int64_t both = first_shared(vert_idx, n, c->sdef.idx_host);
        if (both >= 0) return fail(RZ_ERR_INVALID, "rz_upload_qdef: vertex %lld is in the SDEF table already (a vertex has one weight type)", (long long)both);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    free_qdef(c);
    if (n == 0) return RZ_OK;
    RzStatic::VertexTable t;
    if (int r = to_device(t.tab, vert_idx, (size_t)n)) return r;
    t.n = n;
    t.idx_host.assign(vert_idx, vert_idx + n);
    c->qdef = std::move(t);
    return RZ_OK;
}

int rz_upload_ik(rz_ctx *c, uint32_t n_chains, const uint32_t *goal, const uint32_t *effector, const uint32_t *loops, const float *limit_angle,
                 const uint32_t *link_off, const uint32_t *link_bone, const uint8_t *link_limited, const float *link_min3, const float *link_max3)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_ik")) return r;
    if (n_chains == 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        free_ik(c);
        return RZ_OK;
    }
    if (!c->fk.has_topology || c->fk.host.size() != (size_t)c->skel.B * 4) return fail(RZ_ERR_INVALID, "IK acts on device-solved poses: call rz_upload_skeleton_topology first");
    if (n_chains > 65535) return fail(RZ_ERR_INVALID, "rz_upload_ik: %u chains (at most 65535)", n_chains);
    if (!goal || !effector || !loops || !limit_angle || !link_off) return fail(RZ_ERR_INVALID, "rz_upload_ik: null chain arrays for %u chains", n_chains);
    for (uint32_t k = 0; k < n_chains; ++k)
        if (link_off[k] > link_off[k + 1]) return fail(RZ_ERR_INVALID, "rz_upload_ik: link offsets must be non-decreasing (chain %u)", k);
    if (link_off[0] != 0) return fail(RZ_ERR_INVALID, "rz_upload_ik: link offsets start at %u, not 0", link_off[0]);
    const uint32_t NL = link_off[n_chains];
    if (NL && (!link_bone || !link_limited || !link_min3 || !link_max3)) return fail(RZ_ERR_INVALID, "rz_upload_ik: null link arrays for %u links", NL);
    const uint32_t B = c->skel.B;
    auto parent_of = [&](uint32_t b) { return (int32_t)c->fk.host[4 * (size_t)b].x; };
    auto append_of = [&](uint32_t b) -> int32_t {          // the bone whose local rotation b's local matrix reads, or -1 (fk_local_matrix)
        const uint4 r = c->fk.host[4 * (size_t)b];
        float ratio;
        memcpy(&ratio, &r.z, 4);
        return ((int32_t)r.y >= 0 && fabsf(fminf(1.0f, fmaxf(-1.0f, ratio))) > 1e-6f) ? (int32_t)r.y : -1;
    };
    // per chain: the path, outermost link ... effector (parents first), and the checks of "a valid table"
    std::vector<std::vector<uint32_t>> path(n_chains);
    std::vector<uint8_t> is_link((size_t)n_chains * B, 0), any_link(B, 0);
    for (uint32_t k = 0; k < n_chains; ++k) {
        const uint32_t nl = link_off[k + 1] - link_off[k];
        if (goal[k] >= B || effector[k] >= B) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u names bone %u / %u of %u", k, goal[k], effector[k], B);
        if (goal[k] == effector[k]) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u: the effector is the goal (bone %u)", k, goal[k]);
        if (nl > 255) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u has %u links (at most 255)", k, nl);
        if ((int32_t)loops[k] < 0) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u: loop count out of range", k);
        if (!(limit_angle[k] == limit_angle[k]) || limit_angle[k] - limit_angle[k] != 0.0f) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u: the angle limit is not finite", k);
        std::vector<uint32_t> rev{effector[k]};             // effector upwards
        uint32_t cur = effector[k];
        for (uint32_t e = link_off[k]; e < link_off[k + 1]; ++e) {
            const uint32_t L = link_bone[e];
            if (L >= B) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u: link %u names bone %u of %u", k, e - link_off[k], L, B);
            for (int j = 0; j < 3; ++j) {
                const float lo = link_min3[(size_t)e * 3 + j], hi = link_max3[(size_t)e * 3 + j];
                if (link_limited[e] && (!(lo == lo) || lo - lo != 0.0f || !(hi == hi) || hi - hi != 0.0f))
                    return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u: the limits of link %u are not finite", k, e - link_off[k]);
            }
            // every link is a proper ancestor of the one before it (the first: of the effector)
            int32_t p = parent_of(cur);
            while (p >= 0 && (uint32_t)p != L) { rev.push_back((uint32_t)p); p = parent_of((uint32_t)p); }
            if (p < 0) return fail(RZ_ERR_INVALID, "rz_upload_ik: chain %u: link bone %u is not a proper ancestor of bone %u", k, L, cur);
            rev.push_back(L);
            is_link[(size_t)k * B + L] = 1; any_link[L] = 1;
            cur = L;
        }
        path[k].assign(rev.rbegin(), rev.rend());
    }
    for (uint32_t k = 0; k < n_chains; ++k) {
        if (path[k].size() > 64 && link_off[k + 1] > link_off[k])
            return fail(RZ_ERR_UNSUPPORTED, "rz_upload_ik: chain %u spans %zu bones from its outermost link to its effector: a chain is solved by one wave, one path bone per lane (at most 64)", k, path[k].size());
        for (uint32_t b : path[k])
            if (append_of(b) >= 0 && any_link[(uint32_t)append_of(b)])
                return fail(RZ_ERR_UNSUPPORTED, "rz_upload_ik: bone %u on the path of chain %u takes its append rotation from bone %d, a link of an IK chain: every step would need the whole solve", b, k, append_of(b));
        // ... and so would a step when a bone ABOVE the path (an ancestor of the effector) copies the rotation of one of the chain's own links:
        // turning the link would move the whole path under it
        for (int32_t x = parent_of(path[k][0]); x >= 0; x = parent_of((uint32_t)x))
            if (append_of((uint32_t)x) >= 0 && is_link[(size_t)k * B + (uint32_t)append_of((uint32_t)x)])
                return fail(RZ_ERR_UNSUPPORTED, "rz_upload_ik: bone %d, an ancestor of the effector of chain %u, takes its append rotation from bone %d, a link of that chain: every step would need the whole solve", x, k, append_of((uint32_t)x));
        // the goal must hold still while its chain is solved
        for (int32_t x = (int32_t)goal[k]; x >= 0; x = parent_of((uint32_t)x))
            if (is_link[(size_t)k * B + (uint32_t)x] || (append_of((uint32_t)x) >= 0 && is_link[(size_t)k * B + (uint32_t)append_of((uint32_t)x)]))
                return fail(RZ_ERR_UNSUPPORTED, "rz_upload_ik: the goal of chain %u (bone %u) hangs below its own link %d: the goal would move with every step", k, goal[k], x);
    }
    // rz_upload_after_physics: a listed bone on a chain's path would be posed twice — by the chain, and again from its pose quaternion behind
    // the overrides, which undoes the chain (IK chains whose bones are listed are not re-solved after physics). A goal may be listed.
    for (uint32_t k = 0; k < n_chains; ++k)
        for (uint32_t b : path[k])
            if (std::find(c->af.bones.begin(), c->af.bones.end(), b) != c->af.bones.end())
                return fail(RZ_ERR_UNSUPPORTED, "rz_upload_ik: bone %u on the path of chain %u is an after-physics bone (rz_upload_after_physics): the stage does not solve IK again", b, k);
    // solve order: ascending IK bone (stable). Stages: a chain comes after every earlier chain whose links move a bone it reads (goal,
    // effector — whose ancestors cover the path —, through parents or an append rotation), and not before an earlier chain that reads a
    // bone ITS links move (that chain must not see it)
    std::vector<uint32_t> ord(n_chains);
    for (uint32_t k = 0; k < n_chains; ++k) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return goal[a] < goal[b]; });
    for (uint32_t k = 1; k < n_chains; ++k)
        if (goal[ord[k]] == goal[ord[k - 1]]) return fail(RZ_ERR_INVALID, "rz_upload_ik: two chains share the IK bone %u", goal[ord[k]]);
    auto moves = [&](uint32_t mover, uint32_t reader) {      // do the links of `mover` change the world matrix of a bone `reader` reads?
        const uint32_t reads[2] = { goal[reader], effector[reader] };
        for (uint32_t s : reads)
            for (int32_t x = (int32_t)s; x >= 0; x = parent_of((uint32_t)x)) {
                if (is_link[(size_t)mover * B + (uint32_t)x]) return true;
                const int32_t ap = append_of((uint32_t)x);
                if (ap >= 0 && is_link[(size_t)mover * B + (uint32_t)ap]) return true;
            }
        return false;
    };
    std::vector<uint32_t> stage(n_chains, 0);
    uint32_t n_stages = 0;
    for (uint32_t i = 0; i < n_chains; ++i) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < i; ++j) {
            if (moves(ord[j], ord[i])) s = std::max(s, stage[j] + 1);
            else if (moves(ord[i], ord[j])) s = std::max(s, stage[j]);
        }
        stage[i] = s;
        n_stages = std::max(n_stages, s + 1);
    }
    std::vector<uint32_t> by_stage(n_chains);
    for (uint32_t i = 0; i < n_chains; ++i) by_stage[i] = i;
    std::stable_sort(by_stage.begin(), by_stage.end(), [&](uint32_t a, uint32_t b) { return stage[a] < stage[b]; });
    std::vector<uint4> rec((size_t)n_chains * 2);
    std::vector<uint32_t> pth, soff(n_stages + 1, 0);
    std::vector<float4> lnk;
    for (uint32_t i = 0; i < n_chains; ++i) {
        const uint32_t k = ord[by_stage[i]];
        soff[stage[by_stage[i]] + 1]++;
        const uint32_t nl = link_off[k + 1] - link_off[k];
        uint32_t tb;
        memcpy(&tb, &limit_angle[k], 4);
        rec[2 * (size_t)i] = make_uint4(goal[k], (uint32_t)pth.size(), (uint32_t)path[k].size(), (uint32_t)parent_of(path[k][0]));
        rec[2 * (size_t)i + 1] = make_uint4(loops[k], tb, (uint32_t)lnk.size() / 2, nl);
        for (uint32_t e = link_off[k]; e < link_off[k + 1]; ++e) {
            uint32_t pos = 0;
            while (path[k][pos] != link_bone[e]) ++pos;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            if (link_limited[e]) {
                lo = make_float4(link_min3[(size_t)e * 3], link_min3[(size_t)e * 3 + 1], link_min3[(size_t)e * 3 + 2], 0.f);
                hi = make_float4(link_max3[(size_t)e * 3], link_max3[(size_t)e * 3 + 1], link_max3[(size_t)e * 3 + 2], 0.f);
            }
            const uint32_t lim = link_limited[e] ? 1u : 0u;
            memcpy(&lo.w, &pos, 4); memcpy(&hi.w, &lim, 4);
            lnk.push_back(lo); lnk.push_back(hi);
        }
        for (uint32_t b : path[k]) pth.push_back(b | (is_link[(size_t)k * B + b] ? 0x80000000u : 0u));
    }
    for (uint32_t s = 0; s < n_stages; ++s) soff[s + 1] += soff[s];
    if (lnk.empty()) { lnk.push_back(make_float4(0.f, 0.f, 0.f, 0.f)); lnk.push_back(make_float4(0.f, 0.f, 0.f, 0.f)); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_ik(c);
    drop_graph(c);
    RzStatic::Ik t;                     // (a local: a failure on any array takes the others with it)
    if (int r = to_device(t.chain, rec.data(), rec.size())) return r;
    if (int r = to_device(t.path, pth.data(), pth.size())) return r;
    if (int r = to_device(t.link, lnk.data(), lnk.size())) return r;
    if (int r = to_device(t.stage_off, soff.data(), soff.size())) return r;
    t.n = n_chains; t.stages = n_stages;
    // chain switches arrive in this call's chain order and travel in the device's: where each chain went
    t.on_path.assign(B, 0);
    for (uint32_t k = 0; k < n_chains; ++k)
        for (uint32_t b : path[k]) t.on_path[b] = 1;
    t.dev_pos.assign(n_chains, 0u);
    for (uint32_t i = 0; i < n_chains; ++i) t.dev_pos[ord[by_stage[i]]] = i;
    c->ik = std::move(t);
    return RZ_OK;
}

int rz_upload_after_physics(rz_ctx *c, uint32_t n, const uint32_t *bones)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_after_physics")) return r;
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->af.n) c->fk_stale = c->fk_stale || c->ovr_count != 0;       // world matrices in memory carry the stage: rz_read_world solves again
        free_after(c);
        return RZ_OK;
    }
    if (!c->fk.has_topology || c->fk.host.size() != (size_t)c->skel.B * 4)
        return fail(RZ_ERR_INVALID, "rz_upload_after_physics acts on device-solved poses: call rz_upload_skeleton_topology first");
    if (!bones) return fail(RZ_ERR_INVALID, "rz_upload_after_physics: null list of %u bones", n);
    rzafter::Table t;
    std::string err;
    if (rzafter::build(c->skel.B, reinterpret_cast<const uint32_t *>(c->fk.host.data()), n, bones, t, err)) return fail(RZ_ERR_INVALID, "%s", err.c_str());
    if (c->ik.n)
        for (uint32_t k = 0; k < n; ++k)
            if (c->ik.on_path[bones[k]])
                return fail(RZ_ERR_UNSUPPORTED, "rz_upload_after_physics: bone %u (entry %u) is a link or the effector of a resident IK chain, or lies on its path: the stage does not solve IK again", bones[k], k);
    const size_t lds = rzafter::lds_bytes(c->skel.B, n);
    if (lds > rzlds::kCuLds)
        return fail(RZ_ERR_UNSUPPORTED, "skeleton too large for the after-physics stage on the device: %u bones x 48 B + %u entries x 1 B = %zu B of LDS (the limit is 160 KB = %d B)", c->skel.B, n, lds, (int)rzlds::kCuLds);
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_after(c);
    drop_graph(c);
    RzStatic::After af;
    if (int r = to_device(af.rec, t.rec.data(), (size_t)n * 3)) return r;
    if (int r = to_device(af.level_off, t.level_off.data(), t.level_off.size())) return r;
    if (int r = to_device(af.index, t.index.data(), t.index.size())) return r;
    af.bones.assign(bones, bones + n);
    af.n = n; af.levels = (uint32_t)t.levels;
    c->af = std::move(af);
    if (c->ovr_count) c->fk_stale = true;       // world matrices and palettes in memory are the frame's without the stage: rz_read_world / rz_read_palette solve again
    return RZ_OK;
}

int rz_upload_ik_keys(rz_ctx *c, uint32_t clip, const rz_ik_keys *keys)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_ik_keys")) return r;
    if (!c->ik.n) return fail(RZ_ERR_INVALID, "rz_upload_ik_keys: no IK table is resident (rz_upload_ik names the chains the keys switch)");
    if (clip != RZ_NO_CLIP && clip >= c->lib.clips) return fail(RZ_ERR_INVALID, "rz_upload_ik_keys: clip %u of %u", clip, c->lib.clips);
    const uint32_t n = keys ? keys->n_keys : 0, nc = c->ik.n, W = (nc + 31) / 32;
    if (keys && n && (!keys->key_frame || !keys->key_enabled)) return fail(RZ_ERR_INVALID, "rz_upload_ik_keys: null key arrays for %u keys", n);
    for (uint32_t k = 0; k < n; ++k) {
        const float f = keys->key_frame[k];
        if (!(f == f) || f - f != 0.0f) return fail(RZ_ERR_INVALID, "rz_upload_ik_keys: the frame of key %u is not finite", k);
        if (k && f < keys->key_frame[k - 1]) return fail(RZ_ERR_INVALID, "rz_upload_ik_keys: key frames must not descend (key %u)", k);
    }
    RzIkKeySet set;
    set.resident = keys != nullptr;     // NULL removes the set
    if (n) {
        set.frame.assign(keys->key_frame, keys->key_frame + n);
        set.bits.assign((size_t)n * W, 0u);
        for (uint32_t k = 0; k < n; ++k)
            for (uint32_t ch = 0; ch < nc; ++ch)
                if (keys->key_enabled[(size_t)k * nc + ch]) { const uint32_t d = c->ik.dev_pos[ch]; set.bits[(size_t)k * W + (d >> 5)] |= 1u << (d & 31u); }
    }
    // host data of the pose calls alone: no frame in flight reads it, nothing to drain
    if (clip == RZ_NO_CLIP) { c->ik_keys_an = std::move(set); return RZ_OK; }
    if (c->ik_keys_mo.empty()) { if (!set.resident) return RZ_OK; c->ik_keys_mo.resize(c->lib.clips); }
    c->ik_keys_mo[clip] = std::move(set);
    bool any = false;
    for (const RzIkKeySet &s : c->ik_keys_mo) any = any || s.resident;
    if (!any) c->ik_keys_mo.clear();
    return RZ_OK;
}

int rz_enable_aabb(rz_ctx *c, int enable)
{
    if (int r = use(c)) return r;
    drop_graph(c);
    c->aabb_on = enable != 0;
    c->aabb_rearm = true;
    return ensure_outputs(c);
}

}  // extern "C"
