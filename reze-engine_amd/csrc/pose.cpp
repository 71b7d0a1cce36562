// pose.cpp — per-frame inputs: the pose transport (ctx.h: RzPoseLink) — its pinned staging ring, zero-copy slots and their prefetch protocol,
// big-pose ring, the transitions of the current pose — and the copies.
#include "ctx.h"

#include <immintrin.h>

using namespace rzi;

namespace rzi {

// Where the kernels read the current pose from: the device pose block, or (zero-copy, not yet resident) the pinned slot.
static const char *cur_slot_dev(const rz_ctx *c) { return static_cast<const char *>(c->pl.zc.slot[c->pl.cur.zc_slot].dev); }

const float *src_world(const rz_ctx *c)
{
    const RzPoseLink::Current &p = c->pl.cur;
    return (p.zc_slot >= 0 && !p.world_resident && !p.zc_local) ? reinterpret_cast<const float *>(cur_slot_dev(c)) : c->world;
}

const float *src_morph_w(const rz_ctx *c)
{
    const RzPoseLink::Current &p = c->pl.cur;
    return (p.zc_slot < 0 || p.mw_resident) ? c->morph_w : reinterpret_cast<const float *>(cur_slot_dev(c) + p.zc_mw_off);
}

const float4 *src_local_q(const rz_ctx *c)
{
    const RzPoseLink::Current &p = c->pl.cur;
    return (p.zc_slot < 0 || p.local_resident || !p.zc_local) ? c->local_q : reinterpret_cast<const float4 *>(cur_slot_dev(c) + p.zc_lq_off);
}

// Bring every part of a zero-copy pose into the device pose block (one copy out of the pinned slot, stream-ordered).
int make_resident(rz_ctx *c)
{
    RzPoseLink::Current &p = c->pl.cur;
    if (p.resident()) return RZ_OK;
    void *dst = p.zc_local ? static_cast<void *>(c->morph_w) : static_cast<void *>(c->world);
    HIP_TRY(hipMemcpyAsync(dst, c->pl.zc.slot[p.zc_slot].host, p.zc_total, hipMemcpyHostToDevice, c->stream));
    p.world_resident = p.mw_resident = p.local_resident = true;
    return RZ_OK;
}

// Sequence number of a zero-copy pose, the value its slot header and — once staged — its device tag hold:
// ring epoch << 32 | pose kind << 30 | upload index (1-based, 30 bits). The KIND (0 world matrices, 1 local rotations, 2 local
// rotations + translations) is part of the number because a helper workgroup stages the next slot assuming the next pose has the
// layout and size of its own frame's: a pose of another kind can then never match what the helper expected. Sizes inside a kind
// only change with the skeleton / morph set / instance count, which start a new epoch.
uint64_t zc_seq(const rz_ctx *c, uint64_t upload_index_1, int kind)
{
    return ((uint64_t)c->pl.epoch << 32) | ((uint64_t)(kind & 3) << 30) | (upload_index_1 & 0x3fffffffull);
}

// A new ring epoch: no slot header published so far and no tag a helper workgroup left in a pose block can match a later pose. For whatever changes
// what a staged pose would mean: the skeleton, the morph set, the crowd, the blocks' layout, a re-built ring, a block overwritten from the device side.
void retire_pose_tags(rz_ctx *c)
{
    c->pl.epoch++;
    c->pl.cur.seq = 0;
}

// The HIP side of the reuse proof (pose_ring.h), for both rings: record the event that is due in front of this upload on the compute stream —
// everything launched before upload u, i.e. every reader of uploads < u (a zero-copy slot is also read, speculatively, by the helper workgroup of
// the frame before its own: launched earlier still) — poll the one that covers the readers of the slot's previous tenant, and take the slot.
template <int N>
static int ring_take(rz_ctx *c, rzring::ReuseProof<N> &proof, const Events<2> &ev, const char *ring, const char *polled, int *slot_out)
{
    const int rec = proof.record_event();
    if (rec >= 0) {
        HIP_TRY(hipEventRecord(ev[rec], c->stream));
        proof.recorded(rec);
    }
    if (proof.reuses()) {
        if (!proof.held()) return fail(RZ_ERR_HIP, "%s ring bookkeeping is inconsistent (upload %llu)", ring, (unsigned long long)proof.uploads);
        if (int r = poll_event(ev[proof.poll_event()], polled)) return r;
    }
    *slot_out = proof.take();
    return RZ_OK;
}

}  // namespace rzi

extern "C" {

// Pinned staging ring for per-frame inputs: a slot is reused only after the copy that read it has completed.
static int stage_acquire(rz_ctx *c, size_t need, int *slot_out)
{
    RzPoseLink::Stage &sg = c->pl.stage;
    if (need > sg.bytes || !sg.slot[0].host) {
        RzPoseLink::Stage fresh;
        fresh.bytes = (need + 4095) / 4096 * 4096;
        fresh.next = sg.next;
        // device-mapped, so that a crowd's pose can be pulled out of the slot by a kernel; a slot that cannot be mapped is still good for copies
        for (Pinned &s : fresh.slot) HIP_TRY(s.alloc(fresh.bytes, false));
        HIP_TRY(fresh.ev.create());
        if (int r = drain(c)) return r;
        sg = std::move(fresh);
    }
    const int slot = sg.next;
    sg.next = (slot + 1) % kStageSlots;
    if (sg.used[slot]) {
        // the copy that read this slot kStageSlots uploads ago: normally long done
        if (int r = poll_event(sg.ev[slot], "pinned staging slot")) return r;
    }
    *slot_out = slot;
    return RZ_OK;
}

// What sits in staging slot `slot` has been enqueued on `us`. One event says both "the ring slot may be written again" (the host polls it
// eight uploads later) and, for a pose that travelled on the upload stream, "the pose has landed" (the compute stream waits for it): a record
// is ~1.4 us of stream time, and the upload stream is what a host-animated crowd is bound by.
static int staged_sent(rz_ctx *c, int slot, hipStream_t us, bool piped)
{
    HIP_TRY(hipEventRecord(c->pl.stage.ev[slot], us));
    c->pl.stage.used[slot] = true;
    if (piped) HIP_TRY(hipStreamWaitEvent(c->stream, c->pl.stage.ev[slot], 0));
    return RZ_OK;
}

}  // extern "C"

namespace rzi {

// ---- chain switches of the IK stage (rz_set_ik_enabled / rz_upload_ik_keys; tests/ik_switch_ref.py is the definition) ----
static uint32_t ik_sw_words(const rz_ctx *c) { return (c->ik.n + 31) / 32; }

// A change of the mask in two halves, so that a pose call can do everything that may fail BEFORE it touches the resident pose:
// plan_ik_words allocates, waits and fills the pinned slot; commit_ik_words enqueues the copy and takes the words into the mirror.
int plan_ik_words(rz_ctx *c, uint32_t I, std::vector<uint32_t> &&w, IkWordsPlan *pl)
{
    rz_ctx::IkSwitch &s = c->iksw;
    uint64_t on = 0;
    for (uint32_t x : w) on += (uint64_t)__builtin_popcount(x);
    pl->off = w.empty() ? 0u : (uint32_t)((uint64_t)I * c->ik.n - on);
    if (pl->off == 0) w.clear();
    pl->w = std::move(w);
    pl->slot = -1;
    pl->inline_words = I == 1 && ik_sw_words(c) <= (uint32_t)kRzIkSwInline;
    pl->change = pl->w != s.words || pl->inline_words != (c->I == 1 && ik_sw_words(c) <= (uint32_t)kRzIkSwInline);
    if (!pl->change || pl->w.empty() || pl->inline_words) return RZ_OK;
    // a crowd's bits: one pinned slot, one copy on the stream the hierarchy solve runs on, in order with the frames
    if (pl->w.size() > s.dev.capacity()) {
        if (int r = grow(c, s.dev.to(std::max<size_t>(pl->w.size(), 64)))) return r;
        // (the array moved, drained: until the commit the mirror's words are what a frame must find in it)
        if (s.off && !(c->I == 1 && ik_sw_words(c) <= (uint32_t)kRzIkSwInline))
            HIP_TRY(hipMemcpy(s.dev, s.words.data(), s.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (int r = stage_acquire(c, std::max<size_t>(pl->w.size() * sizeof(uint32_t), 4096), &pl->slot)) return r;
    memcpy(c->pl.stage.slot[pl->slot].host, pl->w.data(), pl->w.size() * sizeof(uint32_t));
    return RZ_OK;
}

int commit_ik_words(rz_ctx *c, IkWordsPlan &pl)
{
    if (!pl.change) return RZ_OK;
    rz_ctx::IkSwitch &s = c->iksw;
    int rc = RZ_OK;
    if (pl.slot >= 0) {
        hipStream_t us = front_stream(c);
        hipError_t e = hipMemcpyAsync(s.dev, c->pl.stage.slot[pl.slot].host, pl.w.size() * sizeof(uint32_t), hipMemcpyHostToDevice, us);
        if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(RZ_ERR_HIP, "the copy of the IK chain switches failed: %s", hipGetErrorString(e)); }
        else rc = staged_sent(c, pl.slot, us, false);
    }
    if (rc) { s.words.clear(); s.off = 0; return rc; }      // the array holds nobody knows what: all on, which never reads it
    s.words = std::move(pl.w);
    s.off = pl.off;
    pl.change = false;
    return RZ_OK;
}

int set_ik_words(rz_ctx *c, std::vector<uint32_t> &&w)
{
    IkWordsPlan pl;
    if (int r = plan_ik_words(c, c->I, std::move(w), &pl)) return r;
    return commit_ik_words(c, pl);
}

int plan_ik_resize(rz_ctx *c, uint32_t I, IkWordsPlan *pl)
{
    pl->change = false;
    if (c->iksw.words.empty() || I == c->I) return RZ_OK;
    const uint32_t W = ik_sw_words(c), n = c->ik.n;
    std::vector<uint32_t> w((size_t)I * W);
    for (uint32_t i = 0; i < I; ++i)
        for (uint32_t k = 0; k < W; ++k)
            w[(size_t)i * W + k] = i < c->I ? c->iksw.words[(size_t)i * W + k] : (k + 1 < W || (n & 31u) == 0 ? 0xffffffffu : (1u << (n & 31u)) - 1u);
    // (one character's words ride in the arguments, a crowd's lie in the device array: a change of the count may move them)
    return plan_ik_words(c, I, std::move(w), pl);
}

// the row of the LAST key whose frame is <= `frame` (before the first key: the first key's row); nullptr = the set holds no key: all on
static const uint32_t *ik_state_at(const RzIkKeySet &ks, uint32_t W, float frame)
{
    const size_t n = ks.frame.size();
    if (!n) return nullptr;
    const size_t k = (size_t)(std::upper_bound(ks.frame.begin(), ks.frame.end(), frame) - ks.frame.begin());
    return &ks.bits[(k ? k - 1 : 0) * W];
}

static void ik_row_into(const rz_ctx *c, const uint32_t *row, uint32_t *dst)
{
    const uint32_t W = ik_sw_words(c), n = c->ik.n;
    for (uint32_t k = 0; k < W; ++k) dst[k] = row ? row[k] : (k + 1 < W || (n & 31u) == 0 ? 0xffffffffu : (1u << (n & 31u)) - 1u);
}

}  // namespace rzi

extern "C" {

// One per-frame pose as the host handed it over, and where its parts go inside a slot (pinned slot and device pose block share
// the layout):   world pose [world | weights]     local pose [weights | rotations | translations]
struct PoseParts {
    const void *primary; size_t pbytes;       // world matrices or local rotations
    const void *secondary; size_t sbytes;     // local translations (local poses only, may be absent)
    const float *morph_weights;               // may be null (= all zero)
    bool local;
    size_t mb, mwb, total;                    // weight bytes handed over / their padded place / bytes of the whole range
};

// World matrices of a crowd travel as their upper three rows: 48 B per bone — the four columns' x y z, in the reference's
// column-major order (math.ts) — instead of 64. Only rows 0..2 of world * inverseBind ever reach a vertex (engine.ts:926-928 forms
// the product, vs() :262-272 keeps xyz), and they depend on rows 0..2 of the world matrix alone; the bottom row of an affine matrix
// is 0 0 0 1 and rz_pull_pose_kernel writes it back, so the device block holds what the host handed over — IF every bottom row is
// exactly that (bit patterns: -0 is not 0), which the packing loop checks in passing (returns false: the caller sends the pose as it
// is). Four bones per step: four 64-byte loads, three two-source permutes, three 64-byte NON-TEMPORAL stores — measured on the GPU
// box's EPYC 9575F (tools/archive/packbench, profiles/r5_packbench.txt) as fast as the memcpy it replaces while the ring is cache-resident
// (43 us for C4's 51 200 bones), and unlike cached stores it stays there when two contexts' rings (2 x 8 x 2.5 MB) no longer fit a
// CCD's L3: masked 48-byte stores then read every line for ownership first and the per-frame loop of a context and its fork went from
// 63 to 127-180 us per frame. (Needs AVX-512; without it the pose is not packed.)
__attribute__((target("avx512f"))) static bool pack_rows_avx512(const float *world, size_t bones, float *out)
{
    // out0 = m0[xyz of columns 0..3] m1[c0.xyz c1.x] | out1 = m1[c1.yz c2.xyz c3.xyz] m2[c0.xyz c1.xyz c2.xy] | out2 = m2[c2.z c3.xyz] m3[all twelve]
    const __m512i i0 = _mm512_setr_epi32(0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 16 + 0, 16 + 1, 16 + 2, 16 + 4);
    const __m512i i1 = _mm512_setr_epi32(5, 6, 8, 9, 10, 12, 13, 14, 16 + 0, 16 + 1, 16 + 2, 16 + 4, 16 + 5, 16 + 6, 16 + 8, 16 + 9);
    const __m512i i2 = _mm512_setr_epi32(10, 12, 13, 14, 16 + 0, 16 + 1, 16 + 2, 16 + 4, 16 + 5, 16 + 6, 16 + 8, 16 + 9, 16 + 10, 16 + 12, 16 + 13, 16 + 14);
    const __m512i bottom = _mm512_setr_epi32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x3f800000);
    __m512i acc = _mm512_setzero_si512();
    size_t b = 0;
    if ((reinterpret_cast<uintptr_t>(out) & 63u) == 0) {
        for (; b + 4 <= bones; b += 4) {
            const float *w = world + b * 16;
            const __m512 m0 = _mm512_loadu_ps(w), m1 = _mm512_loadu_ps(w + 16), m2 = _mm512_loadu_ps(w + 32), m3 = _mm512_loadu_ps(w + 48);
            _mm512_stream_ps(out + b * 12, _mm512_permutex2var_ps(m0, i0, m1));
            _mm512_stream_ps(out + b * 12 + 16, _mm512_permutex2var_ps(m1, i1, m2));
            _mm512_stream_ps(out + b * 12 + 32, _mm512_permutex2var_ps(m2, i2, m3));
            // lanes 3, 7, 11, 15 of every matrix against 0 0 0 1
            const __m512i x01 = _mm512_or_si512(_mm512_xor_si512(_mm512_castps_si512(m0), bottom), _mm512_xor_si512(_mm512_castps_si512(m1), bottom));
            const __m512i x23 = _mm512_or_si512(_mm512_xor_si512(_mm512_castps_si512(m2), bottom), _mm512_xor_si512(_mm512_castps_si512(m3), bottom));
            acc = _mm512_or_si512(acc, _mm512_or_si512(x01, x23));
        }
    }
    __mmask16 bad = _mm512_mask_test_epi32_mask((__mmask16)0x8888, acc, acc);
    const __m512i pick = _mm512_setr_epi32(0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 3, 7, 11, 15);
    for (; b < bones; ++b) {                    // the last one to three bones
        const __m512 m = _mm512_loadu_ps(world + b * 16);
        _mm512_mask_storeu_ps(out + b * 12, (__mmask16)0x0fff, _mm512_permutexvar_ps(pick, m));
        bad |= _mm512_mask_cmpneq_epi32_mask((__mmask16)0x8888, _mm512_castps_si512(m), bottom);
    }
    _mm_sfence();                               // the streaming stores are visible before anything that follows (the pull's launch)
    return bad == 0;
}

static bool can_pack_rows()
{
    static const bool ok = __builtin_cpu_supports("avx512f");
    return ok;
}

// the morph weights' place in a slot: the weights handed over (none: zeros), then zeros up to their padded size
static void lay_out_weights(const PoseParts &pp, char *st_mw)
{
    if (pp.morph_weights && pp.mb) memcpy(st_mw, pp.morph_weights, pp.mb); else memset(st_mw, 0, pp.mb);
    if (pp.mwb > pp.mb) memset(st_mw + pp.mb, 0, pp.mwb - pp.mb);
}

static void lay_out_pose(const rz_ctx *c, const PoseParts &pp, char *st)
{
    char *st_pr = pp.local ? st + pp.mwb : st;
    memcpy(st_pr, pp.primary, pp.pbytes);
    if (pp.sbytes) memcpy(st_pr + pp.pbytes, pp.secondary, pp.sbytes);
    if (pp.local || c->morphs.M > 0) lay_out_weights(pp, pp.local ? st : st + pp.pbytes);
}

// One character: no copy at all. The pose is laid out in a pinned, device-mapped slot; the frame's own kernels read it.
// Header protocol of the pose prefetch: invalid while the pose is being written, its sequence number once it is complete (x86 stores
// retire in program order; the fences keep the compiler from moving them). World-matrix poses are prefetched by the one-launch frame's
// helper, local poses by the fused-hierarchy frame's (zc_seq: the kind is part of the number). zc_open takes the next slot and marks it
// invalid (RZ_ERR_UNSUPPORTED when no such memory can be had: the caller copies instead); the pose is written (lay_out_pose, or the
// caller of rz_map_pose); zc_publish writes the number and makes the slot the current pose.
static int zc_open(rz_ctx *c, const PoseParts &pp, int *zs)
{
    const size_t need = std::max<size_t>(std::max<size_t>((size_t)c->skel.B * 64 + pp.mwb, pp.mwb + (size_t)c->skel.B * 28), 4096);
    if (need > c->pl.zc.bytes) {        // the ring is (re)built when the pose outgrew it
        RzPoseLink::ZeroCopy fresh;
        fresh.bytes = need; fresh.hdr_off = (need + 63) / 64 * 64;
        for (Pinned &s : fresh.slot) {
            // no pinned, device-mapped memory to be had (locked-memory limits ...): not an error, the caller copies instead
            if (s.alloc(fresh.hdr_off + 64, true) != hipSuccess) return RZ_ERR_UNSUPPORTED;
            memset(static_cast<char *>(s.host) + fresh.hdr_off, 0, 64);
        }
        HIP_TRY(fresh.ev.create());
        if (int r = drain(c)) return r;
        drop_graph(c);
        c->pl.zc = std::move(fresh);
        c->pl.cur.zc_slot = -1;
        retire_pose_tags(c);            // (before zc_publish forms this upload's sequence number: a re-built ring never matches old tags)
    }
    if (int r = ring_take(c, c->pl.zc.proof, c->pl.zc.ev, "zero-copy", "zero-copy pose ring", zs)) return r;
    *reinterpret_cast<volatile uint64_t *>(static_cast<char *>(c->pl.zc.slot[*zs].host) + c->pl.zc.hdr_off) = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    return RZ_OK;
}

static void zc_publish(rz_ctx *c, const PoseParts &pp, int zs, uint64_t upload_index_1)
{
    RzPoseLink::Current &p = c->pl.cur;
    volatile uint64_t *hdr = reinterpret_cast<volatile uint64_t *>(static_cast<char *>(c->pl.zc.slot[zs].host) + c->pl.zc.hdr_off);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    const int kind = pp.local ? (pp.sbytes ? 2 : 1) : 0;
    p.seq = zc_seq(c, upload_index_1, kind);
    *hdr = p.seq;
    point_pose_slot(c, c->pl.pose_slot ^ 1);   // where the pose will live once something makes it resident
    p.zc_slot = zs; p.zc_local = pp.local; p.zc_kind = kind; p.zc_total = pp.total;
    p.zc_mw_off = pp.local ? 0 : pp.pbytes; p.zc_lq_off = pp.mwb;
    p.world_resident = pp.local;            // a local pose has no world matrices to bring over: rz_fk_kernel writes them
    p.mw_resident = false;
    p.local_resident = !pp.local;
}

// The pose block is about to be written from the device side — a copy, a pull, a kernel that produces the pose there: nothing of the
// current pose sits in a pinned slot any more, and a block a helper workgroup may have staged and tagged is overwritten, so no later
// zero-copy pose may match that tag.
static void pose_leaves_pinned_slots(rz_ctx *c)
{
    RzPoseLink::Current &p = c->pl.cur;
    p.zc_slot = -1;
    retire_pose_tags(c);
    p.world_resident = p.mw_resident = p.local_resident = true;
}

// ... and the block it is written into: the other of the two pose blocks, or for a piped pose (more than 256 KB) the next block of the
// big-pose ring (ctx.h), (re)built when the layout grew. c->world / c->morph_w / c->local_q name it under the current counts afterwards.
static int take_pose_block(rz_ctx *c, bool piped)
{
    pose_leaves_pinned_slots(c);
    if (!piped) {
        point_pose_slot(c, (c->pl.pose_slot & 1) ^ 1);
        return RZ_OK;
    }
    const RzPoseLink &pl = c->pl;
    const size_t Mq = std::max<uint32_t>(c->morphs.M, 1);
    const size_t need = pl.alloc_I * pl.alloc_B * 16 + ((pl.alloc_I * std::max<size_t>(pl.alloc_M, Mq) + 3) / 4 * 4) + pl.alloc_I * pl.alloc_B * 7 + 4;
    if (!pl.big.blk[0] || pl.big.floats < need) {
        RzPoseLink::Big fresh;
        fresh.floats = need;
        for (Scratch<float> &b : fresh.blk) {
            HIP_TRY(b.alloc(need));
            HIP_TRY(hipMemsetAsync(b, 0, need * sizeof(float), c->stream));
        }
        HIP_TRY(fresh.ev.create());
        if (int r = drain(c)) return r;         // (the memsets with it)
        drop_graph(c);
        c->pl.big = std::move(fresh);
    }
    int k = 0;
    if (int r = ring_take(c, c->pl.big.proof, c->pl.big.ev, "big-pose", "big-pose ring", &k)) return r;
    point_pose_at(c, c->pl.big.blk[k]);
    return RZ_OK;
}

// A pose that is copied (or pulled) to the device: it goes through a pinned ring slot into a device block the running frames do not read
// — on the upload stream for big poses, so the upload overlaps whatever the compute stream is still running; the compute stream then
// waits for it. Three steps, shared by rz_set_pose* (the library fills the slot: upload_pose_copy) and rz_map_pose / rz_commit_pose (the
// caller does): copy_begin takes the slot, the slot is filled, copy_send enqueues everything.
static int copy_begin(rz_ctx *c, const PoseParts &pp, int *slot)
{
    return stage_acquire(c, std::max<size_t>((size_t)c->I * c->skel.B * 64 + pp.mwb, pp.mwb + (size_t)c->I * c->skel.B * 28), slot);
}

// Large poses (instanced crowds: MBs) take the upload stream and a block of the big-pose ring (ctx.h): nothing enqueued so far
// reads that block. Small ones that are copied at all (zero_copy = 0, small crowds) go down the compute stream itself, into the
// other of the two pose blocks — measured on C5, the two extra packets of a cross-stream hand-off (marker + barrier) cost 3 us
// more per frame than the copy they hide.
// Overlapped-front protocol (crowds, opt-in): EVERY per-frame input travels on the upload stream and is consumed there,
// by the front kernels — stream order is the only ordering needed, no event at all.
static bool pose_piped(const rz_ctx *c, const PoseParts &pp) { return !c->overlap_on && pp.total > (256u << 10); }
// the stream a pose travels on ...
static hipStream_t pose_stream(const rz_ctx *c, bool piped) { return (piped || c->overlap_on) ? c->up_stream : c->stream; }
// ... and whether what a device-produced pose of one character is made from (a frame number, a motion state with its layers) rides in the
// kernel arguments instead: nothing is uploaded at all
static bool rides_in_arguments(const rz_ctx *c, bool piped) { return c->I == 1 && !piped && !c->overlap_on && c->t_zerocopy != 0; }

// How it crosses the host link (tools/archive/overlapbench, tools/pullbench: profiles/r5_overlapbench.txt, r5_pullbench.txt):
//  * world matrices of a crowd are PULLED out of the slot by rz_pull_pose_kernel (kernels/front.hip), three rows per bone: the
//    upload is what such a frame is bound by (3.28 MB: 84 us per hipMemcpyAsync back to back, 62 us pulled, 47 us pulled as rows),
//    and that the pull's 16 workgroups slow a concurrent skin kernel down (27 -> 35 us) hides under it;
//  * local rotations (a quarter of the bytes) are shorter than the frame they run under: the copy engine leaves that frame alone
//    (27.7 us per frame with the copy running, 35.5 us with the pull), so they stay with hipMemcpyAsync ("pose_pull" = 1 pulls them too).
static bool pose_pullable(const rz_ctx *c, const PoseParts &pp, int slot)
{
    return (pose_piped(c, pp) || c->overlap_on) && c->pl.stage.slot[slot].dev && (pp.total & 3u) == 0;
}

// `rows`: the slot holds the world matrices as 48 B per bone (pack_rows_avx512's layout) followed by the weights; otherwise the pose in
// lay_out_pose's layout. `pull`: rz_pull_pose_kernel instead of hipMemcpyAsync (always with `rows`).
static int copy_send(rz_ctx *c, const PoseParts &pp, int slot, bool pull, bool rows)
{
    const bool piped = pose_piped(c, pp);
    hipStream_t us = pose_stream(c, piped);
    if (int r = take_pose_block(c, piped)) return r;
    void *dst = pp.local ? static_cast<void *>(c->morph_w) : static_cast<void *>(c->world);
    const size_t bones = (size_t)c->I * c->skel.B;
    if (pull) HIP_TRY(rz_launch_pull_pose(c->pl.stage.slot[slot].dev, dst, rows ? (uint32_t)bones : 0u, rows ? pp.total - pp.pbytes : pp.total, us));
    else HIP_TRY(hipMemcpyAsync(dst, c->pl.stage.slot[slot].host, pp.total, hipMemcpyHostToDevice, us));
    c->pl.last_pulled = pull; c->pl.last_rows = rows;
    return staged_sent(c, slot, us, piped);
}

static int upload_pose_copy(rz_ctx *c, const PoseParts &pp)
{
    int slot = 0;
    if (int r = copy_begin(c, pp, &slot)) return r;
    char *st = static_cast<char *>(c->pl.stage.slot[slot].host);
    const bool pull = pose_pullable(c, pp, slot) && (c->t_pull == 1 || (c->t_pull < 0 && !pp.local));
    const size_t bones = (size_t)c->I * c->skel.B;
    bool rows = false;
    if (pull && !pp.local && can_pack_rows()) {
        rows = pack_rows_avx512(static_cast<const float *>(pp.primary), bones, reinterpret_cast<float *>(st));
        if (rows && c->morphs.M > 0) lay_out_weights(pp, st + bones * 48);
    }
    if (!rows) lay_out_pose(c, pp, st);     // (a matrix that is not affine: the whole pose as it was handed over)
    return copy_send(c, pp, slot, pull, rows);
}

// A pose of another kind is about to replace the current one — what that does to the context BEFORE its bytes move: the pose kind decides
// the plan, the plan decides which stream protocol the frame (and therefore this upload) follows.
static int pose_begins(rz_ctx *c, bool local, bool local_t = false, bool sampled = false)
{
    RzPoseLink::Current &p = c->pl.cur;
    p.set = false;
    p.local = local; p.local_t = local_t; p.sampled = sampled;
    c->fk_stale = false;                // (it spoke of the pose this one replaces: rz_read_world / rz_read_palette must not solve THAT on demand any more)
    Plan upl;
    if (int r = frame_plan(c, &upl)) return r;          // the plan frames will use (run lists first), not the whole-palette fallback
    return set_overlap(c, want_overlap(c, upl));
}

static PoseParts pose_parts(const rz_ctx *c, const void *primary, size_t pbytes, const void *secondary, size_t sbytes, bool local, const float *morph_weights)
{
    PoseParts pp;
    pp.primary = primary; pp.pbytes = pbytes; pp.secondary = secondary; pp.sbytes = sbytes; pp.morph_weights = morph_weights; pp.local = local;
    pp.mb = (size_t)c->I * c->morphs.M * sizeof(float);
    pp.mwb = ((size_t)c->I * std::max<uint32_t>(c->morphs.M, 1) + 3) / 4 * 4 * sizeof(float);
    pp.total = local ? pp.mwb + pbytes + sbytes : pbytes + (c->morphs.M > 0 ? pp.mwb : 0);
    return pp;
}

static bool pose_zero_copy(const rz_ctx *c, const PoseParts &pp) { return !c->overlap_on && c->I == 1 && pp.total <= (256u << 10) && c->t_zerocopy != 0; }

// The pose is in place. `morph_weights`: the weight vector the host handed over (null: all zero) — the non-zero weights of instance 0 are
// compacted, in order, for the one-launch path; `on_device`: the weights only exist on the device — the prep kernel compacts them.
static void pose_in_place(rz_ctx *c, const float *morph_weights, bool on_device = false)
{
    RzMorphList &ml = c->pl.cur.ml;
    memset(&ml, 0, sizeof ml);
    if (c->morphs.M > 0 && morph_weights && c->I == 1) {
        int n = 0;
        for (uint32_t m = 0; m < c->morphs.M; ++m) {
            const float w = morph_weights[m];
            if (w == 0.0f) continue;
            // (24-bit dense planes: the listed weight carries the morph's scale — exact, a power of two; kernels/common.hip.h)
            if (n < kKargMorphs) { ml.idx[n] = m; ml.w[n] = c->morphs.dense_fold_host.empty() ? w : w * c->morphs.dense_fold_host[m]; }
            ++n;
        }
        ml.count = n <= kKargMorphs ? n : -1;
    }
    if (on_device && c->morphs.M > 0) ml.count = -1;
    c->pl.cur.I = c->I;
    c->pl.cur.set = true;
}

// Shared tail of rz_set_pose / rz_set_pose_local.
static int upload_pose(rz_ctx *c, const void *primary, size_t pbytes, const void *secondary, size_t sbytes, bool local,
                       const float *morph_weights)
{
    c->pl.map.layout = -1;              // a pose handed over whole cancels a mapping that was never committed
    if (int r = pose_begins(c, local, sbytes != 0)) return r;
    const PoseParts pp = pose_parts(c, primary, pbytes, secondary, sbytes, local, morph_weights);
    int rc = RZ_ERR_UNSUPPORTED, zs = 0;
    if (pose_zero_copy(c, pp)) {
        rc = zc_open(c, pp, &zs);
        if (rc == RZ_ERR_UNSUPPORTED) c->t_zerocopy = 0;      // no pinned device-mapped memory: from now on every pose is copied
        if (rc == RZ_OK) {
            lay_out_pose(c, pp, static_cast<char *>(c->pl.zc.slot[zs].host));
            zc_publish(c, pp, zs, c->pl.zc.proof.uploads);      // (already this upload's index + 1)
        }
    }
    if (rc == RZ_ERR_UNSUPPORTED) rc = upload_pose_copy(c, pp);
    if (rc) return rc;
    pose_in_place(c, morph_weights);
    return RZ_OK;
}

#ifdef RZ_ALL_VARIANTS
// tools-only build (make variants), test hook — not part of the C ABI: the host-side packing loop of a crowd's world matrices on its own
// (no GPU involved), so that the CPU suite can hold it to its contract. Returns 1 = packed, 0 = some bottom row is not 0 0 0 1 (the pose
// would travel whole), -1 = this host cannot pack (no AVX-512).
__attribute__((visibility("default"))) int rz_debug_pack_rows(const float *world16, uint32_t bones, float *rows12)
{
    if (!can_pack_rows()) return -1;
    return pack_rows_avx512(world16, bones, rows12) ? 1 : 0;
}
#endif

int rz_set_pose(rz_ctx *c, const float *world, const float *morph_weights)
{
    if (int r = use(c)) return r;
    if (c->skel.B == 0) return fail(RZ_ERR_INVALID, "no skeleton uploaded");
    if (!world) return fail(RZ_ERR_INVALID, "null world matrices");
    if (int r = ensure_pose_buffers(c)) return r;
    return upload_pose(c, world, (size_t)c->I * c->skel.B * 16 * sizeof(float), nullptr, 0, false, morph_weights);
}

// ---- caller-written poses (ABI 7) ----
// rz_map_pose hands out the very memory the next pose upload would have copied the caller's matrices INTO — the next slot of the pinned
// ring a crowd's pull kernel / the copy engine reads (poses of more than 256 KB), or of the zero-copy ring one character's frame reads
// in place — and rz_commit_pose does what is left of rz_set_pose: nothing is packed, nothing is copied on the host. Which ring, and
// whether the slot can hold the 48-byte rows form, is decided at map time from the state the context is in; if that state changed by
// commit time (another instance count, tuning keys) the commit falls back to a plain rz_set_pose FROM the mapped memory (WORLD16) or
// refuses (ROWS12: there is nothing on the host side that could expand the rows).
int rz_map_pose(rz_ctx *c, int layout, float **matrices, float **morph_weights)
{
    if (int r = use(c)) return r;
    if (matrices) *matrices = nullptr;
    if (morph_weights) *morph_weights = nullptr;
    if (!matrices) return fail(RZ_ERR_INVALID, "rz_map_pose: null out pointer");
    if (layout != RZ_POSE_WORLD16 && layout != RZ_POSE_ROWS12) return fail(RZ_ERR_INVALID, "rz_map_pose: layout must be RZ_POSE_WORLD16 or RZ_POSE_ROWS12");
    if (c->skel.B == 0) return fail(RZ_ERR_INVALID, "no skeleton uploaded");
    if (int r = ensure_pose_buffers(c)) return r;
    RzPoseLink::Map &map = c->pl.map;
    map.layout = -1;
    const size_t bones = (size_t)c->I * c->skel.B;
    // (the opt-in overlapped-front protocol moves every per-frame input onto the upload stream and decides that per pose KIND at upload
    // time: such a context hands its poses over with rz_set_pose)
    if (c->t_overlap == 1 || c->overlap_on) return fail(RZ_ERR_UNSUPPORTED, "rz_map_pose: not with the overlapped-front protocol (\"overlap\" = 1); hand the pose over with rz_set_pose");
    const PoseParts pp = pose_parts(c, nullptr, bones * 64, nullptr, 0, false, nullptr);
    char *st = nullptr;
    if (pose_zero_copy(c, pp)) {
        if (layout == RZ_POSE_ROWS12)
            return fail(RZ_ERR_UNSUPPORTED, "rz_map_pose: a pose of %zu bytes is read in place by its frame, which wants whole 4 x 4 matrices: map it as RZ_POSE_WORLD16 (rows are for poses of more than 256 KB)", pp.total);
        // Frames of the RESIDENT pose may be launched between this call and the commit. The ring's reuse proof (pose_ring.h) counts every
        // reader of an earlier upload as launched before this upload's slot was taken — so such a frame must not be the first one of a
        // zero-copy pose, which reads its pinned slot: bring that pose into its device block now (one stream-ordered copy, rare).
        if (c->pl.cur.set)
            if (int r = make_resident(c)) return r;
        int zs = 0;
        const int rc = zc_open(c, pp, &zs);
        if (rc == RZ_OK) { map.zc = true; map.slot = zs; map.upload = c->pl.zc.proof.uploads; st = static_cast<char *>(c->pl.zc.slot[zs].host); }
        else if (rc == RZ_ERR_UNSUPPORTED) c->t_zerocopy = 0;       // no pinned device-mapped memory: from now on every pose is copied
        else return rc;
    }
    if (!st) {
        int slot = 0;
        if (int r = copy_begin(c, pp, &slot)) return r;
        if (layout == RZ_POSE_ROWS12 && !(pose_pullable(c, pp, slot) && c->t_pull != 0))
            return fail(RZ_ERR_UNSUPPORTED, "rz_map_pose: rows need the pull kernel (a pose of more than 256 KB, a device-mapped ring, \"pose_pull\" != 0): map this pose as RZ_POSE_WORLD16");
        map.zc = false; map.slot = slot;
        st = static_cast<char *>(c->pl.stage.slot[slot].host);
    }
    const size_t mat_bytes = bones * (layout == RZ_POSE_ROWS12 ? 48 : 64);
    if (c->morphs.M > 0) {
        lay_out_weights(pp, st + mat_bytes);        // weights the caller does not write are zero
        if (morph_weights) *morph_weights = reinterpret_cast<float *>(st + mat_bytes);
    }
    *matrices = reinterpret_cast<float *>(st);
    map.layout = layout; map.I = c->I; map.B = c->skel.B; map.M = c->morphs.M; map.ptr = st;
    return RZ_OK;
}

int rz_commit_pose(rz_ctx *c)
{
    if (int r = use(c)) return r;
    RzPoseLink::Map &map = c->pl.map;
    if (map.layout < 0) return fail(RZ_ERR_INVALID, "rz_commit_pose without rz_map_pose (a pose call in between cancels a mapping)");
    const bool rows = map.layout == RZ_POSE_ROWS12;
    map.layout = -1;
    if (map.I != c->I || map.B != c->skel.B || map.M != c->morphs.M) return fail(RZ_ERR_INVALID, "rz_commit_pose: the crowd, skeleton or morph set changed since rz_map_pose");
    const size_t bones = (size_t)c->I * c->skel.B;
    char *st = map.ptr;
    const float *mw = c->morphs.M > 0 ? reinterpret_cast<const float *>(st + bones * (rows ? 48 : 64)) : nullptr;
    const PoseParts pp = pose_parts(c, nullptr, bones * 64, nullptr, 0, false, nullptr);
    // the same decisions as at map time, on the state as it is NOW (a context under the overlapped-front protocol was refused at map time
    // and a world-matrix pose never switches it on by itself) — all of them BEFORE anything is changed: a refused commit leaves the
    // resident pose as it was
    if (c->t_overlap == 1 || c->overlap_on) return fail(RZ_ERR_UNSUPPORTED, "rz_commit_pose: the overlapped-front protocol was switched on since rz_map_pose; hand the pose over with rz_set_pose");
    const bool zc_now = pose_zero_copy(c, pp);
    bool same = map.zc ? (zc_now && c->pl.zc.slot[map.slot].host == static_cast<void *>(st) && c->pl.zc.proof.uploads == map.upload)
                       : (!zc_now && c->pl.stage.slot[map.slot].host == static_cast<void *>(st));
    const bool pull = !map.zc && same && pose_pullable(c, pp, map.slot) && c->t_pull != 0;       // ("pose_pull" = 0 since the map: rows are refused below)
    if (rows && !pull) same = false;
    if (!same) {
        if (rows) return fail(RZ_ERR_UNSUPPORTED, "rz_commit_pose: the context changed since rz_map_pose and this pose can no longer be pulled as rows: map it again");
        // a plain rz_set_pose out of the mapped memory (the slot it takes is the NEXT one of its ring, never the source)
        return upload_pose(c, st, bones * 64, nullptr, 0, false, mw);
    }
    if (int r = pose_begins(c, false)) return r;
    if (map.zc) zc_publish(c, pp, map.slot, map.upload);
    else if (int r = copy_send(c, pp, map.slot, pull, rows)) return r;
    pose_in_place(c, mw);
    return RZ_OK;
}

int rz_set_pose_local(rz_ctx *c, const float *local_rotations4, const float *local_translations3, const float *morph_weights)
{
    if (int r = use(c)) return r;
    if (!c->fk.has_topology) return fail(RZ_ERR_INVALID, "rz_upload_skeleton_topology has not been called for this skeleton");
    if (!local_rotations4) return fail(RZ_ERR_INVALID, "null local rotations");
    if (int r = ensure_pose_buffers(c)) return r;
    const size_t nq = (size_t)c->I * c->skel.B;
    return upload_pose(c, local_rotations4, nq * sizeof(float4), local_translations3, local_translations3 ? nq * 3 * sizeof(float) : 0, true,
                       morph_weights);
}

int rz_set_pose_sampled(rz_ctx *c, const float *frames)
{
    if (int r = use(c)) return r;
    if (!c->has_animation) return fail(RZ_ERR_INVALID, "rz_upload_animation has not been called");
    if (!c->fk.has_topology) return fail(RZ_ERR_INVALID, "rz_upload_skeleton_topology has not been called for this skeleton");
    if (c->an.M != c->morphs.M) return fail(RZ_ERR_INVALID, "the motion's morph feeds were built for %u vertex morphs, the context holds %u", c->an.M, c->morphs.M);
    if (!frames) return fail(RZ_ERR_INVALID, "null frames");
    // refused before anything of the resident pose is touched (the wording of rz_set_pose_blended): the span guess turns the frame into a
    // key index, which is undefined for a NaN or an infinite frame
    for (uint32_t i = 0; i < c->I; ++i)
        if (!rzmotion::finite(frames[i])) return fail(RZ_ERR_INVALID, "instance %u: a frame that would be sampled is not finite", i);
    IkWordsPlan sw;
    if (c->ik.n && c->ik_keys_an.resident) {        // the motion's IK on/off keys: every instance's switches at its frame
        const uint32_t W = ik_sw_words(c);
        std::vector<uint32_t> w((size_t)c->I * W);
        for (uint32_t i = 0; i < c->I; ++i) ik_row_into(c, ik_state_at(c->ik_keys_an, W, frames[i]), &w[(size_t)i * W]);
        if (int r = plan_ik_words(c, c->I, std::move(w), &sw)) return r;
    }
    if (int r = ensure_pose_buffers(c)) return r;
    RzPoseLink &pl = c->pl;
    if (int r = grow(c, pl.an_frames.to(c->I))) return r;
    if (int r = pose_begins(c, true, true, true)) return r;
    pose_leaves_pinned_slots(c);            // the pose is produced on the device: its frame writes world matrices / weights into the pose block
    pl.cur.frames_inline = rides_in_arguments(c, false);
    if (pl.cur.frames_inline) {
        pl.cur.frame0 = frames[0];          // one character: the frame number rides in rz_fk_kernel's arguments
    } else {
        int slot = 0;
        if (int r = stage_acquire(c, std::max<size_t>((size_t)c->I * sizeof(float), 4096), &slot)) return r;
        memcpy(pl.stage.slot[slot].host, frames, (size_t)c->I * sizeof(float));
        hipStream_t us = front_stream(c);   // consumed by rz_fk_kernel, which runs on this stream
        HIP_TRY(hipMemcpyAsync(pl.an_frames, pl.stage.slot[slot].host, (size_t)c->I * sizeof(float), hipMemcpyHostToDevice, us));
        if (int r = staged_sent(c, slot, us, false)) return r;
    }
    point_pose_slot(c, pl.pose_slot);       // the sampled pose is written by rz_fk_kernel under the current counts
    if (int r = commit_ik_words(c, sw)) return r;
    pose_in_place(c, nullptr, true);
    return RZ_OK;
}

// A pose blended on the device out of the motion library (kernels/motion.hip). It takes the pose block a COPIED local pose of the same size
// would take — the other block of pose_blk, or a block of the big-pose ring above 256 KB — and rz_motion_kernel writes it there on the
// stream that copy would have travelled on, followed by the event that copy would have recorded (copy_send). The context is left exactly as
// after such a copy: a resident local pose with translations. A state that is refused is refused before anything of the resident pose is
// touched; a device error after that (a staging slot, a block of the ring) leaves the context without a pose, as it does in rz_upload_pose.
static_assert(sizeof(rz_motion_state) == sizeof(RzMotionState) && sizeof(RzMotionState) == 20, "rz_motion_state is RzMotionState");
static int check_motion_states(const rz_ctx *c, const RzMotionState *sv)
{
    for (uint32_t i = 0; i < c->I; ++i) {
        const RzMotionState &s = sv[i];
        if (!rzmotion::finite(s.blend) || s.blend < 0.0f || s.blend > 1.0f) return fail(RZ_ERR_INVALID, "instance %u: blend %g is not in [0, 1]", i, (double)s.blend);
        const bool has_b = s.clip_b != kRzNoClip && s.blend != 0.0f, use_a = !(has_b && s.blend == 1.0f);
        if (s.clip_a >= c->lib.clips) return fail(RZ_ERR_INVALID, "instance %u: clip_a %u of %u", i, s.clip_a, c->lib.clips);
        if (s.clip_b != kRzNoClip && s.clip_b >= c->lib.clips) return fail(RZ_ERR_INVALID, "instance %u: clip_b %u of %u", i, s.clip_b, c->lib.clips);
        if ((use_a && !rzmotion::finite(s.frame_a)) || (has_b && !rzmotion::finite(s.frame_b))) return fail(RZ_ERR_INVALID, "instance %u: a frame that would be sampled is not finite", i);
    }
    return RZ_OK;
}

// What rz_set_pose_layered checks of the layers, before anything of the resident pose is touched. A skipped layer (no clip, or weight 0) is not
// looked at beyond those two fields.
static_assert(sizeof(rz_motion_layer) == sizeof(RzMotionLayer) && sizeof(RzMotionLayer) == 20, "rz_motion_layer is RzMotionLayer");
static_assert(RZ_MAX_MOTION_LAYERS == kRzMaxLayers && RZ_NO_MASK == kRzNoMask, "the layer constants of the C ABI are the kernel's");
static int check_motion_layers(const rz_ctx *c, uint32_t n_layers, const RzMotionLayer *lv)
{
    for (uint32_t i = 0; i < c->I; ++i)
        for (uint32_t l = 0; l < n_layers; ++l) {
            const RzMotionLayer &y = lv[(size_t)i * n_layers + l];
            if (y.clip == kRzNoClip || y.weight == 0.0f) continue;
            if (!rzmotion::finite(y.weight) || y.weight < 0.0f || y.weight > 1.0f) return fail(RZ_ERR_INVALID, "instance %u layer %u: weight %g is not in [0, 1]", i, l, (double)y.weight);
            if (y.clip >= c->lib.clips) return fail(RZ_ERR_INVALID, "instance %u layer %u: clip %u of %u", i, l, y.clip, c->lib.clips);
            if (y.mode > 1u) return fail(RZ_ERR_INVALID, "instance %u layer %u: mode %u is neither RZ_LAYER_OVERRIDE nor RZ_LAYER_ADDITIVE", i, l, y.mode);
            if (!rzmotion::finite(y.frame)) return fail(RZ_ERR_INVALID, "instance %u layer %u: the frame is not finite", i, l);
            if (y.mask != kRzNoMask) {
                if (y.mask >= c->mk.count) return fail(RZ_ERR_INVALID, "instance %u layer %u: mask %u of %u", i, l, y.mask, c->mk.count);
                if (c->mk.M != c->morphs.M)
                    return fail(RZ_ERR_INVALID, "instance %u layer %u: the masks were built for %u vertex morphs, the context holds %u: upload them again", i, l, c->mk.M, c->morphs.M);
            }
        }
    return RZ_OK;
}

// rz_set_pose_blended and rz_set_pose_layered: one path. `layered` picks the instantiation of rz_motion_kernel (rz_set_pose_blended launches the
// one without layers, as ever) and what travels: the states alone into mo_states, or the states with the layers behind them — I x 20 x (1 + n_layers) bytes, one
// ring slot, one copy — into mo_layers.
static int library_pose(rz_ctx *c, const rz_motion_state *states, bool layered, uint32_t n_layers, const rz_motion_layer *layers)
{
    if (int r = use(c)) return r;
    if (!c->lib.clips) return fail(RZ_ERR_INVALID, "rz_upload_motions has not been called");
    if (!c->fk.has_topology) return fail(RZ_ERR_INVALID, "rz_upload_skeleton_topology has not been called for this skeleton");
    if (c->mo.M != c->morphs.M) return fail(RZ_ERR_INVALID, "the library's morph feeds were built for %u vertex morphs, the context holds %u: upload it again", c->mo.M, c->morphs.M);
    if (!states) return fail(RZ_ERR_INVALID, "null motion states");
    if (n_layers > (uint32_t)kRzMaxLayers) return fail(RZ_ERR_INVALID, "%u layers: at most %d", n_layers, kRzMaxLayers);
    if (n_layers && !layers) return fail(RZ_ERR_INVALID, "null motion layers");
    // The states (and layers) are read once, so that what is checked is what travels: one character's onto the stack (they may ride in the
    // kernel arguments), a crowd's straight into the pinned slot they travel in. A refusal hands that slot back.
    struct { RzMotionState st; RzMotionLayer ly[kRzMaxLayers]; } one;
    const size_t n_rec = (size_t)c->I * (1 + n_layers), n_bytes = n_rec * sizeof(RzMotionState);
    const RzMotionState *sv = &one.st;
    const RzMotionLayer *lv = one.ly;
    int slot = -1;
    auto fill = [&](void *dst) {        // [I] states, then [I][n_layers] layers: records of 20 bytes both
        memcpy(dst, states, (size_t)c->I * sizeof(RzMotionState));
        if (n_layers) memcpy(static_cast<RzMotionState *>(dst) + c->I, layers, (size_t)c->I * n_layers * sizeof(RzMotionLayer));
    };
    if (c->I == 1) {
        memset(&one, 0, sizeof one);
        fill(&one);
    } else {
        if (int r = stage_acquire(c, std::max<size_t>(n_bytes, 4096), &slot)) return r;
        fill(c->pl.stage.slot[slot].host);
        sv = static_cast<const RzMotionState *>(c->pl.stage.slot[slot].host);
        lv = reinterpret_cast<const RzMotionLayer *>(sv + c->I);
    }
    int bad = check_motion_states(c, sv);
    if (!bad && n_layers) bad = check_motion_layers(c, n_layers, lv);
    if (bad) {
        if (slot >= 0) c->pl.stage.next = slot;
        return bad;
    }
    IkWordsPlan sw;
    if (c->ik.n && !c->ik_keys_mo.empty()) {
        // the library's IK on/off keys: clip A's row at frame_a, or from blend 0.5 on clip B's at frame_b (a switch does not cross-fade;
        // layers never switch IK); a chosen clip without keys is all on. Planned here, before the resident pose is touched.
        const uint32_t W = ik_sw_words(c);
        std::vector<uint32_t> w((size_t)c->I * W);
        for (uint32_t i = 0; i < c->I; ++i) {
            const RzMotionState &s = sv[i];
            const bool use_b = s.clip_b != kRzNoClip && !(s.blend < 0.5f);
            const RzIkKeySet &ks = c->ik_keys_mo[use_b ? s.clip_b : s.clip_a];
            ik_row_into(c, ks.resident ? ik_state_at(ks, W, use_b ? s.frame_b : s.frame_a) : nullptr, &w[(size_t)i * W]);
        }
        if (int r = plan_ik_words(c, c->I, std::move(w), &sw)) return r;
    }
    if (int r = ensure_pose_buffers(c)) return r;
    RzPoseLink &pl = c->pl;
    pl.map.layout = -1;                 // a pose handed over whole cancels a mapping that was never committed
    if (int r = pose_begins(c, true, true)) return r;
    const size_t nq = (size_t)c->I * c->skel.B;
    const PoseParts pp = pose_parts(c, nullptr, nq * sizeof(float4), nullptr, nq * 3 * sizeof(float), true, nullptr);
    const bool piped = pose_piped(c, pp);
    hipStream_t us = pose_stream(c, piped);
    const bool inline_state = rides_in_arguments(c, piped);
    if (!inline_state) {
        if (!layered)
            if (int r = grow(c, pl.mo_states.to(c->I))) return r;
        if (layered && n_rec > pl.mo_layers.capacity())
            if (int r = grow(c, pl.mo_layers.to((size_t)c->I * (1 + kRzMaxLayers)))) return r;
        if (pl.mo_states_stream && pl.mo_states_stream != us) HIP_TRY(hipStreamSynchronize(pl.mo_states_stream));     // (the protocol changed: rare)
        pl.mo_states_stream = us;
        if (slot < 0) {
            if (int r = stage_acquire(c, 4096, &slot)) return r;
            memcpy(pl.stage.slot[slot].host, &one, n_bytes);
        }
    }
    if (int r = take_pose_block(c, piped)) return r;
    RzLayerParams lp;
    memset(&lp, 0, sizeof lp);
    RzMotionParams &mp = lp.m;
    if (inline_state) {
        mp.state0 = one.st;
        memcpy(lp.layers0, one.ly, sizeof one.ly);
    } else if (layered) {
        HIP_TRY(hipMemcpyAsync(pl.mo_layers, pl.stage.slot[slot].host, n_bytes, hipMemcpyHostToDevice, us));
        mp.states = reinterpret_cast<const RzMotionState *>(pl.mo_layers.get());
        lp.layers = pl.mo_layers + c->I;
    } else {
        HIP_TRY(hipMemcpyAsync(pl.mo_states, pl.stage.slot[slot].host, (size_t)c->I * sizeof(RzMotionState), hipMemcpyHostToDevice, us));
        mp.states = pl.mo_states;
    }
    mp.bone_rec = c->lib.bone_rec; mp.feed_off = c->mo.feed_off;
    mp.sample = sample_params(c->mo);
    mp.local_q = c->local_q; mp.local_t = reinterpret_cast<float *>(c->local_q + nq); mp.morph_w = c->morph_w;
    mp.B = (int)c->skel.B; mp.M = (int)c->morphs.M;
    if (layered) {
        lp.n_layers = (int)n_layers;
        lp.bone_bits = c->mk.bone_bits; lp.bone_words = (int)c->mk.bone_words;
        lp.morph_bits = c->mk.M == c->morphs.M ? c->mk.morph_bits.get() : nullptr; lp.morph_words = (int)c->mk.morph_words;      // (masks of another morph set: no layer names one)
    }
    HIP_TRY(layered ? rz_launch_motion(lp, c->I, us) : rz_launch_motion(mp, c->I, us));
    pl.last_pulled = false; pl.last_rows = false;
    if (slot >= 0)
        if (int r = staged_sent(c, slot, us, piped)) return r;
    if (int r = commit_ik_words(c, sw)) return r;
    pose_in_place(c, nullptr, true);
    return RZ_OK;
}

int rz_set_pose_blended(rz_ctx *c, const rz_motion_state *states)
{
    return library_pose(c, states, false, 0, nullptr);
}

int rz_set_pose_layered(rz_ctx *c, const rz_motion_state *base, uint32_t n_layers, const rz_motion_layer *layers)
{
    return library_pose(c, base, true, n_layers, layers);
}

int rz_override_world(rz_ctx *c, uint32_t n, const uint32_t *instance, const uint32_t *bone, const float *world16)
{
    if (int r = use(c)) return r;
    if (c->ph.nb) return fail(RZ_ERR_INVALID, "rz_override_world while a physics table is resident: rz_physics_step writes the override table (remove the table with rz_upload_physics(ctx, NULL) first)");
    if (n == 0) { c->ovr_count = 0; c->ovr_off_host.clear(); c->ovr_bone_host.clear(); return RZ_OK; }
    if (!c->fk.has_topology) return fail(RZ_ERR_INVALID, "rz_override_world applies to device-solved poses: call rz_upload_skeleton_topology first");
    if (!bone || !world16) return fail(RZ_ERR_INVALID, "null override arrays");
    // sort by (instance, bone); of several entries for one bone the LAST wins, like successive boneWorldMatrices.set() calls
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = instance ? instance[k] : 0;
        if (i >= c->I || bone[k] >= c->skel.B) return fail(RZ_ERR_INVALID, "override %u names instance %u bone %u (have %u x %u)", k, i, bone[k], c->I, c->skel.B);
        for (int e = 0; e < 16; ++e) {
            if (!rzmotion::finite(world16[(size_t)k * 16 + e])) return fail(RZ_ERR_INVALID, "override %u is not finite", k);
        }
        order[k] = k;
    }
    auto key = [&](uint32_t k) { return (uint64_t)(instance ? instance[k] : 0) * c->skel.B + bone[k]; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    std::vector<int> off(c->I + 1, 0), bones;
    std::vector<float> mats;
    for (uint32_t q = 0; q < n; ++q) {
        if (q + 1 < n && key(order[q + 1]) == key(order[q])) continue;
        const uint32_t k = order[q];
        off[(instance ? instance[k] : 0) + 1]++;
        bones.push_back((int)bone[k]);
        mats.insert(mats.end(), world16 + (size_t)k * 16, world16 + (size_t)k * 16 + 16);
    }
    for (uint32_t i = 0; i < c->I; ++i) off[i + 1] += off[i];
    const size_t m = bones.size();
    if (int r = reserve_overrides(c, m, off.size())) return r;
    // rz_override_follow: per-instance sets differ, so the follower lists are rebuilt with every set and travel with it
    std::vector<int> fol_off;
    std::vector<uint2> fol_ent;
    if (c->ovr_follow) {
        build_followers(c, off, bones, fol_off, fol_ent);
        c->fol_count = 0;
        if (int r = reserve_followers(c, fol_ent.size(), fol_off.size())) return r;
    }
    // one pinned ring slot carries offsets | bones | matrices (| follower offsets | follower entries) down the compute stream, in order
    // with the frames
    const size_t b_off = off.size() * sizeof(int), b_bone = m * sizeof(int), b_mat = m * 16 * sizeof(float);
    const size_t b_pad = (b_off + b_bone + b_mat + 7) & ~(size_t)7, b_foff = fol_off.size() * sizeof(int), b_fent = fol_ent.size() * sizeof(uint2);
    int slot = 0;
    if (int r = stage_acquire(c, std::max<size_t>(b_pad + b_foff + b_fent, 4096), &slot)) return r;
    char *st = static_cast<char *>(c->pl.stage.slot[slot].host);
    memcpy(st, off.data(), b_off);
    memcpy(st + b_off, bones.data(), b_bone);
    memcpy(st + b_off + b_bone, mats.data(), b_mat);
    hipStream_t us = front_stream(c);       // consumed by rz_fk_kernel, which runs on this stream
    HIP_TRY(hipMemcpyAsync(c->ovr_off, st, b_off, hipMemcpyHostToDevice, us));
    HIP_TRY(hipMemcpyAsync(c->ovr_bone, st + b_off, b_bone, hipMemcpyHostToDevice, us));
    HIP_TRY(hipMemcpyAsync(c->ovr_world, st + b_off + b_bone, b_mat, hipMemcpyHostToDevice, us));
    if (c->ovr_follow) {
        memcpy(st + b_pad + b_fent, fol_off.data(), b_foff);        // (the 8-byte entries first: aligned)
        HIP_TRY(hipMemcpyAsync(c->fol_off, st + b_pad + b_fent, b_foff, hipMemcpyHostToDevice, us));
        if (b_fent) {
            memcpy(st + b_pad, fol_ent.data(), b_fent);
            HIP_TRY(hipMemcpyAsync(c->fol_ent, st + b_pad, b_fent, hipMemcpyHostToDevice, us));
        }
    }
    if (int r = staged_sent(c, slot, us, false)) return r;
    c->ovr_count = (uint32_t)m;
    if (c->ovr_follow) c->fol_count = (uint32_t)fol_ent.size();
    c->ovr_off_host = std::move(off); c->ovr_bone_host = std::move(bones);
    return RZ_OK;
}

int rz_override_follow(rz_ctx *c, uint32_t on)
{
    if (int r = use(c)) return r;
    if (on > 1) return fail(RZ_ERR_INVALID, "rz_override_follow: on must be 0 or 1 (got %u)", on);
    if (!c->fk.has_topology || c->fk.host.size() != (size_t)c->skel.B * 4)
        return fail(RZ_ERR_INVALID, "rz_override_follow needs the hierarchy: call rz_upload_skeleton_topology first");
    if ((int)on == c->ovr_follow) return RZ_OK;
    if (int r = drain(c)) return r;
    drop_graph(c);
    c->fol_count = 0;
    if (on) {
        // an override set is resident: its follower lists now (a later set brings its own). A physics table's set is laid out with its
        // per-instance buffers and outlives a reset, so it counts as resident once those exist for the current crowd.
        if (c->ph.nb && c->ph.state && c->ph.I == c->I) {
            const size_t I = c->I, nd = c->ph.nd;
            std::vector<int> off(I + 1), bones(I * nd);
            for (size_t i = 0; i <= I; ++i) off[i] = (int)(i * nd);
            for (size_t i = 0; i < I; ++i)
                for (size_t k = 0; k < nd; ++k) bones[i * nd + k] = c->ph.dyn_bone[k];
            if (int r = upload_followers(c, off, bones)) return r;
        } else if (!c->ph.nb && c->ovr_count) {
            if (int r = upload_followers(c, c->ovr_off_host, c->ovr_bone_host)) return r;
        }
    }
    c->ovr_follow = (int)on;
    if (c->ovr_count) c->fk_stale = true;       // world matrices and palettes in memory are the other setting's: rz_read_world / rz_read_palette solve again
    return RZ_OK;
}

int rz_set_ik_enabled(rz_ctx *c, const uint8_t *enabled)
{
    if (int r = use(c)) return r;
    if (!c->ik.n) return fail(RZ_ERR_INVALID, "rz_set_ik_enabled: no IK table is resident (rz_upload_ik)");
    std::vector<uint32_t> w;
    if (enabled) {
        const uint32_t W = ik_sw_words(c), n = c->ik.n;
        w.assign((size_t)c->I * W, 0u);
        for (uint32_t i = 0; i < c->I; ++i)
            for (uint32_t k = 0; k < n; ++k)
                if (enabled[(size_t)i * n + k]) { const uint32_t d = c->ik.dev_pos[k]; w[(size_t)i * W + (d >> 5)] |= 1u << (d & 31u); }
    }
    return set_ik_words(c, std::move(w));
}

int rz_read_ik_enabled(rz_ctx *c, uint8_t *out)
{
    if (int r = use(c)) return r;
    if (!c->ik.n) return fail(RZ_ERR_INVALID, "rz_read_ik_enabled: no IK table is resident (rz_upload_ik)");
    if (!out) return fail(RZ_ERR_INVALID, "rz_read_ik_enabled: null out");
    const uint32_t W = ik_sw_words(c), n = c->ik.n;
    for (uint32_t i = 0; i < c->I; ++i)
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t d = c->ik.dev_pos[k];
            out[(size_t)i * n + k] = c->iksw.words.empty() ? 1 : (uint8_t)((c->iksw.words[(size_t)i * W + (d >> 5)] >> (d & 31u)) & 1u);
        }
    return RZ_OK;
}

int rz_read_world(rz_ctx *c, uint32_t instance, float *world16)
{
    if (int r = use(c)) return r;
    if (instance >= c->I || !world16 || !c->world) return fail(RZ_ERR_INVALID, "bad world read");
    const RzPoseLink::Current &p = c->pl.cur;
    if (p.zc_slot >= 0 && !p.zc_local && !p.world_resident) {     // a zero-copy pose no frame has consumed yet: still in its pinned slot
        memcpy(world16, c->pl.zc.slot[p.zc_slot].host, (size_t)c->skel.B * 16 * sizeof(float));
        return RZ_OK;
    }
    if (solve_on_demand(c)) {                           // a crowd frame that solved its hierarchy in LDS only: the solve as a kernel of its own, now
        if (int r = launch_fk(c, c->stream)) return r;
    }
    if (int r = drain(c)) return r;        // rz_fk_kernel may have written them on the front stream
    HIP_TRY(hipMemcpy(world16, c->world + (size_t)instance * c->skel.B * 16, (size_t)c->skel.B * 16 * sizeof(float), hipMemcpyDeviceToHost));
    return RZ_OK;
}

}  // extern "C"
