// frame.cpp — launching frames: front kernels + the deform / skin kernel, replay (hipGraph), two streams, timing, readbacks (ctx.h).
#include "ctx.h"

using namespace rzi;

namespace rzi {

int check_ready(rz_ctx *c)
{
    if (c->mesh.V == 0 || !c->mesh.geom) return fail(RZ_ERR_INVALID, "no mesh uploaded (rz_upload_mesh)");
    if (c->skel.B == 0 || !c->skel.inv_bind) return fail(RZ_ERR_INVALID, "no skeleton uploaded (rz_upload_skeleton)");
    if (!c->pl.cur.set) return fail(RZ_ERR_INVALID, "no pose set (rz_set_pose)");
    return RZ_OK;
}

// The hierarchy solve of the resident pose with the stages solve_stages lists (plan.cpp), then the after-physics launch behind it on the
// same stream if listed. The launchers refuse what does not fit; the LDS refusals are made here first, where they can say why.
int launch_fk(rz_ctx *c, hipStream_t st, bool overrides)
{
    const RzFkParams fp = fk_params(c, overrides);
    const RzFkStages ss = solve_stages(c, overrides);
    const size_t lds = rz_fk_lds_bytes(fp, ss);
    if (lds > rzlds::kCuLds)
        return fail(RZ_ERR_UNSUPPORTED, "skeleton too large for the hierarchy solve%s on the device: %u bones need %zu B of LDS (%s; the limit is 160 KB)", ss.ik.n_chains ? " with IK" : "", c->skel.B, lds,
                    ss.ik.n_chains ? "156 B per bone + the pose's morph weights: the IK stage keeps the local pose alive beside both matrix buffers" : "108 B per bone + the pose's morph weights");
    HIP_TRY(rz_launch_fk(fp, ss, c->I, st));
    if (ss.af.n) {
        const size_t after_lds = rzafter::lds_bytes(c->skel.B, (uint32_t)ss.af.n);
        if (after_lds > rzlds::kCuLds)
            return fail(RZ_ERR_UNSUPPORTED, "skeleton too large for the after-physics stage on the device: %u bones x 48 B + %d entries x 1 B = %zu B of LDS (the limit is 160 KB)", c->skel.B, ss.af.n, after_lds);
        HIP_TRY(rz_launch_fk_after(fp, ss.af, c->I, st));
    }
    c->palette_stale = false; c->fk_stale = false;
    return RZ_OK;
}

int launch_prep(rz_ctx *c, hipStream_t st)
{
    HIP_TRY(rz_launch_prep(prep_params(c), c->I, st));
    c->palette_stale = false;
    return RZ_OK;
}

// rz_read_world / rz_read_palette after a crowd frame that solved its hierarchy in LDS only (fk_stale): the solve runs as a kernel of its
// own — but only while the device-animated pose that frame deformed is still the current one. A new pose, skeleton or topology clears the
// flag where it goes away (upload_pose, rz_set_pose_sampled, rz_upload_skeleton*); this is the second lock on the same door: rz_fk_kernel
// on a pose block that holds world matrices, or on the records of a replaced skeleton, would overwrite the resident pose.
bool solve_on_demand(const rz_ctx *c) { return c->fk_stale && c->pl.cur.local && c->fk.has_topology && c->pl.cur.set && c->fk.rec; }

// Everything a frame launches in front of the deform kernel: on-device FK (local-rotation poses) and/or the prep
// kernel. The FK kernel already writes the palette, so prep is only still needed for its morph compaction.
// (a frame whose deform / crowd kernel solves the hierarchy itself has none: pl.fuse_fk, pl.subfk — RzFrameKernel::solve)
bool has_front(const rz_ctx *c, const Plan &pl) { return (pl.prep || c->pl.cur.local) && !pl.fuse_fk && !pl.subfk; }

int launch_front(rz_ctx *c, const Plan &pl, hipStream_t st)
{
    if (!has_front(c, pl)) return RZ_OK;
    if (c->pl.cur.local) {
        if (int r = launch_fk(c, st)) return r;
        if (pl.prep && c->morphs.mode == 1)
            if (int r = launch_prep(c, st)) return r;
        return RZ_OK;
    }
    return launch_prep(c, st);
}

// The frame's kernel: frame_kernel (plan.cpp) names the instantiation, rz_launch_frame launches it; then what that family's frame leaves in memory.
int launch_deform(rz_ctx *c, const Plan &pl)
{
    const RzDeformParams p = deform_params(c, pl);
    const RzFrameKernel k = frame_kernel(pl, p);
    const bool one_mesh = k.family == kRzSmall || k.family == kRzDense;
    RzLaunchShape s = { k.family == kRzCrowdReg ? k.poses_per_wg : k.group, (int)c->I, pl.verts_per_wg, pl.grid_x, (size_t)pl.inst_lds };
    if (one_mesh) {
        s.grid_x += p.pf_src ? 1u : 0u;
        s.lds = rz_deform_lds_bytes(p, pl.v);
        if (s.lds > rzlds::kCuLds) return fail(RZ_ERR_UNSUPPORTED, "skeleton too large for the LDS palette (%zu B)", s.lds);
    }
    HIP_TRY(rz_launch_frame(k, p, c->pl.cur.ml, subfk_params(c), s, c->stream));
    if (k.family == kRzCrowdFk) c->fk_stale = true;     // neither world matrices nor palettes of this pose are in memory: formed on demand (rz_read_world / rz_read_palette)
    if (k.family == kRzCrowd && !pl.dma) c->palette_stale = pl.subsets;     // the whole-palette one-launch frame copies its palettes out, the subset form cannot
    if (!one_mesh) return RZ_OK;
    c->palette_stale = false;                          // this frame's palette is in memory: written by its front kernels or by workgroup 0
    if (p.world_copy) c->pl.cur.world_resident = true;        // workgroup 0 of that launch left the pose in the device block
    if (p.morph_w_copy) c->pl.cur.mw_resident = true;
    if (p.fk.copy_q) c->pl.cur.local_resident = c->pl.cur.mw_resident = true;
    if (c->aabb_on) c->aabb_slot ^= 1;     // this launch re-armed the other slot for the next frame
    return RZ_OK;
}

// The passes behind the deform / skin kernel of a frame: SDEF (kernels/sdef.hip) and QDEF (kernels/qdef.hip), each for the vertices its
// table lists. Their parameters are taken BEFORE that launch (sdef_params / qdef_params): the bounding-box slot the frame accumulates
// into, and the morph weights where the frame read them. S is RzSdefParams or RzQdefParams (the frame fields carry the same names).
template <typename S> static void pass_frame_fields(const rz_ctx *c, const Plan &pl, S &s)
{
    s.geom = c->mesh.geom; s.joints01 = c->mesh.j01; s.weights = c->mesh.wq; s.palette = c->palette;
    if (c->morphs.mode != 0 && c->morphs.M > 0) {
        s.mode = c->morphs.mode; s.M = (int)c->morphs.M; s.Mpad = (int)c->morphs.Mpad;
        s.dense = c->morphs.dense; s.dense_fold = s.mode == 1 ? c->morphs.dense_fold.get() : nullptr; s.sp_ptr = c->morphs.sp_ptr; s.sp_entries = c->morphs.sp_entries;
        // The weights where this frame's kernels leave or read them, never a pose block that a later upload may overwrite before the pass
        // runs (under the overlapped-front protocol the next pose goes down the upload stream behind this frame's front):
        //   dense, one-launch frame: its kernel-argument list (the weights may only sit in a pinned slot)
        //   dense behind rz_prep_kernel (every crowd frame, the only frames that overlap): the ring slot's active list
        //   otherwise (a single character's fused-hierarchy frame; sparse targets, which never overlap): the weights themselves — sampled
        //   ones from the device block the front / workgroup 0 wrote, uploaded ones from the device copy workgroup 0 leaves, or where the
        //   frame kernel reads them
        if (s.mode == 1 && pl.v.fast && c->I == 1 && c->pl.cur.ml.count >= 0 && !c->pl.cur.sampled) s.wsrc = 0;
        else if (s.mode == 1 && pl.prep) {
            s.wsrc = 1; s.act_idx = c->act_idx; s.act_w = c->act_w; s.act_count = c->act_count;
        } else {
            s.wsrc = 2;
            const float *copy = deform_params(c, pl).morph_w_copy;
            s.morph_w = c->pl.cur.sampled ? c->morph_w : (copy ? copy : src_morph_w(c));
        }
    }
    s.out_pos = c->ext_pos ? c->ext_pos : c->out_pos; s.out_nrm = c->ext_nrm ? c->ext_nrm : c->out_nrm;
    if (c->edge) { s.edge = c->edge; s.out_hull = c->out_hull; }
    if (c->aabb_on) { s.aabb = c->aabb; s.aabb_slot = c->aabb_slot; }
    s.Vp = c->mesh.Vp; s.B = (int)c->skel.B;
}

RzSdefParams sdef_params(const rz_ctx *c, const Plan &pl)
{
    RzSdefParams s;
    memset(&s, 0, sizeof s);
    if (!c->sdef.tab || c->sdef.n == 0) return s;
    s.tab = c->sdef.tab; s.n = c->sdef.n;
    pass_frame_fields(c, pl, s);
    return s;
}

RzQdefParams qdef_params(const rz_ctx *c, const Plan &pl)
{
    RzQdefParams s;
    memset(&s, 0, sizeof s);
    if (!c->qdef.tab || c->qdef.n == 0) return s;
    s.tab = c->qdef.tab; s.n = c->qdef.n; s.joints23 = c->mesh.j23;
    pass_frame_fields(c, pl, s);
    s.chunks = c->t_qdefchunks > 0 ? c->t_qdefchunks : 1;       // ("qdef_chunks"; the default is the measured one: NOTEBOOK.md, profiles/qdef_cost.txt)
    return s;
}

// Behind the deform / skin kernel on the frame's stream. Crowd forms that formed their palettes in LDS only (palette_stale: the bone-subset
// skin kernel; fk_stale: the one-launch device-animated crowd) get them written first by the palette kernel those flags name, once for
// both passes — crowds of those forms with a table pay that kernel.
int launch_passes(rz_ctx *c, const RzSdefParams &sp, const RzQdefParams &qp)
{
    if (sp.n == 0 && qp.n == 0) return RZ_OK;
    if (solve_on_demand(c) || c->palette_stale) {
        // (never under the overlapped-front protocol: its frames have a front, which writes the ring slot's palettes, and the forms that
        // keep palettes in LDS only have none; a palette kernel here would read the pose block on the wrong stream)
        if (c->overlap_on) return fail(RZ_ERR_INVALID, "SDEF / QDEF pass: an overlapped crowd frame left no palette in memory");
        if (solve_on_demand(c)) {
            if (int r = launch_fk(c, c->stream)) return r;
        } else if (int r = launch_prep(c, c->stream)) return r;
    }
    if (sp.n) HIP_TRY(rz_launch_sdef(sp, c->pl.cur.ml, c->I, c->stream));
    if (qp.n) HIP_TRY(rz_launch_qdef(qp, c->pl.cur.ml, c->I, c->stream));
    return RZ_OK;
}

// the deform / skin kernel of a frame and, when the context has an SDEF or a QDEF table, the passes behind it
static int launch_deform_passes(rz_ctx *c, const Plan &pl)
{
    if (!c->sdef.n && !c->qdef.n) return launch_deform(c, pl);
    const RzSdefParams sp = sdef_params(c, pl);
    const RzQdefParams qp = qdef_params(c, pl);
    if (int r = launch_deform(c, pl)) return r;
    return launch_passes(c, sp, qp);
}

// Crowds overlap the front kernels of a frame with the skin kernel of the frame before it. The protocol
// needs a frame that HAS front kernels and a skin kernel that reads nothing of the pose slots themselves (sparse morph
// frames read the uploaded weights directly), and plain stream capture (the graph key) stays single-stream.
bool want_overlap(const rz_ctx *c, const Plan &pl)
{
    // OPT-IN (overlap = 1): measured on MI355X / ROCm 7.2 the two cross-stream hand-offs per frame cost more than the front
    // kernels they hide — C4 39.0 -> 44.8 us with rz_prep_kernel in front, 43.4 -> 62.1 us with rz_fk_kernel
    return c->t_overlap == 1 && c->I > 1 && c->morphs.mode != 2 && !c->t_graph && has_front(c, pl);
}

// Switching protocols is rare (instance count, tuning keys): drain both streams so that nothing enqueued under the old
// rules is still running when the first frame under the new ones starts.
int set_overlap(rz_ctx *c, bool on)
{
    if (c->overlap_on == on) return RZ_OK;
    if (int r = drain(c)) return r;
    c->overlap_on = on;
    c->skin_recorded[0] = c->skin_recorded[1] = false;
    return RZ_OK;
}

// One whole frame: front kernels (if the plan has any) + the deform / skin kernel.
int run_frame(rz_ctx *c, const Plan &pl)
{
    // rz_prep_kernel (and a skin kernel that is not the one-launch form) reads a device-resident pose
    if (c->pl.cur.zc_slot >= 0 && (pl.prep || (!pl.v.fast && !c->pl.cur.local)))
        if (int r = make_resident(c)) return r;
    if (c->overlap_on) {
        const int s = c->ring_slot ^ 1;                       // the slot the skin kernel of two frames ago read
        if (c->skin_recorded[s]) HIP_TRY(hipStreamWaitEvent(c->up_stream, c->ev_skin[s], 0));
        set_ring(c, s);
        if (int r = launch_front(c, pl, c->up_stream)) return r;
        HIP_TRY(hipEventRecord(c->ev_front[s], c->up_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_front[s], 0));
        if (int r = launch_deform_passes(c, pl)) return r;        // (the SDEF / QDEF passes read the slot's palettes and active lists too: ev_skin goes behind them)
        HIP_TRY(hipEventRecord(c->ev_skin[s], c->stream));
        c->skin_recorded[s] = true;
        return RZ_OK;
    }
    if (int r = launch_front(c, pl, c->stream)) return r;
    return launch_deform_passes(c, pl);
}

// the stream per-frame inputs travel on and front kernels run on
hipStream_t front_stream(const rz_ctx *c) { return c->overlap_on ? c->up_stream : c->stream; }

// What every entry that launches frames does first, behind its own argument checks; leaves the next frame's plan and its stream protocol.
int begin_frames(rz_ctx *c, Plan *pl)
{
    if (int r = use(c)) return r;
    if (int r = check_ready(c)) return r;
    if (int r = ensure_outputs(c)) return r;
    if (int r = frame_plan(c, pl)) return r;
    return set_overlap(c, want_overlap(c, *pl));
}

}  // namespace rzi

extern "C" {

int rz_deform(rz_ctx *c)
{
    Plan pl;
    if (int r = begin_frames(c, &pl)) return r;
    return run_frame(c, pl);
}

// FNV-1a over the plain-data structs a frame's launches are built from: if none of them changed, a captured graph of
// those launches is still the same work.
static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

static uint64_t frame_signature(rz_ctx *c, const Plan &pl)
{
    // every parameter block a frame's launches are built from, whole: device pointers included, so a buffer that was
    // freed and re-allocated (rz_upload_animation, rz_upload_skeleton_topology, a grown pose ring ...) changes the key,
    // and the bounding-box slot parity as it is RIGHT NOW (the captured frames alternate from it)
    uint64_t h = 1469598103934665603ull;
    const RzDeformParams dp = deform_params(c, pl);
    h = fnv(h, &dp, sizeof dp);
    const RzFrameKernel fk = frame_kernel(pl, dp);      // which kernel those launches are
    h = fnv(h, &fk, sizeof fk);
    h = fnv(h, &c->pl.cur.ml, sizeof c->pl.cur.ml);
    h = fnv(h, &pl, sizeof pl);
    const RzPrepParams pp = prep_params(c);
    h = fnv(h, &pp, sizeof pp);
    const RzFkParams fp = fk_params(c);
    h = fnv(h, &fp, sizeof fp);
    const RzSubFk sf = subfk_params(c);
    h = fnv(h, &sf, sizeof sf);
    const RzSdefParams sd = sdef_params(c, pl);
    h = fnv(h, &sd, sizeof sd);
    const RzQdefParams qd = qdef_params(c, pl);
    h = fnv(h, &qd, sizeof qd);
    const RzFkStages ss = solve_stages(c);     // whole and unconditionally: a stage that is off is the same zeros in every frame
    h = fnv(h, &ss, sizeof ss);
    const uint64_t misc[6] = { c->I, c->pl.cur.local, c->pl.cur.local_t, c->pl.cur.sampled, (uint64_t)c->morphs.mode, (uint64_t)c->aabb_on };
    return fnv(h, misc, sizeof misc);
}

constexpr uint32_t kGraphFrames = 16;   // even: the bounding-box slot parity is the same after a replay as before it

int rz_deform_n(rz_ctx *c, uint32_t frames)
{
    Plan pl;
    if (int r = begin_frames(c, &pl)) return r;      // (the overlapped protocol is never on while the graph key is set)
    uint32_t f = 0;
    if (c->t_graph && frames >= 2 * kGraphFrames) {
        // Launch-bound replay (a 30 k-vertex frame is 3-6 us of GPU time per ~3 us of launch work on the host): capture
        // kGraphFrames whole frames once into a hipGraph and replay that; one launch call per 16 frames.
        // The key is taken from the state the capture starts in. A cached graph whose key differs only in the bounding-box
        // slot parity is brought back in phase by one plain frame (which the graph's first build needs anyway: it sets the
        // kernel attributes and loads the modules); kGraphFrames is even, so a replay ends on the parity it began with.
        uint64_t sig = frame_signature(c, pl);
        if (!c->graph_exec || c->graph_sig != sig) {
            if (int r = run_frame(c, pl)) return r;
            ++f;
            sig = frame_signature(c, pl);
        }
        if (!c->graph_exec || c->graph_sig != sig) {
            drop_graph(c);
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            int rc = RZ_OK;
            for (uint32_t k = 0; k < kGraphFrames && rc == RZ_OK; ++k) {
                rc = launch_front(c, pl, c->stream);
                if (rc == RZ_OK) rc = launch_deform_passes(c, pl);
            }
            hipError_t ce = hipStreamEndCapture(c->stream, &g);
            if (rc != RZ_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
            if (ce != hipSuccess || !g) return fail(RZ_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
            hipError_t ie = hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) { c->graph_exec = nullptr; return fail(RZ_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie)); }
            c->graph_sig = sig;
        }
        for (; f + kGraphFrames <= frames; f += kGraphFrames) HIP_TRY(hipGraphLaunch(c->graph_exec, c->stream));
    }
    for (; f < frames; ++f)
        if (int r = run_frame(c, pl)) return r;
    return RZ_OK;
}

int rz_deform_pair(rz_ctx *a, rz_ctx *b, uint32_t frames)
{
    if (!a || !b || a == b) return fail(RZ_ERR_INVALID, "rz_deform_pair needs two different contexts");
    if (a->device != b->device) return fail(RZ_ERR_INVALID, "rz_deform_pair: the contexts live on devices %d and %d", a->device, b->device);
    rz_ctx *cs[2] = { a, b };
    Plan pl[2];
    for (int k = 0; k < 2; ++k)
        if (int r = begin_frames(cs[k], &pl[k])) return r;
    for (uint32_t f = 0; f < frames; ++f)
        if (int r = run_frame(cs[f & 1], pl[f & 1])) return r;
    return RZ_OK;
}

// The K-step span of a benchmark's timed region, by a hipEvent pair ON the stream instead of the host's clock around
// enqueue + synchronize: at 20 steps of a 16.6 us shard frame the host's fixed cost per timed region (first launch, wake-up from the
// final wait: ~30 us, profiles/r6_bench_shard8_steps20.json) is 9 % of the region. `lead` untimed frames go in FRONT of the opening
// event, in the same call: the host enqueues the event and the first timed frames while the GPU is busy with them, so the K timed frames
// run back to back from the first one — a render loop never starts a frame on an idle GPU; without them the first timed frame waits for
// its own launch (~5 us behind the event, another 3 % of 20 shard frames).
int rz_time_span(rz_ctx *a, rz_ctx *b, uint32_t lead, uint32_t frames, double *span_ms)
{
    if (!span_ms || frames == 0) return fail(RZ_ERR_INVALID, "rz_time_span: bad arguments");
    *span_ms = 0.0;
    if (int r = use(a)) return r;
    float ms = 0.f;
    if (!b) {
        if (lead)
            if (int r = rz_deform_n(a, lead)) return r;
        HIP_TRY(hipEventRecord(a->ev0, a->stream));
        if (int r = rz_deform_n(a, frames)) return r;
        HIP_TRY(hipEventRecord(a->ev1, a->stream));
    } else {
        if (a == b || a->device != b->device) return fail(RZ_ERR_INVALID, "rz_time_span needs two different contexts on one device");
        // the span opens on a's stream — behind a's share of the lead frames AND b's (a waits for them) — and b's first timed frame waits
        // for it; it closes on a's stream behind b's last frame
        if (lead) {
            if (int r = rz_deform_pair(a, b, lead + (lead & 1u))) return r;         // (an even count: the timed frames start on a again)
            HIP_TRY(hipEventRecord(b->ev0, b->stream));
            HIP_TRY(hipStreamWaitEvent(a->stream, b->ev0, 0));
        }
        HIP_TRY(hipEventRecord(a->ev0, a->stream));
        HIP_TRY(hipStreamWaitEvent(b->stream, a->ev0, 0));
        if (int r = rz_deform_pair(a, b, frames)) return r;
        HIP_TRY(hipEventRecord(b->ev1, b->stream));
        HIP_TRY(hipStreamWaitEvent(a->stream, b->ev1, 0));
        HIP_TRY(hipEventRecord(a->ev1, a->stream));
    }
    HIP_TRY(hipEventSynchronize(a->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, a->ev0, a->ev1));
    *span_ms = ms;
    return RZ_OK;
}

int rz_read(rz_ctx *c, uint32_t instance, uint32_t v0, uint32_t n, float *pos3, float *nrm3)
{
    if (int r = use(c)) return r;
    if (instance >= c->I) return fail(RZ_ERR_INVALID, "instance %u out of range", instance);
    if ((uint64_t)v0 + n > c->mesh.V) return fail(RZ_ERR_INVALID, "vertex range [%u,%u) exceeds %u", v0, v0 + n, c->mesh.V);
    if (!c->out_pos) return fail(RZ_ERR_INVALID, "nothing deformed yet");
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t off = ((size_t)instance * c->mesh.Vp + v0) * 3;
    const float *sp = c->ext_pos ? c->ext_pos : c->out_pos, *sn = c->ext_nrm ? c->ext_nrm : c->out_nrm;
    if (pos3 && n) HIP_TRY(hipMemcpy(pos3, sp + off, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (nrm3 && n) HIP_TRY(hipMemcpy(nrm3, sn + off, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return RZ_OK;
}

int rz_read_palette(rz_ctx *c, uint32_t instance, float *rows3x4)
{
    if (int r = use(c)) return r;
    if (instance >= c->I || !rows3x4 || !c->palette) return fail(RZ_ERR_INVALID, "bad palette read");
    if (solve_on_demand(c)) {
        // the last frame was a crowd frame that solved its hierarchy in the skin kernel's front: run the solve as a kernel of its own
        // now — the same functions on the same pose, the same bits (kernels/fk.hip.h)
        if (int r = launch_fk(c, c->stream)) return r;
    }
    if (c->palette_stale) {
        // the last frame was a bone-subset crowd frame: its workgroups formed the rows of their own bones in LDS and nobody
        // wrote the skinMatrixBuffer. Form it now from the resident world matrices — rz_prep_kernel's chain is the skin
        // kernel's chain, so these are the bits the frame used.
        if (int r = launch_prep(c, c->stream)) return r;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(rows3x4, c->palette + (size_t)instance * c->skel.B * 3, (size_t)c->skel.B * 12 * sizeof(float), hipMemcpyDeviceToHost));
    return RZ_OK;
}

int rz_read_hull(rz_ctx *c, uint32_t instance, uint32_t v0, uint32_t n, float *pos3)
{
    if (int r = use(c)) return r;
    if (!c->edge || !c->out_hull) return fail(RZ_ERR_INVALID, "the outline hull is off (rz_upload_edge_scale)");
    if (instance >= c->I || (uint64_t)v0 + n > c->mesh.V || !pos3) return fail(RZ_ERR_INVALID, "bad hull read");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(hipMemcpy(pos3, c->out_hull + ((size_t)instance * c->mesh.Vp + v0) * 3, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return RZ_OK;
}

int rz_read_aabb(rz_ctx *c, uint32_t instance, float min_max6[6])
{
    if (int r = use(c)) return r;
    if (!c->aabb_on || !c->aabb) return fail(RZ_ERR_INVALID, "the bounding-box reduction is off (rz_enable_aabb)");
    if (instance >= c->I || !min_max6) return fail(RZ_ERR_INVALID, "bad aabb read");
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t keys[6];
    const int last = c->aabb_slot ^ 1;     // the slot the most recent frame accumulated into
    HIP_TRY(hipMemcpy(keys, c->aabb + ((size_t)instance * 2 + last) * 6, sizeof keys, hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; ++k) {
        const uint32_t bits = (keys[k] & 0x80000000u) ? (keys[k] ^ 0x80000000u) : ~keys[k];
        memcpy(&min_max6[k], &bits, 4);
    }
    return RZ_OK;
}

int rz_time_frames(rz_ctx *c, uint32_t frames, rz_timing *out)
{
    if (int r = use(c)) return r;
    if (!out || frames == 0) return fail(RZ_ERR_INVALID, "rz_time_frames: bad arguments");
    Plan pl;
    if (int r = begin_frames(c, &pl)) return r;
    memset(out, 0, sizeof *out);
    float ms = 0.f;
    // whole frames (front kernels when the plan has any + the deform / skin kernel), back to back exactly as rz_deform
    // issues them — for crowds that is the overlapped protocol: fronts on the upload stream, skin kernels on the
    // context's stream (the events below sit on the context's stream; the last skin kernel waits for the last front)
    if (int r = run_frame(c, pl)) return r;       // the deform-only loop below needs a palette
    if (int r = drain(c)) return r;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (uint32_t f = 0; f < frames; ++f)
        if (int r = run_frame(c, pl)) return r;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    out->frame_ms = ms / frames;
    // the deform / skin kernel alone (reads the ring slot the last frame left current), with the SDEF / QDEF passes when there is a table
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (uint32_t f = 0; f < frames; ++f)
        if (int r = launch_deform_passes(c, pl)) return r;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    out->deform_kernel_ms = ms / frames;
    // the front kernels alone (only part of the frame when the plan is not the one-launch FAST form); everything has
    // drained at this point, so they may run on the context's stream whatever the protocol
    if (has_front(c, pl)) {
        HIP_TRY(hipStreamSynchronize(c->up_stream));
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        for (uint32_t f = 0; f < frames; ++f)
            if (int r = launch_front(c, pl, c->stream)) return r;
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        HIP_TRY(hipEventSynchronize(c->ev1));
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        out->prep_kernel_ms = ms / frames;
    }
    c->skin_recorded[0] = c->skin_recorded[1] = false;      // both streams are idle: no slot has a reader in flight
    out->verts_per_frame = (uint64_t)c->mesh.V * c->I;
    out->algorithmic_bytes_per_frame = algorithmic_bytes(c);
    out->frames = frames;
    return RZ_OK;
}

#ifdef RZ_ALL_VARIANTS
// tools-only build (make variants), test hook — not part of the C ABI. close = 1: everything enqueued on the context's stream from
// here on waits behind a gate kernel; close = 0: the gate opens. (tests: frames are queued behind the gate, the NEXT pose is
// uploaded, the gate opens — the prefetch helper of the queued frame then finds that pose complete by construction.)
__attribute__((visibility("default"))) int rz_debug_gate(rz_ctx *c, int close)
{
    if (int r = use(c)) return r;
    if (!c->gate_host) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c->gate_host), 64, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->gate_dev), c->gate_host, 0));
        *c->gate_host = 1u;
    }
    if (close) {
        HIP_TRY(hipStreamSynchronize(c->stream));       // an earlier gate kernel has gone
        *reinterpret_cast<volatile uint32_t *>(c->gate_host) = 0u;
        std::atomic_thread_fence(std::memory_order_seq_cst);
        HIP_TRY(rz_launch_gate(c->gate_dev, c->stream));
    } else {
        std::atomic_thread_fence(std::memory_order_seq_cst);
        *reinterpret_cast<volatile uint32_t *>(c->gate_host) = 1u;
    }
    return RZ_OK;
}
#endif

#ifdef RZ_ABLATE
// tools-only build (make ablate): per-wave timeline of the frames that follow (tools/archive/timeline.py). Not part of the C ABI.
__attribute__((visibility("default"))) int rz_debug_timeline_arm(rz_ctx *c, uint32_t *waves)
{
    if (int r = use(c)) return r;
    Plan pl;
    if (int r = frame_plan(c, &pl)) return r;
    const size_t wpw = pl.inst_group > 0 ? (size_t)pl.inst_block / 64 : 4;
    const size_t groups = pl.inst_group > 0 ? (c->I + pl.inst_group - 1) / pl.inst_group : c->I;
    const size_t n = ((size_t)pl.grid_x + 1) * groups * wpw;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int r = grow(c, c->tl.to(n * 16))) return r;
    HIP_TRY(hipMemset(c->tl, 0, c->tl.capacity() * sizeof(unsigned long long)));
    c->t_dbg = 100;
    drop_graph(c);
    if (waves) *waves = (uint32_t)n;
    return RZ_OK;
}
__attribute__((visibility("default"))) int rz_debug_timeline_read(rz_ctx *c, unsigned long long *out, uint32_t waves)
{
    if (int r = use(c)) return r;
    if (!c->tl || waves > c->tl.capacity() / 16 || !out) return fail(RZ_ERR_INVALID, "no timeline armed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->tl, (size_t)waves * 128, hipMemcpyDeviceToHost));
    return RZ_OK;
}
#endif

}  // extern "C"
