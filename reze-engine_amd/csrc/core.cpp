// core.cpp — context life cycle, the buffers every unit sizes, error state (part of libreze_deform.so's host side: ctx.h).
//
// One rz_ctx = one MI355X: a HIP stream, the static mesh shard re-laid-out as planar SoA, the skeleton, optional morph targets,
// per-frame pose staging, output buffers, and (optionally) an RCCL communicator for the all-gather of deformed positions. Every entry
// point cites, in the header, the reference call site it replaces; the host side is only plumbing around the kernels in kernels/.
// There is NO CPU fallback: without a working HIP device every call fails.
#include "ctx.h"

#include <cctype>

using namespace rzi;

namespace rzi {

static thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char *last_error() { return g_err.c_str(); }

int use(rz_ctx *c)
{
    if (!c) return fail(RZ_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return RZ_OK;
}

// static data shared between a context and its forks cannot be replaced
int static_unlocked(const rz_ctx *c, const char *what)
{
    if (c->lender) return fail(RZ_ERR_INVALID, "%s on a fork: static data belongs to the context it was forked from", what);
    if (c->n_forks) return fail(RZ_ERR_INVALID, "%s while %d fork(s) of this context share its static data: destroy them first", what, c->n_forks);
    return RZ_OK;
}

// Poll an event (no sleep: a blocking wait wakes tens of microseconds late, which starves a GPU whose frames are 16 us long
// — measured: 36 us per frame). Bounded: a GPU that stops making progress turns into an error after 10 s, not a hang.
int poll_event(hipEvent_t ev, const char *what)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return RZ_OK;
        if (q != hipErrorNotReady) return fail(RZ_ERR_HIP, "%s: %s", what, hipGetErrorString(q));
        if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
            return fail(RZ_ERR_HIP, "%s: the GPU made no progress for 10 s", what);
    }
}

// A captured hipGraph bakes device pointers and launch shapes in. The replay key (frame_signature) covers all of them; on
// top of that every entry point that frees or re-shapes something a frame reads drops the graph outright.
void drop_graph(rz_ctx *c)
{
    if (c->graph_exec) { (void)hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
    c->graph_sig = 0;
}

// nothing this context enqueued is still running: per-frame inputs and front kernels travel on the upload stream, the frame on the compute stream
int drain(rz_ctx *c)
{
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RZ_OK;
}

int ensure_outputs(rz_ctx *c)
{
    // one instance: room for a whole all-gather chunk; instances are strided by Vp
    const size_t need = (c->I == 1) ? std::max<size_t>(c->mesh.Vp, c->chunk) * 3 : (size_t)c->I * c->mesh.Vp * 3;
    if (need == 0) return RZ_OK;
    if (need > c->out_pos.capacity()) {
        if (int r = grow(c, c->out_pos.to(need), c->out_nrm.to(need))) return r;
        HIP_TRY(hipMemsetAsync(c->out_pos, 0, need * sizeof(float), c->stream));
        HIP_TRY(hipMemsetAsync(c->out_nrm, 0, need * sizeof(float), c->stream));
    }
    if (c->edge && need > c->out_hull.capacity()) {
        if (int r = grow(c, c->out_hull.to(need))) return r;
        HIP_TRY(hipMemsetAsync(c->out_hull, 0, need * sizeof(float), c->stream));
    }
    // Bounding-box keys: a frame accumulates into one slot and re-arms the other FOR THE INSTANCES IT LAUNCHES, so the
    // buffer is armed from scratch whenever the reduction is switched on or the instance count changes (aabb_rearm) —
    // otherwise an instance that sat out some frames would come back onto a slot still holding its old extents.
    if (c->aabb_on && ((size_t)c->I * 12 > c->aabb.capacity() || c->aabb_rearm)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int r = grow(c, c->aabb.to((size_t)c->I * 12))) return r;
        std::vector<uint32_t> init(c->aabb.capacity());
        for (size_t i = 0; i < init.size(); ++i) init[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
        HIP_TRY(hipMemcpy(c->aabb, init.data(), init.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->aabb_slot = 0;
        c->aabb_rearm = false;
    }
    return RZ_OK;
}

void set_ring(rz_ctx *c, int slot)
{
    c->ring_slot = slot;
    c->palette = c->palette_ring[slot]; c->act_idx = c->act_idx_ring[slot]; c->act_w = c->act_w_ring[slot]; c->act_count = c->act_count_ring[slot];
}

// Lay the CURRENT instance / bone / morph counts out over pose slot k and make it the current slot.
void point_pose_at(rz_ctx *c, float *block)
{
    const size_t I = c->I, B = c->skel.B, Mq = std::max<uint32_t>(c->morphs.M, 1);
    c->mw_pad = (I * Mq + 3) / 4 * 4;
    c->world = block;
    c->morph_w = block + I * B * 16;
    c->local_q = reinterpret_cast<float4 *>(block + I * B * 16 + c->mw_pad);
}

void point_pose_slot(rz_ctx *c, int k)
{
    c->pl.pose_slot = k;
    point_pose_at(c, c->pl.pose_blk[k]);
}

int ensure_pose_buffers(rz_ctx *c)
{
    if (c->skel.B == 0) return RZ_OK;
    const uint32_t Mq = std::max<uint32_t>(c->morphs.M, 1);
    if (c->I <= c->pl.alloc_I && c->skel.B <= c->pl.alloc_B && Mq <= c->pl.alloc_M && c->world) return RZ_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    for (int k = 0; k < 2; ++k) c->pl.pose_blk[k] = {};
    c->pl.big = {};
    c->world = nullptr; c->morph_w = nullptr; c->local_q = nullptr;
    for (int k = 0; k < 2; ++k) { c->palette_ring[k] = {}; c->act_idx_ring[k] = {}; c->act_w_ring[k] = {}; c->act_count_ring[k] = {}; c->skin_recorded[k] = false; }
    c->palette = nullptr; c->act_idx = nullptr; c->act_w = nullptr; c->act_count = nullptr;
    const size_t I = c->I, B = c->skel.B;
    const size_t Mpad = round_up(Mq + 8, 4);
    const size_t blk_floats = I * B * 16 + ((I * Mq + 3) / 4 * 4) + I * B * 7 + 4;      // + 4: the prefetch helper copies whole 16-byte cells
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c->pl.pose_blk[k].alloc(blk_floats));
        HIP_TRY(hipMemsetAsync(c->pl.pose_blk[k], 0, blk_floats * sizeof(float), c->stream));
    }
    point_pose_slot(c, 0);
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c->palette_ring[k].alloc(I * B * 3));
        HIP_TRY(c->act_idx_ring[k].alloc(I * Mpad));
        HIP_TRY(c->act_w_ring[k].alloc(I * Mpad));
        HIP_TRY(c->act_count_ring[k].alloc(I));
        HIP_TRY(hipMemsetAsync(c->palette_ring[k], 0, I * B * 3 * sizeof(float4), c->stream));
        HIP_TRY(hipMemsetAsync(c->act_idx_ring[k], 0, I * Mpad * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->act_w_ring[k], 0, I * Mpad * sizeof(float), c->stream));
        HIP_TRY(hipMemsetAsync(c->act_count_ring[k], 0, I * sizeof(int), c->stream));
    }
    set_ring(c, 0);
    if (!c->pl.tag) HIP_TRY(c->pl.tag.alloc(2));
    HIP_TRY(hipMemsetAsync(c->pl.tag, 0, 2 * sizeof(uint64_t), c->stream));
    retire_pose_tags(c);                // poses staged under the old layout must never match again
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pl.alloc_I = I; c->pl.alloc_B = B; c->pl.alloc_M = Mq;
    c->pl.cur.set = false;
    return RZ_OK;
}

void free_animation(rz_ctx *c)
{
    drop_graph(c);
    c->an = {};
    c->an_host_range.clear(); c->an_host_mrec.clear();
    c->has_animation = false;
    c->ik_keys_an = {};                 // rz_upload_ik_keys(RZ_NO_CLIP): the keys of this motion
    if (c->pl.cur.sampled) { c->pl.cur.sampled = false; c->pl.cur.set = false; }
}

void free_motions(rz_ctx *c)
{
    if (c->lib.clips) {                   // rz_motion_kernel reads the library on whichever stream the pose travelled on
        if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
    }
    c->mo = {};
    c->lib = {};
    c->ik_keys_mo.clear();              // rz_upload_ik_keys(clip): the keys of this library's clips
}

void free_motion_masks(rz_ctx *c)
{
    if (c->mk.count) {                    // rz_motion_kernel reads the masks on whichever stream the pose travelled on
        if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
    }
    c->mk = {};
}

void free_bone_morphs(rz_ctx *c)
{
    if (c->bm.off) drop_graph(c);
    c->bm = {};
}

// A launch shape found by rz_autotune belongs to the workload it was timed on.
void forget_search(rz_ctx *c)
{
    if (!c->tuned_by_search) return;
    c->t_split = 0; c->t_grid_cap = 0; c->t_instloop = -1;
    c->tuned_by_search = false;
}

void free_sdef(rz_ctx *c)
{
    drop_graph(c);
    c->sdef = {};
}

void free_qdef(rz_ctx *c)
{
    drop_graph(c);
    c->qdef = {};
}

void free_ik(rz_ctx *c)
{
    // chain switches name chains of this table: the mask is all on again and every key set goes
    c->ik_keys_an = {}; c->ik_keys_mo.clear();
    c->iksw.words.clear(); c->iksw.off = 0;
    if (c->ik.n) drop_graph(c);
    c->ik = {};
}

void free_after(rz_ctx *c)
{
    if (c->af.n) drop_graph(c);
    c->af = {};
}

void free_morphs(rz_ctx *c)
{
    forget_search(c);
    drop_graph(c);
    c->morphs = {};
    free_bone_morphs(c);                  // their entries name morphs of the old set
    retire_pose_tags(c);                  // ... and so does a pose staged ahead of its frame
    c->pl.cur.set = false;                // morph weights belong to the old target set
}

}  // namespace rzi

extern "C" {

const char *rz_last_error(void) { return last_error(); }
int rz_abi_version(void) { return RZ_ABI_VERSION; }

int rz_device_count(int *count)
{
    if (!count) return fail(RZ_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(RZ_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return RZ_OK;
}

int rz_device_numa_node(int device, int *node)
{
    if (!node) return fail(RZ_ERR_INVALID, "null node");
    *node = -1;
    char bus[32] = {0};
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();        // (the runtime keeps a failed call's error for the next hipGetLastError(): a launch check would report it)
        return fail(RZ_ERR_NO_DEVICE, "no device %d (%d visible)", device, n_dev);
    }
    hipError_t e = hipDeviceGetPCIBusId(bus, (int)sizeof bus, device);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(RZ_ERR_NO_DEVICE, "hipDeviceGetPCIBusId(%d): %s", device, hipGetErrorString(e)); }
    for (char *p = bus; *p; ++p) *p = (char)tolower((unsigned char)*p);      // sysfs spells the address in lower case
    char path[128];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE *f = fopen(path, "r")) {
        int n = -1;
        if (fscanf(f, "%d", &n) == 1) *node = n;
        fclose(f);
    }
    return RZ_OK;
}

int rz_create(int device, rz_ctx **out)
{
    if (!out) return fail(RZ_ERR_INVALID, "null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(RZ_ERR_NO_DEVICE, "no HIP device: %s", e == hipSuccess ? "count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(RZ_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RZ_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", device,
                    prop.gcnArchName);
    rz_ctx *c = new rz_ctx();
    memset(&c->pl.cur.ml, 0, sizeof c->pl.cur.ml);
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se == hipSuccess) se = hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking);
    if (se == hipSuccess) se = c->ev_front.create();
    if (se == hipSuccess) se = c->ev_skin.create();
    if (se == hipSuccess) se = hipEventCreate(&c->ev0);
    if (se == hipSuccess) se = hipEventCreate(&c->ev1);
    if (se != hipSuccess) {
        rz_destroy(c);
        return fail(RZ_ERR_HIP, "context setup failed: %s", hipGetErrorString(se));
    }
    *out = c;
    return RZ_OK;
}

int rz_destroy(rz_ctx *c)
{
    if (!c) return RZ_OK;
    if (c->n_forks) return fail(RZ_ERR_INVALID, "%d fork(s) still borrow this context's static data: destroy them first", c->n_forks);
    (void)hipSetDevice(c->device);
#ifdef RZ_ALL_VARIANTS
    if (c->gate_host) *reinterpret_cast<volatile uint32_t *>(c->gate_host) = 1u;      // a test died with the gate closed: open it before draining the stream
#endif
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
    if (c->lender) {                      // (what a fork borrowed it holds as aliases, which free nothing: dev_buf.h, Lent)
        c->lender->n_forks--;
        c->lender = nullptr;
    }
    drop_direct_gather(c);
    drop_graph(c);
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    // what was created by hand; every device buffer, pinned slot and ring event has its owner in the context and goes with it
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
#ifdef RZ_ALL_VARIANTS
    if (c->gate_host) { (void)hipHostFree(c->gate_host); c->gate_host = nullptr; }
#endif
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RZ_OK;
}

int rz_fork(rz_ctx *parent, rz_ctx **out)
{
    if (!out) return fail(RZ_ERR_INVALID, "null out");
    *out = nullptr;
    if (int r = use(parent)) return r;
    if (parent->lender) return fail(RZ_ERR_INVALID, "rz_fork of a fork: fork the context that owns the static data");
    if (parent->mesh.V == 0 || !parent->mesh.geom || parent->skel.B == 0 || !parent->skel.inv_bind) return fail(RZ_ERR_INVALID, "rz_fork needs a mesh and a skeleton (rz_upload_mesh, rz_upload_skeleton)");
    if (parent->comm || parent->gather_root) return fail(RZ_ERR_UNSUPPORTED, "rz_fork of a context that takes part in a gather");
    HIP_TRY(hipStreamSynchronize(parent->stream));        // every static upload of the lender has landed (before anything is created: nothing to undo on failure)
    rz_ctx *c = nullptr;
    if (int r = rz_create(parent->device, &c)) return r;
    static_cast<RzStatic &>(*c) = *parent;      // borrowed: aliases of the lender's tables (dev_buf.h: a copy of a Lent frees nothing), and copies of the host mirrors the plan reads (plan.cpp: ensure_subfk)
    static_cast<RzTuning &>(*c) = *parent;      // inherited
    c->I = parent->I; c->aabb_on = parent->aabb_on; c->aabb_rearm = parent->aabb_on; c->tuned_by_search = parent->tuned_by_search;
    c->ovr_follow = parent->ovr_follow;         // rz_override_follow: a flag of the context, inherited here; the override set and its followers are each context's own
    c->lender = parent;
    parent->n_forks++;
    int rc = ensure_pose_buffers(c);
    if (rc == RZ_OK) rc = ensure_outputs(c);
    if (rc != RZ_OK) { rz_destroy(c); return rc; }
    *out = c;
    return RZ_OK;
}

int rz_sync(rz_ctx *c)
{
    if (int r = use(c)) return r;
    return drain(c);
}

int rz_output_ptrs(rz_ctx *c, void **pos, void **nrm, uint32_t *v_padded)
{
    if (int r = use(c)) return r;
    if (int r = ensure_outputs(c)) return r;
    if (pos) *pos = c->ext_pos ? c->ext_pos : c->out_pos;
    if (nrm) *nrm = c->ext_nrm ? c->ext_nrm : c->out_nrm;
    if (v_padded) *v_padded = c->mesh.Vp;
    return RZ_OK;
}

}  // extern "C"
