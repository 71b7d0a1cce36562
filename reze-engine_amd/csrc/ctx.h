// ctx.h — what the translation units of libreze_deform.so's host side share: the context (struct rz_ctx), the error / HIP / RCCL
// plumbing, the frame plan, and the internal entry points of each unit. Nothing here is part of the C ABI (include/reze_deform.h);
// everything internal lives in namespace rzi with hidden visibility.
// The context is three parts, and rz_fork follows them: a fork BORROWS RzStatic (a copy of the struct: its tables are Lent<T>, whose copy
// aliases the lender's pointer and frees nothing), INHERITS RzTuning (by value), and OWNS everything else: streams, palettes, outputs, and
// two members that are empty in a fresh fork — the per-frame pose transport (RzPoseLink pl: its rings, and where the current pose is) and
// physics (RzPhysics ph). Every device buffer, pinned slot and ring event is a member with an owner type (dev_buf.h; Pinned and Events
// below), so rz_destroy releases them by deleting the context; only streams, the events made by hand, the graph, the communicator, the
// gather links and the gate's pinned word are destroyed explicitly, in the order that matters there.
//   core.cpp    context life cycle, buffers every unit sizes, error state            rz_create / rz_destroy / rz_fork / rz_sync ...
//   upload.cpp  static data: mesh, skeleton, topology, morph targets, motion            rz_upload_* / rz_set_instances / rz_shard_range
//   pose.cpp    per-frame inputs: RzPoseLink's rings and transitions, copies            rz_set_pose* / rz_override_world / rz_read_world
//   dev_buf.h   the owners of device memory: Scratch, Grown + grow(), Lent (HIP allocator only)    (no exports)
//   pose_ring.h the reuse proof of the zero-copy and big-pose rings (no HIP)            (no exports)
//   plan.cpp    launch shapes and the parameter blocks of the kernels                   (no exports)
//   frame.cpp   launching frames, replay, timing, readbacks                             rz_deform* / rz_time_frames / rz_read*
//   tune.cpp    launch-shape search and the tuning keys                                 rz_autotune* / rz_set_tuning / rz_get_tuning
//   physics_host.cpp  rigid-body physics: table upload, stepping, reset, readback           rz_upload_physics / rz_physics_* / rz_read_physics
//   comm.cpp    RCCL binding, all-gather, peer-direct gather                            rz_comm_* / rz_allgather* / rz_gather_*
#pragma once
#include "../../include/reze_deform.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "deform_kernels.h"
#include "after_table.h"
#include "motion_table.h"
#include "physics_table.h"
#include "pose_ring.h"
#include "dev_buf.h"

#pragma GCC visibility push(hidden)
namespace rzi {

int fail(int code, const char *fmt, ...);
const char *last_error();

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (void)hipGetLastError();    /* reported here: a later launch's hipGetLastError() must not see it again */ \
            return fail(e_ == hipErrorOutOfMemory ? RZ_ERR_OOM : RZ_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                 \
        }                                                                                           \
    } while (0)


inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// Pinned host memory with one owner, in Scratch's way, and its device address where the device can read it in place.
struct Pinned {
    void *host = nullptr, *dev = nullptr;
    Pinned &operator=(Pinned &&o) noexcept { std::swap(host, o.host); std::swap(dev, o.dev); return *this; }
    ~Pinned() { if (host) (void)hipHostFree(host); }
    // device-mapped where that can be had; `must_map` = false: memory that cannot be mapped is still good for copies (dev stays null)
    hipError_t alloc(size_t bytes, bool must_map)
    {
        hipError_t e = hipHostMalloc(&host, bytes, hipHostMallocMapped);
        if (e != hipSuccess) host = nullptr;
        else if ((e = hipHostGetDevicePointer(&dev, host, 0)) == hipSuccess) return e;
        (void)hipGetLastError();
        dev = nullptr;
        if (must_map || host) return must_map ? e : hipSuccess;
        return hipHostMalloc(&host, bytes, hipHostMallocDefault);
    }
};

// N events without timing, one owner. A ring's events are made when the ring is built (a drain, rare), never on a per-frame path.
template <int N> struct Events {
    hipEvent_t e[N] = {};
    Events &operator=(Events &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t create()
    {
        hipError_t r = hipSuccess;
        for (int i = 0; i < N && r == hipSuccess; ++i) r = hipEventCreateWithFlags(&e[i], hipEventDisableTiming);
        return r;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};

constexpr uint32_t kVertPad = 1024;   // planes are padded to a whole S=1 tile (256 quads)
// Shards of one mesh are equal-sized except the last; their size is a multiple of 256 vertices (whole quads, whole S = 1 wave
// steps, 16-byte aligned float3 boundaries in the gathered buffer). 1024 (rounds 1-3) made the ranks of a 1 M-vertex mesh over
// 8 GPUs carry 125 952 vertices and the last 118 336; now 125 184 / 123 712: the slowest rank has 0.6 % less to do.
constexpr uint32_t kShardGrain = 256;
constexpr int kStageSlots = 8;

// ---- lazily bound RCCL (librccl.so.1 is only needed by the multi-GPU entry points) ----
struct Rccl {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    bool reused = false;                // bound to a copy the process had already loaded (e.g. PyTorch's)
};
extern Rccl g_rccl;
int rccl_bind();

#define NCCL_TRY(expr)                                                                              \
    do {                                                                                            \
        ncclResult_t r_ = (expr);                                                                   \
        if (r_ != ncclSuccess)                                                                      \
            return fail(RZ_ERR_RCCL, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));            \
    } while (0)

}  // namespace rzi
using rzi::kStageSlots;

// One set of VMD IK on/off keys (rz_upload_ik_keys): the frames, non-descending, and per key one bit per chain in the DEVICE's chain order
// (RzIkSwitchParams), [n][words]. Host data only: the step function is evaluated where the frames and states are handed over (pose.cpp).
struct RzIkKeySet {
    std::vector<float> frame;
    std::vector<uint32_t> bits;
    bool resident = false;              // (a set of no keys is resident too: it says "all on")
};

// Everything rz_upload_* writes and a frame only reads. A new static table goes here and nowhere else: rz_fork copies the struct as a whole,
// and a copy of a Lent<T> borrows (dev_buf.h), so a fork neither misses a table nor frees one. What one upload writes is one sub-struct:
// the upload releases it as a whole (`c->ik = {}`: every array with its counts and host mirrors), then builds the new one, and resets it
// again if that fails part-way — no count is ever non-zero over a null array, and a new member cannot be forgotten.
struct RzStatic {
    template <class T> using Lent = rzi::Lent<T>;
    // static mesh shard (rz_upload_mesh*)
    struct Mesh {
        uint32_t V = 0, Vp = 0;
        Lent<float> geom;               // 6 x Vp
        Lent<uint32_t> j01, j23, wq;
    } mesh;
    // skeleton (rz_upload_skeleton)
    struct Skeleton {
        uint32_t B = 0;
        Lent<float> inv_bind;           // B x 16
    } skel;
    // optional topology for on-device FK (rz_upload_skeleton_topology), and the hierarchy's static block (kernels/fk.hip.h): [B][4] bone
    // records (topology | bind | the motion's track | ancestors of the first two doubling rounds) + [an.M][2] vertex-morph records; `rec`
    // alone is rebuilt by rebuild_fk_static when the topology or the motion changes
    struct Hierarchy {
        bool has_topology = false;
        Lent<uint4> rec;
        Lent<uint2> anc_more;           // [rounds - 2][B] ancestor tables of the doubling rounds beyond the second (depth > 16)
        int rounds = 0;                 // radix-4 doubling rounds = ceil(log4(depth))
        std::vector<uint4> host;        // host copy of the bone records (w2 is filled in from an_host_range)
    } fk;
    uint64_t fk_gen = 0;                // bumped when the hierarchy's static block is rebuilt or goes (never reset: what was built against it compares)
    // The motion stores: the single motion (rz_upload_animation / rz_set_pose_sampled, sampled inside rz_fk_kernel) and the motion library
    // (rz_upload_motions / rz_set_pose_blended / rz_set_pose_layered; kernels/motion.hip) are the same arrays — motion_table.h's flattening of
    // one clip, or of all clips concatenated with absolute indices — independent of each other.
    struct RzKeys {
        Lent<float> key_frame, key_pos, mkey_frame, mkey_weight, feed_ratio;
        Lent<float4> key_rot;
        Lent<uint4> key_interp;         // null: no clip carries interpolation bytes
        Lent<uint32_t> feed_off;        // [clips][M + 1]
        Lent<uint4> feed_range;         // (first key, end, first frame, last frame) per morph feed
        uint32_t M = 0;                 // vertex-morph count the feeds were built for
    };
    RzKeys an;
    bool has_animation = false;
    std::vector<uint4> an_host_range, an_host_mrec;     // the motion's per-bone track records / per-morph records (host copies)
    RzKeys mo;
    struct Library {
        uint32_t clips = 0;             // clips resident (0 = no library)
        Lent<uint4> bone_rec;           // [clips][B] per clip one 16-byte track record per bone
    } lib;
    // the masks of layered poses (rz_upload_motion_masks / rz_set_pose_layered; kernels/motion.hip): bit sets, one 32-bit word per 32
    // bones / vertex morphs, bone_words / morph_words words per mask. morph_bits null: every mask includes every morph.
    struct Masks {
        uint32_t count = 0, M = 0;      // masks resident (0 = none) / vertex-morph count the morph masks were built for
        Lent<uint32_t> bone_bits, morph_bits;
        uint32_t bone_words = 0, morph_words = 0;
    } mk;
    // PMX bone morphs (rz_upload_bone_morphs): entries grouped by bone, ascending morph index inside a bone
    struct BoneMorphs {
        Lent<uint32_t> off, morph;
        Lent<float4> rot, tr;
        uint32_t count = 0;
    } bm;
    // SDEF vertices of this shard (rz_upload_sdef): [10][n] planes (kernels/sdef.hip); QDEF vertices (rz_upload_qdef): [n] indices
    // (kernels/qdef.hip). tab null = every vertex is skinned as the frame kernel skins it. idx_host: the table's vertex list (a vertex may
    // be in one of the two only); read by the two uploads only, which a fork is refused
    struct VertexTable {
        Lent<uint32_t> tab;
        uint32_t n = 0;
        std::vector<uint32_t> idx_host;
    } sdef, qdef;
    // PMX IK chains of this skeleton (rz_upload_ik), grouped into stages (deform_kernels.h: RzIkParams); n = 0: no IK stage, rz_fk_kernel as ever
    struct Ik {
        Lent<uint4> chain;
        Lent<uint32_t> path, stage_off;
        Lent<float4> link;
        uint32_t n = 0, stages = 0;
        std::vector<uint32_t> dev_pos;  // where chain k of rz_upload_ik's order sits in the device's order (chain switches: rz_set_ik_enabled / rz_upload_ik_keys)
        std::vector<uint8_t> on_path;   // [B] 1 = the bone lies on a chain's path (outermost link ... effector): what rz_upload_after_physics refuses
    } ik;
    // PMX after-physics bones (rz_upload_after_physics; after_table.h, kernels/after.hip): the list in evaluation order as uploaded, and
    // its device tables (deform_kernels.h: RzAfterParams). n = 0: no list, no frame launches rz_fk_after_kernel. A new skeleton or
    // topology clears it (free_after).
    struct After {
        std::vector<uint32_t> bones;
        Lent<uint4> rec;
        Lent<int> level_off, index;
        uint32_t n = 0, levels = 0;
    } af;
    // the key sets of the chain switches — of the single motion, and one per clip of the library (empty: no clip holds keys). They go
    // with the IK table (free_ik), the motion (free_animation) and the library (free_motions). The MASK is pose state: rz_ctx::iksw.
    RzIkKeySet ik_keys_an;
    std::vector<RzIkKeySet> ik_keys_mo;
    // morph targets (rz_upload_morphs_dense* / rz_upload_morphs_sparse)
    struct Morphs {
        int mode = 0;                   // 0 none, 1 dense, 2 sparse
        uint32_t M = 0, Mpad = 12;
        Lent<float> dense_base;         // the allocation behind `dense`
        float *dense = nullptr;         // M x 3 x Vp: fp32 planes, or (storage 24) 24-bit integers, 3 * Vp bytes a plane. What frames read: dense_base, or (tools-only build) a place RZ_DENSE_OFFSET bytes into it
        // 24-bit dense storage (upload.cpp: rz_upload_morphs_dense; kernels/common.hip.h): per morph s_m * 2^-8, s_m = the power of two its
        // integers are multiples of — folded into the weights of every active list. Empty / null with fp32 planes.
        int storage = 32;               // bits per stored delta of the resident dense set: 24 or 32
        Lent<float> dense_fold;         // [M] device
        std::vector<float> dense_fold_host;     // [M] host mirror (the one-launch frame's list is compacted on the host)
        Lent<uint32_t> sp_ptr;          // Vp + 1
        Lent<float4> sp_entries;
        uint64_t sp_count = 0;
    } morphs;
    Lent<float> edge;                   // Vp: the fused hull consumer's edge scale (rz_upload_edge_scale)
};

// The settable tuning keys (tune.cpp: kTuneKeys names each one; 0 / -1 = automatic). A fork starts with its lender's values.
struct RzTuning {
    int t_split = 0, t_unroll = 0, t_grid_cap = 0, t_nt = 1, t_nts = -1, t_geo = 0, t_fast = -1, t_instloop = -1, t_outcap = -1, t_instblock = 0, t_instorder = 1, t_overlap = -1, t_zerocopy = -1, t_fusefk = -1, t_qdefchunks = 0;
    int t_fkplain = -1;                 // "fuse_fk_plain": -1 / 1 = the fused frame of a plain pose runs the specialised kernel variant, 0 = always the generic one
    int t_pull = -1;                    // "pose_pull": -1 = world-matrix poses, 1 = every pose of more than 256 KB, 0 = hipMemcpyAsync of the pose as the host handed it over
    int t_prefetch = -1;                // "pose_prefetch": -1 / 1 on, 0 off
    int t_subsets = -1;                 // "inst_subsets": -1 / 1 = stage only the bones a vertex run names when that is a gain, 0 = always the whole palette
    int t_graph = 0;                    // "graph" tuning key: rz_deform_n replays captured hipGraphs of kGraphFrames frames
    int t_sppiece = 0;                  // "sparse_piece": 0 = the plan sizes a wave's LDS piece of the sparse CSR, else that many entries (16..2048, a multiple of 16) where they fit
    int t_instmorphs = -1;              // "inst_morphs": 1 = a crowd with sparse morph targets takes the crowd kernels (kernels/crowd_morph.hip), 0 = never, -1 = auto (= off)
};

// Rigid-body physics (rz_upload_physics; physics_host.cpp, kernels/physics.hip): static records, per-instance state, and what the next step must
// do first. nb = 0: no table. A fork's own, and empty from the start (physics is refused while forks exist). Every device array has its owner
// here, so a stage is released by resetting its part as a whole (`part = {}`) and the table by resetting the struct: a new member cannot be
// forgotten.
struct RzPhysics {
    rzi::Scratch<float4> body, joint, state;
    rzi::Scratch<int> colour_off;
    uint32_t nb = 0, nj = 0, ncol = 0, nd = 0, I = 0;
    int iterations = 0, block = 64;
    float h = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
    bool reset = true;                  // the next step places every body on its bone first
    std::vector<int> dyn_bone;          // [nd] bones of the dynamic bodies
    rzphys::Kept kept;                  // the columns as uploaded: rz_physics_contacts and rz_physics_springs derive their records from its view()
    std::vector<int> order;             // [nj] the joints' solve order
    double hd = 0.0;                    // h as derived at upload, before its rounding to h
    // rz_physics_aligned: on = the resident records were derived with the table's type-2 bodies read as dynamic (kept stays the caller's
    // table); types = the type column as the solver reads it then (what the contact lists derive from), n = the aligned bodies
    struct Aligned {
        int on = 0;
        uint32_t n = 0;
        std::vector<uint8_t> types;
    } aligned;
    // the contact stage (rz_physics_contacts): off unless mode; the lists are constants of the resident table
    struct Contacts {
        int mode = 0;                   // 0 off | 1 spheres and capsules | 2 boxes take part as well | 3 and box against box
        rzi::Scratch<float4> shape, box;
        rzi::Scratch<int> follow_off, follow_idx, colour_off;
        rzi::Scratch<int2> pair;
        uint32_t follow = 0, pairs = 0, ncol = 0, boxes = 0, box_pairs = 0, box_box = 0;
    } contacts;
    // the linear springs (rz_physics_springs): off unless on; lin is null while no axis of the table has a spring
    struct Springs {
        int on = 0;
        uint32_t axes = 0;
        rzi::Scratch<float4> lin;       // [nj] in solve order (deform_kernels.h: RzPhysicsParams::lin)
    } springs;
};

// The per-frame pose transport (pose.cpp): where the current pose is, how it got there, and which slot of which ring may be written next. A
// fork's own, and empty from the start. Pinned slots, device blocks and events have their owners here: a ring is re-allocated by building its
// replacement, draining and assigning it, and the whole transport is released by resetting this struct.
struct RzPoseLink {
    // Two device blocks per context, and a ring of them for big poses: [world I*B*16 | morph weights pad4(I*max(M,1)) | local rotations I*B*4 | local
    // translations I*B*3] floats. A world-matrix pose fills [world | weights], a local pose [weights | rotations (| translations)] — each a
    // CONTIGUOUS range, so every upload is one copy (measured: a small H2D copy is a 4.5 us blit kernel on this runtime, and a second one for 256
    // bytes of morph weights cost as much as the first). The offsets are those of the instance / bone / morph counts AT UPLOAD TIME
    // (point_pose_slot): shrinking the crowd afterwards leaves the resident pose where it is.
    rzi::Scratch<float> pose_blk[2];
    int pose_slot = 0;
    size_t alloc_I = 0, alloc_B = 0, alloc_M = 0;       // what the blocks (and the context's palette ring) were sized for

    // The pinned staging ring: everything per-frame that is copied or pulled to the device goes through a slot of it — poses, the frames of a sampled
    // pose, motion states and layers, override sets and their follower lists. ev[slot] = what was sent out of the slot has landed: the host polls it
    // before the slot's next use, kStageSlots uploads later, and the compute stream waits for it where the pose travelled on the upload stream
    // (staged_sent).
    struct Stage {
        rzi::Pinned slot[kStageSlots];  // (dev null: this ring can only be copied from)
        size_t bytes = 0;
        rzi::Events<kStageSlots> ev;
        bool used[kStageSlots] = {};
        int next = 0;
    } stage;

    // Zero-copy poses (one character, <= 256 KB): rz_set_pose* only writes the pose into a slot of this pinned, device-mapped ring — no copy is
    // enqueued at all. The first frame's kernels read it over the host link (rz_fk_kernel the local pose; the one-launch deform kernel the world
    // matrices, whose workgroup 0 also leaves them in the device pose block for the frames that replay the pose); anything that needs a
    // device-resident pose first (rz_prep_kernel) gets it through make_resident(). Measured on MI355X (tools/archive/uploadbench): a 16.6 KB
    // hipMemcpyAsync in front of a frame costs 18 us, two of <= 16 KB 9.5 us, reading the pinned slot from the kernel 7 us with the loads fully
    // exposed. A slot is reused kSlots uploads later; that its readers are done is `proof`'s to say (pose_ring.h), so there is no per-frame marker.
    // One hipEventRecord per kSlots / 2 uploads, and a record costs ~1.4 us of stream time: measured on a 1/8 shard of C5
    // (tools/archive/live_shard.py, per-frame-pose loop over the resident replay): 8 slots +0.86 us per frame, 16 slots +0.50 us, 32 slots +0.37 us.
    // 32 x <= 256 KB of pinned memory per context. Pose prefetch (deform_kernels.h: pf_*): every slot carries a header behind its payload — the
    // sequence number of the pose it holds, written LAST — and the device keeps one tag per pose block: the sequence number a frame's helper
    // workgroup staged there. Sequence numbers are (ring epoch << 32 | upload index + 1): a re-allocated ring never matches old tags.
    struct ZeroCopy {
        static constexpr int kSlots = 32;
        rzi::Pinned slot[kSlots];
        size_t bytes = 0, hdr_off = 0;  // payload bytes a slot holds / byte offset of the header inside it
        rzring::ReuseProof<kSlots> proof;
        rzi::Events<2> ev;
    } zc;
    uint32_t epoch = 0;                 // the ring epoch of the sequence numbers (pose.cpp: retire_pose_tags bumps it, nothing else)
    rzi::Scratch<uint64_t> tag;         // device: [2], one per pose block

    // Poses of more than 256 KB (crowds) travel on the upload stream into a ring of kBlocks device blocks of their own (the layout of pose_blk), so
    // the upload of pose f+1 runs under the frame of pose f. A block is overwritten kBlocks uploads after it was filled; the same proof says its
    // readers are done — no per-frame "slot is free" hand-off between the streams (round 4 had one: a record on the compute stream + a wait on the
    // upload stream per frame, measured at 5 - 8 us per frame: tools/archive/overlapbench, profiles/r5_overlapbench.txt). 8 x 3.3 MB for C4.
    struct Big {
        static constexpr int kBlocks = 8;
        rzi::Scratch<float> blk[kBlocks];
        size_t floats = 0;
        rzring::ReuseProof<kBlocks> proof;
        rzi::Events<2> ev;
    } big;

    // rz_map_pose / rz_commit_pose: the slot handed out to the caller (layout < 0 = nothing mapped), and what it was sized for
    struct Map {
        int layout = -1;
        bool zc = false;                // a slot of the zero-copy ring (one character) or of the staging ring (crowds)
        int slot = 0;
        uint64_t upload = 0;            // zero-copy: the upload index (1-based) zc_open gave the slot
        uint32_t I = 0, B = 0, M = 0;
        char *ptr = nullptr;
    } map;

    struct Current {                    // the current pose
        bool set = false;
        uint32_t I = 0;                 // instance count the pose was uploaded for
        bool local = false;             // it is a local pose (rz_set_pose_local, or produced on the device), not world matrices
        bool local_t = false;           // ... that carries translations (behind the rotations in its slot)
        bool sampled = false;           // ... sampled on the device from the uploaded motion (rz_set_pose_sampled)
        bool frames_inline = false;     // one character: the frame rides in the kernel arguments (frame0), nothing is uploaded
        float frame0 = 0.0f;
        int zc_slot = -1;               // its slot of the zero-copy ring, -1 = it came down as a copy or was produced on the device
        bool zc_local = false;          // layout of that slot: [weights | rotations | translations] or [world | weights]
        int zc_kind = 0;                // 0 world, 1 local rotations, 2 local rotations + translations (part of the sequence number)
        size_t zc_total = 0, zc_mw_off = 0, zc_lq_off = 0;      // bytes in the slot, and where the weights / rotations sit in it
        uint64_t seq = 0;               // its sequence number (0 = not prefetchable)
        bool world_resident = true, mw_resident = true, local_resident = true;   // which parts the device pose block holds
        bool resident() const { return zc_slot < 0 || (world_resident && mw_resident && local_resident); }
        // host-compacted active-morph list (single-instance FAST path); count < 0 means "more than kKargMorphs active: use the prep kernel"
        RzMorphList ml = {};
    } cur;

    // what device-produced poses are made from: [I] frames (sampled), [I] states or [I] states + [I][n_layers] layers of a crowd (blended / layered)
    rzi::Grown<float> an_frames;
    rzi::Grown<RzMotionState> mo_states;
    rzi::Grown<RzMotionLayer> mo_layers;
    hipStream_t mo_states_stream = nullptr;     // the stream that last wrote and read mo_states (and mo_layers)
    // what the most recent copy upload did (rz_get_tuning: pose_pulled / pose_rows): a crowd's pose (more than 256 KB) is PULLED out of the ring
    // slot by rz_pull_pose_kernel on the upload stream instead of copied, world matrices as their upper three rows (pose.cpp: upload_pose_copy)
    bool last_pulled = false, last_rows = false;
};

struct rz_ctx : RzStatic, RzTuning {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    RzPoseLink pl;                      // the per-frame pose transport; world / morph_w / local_q below point into its current block
    float4 *local_q = nullptr;          // I x B   (current pose slot)

    // physics hand-off for device-solved frames (rz_override_world)
    rzi::Grown<int> ovr_off, ovr_bone;   // the three grow as a set (plan.cpp: reserve_overrides)
    rzi::Grown<float> ovr_world;
    uint32_t ovr_count = 0;
    // rz_override_follow: bones below an overridden bone follow it (kernels/fk.hip.h: FOLLOW). A flag of the context (a fork starts with its
    // lender's value); the lists exist only while it is on and are valid whenever ovr_count != 0 — built wherever the override set is
    // built (rz_override_world, the physics table's per-instance buffers, and the flag's own flip while overrides are resident)
    int ovr_follow = 0;
    rzi::Grown<int> fol_off;            // [I + 1]
    rzi::Grown<uint2> fol_ent;          // [fol_count] (follower bone, entry of its nearest overridden ancestor in the override table); grows with fol_off as a set (reserve_followers)
    uint32_t fol_count = 0;
    std::vector<int> ovr_off_host, ovr_bone_host;       // the hand-fed override set as uploaded (rz_override_world), for a later flip of the flag

    // The per-instance chain switches the next solve uses: [I][words] in the device's chain order, set = on, padding bits clear; EMPTY =
    // every chain of every instance is on (the only form `off` == 0 takes), and then the solve is launched without the switch stage, as ever. One character's
    // words ride in the kernel arguments; a crowd's are copied into `dev` when they CHANGE (a switch flips a few times per motion, so a
    // frame whose bits did not change sends nothing). A fork's own, all on from the start.
    struct IkSwitch {
        std::vector<uint32_t> words;
        uint32_t off = 0;               // (instance, chain) bits clear
        rzi::Grown<uint32_t> dev;
    } iksw;

    RzPhysics ph;                       // rigid-body physics; with a table the override table above is physics' own ([I][ph.nd] slots, fixed addresses)

    // per-frame state
    uint32_t I = 1;
    float *world = nullptr;             // I x B x 16   (current pose slot)
    size_t mw_pad = 0;                              // floats reserved for the morph weights in the current layout (multiple of 4)
    hipStream_t up_stream = nullptr;    // per-frame inputs travel here where that is a gain (pose.cpp: pose_stream): the upload of pose f+1 overlaps the kernels of pose f
    float4 *palette = nullptr;         // I x B x 3   (current ring slot)
    float *morph_w = nullptr;           // I x M   (current pose slot)
    uint32_t *act_idx = nullptr;        // I x Mpad    (current ring slot)
    float *act_w = nullptr;             // I x Mpad    (current ring slot)
    int *act_count = nullptr;           // I           (current ring slot)
    // Everything the FRONT kernels (rz_prep_kernel / rz_fk_kernel) hand to the skin kernel lives in a 2-slot ring, so the
    // front kernels of frame f+1 can run on the upload stream while the skin kernel of frame f is still reading slot f:
    // ev_front[s] = slot s is ready (compute stream waits), ev_skin[s] = the skin kernel that read slot s has been enqueued
    // up to here (the front stream waits before overwriting the slot, two frames later). Used by crowds (overlap_on).
    rzi::Scratch<float4> palette_ring[2];
    rzi::Scratch<uint32_t> act_idx_ring[2];
    rzi::Scratch<float> act_w_ring[2];
    rzi::Scratch<int> act_count_ring[2];
    int ring_slot = 0;
    rzi::Events<2> ev_front, ev_skin;
    bool skin_recorded[2] = {false, false};
    bool overlap_on = false;            // the two streams currently follow the overlapped-front protocol

    // outputs
    rzi::Grown<float> out_pos, out_nrm; // the two grow as a set (core.cpp: ensure_outputs)
    // fused consumers
    rzi::Grown<float> out_hull;         // I x Vp x 3
    rzi::Grown<uint32_t> aabb;          // I x 2 x 6 keys
    bool aabb_on = false;
    int aabb_slot = 0;                  // slot the NEXT frame accumulates into
    bool aabb_rearm = false;            // both slots must be armed again before the next frame

    int t_dbg = 0;                      // "dbg": ablation switches of the tools-only build; not in RzTuning, a fork starts without them
    // Bone-subset crowd frames: per vertex run of the CURRENT launch shape, the ascending list of bones the run's
    // vertices name, and the joints rewritten as slots of that list. Derived from the static mesh, rebuilt (one small kernel +
    // one readback of the counts) whenever the shape (vertices per run, runs), the mesh or the skeleton changes.
    rzi::Scratch<uint32_t> rj01, rj23;              // [Vp]
    rzi::Grown<uint16_t> sub_list;                  // [sub_runs][sub_B]
    rzi::Grown<uint32_t> sub_count;                 // [sub_runs]
    uint32_t sub_per = 0, sub_runs = 0, sub_B = 0, sub_max = 0;
    bool sub_valid = false;
    bool palette_stale = false;         // the last crowd frame formed its palettes in LDS only (subset form): rz_read_palette forms them on demand
    // Crowd frames of device-animated poses with the hierarchy solved in the skin kernel's front (kernels/crowd.hip:
    // rz_skin_instances_fk_kernel): per vertex run the closure of its named bones under "parent of", one 80-byte record per closure
    // slot — derived from the run lists and the hierarchy's static data, rebuilt when either changes (plan.cpp: ensure_subfk)
    rzi::Grown<uint4> subfk_rec;
    rzi::Grown<uint32_t> subfk_count;
    uint32_t subfk_stride = 0, subfk_rounds = 0;
    bool subfk_valid = false;
    uint64_t subfk_sub_gen = 0, subfk_fk_gen = 0;   // what it was built against
    uint64_t sub_gen = 0;               // bumped when the run lists are rebuilt (RzStatic::fk_gen: the hierarchy's static block)
    bool fk_stale = false;              // the last crowd frame solved its hierarchy in LDS only: rz_read_world / rz_read_palette run rz_fk_kernel on demand
    hipGraphExec_t graph_exec = nullptr;
    uint64_t graph_sig = 0;             // signature of everything the captured launches depend on
    bool tuned_by_search = false;       // rz_autotune set morph_split / grid_cap / inst_loop for the CURRENT mesh, morphs and instance count

    // multi-GPU
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    uint32_t v_total = 0, chunk = 0;
    rzi::Scratch<float> g_pos, g_nrm;           // nranks x chunk x 3
    // peer-direct gather (rz_gather_direct): this context's kernels store straight into the root's gathered buffer
    float *ext_pos = nullptr, *ext_nrm = nullptr;
    rz_ctx *gather_root = nullptr;              // set on every contributor (the root contributes too)
    // rz_fork: a fork borrows RzStatic, inherits RzTuning, and owns everything else. While forks exist neither side may replace static
    // data (static_unlocked), and physics, whose tables live in this struct and not in RzStatic, is refused on both (physics_usable).
    rz_ctx *lender = nullptr;
    int n_forks = 0;
#ifdef RZ_ABLATE
    rzi::Grown<unsigned long long> tl;          // tools-only build: per-wave timeline of the last frame (dbg = 100), 16 words a wave
#endif
#ifdef RZ_ALL_VARIANTS
    uint32_t *gate_host = nullptr, *gate_dev = nullptr;     // tools-only build: rz_debug_gate
#endif
    std::vector<rz_ctx *> contributors;         // set on the root
    hipEvent_t ev_done = nullptr;               // "my last frame has been enqueued up to here" for rz_gather_fence
};

namespace rzi {

// ---- core.cpp ----
int use(rz_ctx *c);
int static_unlocked(const rz_ctx *c, const char *what);       // static data shared between a context and its forks cannot be replaced
int poll_event(hipEvent_t ev, const char *what);
void drop_graph(rz_ctx *c);
int drain(rz_ctx *c);                  // the upload stream, then the compute stream
int ensure_outputs(rz_ctx *c);
void set_ring(rz_ctx *c, int slot);
void point_pose_slot(rz_ctx *c, int k);
void point_pose_at(rz_ctx *c, float *block);     // the current pose lives in `block` (pose_blk[k] or a block of the big-pose ring)
int ensure_pose_buffers(rz_ctx *c);
RzSampleParams sample_params(const RzStatic::RzKeys &k);      // plan.cpp: the sampler's block with the store's pointers set, everything else zero
void free_animation(rz_ctx *c);
void free_motions(rz_ctx *c);
void free_motion_masks(rz_ctx *c);
int rebuild_fk_static(rz_ctx *c);      // upload.cpp: the device block behind fk_rec from the host copies
void free_bone_morphs(rz_ctx *c);
void forget_search(rz_ctx *c);
void free_morphs(rz_ctx *c);
void free_sdef(rz_ctx *c);
void free_qdef(rz_ctx *c);
void free_ik(rz_ctx *c);
void free_after(rz_ctx *c);
void free_physics(rz_ctx *c);          // physics_host.cpp
// a table's array from host data, into an EMPTY owner (Lent or Scratch: the table was reset first). A failure leaves the table to its caller, which resets it as a whole
template <template <class> class Owner, class T> int to_device(Owner<T> &dst, const void *src, size_t count)
{
    HIP_TRY(dst.alloc(std::max<size_t>(count, 4)));       // (never fewer than four elements: the specialised sampler asks for key 0 unpredicated — three floats of a position)
    if (count) HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return RZ_OK;
}
// A buffer of the context outgrown, or several that grow as a set (`c->sub_list.to(n), ...`): dev_buf.h's grow with the context's drain —
// replacements first, then both streams empty, then every array of the set moves at once. Returns RZ_OK with nothing done while all fit.
template <class... G> int grow(rz_ctx *c, G &&...g)
{
    HIP_TRY(grow([c] { const hipError_t e = hipStreamSynchronize(c->up_stream); return e != hipSuccess ? e : hipStreamSynchronize(c->stream); }, std::forward<G>(g)...));
    return RZ_OK;
}

// ---- plan.cpp ----
struct Plan { RzVariant v; uint32_t grid_x, n_quads, quads_per_wave; bool prep, dma; int inst_group; uint32_t verts_per_wg; int poses_per_wg; uint32_t out_cap; int inst_block; bool fuse_fk; bool subsets; uint32_t sub_bones; uint64_t inst_lds; bool pf; uint32_t sp_cap; bool subfk; bool inst_morphs; };
// Launch shape of an instanced crowd frame without dense morphs (rz_skin_instances_kernel): G poses per workgroup share one decode of each
// vertex; the grid is (vertex runs, pose groups), `total` workgroups in all. morphs: the context has sparse targets and "inst_morphs" asks
// for the crowd kernels — the MORPH instantiations, whose LDS holds the group's G x Mpad morph weights behind the palettes.
struct InstShape { int G, blk, blk_full; bool want_in_kernel; uint32_t per, runs; bool morphs; };
bool inst_shape(const rz_ctx *c, InstShape *s);
Plan make_plan(const rz_ctx *c);
int ensure_run_subsets(rz_ctx *c);
int ensure_subfk(rz_ctx *c);
RzSubFk subfk_params(const rz_ctx *c);
int frame_plan(rz_ctx *c, Plan *pl);
RzDeformParams deform_params(const rz_ctx *c, const Plan &pl);
// Which kernel that frame launches (frame_kernel.h), the one owner of that decision: launch_deform, frame_signature and rz_get_tuning's effective_* keys read it.
RzFrameKernel frame_kernel(const Plan &pl, const RzDeformParams &p);
RzPrepParams prep_params(const rz_ctx *c);
RzFkParams fk_params(const rz_ctx *c, bool overrides = true);      // overrides = false: without the override table (rz_physics_step's solve)
// Which stages the next hierarchy solve runs (deform_kernels.h: RzFkStages), the one owner of that decision: IK while a table is resident,
// chain switches while at least one bit is clear, the follow stage while rz_override_follow is on, overrides are resident and a bone follows
// one, the after-physics launch while its list and a non-empty override table are resident. A stage that is off leaves its block empty.
// overrides = false as in fk_params: no follow and no after stage either.
RzFkStages solve_stages(const rz_ctx *c, bool overrides = true);
// the follower lists of an override set (off [I + 1], bones ascending inside an instance) from the resident parents: fol_off [I + 1] and per
// entry (follower bone, index of its nearest overridden ancestor's entry), ascending by bone inside an instance
void build_followers(const rz_ctx *c, const std::vector<int> &off, const std::vector<int> &bones, std::vector<int> &fol_off, std::vector<uint2> &ent);
int reserve_overrides(rz_ctx *c, size_t entries, size_t offsets);       // grows ovr_off / ovr_bone / ovr_world as a set (drains and drops the graph when it must; the resident set goes)
int reserve_followers(rz_ctx *c, size_t entries, size_t offsets);       // grows fol_off / fol_ent (drains and drops the graph when it must)
int upload_followers(rz_ctx *c, const std::vector<int> &off, const std::vector<int> &bones);       // build + blocking upload; the caller has drained
uint64_t algorithmic_bytes(const rz_ctx *c);

// ---- pose.cpp ----
const float *src_world(const rz_ctx *c);
const float *src_morph_w(const rz_ctx *c);
const float4 *src_local_q(const rz_ctx *c);
int make_resident(rz_ctx *c);
uint64_t zc_seq(const rz_ctx *c, uint64_t upload_index_1, int kind);
void retire_pose_tags(rz_ctx *c);     // nothing a helper workgroup staged and tagged so far, or a slot header published so far, may match a later pose
// The chain switches become `words` ([I][ceil(ik_n / 32)], device order, padding bits clear; empty = all on) in two halves, so that a caller
// can do everything that may fail before it changes anything else: plan (allocates, waits for a staging slot, fills it; `I` = the instance
// count the words are for), then commit (enqueues a crowd's changed bits and takes the words into the mirror; if the enqueue fails the
// mask is all on, which reads no device array). set_ik_words is both at once.
struct IkWordsPlan { std::vector<uint32_t> w; uint32_t off = 0; int slot = -1; bool change = false, inline_words = false; };
int plan_ik_words(rz_ctx *c, uint32_t I, std::vector<uint32_t> &&words, IkWordsPlan *pl);
int commit_ik_words(rz_ctx *c, IkWordsPlan &pl);
int set_ik_words(rz_ctx *c, std::vector<uint32_t> &&words);
int plan_ik_resize(rz_ctx *c, uint32_t I, IkWordsPlan *pl);      // rz_set_instances, before the count changes: shrinking keeps the mask, members that appear are all on

// ---- frame.cpp ----
int check_ready(rz_ctx *c);
int launch_fk(rz_ctx *c, hipStream_t st, bool overrides = true);       // the solve + the after launch solve_stages(c, overrides) lists
bool solve_on_demand(const rz_ctx *c);
int launch_prep(rz_ctx *c, hipStream_t st);
bool has_front(const rz_ctx *c, const Plan &pl);       // does a frame of this plan launch kernels in front of its deform / skin kernel?
int launch_front(rz_ctx *c, const Plan &pl, hipStream_t st);
int launch_deform(rz_ctx *c, const Plan &pl);
bool want_overlap(const rz_ctx *c, const Plan &pl);
int set_overlap(rz_ctx *c, bool on);
int begin_frames(rz_ctx *c, Plan *pl);      // use -> check_ready -> ensure_outputs -> frame_plan -> set_overlap(want_overlap)
int run_frame(rz_ctx *c, const Plan &pl);
RzSdefParams sdef_params(const rz_ctx *c, const Plan &pl);
RzQdefParams qdef_params(const rz_ctx *c, const Plan &pl);
int launch_passes(rz_ctx *c, const RzSdefParams &sp, const RzQdefParams &qp);
hipStream_t front_stream(const rz_ctx *c);       // the stream per-frame inputs travel on and front kernels run on

// ---- comm.cpp ----
void drop_direct_gather(rz_ctx *c);

}  // namespace rzi
#pragma GCC visibility pop
