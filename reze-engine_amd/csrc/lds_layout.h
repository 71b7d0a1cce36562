// lds_layout.h — the LDS ledger: how every kernel family lays out its dynamic LDS, and the limits a plan holds the sizes to. ONE spelling
// each: the kernels carve their pointers from these layouts, the launchers size their launches from total(), and the host (plan.cpp,
// frame.cpp, upload.cpp) decides what fits by calling the same functions with explicit scalars. Plain C++ without a HIP header, so a host
// compiler builds it alone (tests/lds_layout_main.cpp); under a HIP compile every function is __host__ __device__.
// (The physics stage keeps its arithmetic beside its table, physics_table.h: rzphys::lds_bytes, held to kCuLds here.)
//
// Units. A layout returns what its kernel adds, in the kernel's own order of operations: a byte offset where the kernel steps a byte
// pointer, a count of floats or of float4 rows where it steps a typed one. Spelled so, the compiler emits the instruction streams it
// emitted for the hand-written carves; one byte offset per region from the start of LDS did not (NOTEBOOK.md, "LDS ledger").
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIP__
#define RZ_LDS_FN __host__ __device__ inline
#else
#define RZ_LDS_FN inline
#endif

namespace rzlds {

// ---- limits (bytes) ----
constexpr size_t kCuLds = 160 * 1024;           // the LDS of one CU of gfx950: what one workgroup may take at most
constexpr size_t kOptIn = 48 * 1024;            // dynamic LDS a kernel gets unasked; above it the launcher opts in (kernels/common.hip.h: rz_opt_in_lds)
constexpr size_t kHalfCu = 80 * 1024;           // the share of a workgroup where a plan wants two per CU (256-thread crowd kernels, large sparse frames)
constexpr size_t kCrowdLarge = 156 * 1024;      // budget of a 512- / 1024-thread crowd workgroup, alone on its CU
constexpr size_t kSkeletonReserve = 8192;       // rz_upload_skeleton admits B x 48 B of palette + this much work area
constexpr size_t kFuseFitPerMorph = 12, kFuseFitMargin = 4096;      // fused_fit_bytes below
// the sparse piece (plan.cpp) takes the planned share only where more than kPieceRoom is left of it, and leaves kPieceSlack unused
constexpr size_t kPieceRoom = 4096, kPieceSlack = 1024;
constexpr int kMinPiece = 16;                   // CSR entries per wave: the smallest piece the sparse row walk works with

constexpr int kFrameWaves = 4;                  // waves per workgroup of the generic frame kernels (kBlock / 64)

RZ_LDS_FN size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }
RZ_LDS_FN size_t larger(size_t a, size_t b) { return a > b ? a : b; }

// ---- hierarchy solve (kernels/front.hip: rz_fk_kernel; the same scratch serves the fused frame's prologue) ----
// palette rows | solve scratch | the pose's morph weights (bone morphs; n_weights = 0 without) | IK: the doubling rounds' second matrix buffer.
// Scratch per bone: 48 B (local rotation | record | bind translation, then the second matrix buffer of the doubling rounds) + 12 B (local
// translation), 16-byte rounded. With IK region X of the solve stays alive across the rounds, which get a buffer of their own, 48 B per
// bone more, behind the weights ROUNDED so that it is 16-byte aligned; without IK the weights are counted as they are.
struct Solve {
    size_t palette, scratch, weights, second;       // bytes, in this order
    RZ_LDS_FN size_t total() const { return palette + scratch + weights + second; }
};
RZ_LDS_FN size_t palette_bytes(int B) { return (size_t)B * 48; }       // 3 float4 rows per bone: what every family keeps in front
RZ_LDS_FN size_t solve_scratch(int B) { return ((size_t)B * 60 + 15) & ~(size_t)15; }
RZ_LDS_FN Solve solve(int B, bool ik, int n_weights)
{
    const size_t w = (size_t)n_weights * 4;
    return { palette_bytes(B), solve_scratch(B), ik ? round16(w) : w, ik ? palette_bytes(B) : 0 };
}

// ---- generic frame (kernels/deform_small.hip, kernels/deform_dense.hip) ----
// palette | list (indices, then weights: `pad` entries each, Mpad or 0) | work. Work = step scratch | parked outputs | sparse pieces; the
// fused solve's scratch and morph weights (kernels/deform_parts.hip.h: fused_hierarchy_prologue) ALIAS it, before anything else uses it.
struct Frame {
    size_t list_off;            // bytes: the palette in front of the lists, B x 48
    int pad;                    // entries of each list; the step scratch starts at (float *)(smem + list_off) + 2 x pad
    size_t scratch;             // floats: waves x planes x vertices per wave step
    size_t parked;              // floats: waves x out_cap x 6 (position + normal)
    size_t pieces;              // bytes: waves x sp_cap x 16
    size_t fused;               // bytes: the aliased solve's scratch + weights (+ 16), 0 without
    RZ_LDS_FN size_t work() const { return larger((scratch + parked) * 4 + pieces, fused); }
    RZ_LDS_FN size_t total() const { return list_off + (size_t)pad * 8 + work(); }
};
RZ_LDS_FN Frame frame(int B, int pad, int planes, int verts_per_step, uint32_t out_cap, uint32_t sp_cap, bool fused = false, int M = 0)
{
    return { (size_t)B * 48, pad, (size_t)kFrameWaves * planes * verts_per_step, (size_t)kFrameWaves * out_cap * 6, (size_t)kFrameWaves * sp_cap * 16,
             fused ? solve_scratch(B) + (size_t)(M > 1 ? M : 1) * 4 + 16 : 0 };
}
// What make_plan holds a fused frame to (pl.fuse_fk): palette + solve scratch + 12 B per morph + 4 KB. Older than the exact layout and
// conservative for the side of it that the fused solve adds: frame(..., true, M) has palette + lists (8 B x Mpad, Mpad < M + 12) +
// `fused` (solve scratch + 4 B x M + 16), at most 120 B above the first three terms, against a 4 KB margin. The other side of work()'s max
// — step scratch, parked outputs, pieces — is not its business: the write-batching and piece fits and launch_deform hold the total.
// Kept as it is: the exact form would change plans near the limit.
RZ_LDS_FN size_t fused_fit_bytes(int B, uint32_t M) { return (size_t)B * 48 + solve_scratch(B) + (size_t)M * kFuseFitPerMorph + kFuseFitMargin; }

// ---- crowd, pose-group form (kernels/crowd.hip: rz_skin_instances_kernel and its MORPH twin) ----
// G poses x `bones` staged bones (the whole skeleton, or the longest run list) x slot | the group's morph weights, G x morph_pad floats.
// slot: 48 B = a finished palette row set (dma: behind rz_prep_kernel / rz_fk_kernel); one-launch frame: 64 B, the world matrix, re-packed
// in place to 48 (whole palettes), or 112 = 48 of palette region with the 64 of staged world matrices BEHIND all palettes (subsets).
struct Crowd {
    int slot;                   // bytes per (pose, bone)
    size_t weights_off;         // bytes: G x bones x slot
    size_t weights;             // bytes
    size_t staged_off;          // bytes: subsets, one-launch: the staged world matrices behind the palette region (G x bones x 48)
    RZ_LDS_FN size_t total() const { return weights_off + weights; }
};
RZ_LDS_FN int crowd_slot(bool dma, bool subsets) { return dma ? 48 : (subsets ? 112 : 64); }
RZ_LDS_FN size_t crowd_poses_bytes(int G, int bones, bool dma, bool subsets) { return (size_t)G * bones * crowd_slot(dma, subsets); }
RZ_LDS_FN Crowd crowd(int G, int bones, bool dma, bool subsets, uint32_t morph_pad)
{
    return { crowd_slot(dma, subsets), crowd_poses_bytes(G, bones, dma, subsets), (size_t)G * morph_pad * 4, (size_t)G * bones * 48 };
}

// ---- crowd, fused-front form (kernels/crowd.hip: rz_skin_instances_fk_kernel) ----
// matrix buffer A | matrix buffer B (G x closure x 3 float4 each) | palettes (G x named x 3 float4) | the group's morph weights
struct CrowdFront {
    size_t buffer_rows;         // float4: one matrix buffer; B starts one behind A, the palettes two
    size_t weights_off;         // bytes: G x (2 closure + named) x 48
    size_t weights;             // bytes
    RZ_LDS_FN size_t total() const { return weights_off + weights; }
};
RZ_LDS_FN CrowdFront crowd_front(int G, int closure, int named, uint32_t morph_pad)
{
    return { (size_t)G * closure * 3, (size_t)G * (2 * (size_t)closure + named) * 48, (size_t)G * morph_pad * 4 };
}

// ---- after-physics (kernels/after.hip): the instance's world rows, 48 B per bone | one skip byte per entry, rounded ----
struct After {
    size_t skip_off, skip;      // bytes
    RZ_LDS_FN size_t total() const { return skip_off + skip; }
};
RZ_LDS_FN After after(int B, int n) { return { (size_t)B * 48, round16((size_t)n) }; }

// ---- QDEF pass (kernels/qdef.hip): the skeleton's dual quaternions, 2 float4 per bone ----
struct Qdef {
    size_t dq;                  // bytes
    RZ_LDS_FN size_t total() const { return dq; }
};
RZ_LDS_FN Qdef qdef(int B) { return { (size_t)B * 32 }; }

}  // namespace rzlds
