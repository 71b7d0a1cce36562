// tests/lds_layout_main.cpp — reze-engine_amd/csrc/lds_layout.h compiled alone by a host compiler (tests/test_lds_layout_cpu.py, under
// AddressSanitizer and UBSan): every family's regions over a small grid, each as `name offset bytes`, placed by the offsets and sizes the
// layout returns, added the way its kernel adds them (the comments name the kernel's lines), and the layout's total(). The test restates
// every region in Python. The physics stage's arithmetic (physics_table.h) rides along for its limit.
#include <stdio.h>

#include "../reze-engine_amd/csrc/lds_layout.h"
#include "../reze-engine_amd/csrc/physics_table.h"

using namespace rzlds;

static void begin(const char *what) { printf("%s :", what); }
static void region(const char *name, size_t off, size_t bytes) { printf(" %s %zu %zu ;", name, off, bytes); }
static void end(size_t total) { printf(" total %zu\n", total); }

int main()
{
    char what[256];
    printf("limits cu %zu optin %zu half %zu crowd %zu reserve %zu fit %zu %zu piece %zu %zu %d physics %zu\n", kCuLds, kOptIn, kHalfCu, kCrowdLarge, kSkeletonReserve,
           kFuseFitPerMorph, kFuseFitMargin, kPieceRoom, kPieceSlack, kMinPiece, rzphys::kLdsLimit);

    // hierarchy solve (kernels/front.hip: scr = smem + palette, mw = scr + scratch, IK: second buffer = mw + weights)
    for (int B : { 1, 7, 200, 513, 1051 }) for (int ik = 0; ik < 2; ++ik) for (int n : { 0, 1, 5, 64, 301 }) {
        const Solve L = solve(B, ik != 0, n);
        snprintf(what, sizeof what, "solve B=%d ik=%d n=%d", B, ik, n);
        begin(what);
        region("palette", 0, L.palette);
        region("scratch", L.palette, L.scratch);
        region("weights", L.palette + L.scratch, L.weights);
        region("second", L.palette + L.scratch + L.weights, L.second);
        printf(" scalars %zu %zu ;", palette_bytes(B), solve_scratch(B));     // what rz_fk_kernel adds for the first two regions
        end(L.total());
    }
    // generic frame (kernels/deform_small.hip / deform_dense.hip: s_idx = smem + list_off, s_w = s_idx + pad, scratch_all = s_w + pad,
    // ob_pos = scratch_all + scratch, sp_all = scratch_all + scratch + parked; the fused solve aliases scratch_all)
    for (int B : { 1, 349, 3200, 3242 }) for (int pad : { 0, 12, 72 }) for (int planes : { 3, 9 }) for (int vw : { 32, 64, 256 }) for (uint32_t oc : { 0u, 64u, 640u })
        for (uint32_t sp : { 0u, 16u, 64u, 2048u }) for (int fused = 0; fused < 2; ++fused) {
            const int M = pad ? pad - 8 : 0;
            const Frame L = frame(B, pad, planes, vw, oc, sp, fused != 0, M);
            snprintf(what, sizeof what, "frame B=%d pad=%d planes=%d vw=%d out_cap=%u sp_cap=%u fused=%d M=%d", B, pad, planes, vw, oc, sp, fused, M);
            begin(what);
            region("palette", 0, L.list_off);
            region("idx", L.list_off, (size_t)L.pad * 4);
            region("w", L.list_off + (size_t)L.pad * 4, (size_t)L.pad * 4);
            const size_t work = L.list_off + (size_t)L.pad * 8;
            region("scratch", work, L.scratch * 4);
            region("parked", work + L.scratch * 4, L.parked * 4);
            region("pieces", work + (L.scratch + L.parked) * 4, L.pieces);
            printf(" alias %zu %zu ; work %zu ;", work, L.fused, L.work());
            end(L.total());
        }
    for (int B : { 200, 1478, 1479, 1480 }) for (uint32_t M : { 0u, 64u, 300u }) printf("fused_fit B=%d M=%u : %zu\n", B, M, fused_fit_bytes(B, M));
    // crowd, pose-group form (kernels/crowd.hip: stage = smem + staged_off, s_mw = smem + weights_off)
    for (int G : { 2, 3, 8, 64 }) for (int bones : { 1, 34, 200 }) for (int dma = 0; dma < 2; ++dma) for (int sub = 0; sub < 2; ++sub) for (uint32_t mp : { 0u, 12u, 40u, 608u }) {
        const Crowd L = crowd(G, bones, dma != 0, sub != 0, mp);
        snprintf(what, sizeof what, "crowd G=%d bones=%d dma=%d subsets=%d morph_pad=%u slot=%d", G, bones, dma, sub, mp, L.slot);
        begin(what);
        region("slots", 0, L.weights_off);
        region("weights", L.weights_off, L.weights);
        printf(" staged_off %zu ; poses_bytes %zu ;", L.staged_off, crowd_poses_bytes(G, bones, dma != 0, sub != 0));       // the subset form's split of a slot; the MORPH kernels' scalar
        end(L.total());
    }
    // crowd, fused-front form (mA = smem, mB = mA + buffer_rows, pal = mB + buffer_rows, s_mw = smem + weights_off)
    for (int G : { 2, 4, 8 }) for (int closure : { 1, 43, 138, 139 }) for (int named : { 1, 34, 138 }) for (uint32_t mp : { 0u, 40u }) {
        const CrowdFront L = crowd_front(G, closure, named, mp);
        snprintf(what, sizeof what, "crowd_front G=%d closure=%d named=%d morph_pad=%u", G, closure, named, mp);
        begin(what);
        region("A", 0, L.buffer_rows * 16);
        region("B", L.buffer_rows * 16, L.buffer_rows * 16);
        region("palettes", 2 * L.buffer_rows * 16, (size_t)G * named * 48);
        region("weights", L.weights_off, L.weights);
        end(L.total());
    }
    // after-physics (kernels/after.hip: skip = smem + skip_off) and QDEF
    for (int B : { 1, 200, 3242 }) for (int n : { 1, 15, 16, 17, 513 }) {
        const After L = after(B, n);
        snprintf(what, sizeof what, "after B=%d n=%d", B, n);
        begin(what);
        region("rows", 0, L.skip_off);
        region("skip", L.skip_off, L.skip);
        end(L.total());
    }
    for (int B : { 1, 200, 3242 }) {
        snprintf(what, sizeof what, "qdef B=%d", B);
        begin(what);
        region("dq", 0, qdef(B).dq);
        end(qdef(B).total());
    }
    for (int nb : { 1, 25, 64, 65, 1516, 1706, 1707 }) for (int nj : { 0, 20, 64, 65, 256, 257, 1516 }) {
        const int block = nb <= 64 ? 64 : 256;
        printf("physics nb=%d nj=%d block=%d : %zu %zu\n", nb, nj, block, rzphys::lds_bytes(nb, nj, block, false), rzphys::lds_bytes(nb, nj, block, true));
    }
    printf("ok all\n");
    return 0;
}
