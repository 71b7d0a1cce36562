// frame_kernel.h — which instantiation of the frame's kernel a frame launches. ONE statement: rz_frame_kernel() resolves an RzFrameKernel from the
// facts it depends on; frame.cpp launches it and hashes it into the graph key, the kernel files switch on its fields and decide nothing, rz_get_tuning
// reads the effective_* keys from it. Plain C++ without a HIP header, so a host compiler builds it alone (tests/frame_kernel_main.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <type_traits>
#pragma GCC visibility push(hidden)     // nothing here is part of the C ABI: an inline function a host file keeps out of line must not become an export

// Compile-time variant selection of the single-mesh frame kernels (kernels/deform_dense.hip, kernels/deform_small.hip), as a plan asks for it.
struct RzVariant {
    int mode, S, U;             // morph targets 0 none, 1 dense, 2 sparse; morph split 1,2,4,8 (mode 1 only); 4 or 8 morphs in flight
    bool nt, nts, geo, fast;    // nontemporal morph loads; nontemporal output stores; rest geometry through LDS; fused palette + kernarg morph list (single instance)
};
enum RzFrameFamily : int32_t {
    kRzSmall,       // rz_deform_small_kernel<S, MODE, NTS, GEO, FAST, FKV>             one mesh without dense targets
    kRzDense,       // rz_deform_dense_kernel<S, U, NT, NTS, GEO, FAST, FKV, Q24>       one mesh, the dense morph stream
    kRzCrowd,       // rz_skin_instances[_morph]_kernel<BLOCK, NTS, SUB>                pose groups of a crowd
    kRzCrowdFk,     // rz_skin_instances_fk[_morph]_kernel<BLOCK, NTS>                  ... with the hierarchy solved in the kernel's front
    kRzCrowdReg,    // rz_skin_instances_reg_kernel<KV, NTS>                            the register-resident crowd form (tools-only)
};
// What the resolver reads: the plan's variant and crowd fields, and three facts of the parameter block (RzDeformParams).
struct RzFrameKernelIn {
    RzVariant v;
    bool consumer;              // a fused consumer is on: the outline hull or the bounding box (edge || aabb)
    bool fk_on; int fk_kind;    // the frame solves its hierarchy in the kernel; the solve specialised for a plain uploaded (1) / sampled (2) pose
    bool q24;                   // 24-bit dense morph planes are resident
    int inst_group, inst_block; bool subsets, subfk, inst_morphs; int poses_per_wg;      // Plan
};
// The complete compile-time identity of a frame's kernel: the family and its template arguments. The variant's fields are filled for
// every family (a crowd frame's are those of the single-mesh kernel it would otherwise run: the effective_* keys report them), the
// crowd fields are zero outside the crowd families. No padding: frame_signature() hashes the struct.
struct RzFrameKernel {
    int32_t family;             // RzFrameFamily
    int32_t S, U, mode, fkv;    // S, U as the kernels are instantiated (1 / 2 / 4 / 8 dense, 1 / 4 else; 4 / 8); mode = MODE (0 / 2) or 1 = dense
    int32_t block, group, poses_per_wg, kv;     // BLOCK and poses per workgroup of the pose-group forms; poses per workgroup and KV of the register form
    bool nt, nts, geo, fast, q24;
    bool sub, morph;            // SUB; the MORPH half (kernels/crowd_morph.hip)
    bool solve;                 // the kernel solves the hierarchy itself: the frame has no rz_fk_kernel in front

    // Is this instantiation compiled into the build — the product's (all_variants = false) or the tools-only one with every variant? The
    // product carries the shapes a plan selects by default; no build carries an FKV the rule in rz_frame_kernel cannot give, or a 1024-thread
    // MORPH front (128 VGPRs do not hold its two work items beside the row walk without scratch: the plan keeps rz_fk_kernel in front there).
    constexpr bool carried(bool all_variants) const
    {
        const bool selectable = !geo && (family != kRzDense || (nt && U == 8));
        switch (family) {
        case kRzSmall: case kRzDense: return (all_variants || selectable) && (fkv == 0 || (selectable && (fkv == 3 || !fast)));
        case kRzCrowd: return true;
        case kRzCrowdFk: return !(morph && block == 1024);
        default: return all_variants;
        }
    }
    constexpr bool in_product() const { return carried(false); }
    // The demangled symbol with ALL template arguments, as the compiler spells it (DeformContext.kernel_name() leaves the dense kernel's eighth out).
    int symbol(char *out, size_t n) const
    {
        auto tf = [](bool b) { return b ? "true" : "false"; };
        switch (family) {
        case kRzSmall: return snprintf(out, n, "rz_deform_small_kernel<%d, %d, %s, %s, %s, %d>", S, mode, tf(nts), tf(geo), tf(fast), fkv);
        case kRzDense: return snprintf(out, n, "rz_deform_dense_kernel<%d, %d, %s, %s, %s, %s, %d, %s>", S, U, tf(nt), tf(nts), tf(geo), tf(fast), fkv, tf(q24));
        case kRzCrowd: return snprintf(out, n, "rz_skin_instances%s_kernel<%d, %s, %s>", morph ? "_morph" : "", block, tf(nts), tf(sub));
        case kRzCrowdFk: return snprintf(out, n, "rz_skin_instances_fk%s_kernel<%d, %s>", morph ? "_morph" : "", block, tf(nts));
        default: return snprintf(out, n, "rz_skin_instances_reg_kernel<%d, %s>", kv, tf(nts));
        }
    }
};
static_assert(sizeof(RzFrameKernel) == 9 * 4 + 8, "RzFrameKernel has no padding: frame_signature() hashes it");

constexpr RzFrameKernel rz_frame_kernel(const RzFrameKernelIn &in)
{
    const RzVariant &v = in.v;
    RzFrameKernel k{};
    k.family = in.poses_per_wg > 0 ? kRzCrowdReg : in.inst_group > 0 ? (in.subfk ? kRzCrowdFk : kRzCrowd) : v.mode == 1 ? kRzDense : kRzSmall;
    k.mode = v.mode == 1 ? 1 : (v.mode == 0 ? 0 : 2);
    k.S = v.mode == 1 ? ((v.S == 2 || v.S == 4 || v.S == 8) ? v.S : 1) : (v.S == 4 ? 4 : 1);
    k.U = v.U >= 8 ? 8 : 4;
    k.nt = v.nt; k.nts = v.nts; k.geo = v.geo; k.fast = v.fast;
    // The one FKV rule. 3 (no fused consumers compiled in) only for a shape a plan selects by default — rest geometry by plain loads, and
    // for dense targets nontemporal loads eight deep — with no consumer on; 1 / 2 (3 with the specialised solve) only when such a frame is
    // not the one-launch form and solves a plain uploaded / sampled pose itself; 0 (everything compiled in) for everything else.
    const bool selectable = !v.geo && (v.mode != 1 || (v.nt && v.U >= 8));
    k.fkv = (!selectable || in.consumer) ? 0 : (!v.fast && in.fk_on && (in.fk_kind == 1 || in.fk_kind == 2)) ? in.fk_kind : 3;
    k.q24 = k.family == kRzDense && in.q24;
    if (k.family == kRzCrowd || k.family == kRzCrowdFk) {
        k.block = in.inst_block == 1024 ? 1024 : (in.inst_block == 512 ? 512 : 256);
        k.group = in.inst_group;
        k.sub = in.subsets; k.morph = in.inst_morphs;
    }
    if (k.family == kRzCrowdReg) { k.poses_per_wg = in.poses_per_wg; k.kv = 8; }
    k.solve = in.fk_on || k.family == kRzCrowdFk;
    return k;
}

// run-time value -> template argument: f(std::integral_constant<T, V>{}) for the V of Vs that equals v, `none` when there is none
#define RZ_V(x) decltype(x)::value      // ... and the V of such an argument
template <typename T, T... Vs, typename R, typename F> inline R rz_pick(T v, R none, F &&f)
{
    R r = none;
    (void)((v == Vs && ((r = f(std::integral_constant<T, Vs>{})), true)) || ...);
    return r;
}

#pragma GCC visibility pop
