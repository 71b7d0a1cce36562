// The frame kernel's record (reze-engine_amd/csrc/frame_kernel.h) over the whole input domain of its resolver, for
// tests/test_frame_kernel_cpu.py: one line per input with the input, the record, whether the product / the all-variants build carries the
// instantiation, and its full symbol. Includes the header alone; built under AddressSanitizer and UBSan and run as a program.
#include "../reze-engine_amd/csrc/frame_kernel.h"

#include <stdlib.h>
#include <string.h>

static long n_lines = 0;

static void emit(const RzFrameKernelIn &in)
{
    const RzFrameKernel k = rz_frame_kernel(in);
    char sym[160];
    const int n = k.symbol(sym, sizeof sym);
    if (n <= 0 || n >= (int)sizeof sym || strlen(sym) != (size_t)n) { printf("bad symbol length %d\n", n); exit(1); }
    // the no-padding claim frame_signature() relies on: two resolutions of one input are the same bytes
    const RzFrameKernel again = rz_frame_kernel(in);
    if (memcmp(&k, &again, sizeof k) != 0) { printf("records of one input differ\n"); exit(1); }
    printf("in mode=%d S=%d U=%d nt=%d nts=%d geo=%d fast=%d consumer=%d fk_on=%d fk_kind=%d q24=%d group=%d block=%d subsets=%d subfk=%d morphs=%d ppw=%d"
           " : family=%d S=%d U=%d mode=%d fkv=%d block=%d group=%d ppw=%d kv=%d nt=%d nts=%d geo=%d fast=%d q24=%d sub=%d morph=%d solve=%d"
           " : product=%d all=%d : %s\n",
           in.v.mode, in.v.S, in.v.U, in.v.nt, in.v.nts, in.v.geo, in.v.fast, in.consumer, in.fk_on, in.fk_kind, in.q24, in.inst_group, in.inst_block, in.subsets,
           in.subfk, in.inst_morphs, in.poses_per_wg, k.family, k.S, k.U, k.mode, k.fkv, k.block, k.group, k.poses_per_wg, k.kv, k.nt, k.nts, k.geo, k.fast,
           k.q24, k.sub, k.morph, k.solve, k.in_product(), k.carried(true), sym);
    ++n_lines;
}

int main()
{
    static_assert(rz_frame_kernel(RzFrameKernelIn{ { 1, 2, 8, true, true, false, true }, false, false, 0, false, 0, 0, false, false, false, 0 }).fkv == 3, "the resolver is a constant expression");
    const int splits[4] = { 1, 2, 4, 8 }, unrolls[2] = { 4, 8 }, blocks[3] = { 256, 512, 1024 }, groups[2] = { 2, 8 };
    // one mesh: every variant x consumer x the fused solve and its kinds x 24-bit planes
    for (int mode = 0; mode < 3; ++mode)
        for (int S : splits)
            for (int U : unrolls)
                for (int bits = 0; bits < 64; ++bits)
                    for (int fk_on = 0; fk_on < 2; ++fk_on)
                        for (int kind = 0; kind < 3; ++kind) {
                            RzFrameKernelIn in = {};
                            in.v.mode = mode; in.v.S = S; in.v.U = U;
                            in.v.nt = bits & 1; in.v.nts = bits & 2; in.v.geo = bits & 4; in.v.fast = bits & 8; in.consumer = bits & 16; in.q24 = bits & 32;
                            in.fk_on = fk_on; in.fk_kind = kind;
                            emit(in);
                        }
    // crowds (no dense targets: modes 0 / 2 with the MORPH half): block x subsets x fk front x morphs x nts, two pose-group sizes
    for (int block : blocks)
        for (int bits = 0; bits < 16; ++bits)
            for (int G : groups) {
                RzFrameKernelIn in = {};
                in.v.mode = (bits & 4) ? 2 : 0; in.v.S = 4; in.v.U = 8; in.v.nt = true; in.v.nts = bits & 8;
                in.inst_group = G; in.inst_block = block; in.subsets = bits & 1; in.subfk = bits & 2; in.inst_morphs = bits & 4;
                if (in.subfk && !in.subsets) continue;       // the fk front is a subset form (plan.cpp: subfk is decided inside the subset branch)
                emit(in);
            }
    // the register form
    for (int nts = 0; nts < 2; ++nts) {
        RzFrameKernelIn in = {};
        in.v.S = 1; in.v.U = 8; in.v.nt = true; in.v.nts = nts; in.poses_per_wg = 5;
        emit(in);
    }
    printf("ok all %ld\n", n_lines);
    return 0;
}
