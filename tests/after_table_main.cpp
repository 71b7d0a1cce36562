// A stand-alone program around reze-engine_amd/csrc/after_table.h (the GPU-free half of rz_upload_after_physics): it reads a hierarchy and
// an ordered list of after-physics bones as text and prints what the call would refuse or upload, for tests/test_after_cpu.py to compare
// with the level arithmetic restated in tests/after_ref.py. Also the program to build under -fsanitize=address,undefined.
//   input:  B; then per bone: parent append_parent append_ratio append_move bind3; then n; then the n bones
//   output: "error <message>", or the lines level / level_off / index / sorted (the entries' bones in record order) / rec (12 words per entry)
#include "../reze-engine_amd/csrc/after_table.h"

#include <cstdio>
#include <iostream>

int main()
{
    uint32_t B, n;
    std::cin >> B;
    if (!std::cin || B == 0 || B > (1u << 20)) { std::cerr << "bad count\n"; return 2; }
    std::vector<uint32_t> rec((size_t)B * 16, 0u);
    for (uint32_t b = 0; b < B; ++b) {
        int parent, ap, move;
        float ratio, bind[3];
        std::cin >> parent >> ap >> ratio >> move >> bind[0] >> bind[1] >> bind[2];
        uint32_t *r = rec.data() + (size_t)b * 16;
        r[0] = (uint32_t)parent; r[1] = (uint32_t)ap; r[3] = move ? 1u : 0u;
        memcpy(&r[2], &ratio, 4);
        memcpy(&r[4], bind, 12);
    }
    std::cin >> n;
    if (!std::cin || n > (1u << 20)) { std::cerr << "short input\n"; return 2; }
    std::vector<uint32_t> bones(n);
    for (uint32_t k = 0; k < n; ++k) std::cin >> bones[k];
    if (!std::cin) { std::cerr << "short input\n"; return 2; }
    rzafter::Table t;
    std::string err;
    if (rzafter::build(B, rec.data(), n, bones.data(), t, err)) { printf("error %s\n", err.c_str()); return 0; }
    printf("level");
    for (int v : t.level) printf(" %d", v);
    printf("\nlevel_off");
    for (int v : t.level_off) printf(" %d", v);
    printf("\nindex");
    for (int v : t.index) printf(" %d", v);
    printf("\nsorted");
    for (uint32_t k = 0; k < n; ++k) printf(" %u", t.rec[(size_t)k * 12 + 7]);
    printf("\nrec");
    for (uint32_t v : t.rec) printf(" %u", v);
    printf("\nlds %zu\n", rzafter::lds_bytes(B, n));
    return 0;
}
