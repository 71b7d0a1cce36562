// A stand-alone program around reze-engine_amd/csrc/contact_table.h (the GPU-free half of rz_physics_contacts): it reads the columns of a
// table that decide contacts as text and prints the lists rz_physics_contacts(ctx, mode) would upload, for tests/test_contact_cpu.py,
// tests/test_contact_box_cpu.py and tests/test_contact_boxbox_cpu.py to compare with tests/contact_ref.py's contact_lists(table, mode).
// Also the program to build under -fsanitize=address,undefined.
//   usage:  contact_table_main [mode: 1 | 2 | 3]  (1 without the argument; the same lines under every mode)
//   input:  nb; then per body: type shape group mask size3 mass friction
#include "../reze-engine_amd/csrc/contact_table.h"

#include <iostream>

int main(int argc, char **argv)
{
    const int mode = argc > 1 ? argv[1][0] - '0' : 1;
    if (argc > 2 || mode < 1 || mode > 3 || (argc > 1 && argv[1][1])) { std::cerr << "usage: contact_table_main [1 | 2 | 3]\n"; return 2; }
    uint32_t nb;
    std::cin >> nb;
    if (!std::cin || nb > (1u << 20)) { std::cerr << "bad count\n"; return 2; }
    std::vector<uint8_t> type(nb), shape(nb), group(nb);
    std::vector<uint16_t> mask(nb);
    std::vector<float> size(nb * 3), mass(nb), friction(nb);
    for (uint32_t b = 0; b < nb; ++b) {
        int ty, sh, gr, mk;
        std::cin >> ty >> sh >> gr >> mk;
        type[b] = (uint8_t)ty; shape[b] = (uint8_t)sh; group[b] = (uint8_t)gr; mask[b] = (uint16_t)mk;
        for (int k = 0; k < 3; ++k) std::cin >> size[b * 3 + k];
        std::cin >> mass[b] >> friction[b];
    }
    if (!std::cin) { std::cerr << "short input\n"; return 2; }
    rz_physics t;
    memset(&t, 0, sizeof t);
    t.n_bodies = nb; t.type = type.data(); t.shape = shape.data(); t.group = group.data(); t.mask = mask.data(); t.size3 = size.data();
    t.mass = mass.data(); t.friction = friction.data();
    rzphys::Contacts o;
    rzphys::build_contacts(&t, o, mode);
    printf("counts %zu %zu %d %d\n", o.n_follow, o.n_pairs, o.ncol, o.boxes);
    printf("refused %d %s\n", o.too_many ? 1 : 0, o.too_many ? rzphys::contacts_refusal(o).c_str() : "");
    printf("shape");
    for (uint32_t b = 0; b < nb; ++b) {
        int32_t flags;
        memcpy(&flags, &o.shape[(size_t)b * 4 + 3], 4);
        printf(" %.9g %.9g %.9g %d", o.shape[(size_t)b * 4], o.shape[(size_t)b * 4 + 1], o.shape[(size_t)b * 4 + 2], flags);
    }
    printf("\nfollow_off");
    for (int v : o.follow_off) printf(" %d", v);
    printf("\nfollow_idx");
    for (int v : o.follow_idx) printf(" %d", v);
    printf("\npair");
    for (int v : o.pair) printf(" %d", v);
    printf("\ncolour_off");
    for (int v : o.colour_off) printf(" %d", v);
    printf("\nbox_pairs %zu", o.box_pairs);
    printf("\nbox_box %zu", o.n_box_box);
    printf("\nbox");
    for (float v : o.box) printf(" %.9g", v);
    printf("\n");
    return 0;
}
