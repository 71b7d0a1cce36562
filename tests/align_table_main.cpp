// A stand-alone program around reze-engine_amd/csrc/physics_table.h for rz_physics_aligned: it reads a table as text (the input of
// tests/physics_table_main.cpp) and prints what rzphys::derive — the GPU-free half of rz_upload_physics and of rz_physics_aligned — makes
// of it with the feature on or off (argv[1] = 1 | 0): the refusal, or the counts, the colouring, the overridden bones, per body its
// override slot and aligned flag, the body and joint records and the launch form with its LDS; and whether all of that equals, byte for
// byte, what the plain calls of the header (validate + build with the arguments they always had) derive. For tests/test_align_cpu.py to
// compare with tests/align_ref.py and tests/physics_ref.py; built there under -fsanitize=address,undefined.
#include "../reze-engine_amd/csrc/physics_table.h"

#include <cstdlib>
#include <iostream>

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

int main(int argc, char **argv)
{
    const bool on = argc > 1 && atoi(argv[1]) != 0;
    uint32_t B, nb, nj, iterations;
    int has_g, has_column;
    float h, g[3] = { 0, 0, 0 };
    std::cin >> B >> nb >> nj >> h >> iterations >> has_g >> has_column;
    if (has_g) std::cin >> g[0] >> g[1] >> g[2];
    std::vector<int32_t> parents(B), bone(nb);
    std::vector<float> bind(B * 3), size(nb * 3), op(nb * 3), oq(nb * 4), mass(nb), ld(nb), ad(nb);
    std::vector<uint8_t> type(nb), shape(nb);
    std::vector<uint32_t> ja(nj), jb(nj);
    std::vector<float> jf[8];
    for (auto &v : jf) v.resize(nj * 3);
    for (auto &p : parents) std::cin >> p;
    for (auto &x : bind) std::cin >> x;
    for (uint32_t b = 0; b < nb; ++b) {
        int ty, sh;
        std::cin >> bone[b] >> ty >> sh;
        type[b] = (uint8_t)ty; shape[b] = (uint8_t)sh;
        for (int k = 0; k < 3; ++k) std::cin >> size[b * 3 + k];
        for (int k = 0; k < 3; ++k) std::cin >> op[b * 3 + k];
        for (int k = 0; k < 4; ++k) std::cin >> oq[b * 4 + k];
        std::cin >> mass[b] >> ld[b] >> ad[b];
    }
    for (uint32_t j = 0; j < nj; ++j) {
        std::cin >> ja[j] >> jb[j];
        for (auto &v : jf)
            for (int k = 0; k < 3; ++k) std::cin >> v[j * 3 + k];
    }
    if (!std::cin) { std::cerr << "short input\n"; return 2; }
    rz_physics t;
    memset(&t, 0, sizeof t);
    t.n_bodies = nb; t.bone = bone.data(); t.type = type.data(); t.shape = shape.data(); t.size3 = size.data(); t.offset_pos3 = op.data();
    t.offset_rot4 = oq.data(); t.mass = mass.data(); t.linear_damping = ld.data(); t.angular_damping = ad.data();
    t.n_joints = nj; t.body_a = ja.data(); t.body_b = jb.data();
    t.position3 = jf[0].data(); t.rotation3 = jf[1].data(); t.position_min3 = jf[2].data(); t.position_max3 = jf[3].data();
    t.rotation_min3 = jf[4].data(); t.rotation_max3 = jf[5].data(); t.spring_rotation3 = jf[6].data();
    t.spring_position3 = has_column ? jf[7].data() : nullptr;
    t.gravity3 = has_g ? g : nullptr; t.h = h; t.iterations = iterations;
    // as the host goes: the call works on the kept copy of the table
    rzphys::Kept kept;
    kept.keep(&t);
    const rz_physics view = kept.view();
    rzphys::Derived d;
    std::string bad;
    const int rc = rzphys::derive(&view, B, parents.data(), bind.data(), on, d, bad);
    printf("refused %d %s\n", rc, bad.c_str());
    if (rc) return 0;
    const rzphys::Built &o = d.built;
    printf("counts %d %d %d %d %d %u\n", o.nb, o.nj, o.ncol, o.nd, o.widest, d.n_aligned);
    printf("colour");
    for (int c : o.colour) printf(" %d", c);
    printf("\norder");
    for (int c : o.order) printf(" %d", c);
    printf("\ncolour_off");
    for (int c : o.colour_off) printf(" %d", c);
    printf("\ndyn_bone");
    for (int c : o.dyn_bone) printf(" %d", c);
    printf("\ntypes");
    for (uint8_t c : d.types) printf(" %d", (int)c);
    printf("\nslot");
    for (int b = 0; b < o.nb; ++b) { int32_t v; memcpy(&v, &o.body[(size_t)b * 16 + 14], 4); printf(" %d", v); }
    printf("\nflag");
    for (int b = 0; b < o.nb; ++b) printf(" %.9g", o.body[(size_t)b * 16 + 15]);
    printf("\nbody");
    for (int b = 0; b < o.nb; ++b)
        for (int k = 0; k < 13; ++k) printf(" %.9g", o.body[(size_t)b * 16 + k]);
    printf("\njoint");
    for (int j = 0; j < o.nj; ++j)
        for (int k = 0; k < 32; ++k)
            if (k != 3 && k != 7 && k != 31) printf(" %.9g", o.joint[(size_t)j * 32 + k]);
    printf("\nends");
    for (int j = 0; j < o.nj; ++j) { int32_t a, b; memcpy(&a, &o.joint[(size_t)j * 32 + 3], 4); memcpy(&b, &o.joint[(size_t)j * 32 + 7], 4); printf(" %d %d", a, b); }
    const int block = rzphys::block_for(o.nb, o.widest);
    printf("\nform %d %d\n", block, o.nj <= block ? 1 : 0);
    printf("lds %zu %zu\n", rzphys::lds_bytes(o.nb, o.nj, block, false), rzphys::lds_bytes(o.nb, o.nj, block, true));
    // the plain build, through the calls the header always had
    rzphys::Built p;
    const std::string plain_bad = rzphys::validate(&t, B);
    if (plain_bad.empty()) {
        rzphys::build(&t, B, parents.data(), bind.data(), p);
        const bool eq = same(o.body, p.body) && same(o.joint, p.joint) && same(o.colour, p.colour) && same(o.order, p.order) && same(o.colour_off, p.colour_off) &&
                        same(o.dyn_bone, p.dyn_bone) && o.nb == p.nb && o.nj == p.nj && o.ncol == p.ncol && o.nd == p.nd && o.widest == p.widest &&
                        o.iterations == p.iterations && !memcmp(&o.h, &p.h, 4) && !memcmp(o.g, p.g, 12) && o.hd == p.hd;
        printf("plain_equal %d\n", eq ? 1 : 0);
        printf("plain_form %d %d\n", rzphys::block_for(p.nb, p.widest), p.nj <= rzphys::block_for(p.nb, p.widest) ? 1 : 0);
    }
    // the kept table stays the caller's
    printf("kept_types");
    for (uint8_t c : kept.type) printf(" %d", (int)c);
    printf("\n");
    return 0;
}
