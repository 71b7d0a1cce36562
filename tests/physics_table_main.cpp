// A stand-alone program around reze-engine_amd/csrc/physics_table.h (the GPU-free half of rz_upload_physics): it reads a table as text,
// and prints what the upload would derive from it — the validation message, the colouring, and the body / joint records — for
// tests/test_physics_cpu.py to compare with tests/physics_ref.py. Also the program to build under -fsanitize=address,undefined.
//   input:  B nb nj h iterations has_gravity [gx gy gz]; parents[B]; bind[B*3]; then per body: bone type shape size3 offset_pos3 offset_rot4
//           mass linear_damping angular_damping; per joint: body_a body_b position3 rotation3 position_min3 position_max3 rotation_min3
//           rotation_max3 spring_rotation3
#include "../reze-engine_amd/csrc/physics_table.h"

#include <iostream>

int main()
{
    uint32_t B, nb, nj, iterations;
    int has_g;
    float h, g[3] = { 0, 0, 0 };
    std::cin >> B >> nb >> nj >> h >> iterations >> has_g;
    if (has_g) std::cin >> g[0] >> g[1] >> g[2];
    std::vector<int32_t> parents(B), bone(nb);
    std::vector<float> bind(B * 3), size(nb * 3), op(nb * 3), oq(nb * 4), mass(nb), ld(nb), ad(nb);
    std::vector<uint8_t> type(nb), shape(nb);
    std::vector<uint32_t> ja(nj), jb(nj);
    std::vector<float> jf[7];
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
    t.gravity3 = has_g ? g : nullptr; t.h = h; t.iterations = iterations;
    const std::string bad = rzphys::validate(&t, B);
    printf("valid %d %s\n", bad.empty() ? 1 : 0, bad.c_str());
    if (!bad.empty()) return 0;
    rzphys::Built o;
    rzphys::build(&t, B, parents.data(), bind.data(), o);
    printf("counts %d %d %d %d %d %d %.9g\n", o.nb, o.nj, o.ncol, o.nd, o.widest, o.iterations, o.h);
    printf("gravity %.9g %.9g %.9g\n", o.g[0], o.g[1], o.g[2]);
    printf("colour");
    for (int c : o.colour) printf(" %d", c);
    printf("\norder");
    for (int c : o.order) printf(" %d", c);
    printf("\ncolour_off");
    for (int c : o.colour_off) printf(" %d", c);
    printf("\nbody");
    for (int b = 0; b < o.nb; ++b)
        for (int k = 0; k < 13; ++k) printf(" %.9g", o.body[(size_t)b * 16 + k]);
    printf("\njoint");
    for (int j = 0; j < o.nj; ++j)
        for (int k = 0; k < 32; ++k)
            if (k != 3 && k != 7 && k != 31) printf(" %.9g", o.joint[(size_t)j * 32 + k]);
    printf("\n");
    return 0;
}
