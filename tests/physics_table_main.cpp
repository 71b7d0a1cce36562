// A stand-alone program around reze-engine_amd/csrc/physics_table.h (the GPU-free half of rz_upload_physics and of rz_physics_springs): it
// reads a table as text and prints what the two calls would derive from it — the validation message, the colouring, the body / joint
// records; then, from the kept copy of the table (Kept::keep and view(), as the host goes), the launch form, the LDS of both forms, the
// springs' refusal and the linear records in solve order — for tests/test_physics_cpu.py to compare with tests/physics_ref.py and
// tests/test_spring_cpu.py with tests/spring_ref.py. tests/physics_scenes.py writes the input and builds it under
// -fsanitize=address,undefined.
//   input:  B nb nj h iterations has_gravity has_column [gx gy gz]; parents[B]; bind[B*3]; then per body: bone type shape size3 offset_pos3
//           offset_rot4 mass linear_damping angular_damping; per joint: body_a body_b position3 rotation3 position_min3 position_max3
//           rotation_min3 rotation_max3 spring_rotation3 spring_position3 (has_column = 0: read, and handed on as NULL)
#include "../reze-engine_amd/csrc/physics_table.h"

#include <iostream>

int main()
{
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
    // what rz_physics_springs derives later, from the copy rz_upload_physics keeps
    rzphys::Kept kept;
    kept.keep(&t);
    const float *column = kept.view().spring_position3;
    const int block = rzphys::block_for(o.nb, o.widest);
    rzphys::Linear lin;
    if (column) rzphys::build_linear(column, o.order, o.hd, lin);
    bool invalid = false;
    const std::string no = rzphys::springs_refusal(o.nb, o.nj, block, column != nullptr, lin.axes, invalid);
    printf("form %d %d\n", block, o.nj <= block ? 1 : 0);
    printf("lds %zu %zu\n", rzphys::lds_bytes(o.nb, o.nj, block, false), rzphys::lds_bytes(o.nb, o.nj, block, true));
    printf("refused %d %s\n", no.empty() ? 0 : invalid ? RZ_ERR_INVALID : RZ_ERR_UNSUPPORTED, no.c_str());
    printf("axes %d\n", lin.axes);
    printf("alpha");
    for (size_t k = 0; k < lin.rec.size(); ++k)
        if (k % 4 != 3) printf(" %.9g", lin.rec[k]);
    printf("\nbits");
    for (size_t k = 3; k < lin.rec.size(); k += 4) { int32_t v; memcpy(&v, &lin.rec[k], 4); printf(" %d", v); }
    printf("\n");
    return 0;
}
