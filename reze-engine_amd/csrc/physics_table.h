// physics_table.h — the host half of rz_upload_physics that needs no GPU: checking a table, colouring its joints and deriving the constants
// rz_physics_kernel runs on (deform_kernels.h: RzPhysicsParams); the owned copy of the columns later stages derive from (Kept); the solver's
// LDS arithmetic with its one limit (kLdsLimit, lds_bytes: host and launcher both read them here) and what is refused over it
// (upload_refusal, springs_refusal); the linear springs' records. Plain C++ on purpose, without HIP: tests/physics_table_main.cpp compiles it
// alone and holds it to tests/physics_ref.py and tests/spring_ref.py. Everything is computed in double from the table's floats and rounded
// once, as physics_ref.prepare does.
#pragma once
#include "../../include/reze_deform.h"
#include "lds_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace rzphys {

constexpr double kDefaultH = 1.0 / 75.0;
constexpr int kDefaultIterations = 4;

struct Built {
    std::vector<float> body;            // [nb][16]
    std::vector<float> joint;           // [nj][32], in solve order
    std::vector<int> colour, order, colour_off;
    std::vector<int> dyn_bone;          // bones of the dynamic bodies that have one, in body order: an instance's overrides
    int nb = 0, nj = 0, ncol = 0, nd = 0, widest = 0, iterations = kDefaultIterations;
    float h = (float)kDefaultH, g[3] = { 0.0f, -98.0f, 0.0f };
    double hd = kDefaultH;              // h before its rounding: what the spring constants are derived from
};

inline bool dynamic(const rz_physics *t, uint32_t b) { return t->type[b] == 1 && t->mass[b] > 0.0f; }

// rz_physics_aligned (tests/align_ref.py): with the feature on, a type-2 body with mass > 0 is simulated — read as type 1 —, and ALIGNED when
// it has a bone as well: its bone takes the body's rotation and keeps its own solved position. `types` becomes the table's type column as
// the solver reads it, `aligned` the per-body flag; the count of aligned bodies is returned. Off: the column as it is, no flag, 0.
inline uint32_t read_types(const rz_physics *t, bool on, std::vector<uint8_t> &types, std::vector<uint8_t> &aligned)
{
    const uint32_t nb = t->n_bodies;
    types.assign(t->type, t->type + nb);
    aligned.assign(nb, 0);
    uint32_t n = 0;
    if (on)
        for (uint32_t b = 0; b < nb; ++b)
            if (t->type[b] == 2 && t->mass[b] > 0.0f) {
                types[b] = 1;
                if (t->bone[b] >= 0) { aligned[b] = 1; ++n; }
            }
    return n;
}

inline bool finite_all(const float *p, size_t n)
{
    if (!p) return true;
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(p[k])) return false;
    return true;
}

// RZ_ERR_INVALID cases of rz_upload_physics; an empty string = the table is valid
inline std::string validate(const rz_physics *t, uint32_t B)
{
    char m[200];
    const uint32_t nb = t->n_bodies, nj = t->n_joints;
    if (!t->bone || !t->type || !t->shape || !t->size3 || !t->offset_pos3 || !t->offset_rot4 || !t->mass || !t->linear_damping || !t->angular_damping)
        return "physics table: null body arrays";
    if (nj && (!t->body_a || !t->body_b || !t->position3 || !t->rotation3 || !t->position_min3 || !t->position_max3 || !t->rotation_min3 || !t->rotation_max3 || !t->spring_rotation3))
        return "physics table: null joint arrays";
    const struct { const char *name; const float *p; size_t n; } fl[] = {
        { "size", t->size3, (size_t)nb * 3 }, { "offset_pos", t->offset_pos3, (size_t)nb * 3 }, { "offset_rot", t->offset_rot4, (size_t)nb * 4 },
        { "mass", t->mass, nb }, { "linear_damping", t->linear_damping, nb }, { "angular_damping", t->angular_damping, nb },
        { "restitution", t->restitution, nb }, { "friction", t->friction, nb },
        { "position", t->position3, (size_t)nj * 3 }, { "rotation", t->rotation3, (size_t)nj * 3 },
        { "position_min", t->position_min3, (size_t)nj * 3 }, { "position_max", t->position_max3, (size_t)nj * 3 },
        { "rotation_min", t->rotation_min3, (size_t)nj * 3 }, { "rotation_max", t->rotation_max3, (size_t)nj * 3 },
        { "spring_position", t->spring_position3, (size_t)nj * 3 }, { "spring_rotation", t->spring_rotation3, (size_t)nj * 3 },
        { "gravity", t->gravity3, 3 }, { "h", &t->h, 1 } };
    for (const auto &f : fl)
        if (!finite_all(f.p, f.n)) { snprintf(m, sizeof m, "physics table: %s is not finite", f.name); return m; }
    if (t->h < 0.0f) return "physics table: h must be > 0 (0 = the default 1/75 s)";
    for (uint32_t b = 0; b < nb; ++b) {
        if (t->bone[b] < -1 || t->bone[b] >= (int32_t)B) { snprintf(m, sizeof m, "physics table: body %u names bone %d (have %u)", b, t->bone[b], B); return m; }
        if (t->type[b] > 2) { snprintf(m, sizeof m, "physics table: body %u has type %u (0 follows its bone, 1 dynamic, 2 dynamic + bone)", b, (unsigned)t->type[b]); return m; }
        if (t->shape[b] > 2) { snprintf(m, sizeof m, "physics table: body %u has shape %u (0 sphere, 1 box, 2 capsule)", b, (unsigned)t->shape[b]); return m; }
        if (t->mass[b] < 0.0f) { snprintf(m, sizeof m, "physics table: body %u has a negative mass", b); return m; }
        if (t->linear_damping[b] < 0.0f || t->linear_damping[b] > 1.0f || t->angular_damping[b] < 0.0f || t->angular_damping[b] > 1.0f) {
            snprintf(m, sizeof m, "physics table: body %u has a damping outside [0, 1]", b); return m;
        }
        const float *q = t->offset_rot4 + (size_t)b * 4;
        if (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] <= 0.0f) { snprintf(m, sizeof m, "physics table: body %u has a zero offset rotation", b); return m; }
    }
    for (uint32_t j = 0; j < nj; ++j) {
        if (t->body_a[j] >= nb || t->body_b[j] >= nb) { snprintf(m, sizeof m, "physics table: joint %u names bodies %u and %u (have %u)", j, t->body_a[j], t->body_b[j], nb); return m; }
        if (t->body_a[j] == t->body_b[j]) { snprintf(m, sizeof m, "physics table: joint %u joins body %u to itself", j, t->body_a[j]); return m; }
    }
    std::vector<int> owner(B, -1);
    for (uint32_t b = 0; b < nb; ++b)
        if (dynamic(t, b) && t->bone[b] >= 0) {
            if (owner[t->bone[b]] >= 0) { snprintf(m, sizeof m, "physics table: dynamic bodies %d and %u both drive bone %d", owner[t->bone[b]], b, t->bone[b]); return m; }
            owner[t->bone[b]] = (int)b;
        }
    return "";
}

// Greedy, in file order: a joint takes the smallest colour in which no earlier joint shares a dynamic body with it
inline void colour_joints(const rz_physics *t, std::vector<int> &colour, std::vector<int> &order, int &ncol)
{
    const uint32_t nb = t->n_bodies, nj = t->n_joints;
    std::vector<std::vector<char>> used(nb);
    colour.assign(nj, 0);
    ncol = 0;
    for (uint32_t j = 0; j < nj; ++j) {
        const uint32_t ends[2] = { t->body_a[j], t->body_b[j] };
        int c = 0;
        for (;; ++c) {
            bool taken = false;
            for (uint32_t b : ends)
                if (dynamic(t, b) && (size_t)c < used[b].size() && used[b][c]) taken = true;
            if (!taken) break;
        }
        for (uint32_t b : ends)
            if (dynamic(t, b)) { if (used[b].size() <= (size_t)c) used[b].resize(c + 1, 0); used[b][c] = 1; }
        colour[j] = c;
        ncol = std::max(ncol, c + 1);
    }
    order.resize(nj);
    for (uint32_t j = 0; j < nj; ++j) order[j] = (int)j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return colour[a] < colour[b]; });
}

struct D3 { double x, y, z; };
struct D4 { double x, y, z, w; };
inline D3 cross(D3 a, D3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline D4 qmul(D4 a, D4 b)
{
    return { a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
             a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z };
}
inline D4 qconj(D4 a) { return { -a.x, -a.y, -a.z, a.w }; }
inline D4 qnorm(D4 a) { const double l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w); return { a.x / l, a.y / l, a.z / l, a.w / l }; }
inline D3 qrot(D4 q, D3 v)
{
    const D3 u = { q.x, q.y, q.z };
    D3 t = cross(u, v);
    t = { t.x + t.x, t.y + t.y, t.z + t.z };
    const D3 c = cross(u, t);
    return { v.x + q.w * t.x + c.x, v.y + q.w * t.y + c.y, v.z + q.w * t.z + c.z };
}
// math.ts Quat.fromEuler: how the loader's Euler angles become quaternions
inline D4 quat_from_pmx_euler(const float *r)
{
    const double cx = std::cos(r[0] * 0.5), sx = std::sin(r[0] * 0.5), cy = std::cos(r[1] * 0.5), sy = std::sin(r[1] * 0.5), cz = std::cos(r[2] * 0.5), sz = std::sin(r[2] * 0.5);
    return qnorm({ cy * sx * cz + sy * cx * sz, sy * cx * cz - cy * sx * sz, cy * cx * sz - sy * sx * cz, cy * cx * cz + sy * sx * sz });
}
inline float bits_of(int32_t v) { float f; memcpy(&f, &v, 4); return f; }

// parents[B] (-1 = root) and bind_translation3[B * 3]: the topology the hierarchy solve was given; the bind pose of a body is
// T(sum of the bind translations up its bone's parent chain) x offset. aligned (read_types; null = none): the bodies whose record carries
// the flag in its 16th float, 1.0f; t's type column is then the one read_types made.
inline void build(const rz_physics *t, uint32_t B, const int32_t *parents, const float *bind3, Built &o, const uint8_t *aligned = nullptr)
{
    const uint32_t nb = t->n_bodies, nj = t->n_joints;
    o.nb = (int)nb; o.nj = (int)nj;
    const double h = t->h > 0.0f ? (double)t->h : kDefaultH;
    o.h = (float)h; o.hd = h;
    o.iterations = t->iterations ? (int)t->iterations : kDefaultIterations;
    if (t->gravity3) for (int k = 0; k < 3; ++k) o.g[k] = t->gravity3[k];
    colour_joints(t, o.colour, o.order, o.ncol);
    o.colour_off.assign(o.ncol + 1, 0);
    for (uint32_t j = 0; j < nj; ++j) o.colour_off[o.colour[j] + 1]++;
    o.widest = 0;
    for (int c = 0; c < o.ncol; ++c) { o.widest = std::max(o.widest, o.colour_off[c + 1]); o.colour_off[c + 1] += o.colour_off[c]; }
    std::vector<D3> bx(nb);
    std::vector<D4> bq(nb);
    o.body.assign((size_t)nb * 16, 0.0f);
    o.dyn_bone.clear();
    for (uint32_t b = 0; b < nb; ++b) {
        D3 acc = { 0, 0, 0 };
        uint32_t guard = 0;
        for (int32_t p = t->bone[b]; p >= 0 && guard <= B; p = parents[p], ++guard) { acc.x += bind3[p * 3]; acc.y += bind3[p * 3 + 1]; acc.z += bind3[p * 3 + 2]; }
        const float *op = t->offset_pos3 + (size_t)b * 3, *oq = t->offset_rot4 + (size_t)b * 4, *sz = t->size3 + (size_t)b * 3;
        bx[b] = { acc.x + op[0], acc.y + op[1], acc.z + op[2] };
        bq[b] = qnorm({ oq[0], oq[1], oq[2], oq[3] });
        const bool dyn = dynamic(t, b);
        const double m = t->mass[b];
        double I[3] = { 0, 0, 0 };
        if (dyn) {
            if (t->shape[b] == 0) I[0] = I[1] = I[2] = 0.4 * m * sz[0] * sz[0];
            else {
                const double a = sz[0], bb = t->shape[b] == 1 ? sz[1] : sz[0] + 0.5 * sz[1], c = t->shape[b] == 1 ? sz[2] : sz[0];
                I[0] = m / 3.0 * (bb * bb + c * c); I[1] = m / 3.0 * (a * a + c * c); I[2] = m / 3.0 * (a * a + bb * bb);
            }
        }
        int slot = -1;
        if (dyn && t->bone[b] >= 0) { slot = (int)o.dyn_bone.size(); o.dyn_bone.push_back(t->bone[b]); }
        float *r = o.body.data() + (size_t)b * 16;
        r[0] = op[0]; r[1] = op[1]; r[2] = op[2]; r[3] = dyn ? (float)(1.0 / m) : 0.0f;
        r[4] = (float)bq[b].x; r[5] = (float)bq[b].y; r[6] = (float)bq[b].z; r[7] = (float)bq[b].w;
        for (int k = 0; k < 3; ++k) r[8 + k] = I[k] > 0 ? (float)(1.0 / I[k]) : 0.0f;
        r[11] = (float)std::pow(1.0 - (double)t->linear_damping[b], h);
        r[12] = (float)std::pow(1.0 - (double)t->angular_damping[b], h);
        r[13] = bits_of(t->bone[b]); r[14] = bits_of(slot); r[15] = aligned && aligned[b] ? 1.0f : 0.0f;
    }
    o.nd = (int)o.dyn_bone.size();
    o.joint.assign((size_t)nj * 32, 0.0f);
    for (uint32_t k = 0; k < nj; ++k) {
        const uint32_t j = (uint32_t)o.order[k], a = t->body_a[j], b = t->body_b[j];
        const D4 jq = quat_from_pmx_euler(t->rotation3 + (size_t)j * 3);
        const float *jp = t->position3 + (size_t)j * 3;
        const D3 ra = qrot(qconj(bq[a]), { jp[0] - bx[a].x, jp[1] - bx[a].y, jp[2] - bx[a].z });
        const D3 rb = qrot(qconj(bq[b]), { jp[0] - bx[b].x, jp[1] - bx[b].y, jp[2] - bx[b].z });
        const D4 ja = qmul(qconj(bq[a]), jq), jb = qmul(qconj(bq[b]), jq);
        float *r = o.joint.data() + (size_t)k * 32;
        r[0] = (float)ra.x; r[1] = (float)ra.y; r[2] = (float)ra.z; r[3] = bits_of((int32_t)a);
        r[4] = (float)rb.x; r[5] = (float)rb.y; r[6] = (float)rb.z; r[7] = bits_of((int32_t)b);
        r[8] = (float)ja.x; r[9] = (float)ja.y; r[10] = (float)ja.z; r[11] = (float)ja.w;
        r[12] = (float)jb.x; r[13] = (float)jb.y; r[14] = (float)jb.z; r[15] = (float)jb.w;
        int32_t springs = 0;
        for (int ax = 0; ax < 3; ++ax) {
            const float pl = t->position_min3[j * 3 + ax], ph = t->position_max3[j * 3 + ax], rl = t->rotation_min3[j * 3 + ax], rh = t->rotation_max3[j * 3 + ax];
            r[16 + ax] = std::min(pl, ph); r[20 + ax] = std::max(pl, ph);
            r[24 + ax] = std::min(rl, rh); r[28 + ax] = std::max(rl, rh);
            const double ks = t->spring_rotation3[j * 3 + ax];
            if (ks > 0) { springs |= 1 << ax; r[19 + 4 * ax] = (float)(1.0 / (ks * h * h)); }
        }
        r[31] = bits_of(springs);
    }
}

// An uploaded table, owned: what later stages derive from (rz_physics_contacts: contact_table.h; rz_physics_springs: build_linear;
// rz_physics_aligned: the whole of build again). view() is that table again: its pointers are these vectors, or null where the column was
// not uploaded (or has no element).
struct Kept {
    uint32_t n_bodies = 0, n_joints = 0, iterations = 0;
    float h = 0.0f;
    std::vector<uint8_t> type, shape, group;
    std::vector<uint16_t> mask;
    std::vector<int32_t> bone;
    std::vector<uint32_t> body_a, body_b;
    std::vector<float> size3, mass, friction, spring_position3;
    std::vector<float> offset_pos3, offset_rot4, linear_damping, angular_damping, restitution, gravity3;
    std::vector<float> position3, rotation3, position_min3, position_max3, rotation_min3, rotation_max3, spring_rotation3;

    void keep(const rz_physics *t)
    {
        const size_t nb = n_bodies = t->n_bodies, nj = n_joints = t->n_joints;
        h = t->h; iterations = t->iterations;
        copy(type, t->type, nb); copy(shape, t->shape, nb); copy(group, t->group, nb); copy(mask, t->mask, nb);
        copy(size3, t->size3, nb * 3); copy(mass, t->mass, nb); copy(friction, t->friction, nb); copy(spring_position3, t->spring_position3, nj * 3);
        copy(bone, t->bone, nb); copy(offset_pos3, t->offset_pos3, nb * 3); copy(offset_rot4, t->offset_rot4, nb * 4);
        copy(linear_damping, t->linear_damping, nb); copy(angular_damping, t->angular_damping, nb); copy(restitution, t->restitution, nb);
        copy(gravity3, t->gravity3, 3);
        copy(body_a, t->body_a, nj); copy(body_b, t->body_b, nj); copy(position3, t->position3, nj * 3); copy(rotation3, t->rotation3, nj * 3);
        copy(position_min3, t->position_min3, nj * 3); copy(position_max3, t->position_max3, nj * 3);
        copy(rotation_min3, t->rotation_min3, nj * 3); copy(rotation_max3, t->rotation_max3, nj * 3); copy(spring_rotation3, t->spring_rotation3, nj * 3);
    }
    rz_physics view() const
    {
        rz_physics t;
        memset(&t, 0, sizeof t);
        t.n_bodies = n_bodies; t.n_joints = n_joints; t.h = h; t.iterations = iterations;
        t.type = ptr(type); t.shape = ptr(shape); t.group = ptr(group); t.mask = ptr(mask);
        t.size3 = ptr(size3); t.mass = ptr(mass); t.friction = ptr(friction); t.spring_position3 = ptr(spring_position3);
        t.bone = ptr(bone); t.offset_pos3 = ptr(offset_pos3); t.offset_rot4 = ptr(offset_rot4);
        t.linear_damping = ptr(linear_damping); t.angular_damping = ptr(angular_damping); t.restitution = ptr(restitution); t.gravity3 = ptr(gravity3);
        t.body_a = ptr(body_a); t.body_b = ptr(body_b); t.position3 = ptr(position3); t.rotation3 = ptr(rotation3);
        t.position_min3 = ptr(position_min3); t.position_max3 = ptr(position_max3);
        t.rotation_min3 = ptr(rotation_min3); t.rotation_max3 = ptr(rotation_max3); t.spring_rotation3 = ptr(spring_rotation3);
        return t;
    }

private:
    template <class T> static void copy(std::vector<T> &to, const T *from, size_t n) { if (from) to.assign(from, from + n); else to.clear(); }
    template <class T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
};

// ---- the solver's LDS, and the linear springs (rz_physics_springs; tests/spring_ref.py) ----

constexpr size_t kLdsLimit = rzlds::kCuLds;    // what one workgroup of rz_physics_kernel may take: the CU's LDS, as for every kernel (lds_layout.h)
// lanes per workgroup, chosen at upload: 64 when the bodies and the widest colour fit one wave, else 256 (unmeasured: DESIGN.md 9.7)
inline int block_for(int n_bodies, int widest) { return n_bodies <= 64 && widest <= 64 ? 64 : 256; }
// LDS of one workgroup: 96 B per body; once the joints outnumber the lanes their multipliers live there too, 12 B per joint, 24 B with the
// linear springs' three more
inline size_t lds_bytes(int n_bodies, int n_joints, int block, bool springs)
{
    return (size_t)n_bodies * 96 + (n_joints > block ? (size_t)n_joints * (springs ? 24 : 12) : 0);
}

struct Linear {
    std::vector<float> rec;             // [nj][4] in solve order: alpha~ x | alpha~ y | alpha~ z | bits(axes with spring_position > 0)
    int axes = 0;                       // (joint, axis) pairs with a spring
};
// spring_position3 as uploaded ([nj * 3], file order), the solve order and the h rz_upload_physics derived; alpha~ = 1 / (k h^2) in double,
// rounded once, as build does for the angular ones
inline void build_linear(const float *spring_position3, const std::vector<int> &order, double h, Linear &o)
{
    const size_t nj = order.size();
    o.rec.assign(nj * 4, 0.0f);
    o.axes = 0;
    for (size_t k = 0; k < nj; ++k) {
        const size_t j = (size_t)order[k];
        int32_t bits = 0;
        for (int ax = 0; ax < 3; ++ax) {
            const double ks = spring_position3[j * 3 + ax];
            if (ks > 0) { bits |= 1 << ax; o.rec[k * 4 + ax] = (float)(1.0 / (ks * h * h)); ++o.axes; }
        }
        o.rec[k * 4 + 3] = bits_of(bits);
    }
}

// What rz_physics_springs(ctx, 1) refuses for a resident table, "" = nothing. invalid: RZ_ERR_INVALID (the column is missing), otherwise
// RZ_ERR_UNSUPPORTED (the doubled multipliers no longer fit). A table without a spring axis launches the old kernels at the old size.
inline std::string springs_refusal(int n_bodies, int n_joints, int block, bool have_column, int axes, bool &invalid)
{
    char m[320];
    invalid = false;
    if (n_joints && !have_column) {
        invalid = true;
        return "rz_physics_springs: the resident table was uploaded without spring_position: linear springs need spring_position3";
    }
    const size_t lds = lds_bytes(n_bodies, n_joints, block, true);
    if (axes && lds > kLdsLimit) {
        snprintf(m, sizeof m, "rz_physics_springs: %d bodies and %d joints need %zu B of LDS with linear springs (96 B per body, + 24 B per joint instead of 12 once the joints outnumber the %d lanes; the limit is 160 KB)",
                 n_bodies, n_joints, lds, block);
        return m;
    }
    return "";
}

// What rz_upload_physics refuses of a valid table as too large (RZ_ERR_UNSUPPORTED), "" = nothing. o null: before the table is built, the cap on
// the counts alone (nothing of that size is coloured first); otherwise the LDS its launch form takes.
inline std::string upload_refusal(uint32_t n_bodies, uint32_t n_joints, const Built *o)
{
    char m[320];
    if (!o) {
        if (n_bodies <= (1u << 20) && n_joints <= (1u << 20)) return "";
        snprintf(m, sizeof m, "physics table too large for the device solver: %u bodies and %u joints (96 B of LDS per body, + 12 B per joint once the joints outnumber the lanes; the limit is 160 KB)",
                 n_bodies, n_joints);
        return m;
    }
    const int block = block_for(o->nb, o->widest);
    const size_t lds = lds_bytes(o->nb, o->nj, block, false);
    if (lds <= kLdsLimit) return "";
    snprintf(m, sizeof m, "physics table too large for the device solver: %u bodies and %u joints need %zu B of LDS (96 B per body, + 12 B per joint once the joints outnumber the %d lanes; the limit is 160 KB)",
             n_bodies, n_joints, lds, block);
    return m;
}

// Everything rz_upload_physics (aligned = false) and rz_physics_aligned derive from a table without the GPU, in the order the host owes:
// the table as given is checked, its types are read (read_types), with the feature on the table as read is checked again — two bodies that
// are dynamic now may drive one bone —, it is coloured and built, and the launch form the new colouring selects is held to the LDS limit.
// 0, or RZ_ERR_INVALID / RZ_ERR_UNSUPPORTED with `bad` the message; nothing of `o` is to be used then.
struct Derived {
    Built built;
    std::vector<uint8_t> types;         // the type column as the solver reads it
    std::vector<uint8_t> flags;         // per body: aligned
    uint32_t n_aligned = 0;
};
inline int derive(const rz_physics *given, uint32_t B, const int32_t *parents, const float *bind3, bool aligned, Derived &o, std::string &bad)
{
    bad = validate(given, B);
    if (!bad.empty()) return RZ_ERR_INVALID;
    bad = upload_refusal(given->n_bodies, given->n_joints, nullptr);
    if (!bad.empty()) return RZ_ERR_UNSUPPORTED;
    o.n_aligned = read_types(given, aligned, o.types, o.flags);
    rz_physics read = *given;
    read.type = o.types.data();
    if (aligned) {
        bad = validate(&read, B);
        if (!bad.empty()) { bad = "rz_physics_aligned: " + bad; return RZ_ERR_INVALID; }
    }
    build(&read, B, parents, bind3, o.built, o.n_aligned ? o.flags.data() : nullptr);
    bad = upload_refusal(given->n_bodies, given->n_joints, &o.built);
    if (!bad.empty()) { if (aligned) bad = "rz_physics_aligned: " + bad; return RZ_ERR_UNSUPPORTED; }
    return 0;
}

}  // namespace rzphys
#pragma GCC visibility pop
