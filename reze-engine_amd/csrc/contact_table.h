// contact_table.h — the host half of rz_physics_contacts that needs no GPU: from the table as uploaded, the per-body shape records, the follow
// lists and the coloured dynamic pairs the contact stage of rz_physics_kernel runs on (deform_kernels.h: RzPhysicsParams). Plain C++ without
// HIP, beside physics_table.h: tests/contact_table_main.cpp compiles it alone, and the CPU tests hold the lists it prints under every mode
// of rz_physics_contacts (1; 2, boxes take part; 3, pairs of two boxes kept) to contact_lists(table, mode) of tests/contact_ref.py entry
// for entry.
#pragma once
#include "physics_table.h"

#pragma GCC visibility push(hidden)
namespace rzphys {

constexpr size_t kMaxContactCandidates = 65536;         // follow entries + dynamic pairs: every pair of the table is tested (no broad phase yet)

struct Contacts {
    std::vector<float> shape;           // [nb][4] radius | half length of the segment (0: a sphere) | friction | bits(1 = takes part, 4 = a box)
    std::vector<float> box;             // [nb][4] boxes mode: a box's three half extents | 0; zeros for every other body
    std::vector<int> follow_off;        // [nb + 1] a dynamic body's following partners: follow_idx[follow_off[b] .. follow_off[b + 1]), ascending
    std::vector<int> follow_idx;
    std::vector<int> pair;              // [n_pairs][2] dynamic pairs (a < b) in solve order: (colour, a, b)
    std::vector<int> colour_off;        // [ncol + 1]
    size_t n_follow = 0, n_pairs = 0;   // counted in full even when the limit is passed (the lists are then empty)
    int ncol = 0, boxes = 0;            // boxes: those with a nonzero mask that take no part (boxes mode: the ones with an extent of 0)
    bool too_many = false;
    size_t box_pairs = 0;               // boxes mode: pairs of two boxes that the rule would pair; they are no candidates (left out, counted)
    size_t n_box_box = 0;               // box_pairs kept: the pairs of two boxes among the candidates (box_pairs is then 0)
};

inline bool takes_part(const rz_physics *t, uint32_t b)
{
    return (t->shape[b] == 0 || t->shape[b] == 2) && t->size3[(size_t)b * 3] > 0.0f && t->mask[b] != 0;
}
// Bullet's rule: each body's group is in the other's mask
inline bool groups_meet(const rz_physics *t, uint32_t a, uint32_t b)
{
    const uint32_t ga = t->group[a] < 16 ? 1u << t->group[a] : 0u, gb = t->group[b] < 16 ? 1u << t->group[b] : 0u;
    return (ga & t->mask[b]) && (gb & t->mask[a]);
}

// a box takes part (boxes mode only) when its three half extents are positive
inline bool box_takes_part(const rz_physics *t, uint32_t b)
{
    const float *sz = t->size3 + (size_t)b * 3;
    return t->shape[b] == 1 && sz[0] > 0.0f && sz[1] > 0.0f && sz[2] > 0.0f && t->mask[b] != 0;
}

// t must carry group, mask, friction and size3. mode as rz_physics_contacts takes it: 1 — spheres and capsules; 2 — boxes take part against
// them; 3 — a pair of two boxes is a candidate like any other
inline void build_contacts(const rz_physics *t, Contacts &o, int mode)
{
    const bool boxes = mode >= 2, keep = mode == 3;
    const uint32_t nb = t->n_bodies;
    o = Contacts();
    o.shape.assign((size_t)nb * 4, 0.0f);
    if (boxes) o.box.assign((size_t)nb * 4, 0.0f);
    std::vector<uint32_t> in;           // the bodies that take part
    for (uint32_t b = 0; b < nb; ++b) {
        float *r = o.shape.data() + (size_t)b * 4;
        const float *sz = t->size3 + (size_t)b * 3;
        const bool isbox = boxes && t->shape[b] == 1;
        const bool on = takes_part(t, b) || (isbox && box_takes_part(t, b));
        r[0] = isbox ? 0.0f : sz[0];      // a box counts as a shape of radius 0
        r[1] = t->shape[b] == 2 ? (float)((double)sz[1] * 0.5) : 0.0f;
        r[2] = t->friction[b];
        r[3] = bits_of((on ? 1 : 0) | (isbox ? 4 : 0));
        if (isbox) for (int k = 0; k < 3; ++k) o.box[(size_t)b * 4 + k] = sz[k];
        if (on) in.push_back(b);
        if (t->shape[b] == 1 && t->mask[b] != 0 && !on) o.boxes++;
    }
    // the rule, for a < b that both take part; a pair of two boxes passes it and is left out by both walks unless mode 3
    const auto pairs_up = [t](uint32_t a, uint32_t b) { return (dynamic(t, a) || dynamic(t, b)) && groups_meet(t, a, b); };
    const auto two_boxes = [t](uint32_t a, uint32_t b) { return t->shape[a] == 1 && t->shape[b] == 1; };
    // count first: the limit is checked before any list is built
    std::vector<int> nfol(nb, 0);
    for (size_t i = 0; i < in.size(); ++i)
        for (size_t k = i + 1; k < in.size(); ++k) {
            const uint32_t a = in[i], b = in[k];
            if (!pairs_up(a, b)) continue;
            if (two_boxes(a, b)) {
                if (!keep) { o.box_pairs++; continue; }
                o.n_box_box++;
            }
            const bool da = dynamic(t, a), db = dynamic(t, b);
            if (da && db) o.n_pairs++;
            else { nfol[da ? a : b]++; o.n_follow++; }
        }
    o.follow_off.assign(nb + 1, 0);
    o.colour_off.assign(1, 0);
    if (o.n_follow + o.n_pairs > kMaxContactCandidates) { o.too_many = true; return; }
    for (uint32_t b = 0; b < nb; ++b) o.follow_off[b + 1] = o.follow_off[b] + nfol[b];
    o.follow_idx.assign(o.n_follow, 0);
    std::vector<int> fill(o.follow_off.begin(), o.follow_off.end() - 1);
    std::vector<int> pa, pb, colour;
    std::vector<std::vector<char>> used(nb);
    for (size_t i = 0; i < in.size(); ++i)
        for (size_t k = i + 1; k < in.size(); ++k) {
            const uint32_t a = in[i], b = in[k];
            if (!pairs_up(a, b) || (!keep && two_boxes(a, b))) continue;
            const bool da = dynamic(t, a), db = dynamic(t, b);
            if (!(da && db)) {
                // (a, b) ascends lexicographically, so a dynamic body meets its partners in ascending order whichever side it is on
                if (da) o.follow_idx[fill[a]++] = (int)b; else o.follow_idx[fill[b]++] = (int)a;
                continue;
            }
            int c = 0;
            for (;; ++c) {
                const bool ta = (size_t)c < used[a].size() && used[a][c], tb = (size_t)c < used[b].size() && used[b][c];
                if (!ta && !tb) break;
            }
            for (uint32_t x : { a, b }) { if (used[x].size() <= (size_t)c) used[x].resize(c + 1, 0); used[x][c] = 1; }
            pa.push_back((int)a); pb.push_back((int)b); colour.push_back(c);
            o.ncol = std::max(o.ncol, c + 1);
        }
    std::vector<int> order(pa.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return colour[x] < colour[y]; });
    o.pair.resize(pa.size() * 2);
    o.colour_off.assign(o.ncol + 1, 0);
    for (size_t k = 0; k < order.size(); ++k) {
        o.pair[2 * k] = pa[order[k]]; o.pair[2 * k + 1] = pb[order[k]];
        o.colour_off[colour[order[k]] + 1]++;
    }
    for (int c = 0; c < o.ncol; ++c) o.colour_off[c + 1] += o.colour_off[c];
}

inline std::string contacts_refusal(const Contacts &o)
{
    char m[280], of_boxes[64] = "";
    if (o.n_box_box) snprintf(of_boxes, sizeof of_boxes, " (%zu of them pairs of two boxes)", o.n_box_box);
    snprintf(m, sizeof m, "rz_physics_contacts: %zu follow entries and %zu dynamic pairs%s are more than %zu candidates: every pair of the table is tested, a broad phase does not exist yet",
             o.n_follow, o.n_pairs, of_boxes, kMaxContactCandidates);
    return m;
}

}  // namespace rzphys
#pragma GCC visibility pop
