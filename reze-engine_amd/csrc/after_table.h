// after_table.h — the host half of rz_upload_after_physics that needs no GPU: from the ordered list of after-physics bones and the
// hierarchy's bone records, the checks of "a valid list", the per-bone index, the dependency levels and the per-entry records that
// rz_fk_after_kernel runs on (deform_kernels.h: RzAfterParams; kernels/after.hip). Plain C++ without HIP, beside contact_table.h:
// tests/after_table_main.cpp compiles it alone, and tests/test_after_cpu.py holds what it prints to the level arithmetic restated in Python.
//   level(k) = 1 + the largest level over EARLIER entries that are k's parent, append parent or append parent's parent; 0 if there is none.
// Entries of one level read nothing another entry of that level writes, so a level is evaluated in parallel and the result is the
// sequential evaluation in list order (tests/after_ref.py). A bone that reads an entry listed LATER would have to see that entry's
// first-solve matrix — MMD's one-frame lag, which level-parallel evaluation does not reproduce: such a list is refused.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "lds_layout.h"

#pragma GCC visibility push(hidden)
namespace rzafter {

struct Table {
    std::vector<int> index;             // [B] position of the bone's entry in `rec` (sorted order), -1 = not listed
    std::vector<int> level_off;         // [levels + 1] entries of each level in `rec`
    // [n][12] words, sorted by (level, bone): parent | append parent (-1 = none in effect) | bits(append ratio) | flags (bit 0 append-move)
    //                                          bits(bind translation of the bone) x y z | the bone
    //                                          bits(bind translation of the append parent) x y z | the append parent's parent (-1 = root)
    std::vector<uint32_t> rec;
    std::vector<int> level;             // [n] in LIST order (for the tests)
    int levels = 0;
};

// `bone_rec`: the hierarchy's bone records as rz_upload_skeleton_topology keeps them, 16 words per bone (kernels/fk.hip.h): word 0 parent,
// 1 append parent, 2 bits(ratio), 3 flags, 4..6 bits(bind translation). Returns 0, or 1 with `err` naming the bone (RZ_ERR_INVALID).
inline int build(uint32_t B, const uint32_t *bone_rec, uint32_t n, const uint32_t *bones, Table &o, std::string &err)
{
    o = Table();
    o.index.assign(B, -1);
    std::vector<int> pos(B, -1);        // position in the list
    for (uint32_t k = 0; k < n; ++k) {
        if (bones[k] >= B) { err = "rz_upload_after_physics: entry " + std::to_string(k) + " names bone " + std::to_string(bones[k]) + " of " + std::to_string(B); return 1; }
        if (pos[bones[k]] >= 0) { err = "rz_upload_after_physics: bone " + std::to_string(bones[k]) + " is listed twice (entries " + std::to_string(pos[bones[k]]) + " and " + std::to_string(k) + ")"; return 1; }
        pos[bones[k]] = (int)k;
    }
    auto parent_of = [&](int b) { return (int32_t)bone_rec[16 * (size_t)b]; };
    auto append_of = [&](int b) -> int {            // the append parent fk_local_matrix reads, -1 when the ratio leaves none in effect
        float ratio;
        memcpy(&ratio, &bone_rec[16 * (size_t)b + 2], 4);
        const int ap = (int32_t)bone_rec[16 * (size_t)b + 1];
        const float cl = std::min(1.0f, std::max(-1.0f, ratio));
        return (ap >= 0 && (cl > 1e-6f || cl < -1e-6f)) ? ap : -1;
    };
    o.level.assign(n, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const int b = (int)bones[k], ap = append_of(b);
        const int reads[3] = { parent_of(b), ap, ap >= 0 ? parent_of(ap) : -1 };
        static const char *const what[3] = { "parent", "append parent", "append parent's parent" };
        int lv = 0;
        for (int j = 0; j < 3; ++j) {
            const int r = reads[j];
            if (r < 0 || r == b || pos[r] < 0) continue;
            if (pos[r] > (int)k) {
                err = "rz_upload_after_physics: bone " + std::to_string(b) + " (entry " + std::to_string(k) + ") is evaluated before its " + what[j] + ", bone " +
                      std::to_string(r) + " (entry " + std::to_string(pos[r]) + "): a listed bone must come after the listed bones it reads";
                return 1;
            }
            lv = std::max(lv, o.level[pos[r]] + 1);
        }
        o.level[k] = lv;
        o.levels = std::max(o.levels, lv + 1);
    }
    std::vector<uint32_t> ord(n);
    for (uint32_t k = 0; k < n; ++k) ord[k] = k;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return o.level[a] != o.level[b] ? o.level[a] < o.level[b] : bones[a] < bones[b]; });
    o.level_off.assign((size_t)o.levels + 1, 0);
    o.rec.assign((size_t)n * 12, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = ord[i];
        const int b = (int)bones[k], ap = append_of(b);
        o.index[b] = (int)i;
        o.level_off[(size_t)o.level[k] + 1]++;
        uint32_t *r = o.rec.data() + (size_t)i * 12;
        const uint32_t *br = bone_rec + 16 * (size_t)b;
        r[0] = br[0]; r[1] = (uint32_t)ap; r[2] = br[2]; r[3] = br[3];
        r[4] = br[4]; r[5] = br[5]; r[6] = br[6]; r[7] = (uint32_t)b;
        if (ap >= 0) {
            const uint32_t *ar = bone_rec + 16 * (size_t)ap;
            r[8] = ar[4]; r[9] = ar[5]; r[10] = ar[6]; r[11] = ar[0];
        } else r[11] = (uint32_t)-1;
    }
    for (int l = 0; l < o.levels; ++l) o.level_off[(size_t)l + 1] += o.level_off[l];
    return 0;
}

// dynamic LDS of rz_fk_after_kernel: the instance's world rows, 48 B per bone, and one skip byte per entry (lds_layout.h, where the kernel carves it)
inline size_t lds_bytes(uint32_t B, uint32_t n) { return rzlds::after((int)B, (int)n).total(); }

}  // namespace rzafter
#pragma GCC visibility pop
