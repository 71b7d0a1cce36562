// tune.cpp — the launch-shape search (rz_autotune*) and the tuning keys (ctx.h).
#include "ctx.h"

using namespace rzi;

namespace {

// The settable keys: name, member of RzTuning, and a check that leaves the value to store in v (normalised where the key says so) or
// refuses it: RZ_ERR_INVALID with the row's message, RZ_ERR_UNSUPPORTED for a kernel variant only the tools-only build carries.
// shape: the key is part of the launch shape rz_autotune searches, so setting it clears tuned_by_search.
// kAlways clears it even when the value is then refused as invalid: deliberate, kept for compatibility, not an accident. kAccepted: only with the store.
enum { kNo, kAlways, kAccepted };
struct TuneKey { const char *name; int RzTuning::*field; int (*check)(int &v); const char *refusal; int shape; };
// (the records a key selects: the dense frame with that unroll, those morph loads and that rest-geometry path; the register crowd form)
int tools_only(const RzFrameKernel &k) { return k.carried(rz_has_all_variants()) ? RZ_OK : RZ_ERR_UNSUPPORTED; }
constexpr RzFrameKernel dense(int U, bool nt, bool geo) { return RzFrameKernel{ kRzDense, 1, U, 1, 0, 0, 0, 0, 0, nt, false, geo }; }
constexpr RzFrameKernel kRegForm = { kRzCrowdReg };
int need(bool ok) { return ok ? RZ_OK : RZ_ERR_INVALID; }
template <int lo, int hi> int within(int &v) { return need(v >= lo && v <= hi); }
const TuneKey kTuneKeys[] = {
    { "morph_split", &RzTuning::t_split, [](int &v) { return need(v == 0 || v == 1 || v == 2 || v == 4 || v == 8); }, "morph_split must be 0 (auto),1,2,4,8", kAlways },
    { "unroll", &RzTuning::t_unroll, [](int &v) { return v == 4 ? tools_only(dense(4, true, false)) : need(v == 0 || v == 8); }, "unroll must be 0 (auto), 4 or 8", kNo },
    { "grid_cap", &RzTuning::t_grid_cap, [](int &v) { return need(v >= 0); }, "grid_cap must be >= 0", kAlways },
    { "nontemporal", &RzTuning::t_nt, [](int &v) { v = v ? 1 : 0; return tools_only(dense(8, v != 0, false)); }, nullptr, kNo },
    { "geo_lds", &RzTuning::t_geo, [](int &v) { v = v ? 1 : 0; return tools_only(dense(8, true, v != 0)); }, nullptr, kNo },
    { "nt_store", &RzTuning::t_nts, [](int &v) { v = v < 0 ? -1 : (v ? 1 : 0); return (int)RZ_OK; }, nullptr, kNo },
    { "out_cap", &RzTuning::t_outcap, within<-1, 2048>, "out_cap must be -1 (auto), 0 (off) or 64..2048 vertices per wave", kNo },
    { "sparse_piece", &RzTuning::t_sppiece, [](int &v) { return need(v == 0 || (v >= 16 && v <= 2048 && v % 16 == 0)); },
      "sparse_piece must be 0 (auto) or a multiple of 16 in 16..2048 entries of the sparse CSR per wave", kNo },
    { "inst_morphs", &RzTuning::t_instmorphs, within<-1, 1>, "inst_morphs must be -1 (auto = off), 0 (a crowd with sparse morph targets always runs the generic kernel) or 1 (it takes the crowd kernels where they fit)", kNo },
    { "graph", &RzTuning::t_graph, within<0, 1>, "graph must be 0 or 1", kNo },
    { "inst_loop", &RzTuning::t_instloop, [](int &v) { return v == 9 ? tools_only(kRegForm) : need(v >= -1 && v != 1 && v <= 64); },
      "inst_loop must be -1 (auto), 0 (off), 2..8 / 10..64 (poses per workgroup, LDS form) or 9 (register form)", kAlways },
    { "pose_prefetch", &RzTuning::t_prefetch, within<-1, 1>, "pose_prefetch must be -1 (auto = on), 0 (a zero-copy frame never stages the next pose) or 1", kNo },
    { "inst_subsets", &RzTuning::t_subsets, within<-1, 1>, "inst_subsets must be -1 (auto = on), 0 (crowd frames always stage the whole palette) or 1", kNo },
    { "fuse_fk", &RzTuning::t_fusefk, within<-1, 1>, "fuse_fk must be -1 (auto), 0 (always rz_fk_kernel in front) or 1 (every device-animated single character)", kNo },
    { "zero_copy", &RzTuning::t_zerocopy, within<-1, 1>, "zero_copy must be -1 (auto = on for one character), 0 (every pose is copied to the device) or 1", kNo },
    { "fuse_fk_plain", &RzTuning::t_fkplain, within<-1, 1>, "fuse_fk_plain must be -1 (auto = on), 0 (the fused frame always runs the generic hierarchy solve) or 1", kNo },
    { "pose_pull", &RzTuning::t_pull, within<-1, 1>,
      "pose_pull must be -1 (auto: a crowd's world matrices are pulled, local rotations copied), 0 (every pose is copied by hipMemcpyAsync as it was handed over) or 1 (every pose of more than 256 KB is pulled)", kNo },
    { "overlap", &RzTuning::t_overlap, within<-1, 1>, "overlap must be -1 (auto = off), 0 (off) or 1 (crowds: front kernels on the upload stream)", kNo },
    { "inst_order", &RzTuning::t_instorder, within<0, 1>, "inst_order must be 0 (an XCD takes one vertex run of every pose group) or 1 (every vertex run of its pose groups)", kNo },
    { "inst_block", &RzTuning::t_instblock, [](int &v) { return need(v == 0 || v == 256 || v == 512 || v == 1024); }, "inst_block must be 0 (auto), 256, 512 or 1024 threads per workgroup", kAccepted },
    { "qdef_chunks", &RzTuning::t_qdefchunks, within<0, 64>, "qdef_chunks must be 0 (auto) or 1..64 chunks of 256 QDEF vertices per workgroup", kNo },
    { "fast", &RzTuning::t_fast, [](int &) { return (int)RZ_OK; }, nullptr, kNo },      // -1 auto, 0 never (always prep kernel), 1 when possible
};
const TuneKey *find_key(const char *key)
{
    for (const TuneKey &k : kTuneKeys)
        if (!strcmp(key, k.name)) return &k;
    return nullptr;
}

}  // namespace

extern "C" {

int rz_autotune_measure(rz_ctx *c, uint32_t frames, rz_tune_entry *table, int cap, int *count)
{
    if (int r = use(c)) return r;
    if (!table || cap < 1 || !count) return fail(RZ_ERR_INVALID, "rz_autotune_measure: bad table");
    *count = 0;
    if (int r = check_ready(c)) return r;
    if (int r = ensure_outputs(c)) return r;
    if (frames == 0) frames = 100;
    frames = std::min<uint32_t>(frames, 1000);      // a search, not a benchmark
    // Entry 0 = the heuristic plan. Then: morph split x workgroups per CU (single mesh), poses per workgroup x workgroups per
    // CU (instanced). Every candidate is a legal plan; the search only picks among the variants the parity tests already cover.
    std::vector<rz_tune_entry> cands;
    auto add = [&](int split, int capv, int loop) {
        rz_tune_entry e;
        memset(&e, 0, sizeof e);
        e.morph_split = split; e.grid_cap = capv; e.inst_loop = loop; e.same_as = -1;
        cands.push_back(e);
    };
    const int ncu = c->n_cu;
    const int keep_split = c->t_split, keep_cap = c->t_grid_cap, keep_loop = c->t_instloop;
    const bool keep_tuned = c->tuned_by_search;
    InstShape is;
    const bool instanced = inst_shape(c, &is);      // with the caller's inst_loop: 0 (crowd kernel off) and 9 (register form) are not searched over
    c->t_split = 0; c->t_grid_cap = 0; if (instanced) c->t_instloop = -1;
    add(0, 0, -1);
    if (instanced) {
        // total workgroups: one or two rounds of what the CUs hold at once (two 256-thread workgroups or one larger one);
        // with bone subsets the palettes of 16 poses still fit, which halves the number of workgroup fronts
        for (int loop : {8, 4, 16})
            for (int capv : {ncu, 2 * ncu, 3 * ncu, 4 * ncu}) add(0, capv, loop);
    } else {
        const int smax = c->morphs.mode == 1 ? (int)std::min<uint32_t>(8, std::max<uint32_t>(1, c->morphs.M)) : 4;
        for (int sp = 1; sp <= smax; sp <<= 1)
            for (int capv : {ncu, 2 * ncu, 4 * ncu}) add(sp, (int)(capv * c->I), 0);
    }
    if ((int)cands.size() > cap) cands.resize(cap);
    const int n = (int)cands.size();
    auto restore = [&]() { c->t_split = keep_split; c->t_grid_cap = keep_cap; c->t_instloop = keep_loop; c->tuned_by_search = keep_tuned; };
    std::vector<Plan> plans(n);
    for (int i = 0; i < n; ++i) {
        c->t_split = cands[i].morph_split; c->t_grid_cap = cands[i].grid_cap; c->t_instloop = instanced ? cands[i].inst_loop : keep_loop;
        if (int r = frame_plan(c, &plans[i])) { restore(); return r; }
        const Plan &pl = plans[i];
        cands[i].eff_split = pl.v.S; cands[i].eff_grid = (int)pl.grid_x; cands[i].eff_inst_group = pl.inst_group;
        for (int k = 0; k < i && cands[i].same_as < 0; ++k)      // different requests often resolve to the same launch
            if (plans[k].grid_x == pl.grid_x && (pl.inst_group > 0 || plans[k].quads_per_wave == pl.quads_per_wave) && plans[k].v.S == pl.v.S &&
                plans[k].inst_group == pl.inst_group && plans[k].verts_per_wg == pl.verts_per_wg && plans[k].subsets == pl.subsets &&
                plans[k].inst_block == pl.inst_block)
                cands[i].same_as = cands[k].same_as >= 0 ? cands[k].same_as : k;
    }
    constexpr int kRounds = 5;
    std::vector<float> t((size_t)n * kRounds, 0.f);
    int rc = RZ_OK;
    {
        // the GPU reaches its sustained clocks only after a while of work (measured: the first timed round of the first
        // candidate came out 15-20 % slow on a cold device, which is enough to move a median of three): run the heuristic
        // plan for ~0.25 s first, untimed
        c->t_split = cands[0].morph_split; c->t_grid_cap = cands[0].grid_cap; c->t_instloop = instanced ? cands[0].inst_loop : keep_loop;
        Plan warm;
        rc = begin_frames(c, &warm);    // (a crowd's run lists belong to ONE launch shape: bring them back to entry 0's)
        const auto t0 = std::chrono::steady_clock::now();
        while (rc == RZ_OK && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(250)) {
            for (uint32_t f = 0; f < 64 && rc == RZ_OK; ++f) rc = run_frame(c, warm);
            if (rc == RZ_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(RZ_ERR_HIP, "rz_autotune_measure: warm-up failed");
        }
    }
    for (int round = -1; round < kRounds && rc == RZ_OK; ++round) {          // round -1 warms every variant up, untimed
        for (int i = 0; i < n && rc == RZ_OK; ++i) {
            if (cands[i].same_as >= 0) continue;
            c->t_split = cands[i].morph_split; c->t_grid_cap = cands[i].grid_cap; c->t_instloop = instanced ? cands[i].inst_loop : keep_loop;
            Plan pl;
            if ((rc = begin_frames(c, &pl)) != RZ_OK) break;     // crowd shapes alternate: the run lists follow (a rebuild, untimed)
            const uint32_t nf = round < 0 ? 8 : frames;
            for (uint32_t f = 0; f < 4 && rc == RZ_OK; ++f) rc = run_frame(c, pl);
            if (rc != RZ_OK) break;
            hipError_t he = hipEventRecord(c->ev0, c->stream);
            for (uint32_t f = 0; f < nf && rc == RZ_OK; ++f) rc = run_frame(c, pl);
            if (rc != RZ_OK) break;
            if (he == hipSuccess) he = hipEventRecord(c->ev1, c->stream);
            if (he == hipSuccess) he = hipEventSynchronize(c->ev1);
            float ms = 0.f;
            if (he == hipSuccess) he = hipEventElapsedTime(&ms, c->ev0, c->ev1);
            if (he != hipSuccess) { rc = fail(RZ_ERR_HIP, "rz_autotune_measure: %s", hipGetErrorString(he)); break; }
            if (round >= 0) t[(size_t)i * kRounds + round] = ms / nf;
        }
    }
    restore();
    if (rc != RZ_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const int src = cands[i].same_as >= 0 ? cands[i].same_as : i;
        float v[kRounds];
        for (int k = 0; k < kRounds; ++k) v[k] = t[(size_t)src * kRounds + k];
        std::sort(v, v + kRounds);
        cands[i].ms = v[kRounds / 2]; cands[i].ms_min = v[0]; cands[i].ms_max = v[kRounds - 1];
        table[i] = cands[i];
    }
    *count = n;
    return RZ_OK;
}

int rz_autotune_pick(const rz_tune_entry *table, int count)
{
    if (!table || count < 1) return 0;
    // entry 0 (the heuristics) stays unless something is clearly faster: median >= 2 % lower AND, when the table carries the
    // per-round spread, its slowest round still under the heuristic's fastest one (overlapping ranges are box noise, and a pick that
    // follows noise differs from run to run); among the qualifying entries, the lowest median
    int best = 0;
    float best_ms = table[0].ms * 0.98f;
    const bool spread = table[0].ms_min > 0.f;
    for (int i = 1; i < count; ++i) {
        if (table[i].same_as == 0 || !(table[i].ms > 0.f) || !(table[i].ms < best_ms)) continue;
        if (spread && table[i].ms_max > 0.f && !(table[i].ms_max < table[0].ms_min)) continue;
        best = i; best_ms = table[i].ms;
    }
    return best;
}

int rz_autotune_apply(rz_ctx *c, const rz_tune_entry *e)
{
    if (int r = use(c)) return r;
    if (!e) return fail(RZ_ERR_INVALID, "rz_autotune_apply: null entry");
    const int sp = e->morph_split;
    if (sp != 0 && sp != 1 && sp != 2 && sp != 4 && sp != 8) return fail(RZ_ERR_INVALID, "rz_autotune_apply: morph_split %d", sp);
    if (e->grid_cap < 0 || e->inst_loop < -1 || e->inst_loop == 1 || e->inst_loop > 64) return fail(RZ_ERR_INVALID, "rz_autotune_apply: bad entry");
    if (e->inst_loop == 9 && tools_only(kRegForm))
        return fail(RZ_ERR_UNSUPPORTED, "rz_autotune_apply: inst_loop = 9 selects the register-resident crowd kernel, which the product library does not carry");
    // a caller who switched the crowd kernel off (inst_loop = 0) or chose the register form (9) keeps that choice: the entry's
    // pose-group size only applies where the search itself would have used one
    InstShape is;
    const bool instanced = inst_shape(c, &is);
    c->t_split = sp; c->t_grid_cap = e->grid_cap;
    if (instanced) c->t_instloop = e->inst_loop;
    c->tuned_by_search = true;
    return RZ_OK;
}

int rz_autotune(rz_ctx *c, uint32_t frames)
{
    rz_tune_entry table[32];
    int n = 0;
    if (int r = rz_autotune_measure(c, frames, table, 32, &n)) return r;
    if (n < 1) return RZ_OK;
    return rz_autotune_apply(c, &table[rz_autotune_pick(table, n)]);
}

int rz_set_tuning(rz_ctx *c, const char *key, int value)
{
    if (!c || !key) return fail(RZ_ERR_INVALID, "null argument");
    if (!strcmp(key, "dbg")) {
#ifdef RZ_ABLATE
        c->t_dbg = value;
        return RZ_OK;
#else
        // ablation modes (they make the kernels skip work, i.e. emit garbage) are compiled into the tools-only build only
        return fail(RZ_ERR_INVALID, "tuning key 'dbg' does not exist in the product library (tools-only build: make -C reze-engine_amd/csrc ablate)");
#endif
    }
    const TuneKey *k = find_key(key);
    if (!k) return fail(RZ_ERR_INVALID, "unknown tuning key '%s'", key);
    int v = value;
    const int r = k->check(v);
    // variants that were measured slower everywhere are compiled into the tools-only build (make variants), not the product
    if (r == RZ_ERR_UNSUPPORTED) return fail(r, "%s = %d selects a kernel variant the product library does not carry (tools-only build: make -C reze-engine_amd/csrc variants)", key, value);
    if (k->shape == kAlways || (k->shape == kAccepted && r == RZ_OK)) c->tuned_by_search = false;      // the caller owns the shape now
    if (r != RZ_OK) return fail(r, "%s", k->refusal);
    c->*k->field = v;
    return RZ_OK;
}

}  // extern "C"

namespace {
// The read keys: name, whether the key describes the NEXT frame, and a getter. For a key of the next frame rz_get_tuning resolves that
// frame ONCE — plan, parameter block and the kernel record (frame_kernel.h) — and the getter reads it; which kernel that frame launches
// is read from the record alone. A key that is not in the table (or among the settable ones) is unknown, and refused before any work.
struct Next { Plan pl; RzDeformParams dp; RzFrameKernel k; };
struct ReadKey { const char *name; bool next; int (*get)(rz_ctx *c, const Next &n, int *value); };
#define RZ_GET(expr) [](rz_ctx *c, const Next &n, int *value) -> int { (void)c; (void)n; *value = (int)(expr); return RZ_OK; }
// diagnostics (tools/archive/placement.py): where the allocator put a buffer — bits [12, 43) of its device address, i.e. the address in
// 4 KB pages (where a buffer lands relative to the 2 MB large-page frame moves the C5 frame by 3 %: NOTEBOOK.md R5.3)
int page_of(const void *ptr) { return (int)(((uintptr_t)ptr >> 12) & 0x7fffffffu); }
const ReadKey kReadKeys[] = {
    { "bones", false, RZ_GET(c->skel.B) }, { "morphs", false, RZ_GET(c->morphs.M) }, { "instances", false, RZ_GET(c->I) }, { "verts", false, RZ_GET(c->mesh.V) },
    { "sdef_verts", false, RZ_GET(c->sdef.n) }, { "qdef_verts", false, RZ_GET(c->qdef.n) }, { "ik_chains", false, RZ_GET(c->ik.n) },
    { "motion_clips", false, RZ_GET(c->lib.clips) }, { "motion_masks", false, RZ_GET(c->mk.count) }, { "morph_mode", false, RZ_GET(c->morphs.mode) },
    { "physics_bodies", false, RZ_GET(c->ph.nb) }, { "physics_joints", false, RZ_GET(c->ph.nj) }, { "physics_colours", false, RZ_GET(c->ph.ncol) },
    // the form rz_launch_physics takes for the resident table (kernels/physics.hip): lanes per workgroup, joints kept in registers (1) or
    // strided over a colour (0), dynamic LDS per workgroup; all 0 without a table
    { "physics_block", false, RZ_GET(c->ph.nb ? c->ph.block : 0) }, { "physics_own", false, RZ_GET((c->ph.nb && (int)c->ph.nj <= c->ph.block) ? 1 : 0) },
    { "physics_lds", false, RZ_GET(c->ph.nb ? rzphys::lds_bytes((int)c->ph.nb, (int)c->ph.nj, c->ph.block, c->ph.springs.lin.p != nullptr) : 0) },
    { "physics_contacts", false, RZ_GET(c->ph.contacts.mode) }, { "physics_contact_follow", false, RZ_GET(c->ph.contacts.follow) },
    { "physics_contact_pairs", false, RZ_GET(c->ph.contacts.pairs) }, { "physics_contact_colours", false, RZ_GET(c->ph.contacts.ncol) },
    { "physics_contact_boxes", false, RZ_GET(c->ph.contacts.boxes) }, { "physics_contact_box_pairs", false, RZ_GET(c->ph.contacts.box_pairs) },
    { "physics_contact_box_box", false, RZ_GET(c->ph.contacts.box_box) },
    { "physics_springs", false, RZ_GET(c->ph.springs.on) }, { "physics_spring_axes", false, RZ_GET(c->ph.springs.axes) },
    { "physics_aligned", false, RZ_GET(c->ph.aligned.on) }, { "physics_aligned_bodies", false, RZ_GET(c->ph.aligned.n) },
    { "override_follow", false, RZ_GET(c->ovr_follow) },
    { "override_followers", false, RZ_GET(solve_stages(c).fo.off ? c->fol_count : 0) },     // entries resident over all instances
    { "after_physics", false, RZ_GET(c->af.n) }, { "after_physics_levels", false, RZ_GET(c->af.levels) },       // entries resident (rz_upload_after_physics), their levels
    { "ik_stages", false, RZ_GET(c->ik.stages) }, { "ik_switched", false, RZ_GET(c->iksw.off) },       // ik_switched: (instance, chain) bits currently off
    { "ik_key_sets", false, [](rz_ctx *c, const Next &, int *value) -> int {
          int n = c->ik_keys_an.resident ? 1 : 0;
          for (const RzIkKeySet &s : c->ik_keys_mo) n += s.resident ? 1 : 0;
          *value = n;
          return RZ_OK;
      } },
    { "pose_pulled", false, RZ_GET(c->pl.last_pulled ? 1 : 0) },      // the most recent copied pose came down by rz_pull_pose_kernel ...
    { "pose_rows", false, RZ_GET(c->pl.last_rows ? 1 : 0) },          // ... its world matrices as three rows per bone
    { "pose_resident", false, RZ_GET(c->pl.cur.resident() ? 1 : 0) }, { "all_variants", false, RZ_GET(rz_has_all_variants() ? 1 : 0) },
    { "pose_staged", false, [](rz_ctx *c, const Next &, int *value) -> int {
          // did the helper of an earlier frame stage the CURRENT pose in device memory? (synchronises; for tests and tools)
          *value = 0;
          if (c->pl.tag && c->pl.cur.seq) {
              uint64_t tags[2] = {0, 0};
              HIP_TRY(hipSetDevice(c->device));
              HIP_TRY(hipStreamSynchronize(c->stream));
              HIP_TRY(hipMemcpy(tags, c->pl.tag, sizeof tags, hipMemcpyDeviceToHost));
              *value = tags[c->pl.pose_slot] == c->pl.cur.seq ? 1 : 0;
          }
          return RZ_OK;
      } },
    { "addr_dense", false, RZ_GET(page_of(c->morphs.dense)) }, { "addr_out", false, RZ_GET(page_of(c->out_pos)) },
    { "addr_nrm", false, RZ_GET(page_of(c->out_nrm)) }, { "addr_geom", false, RZ_GET(page_of(c->mesh.geom)) },
    // ---- the next frame's kernel: the record ----
    { "effective_variant", true, RZ_GET(n.k.fkv) },      // the single-mesh frame kernel's last template argument (the FKV rule: rz_frame_kernel)
    { "effective_nt", true, RZ_GET(n.k.nt && n.k.mode == 1 ? 1 : 0) }, { "effective_nt_store", true, RZ_GET(n.k.nts ? 1 : 0) },
    { "effective_geo", true, RZ_GET(n.k.geo ? 1 : 0) }, { "effective_fast", true, RZ_GET(n.k.fast ? 1 : 0) },
    { "effective_split", true, RZ_GET(n.k.S) }, { "effective_unroll", true, RZ_GET(n.k.U) },
    // (block / sub / morph are zero outside the pose-group families; so are the Plan's fields: make_plan fills them in its crowd branch only,
    // which the register form's inst_loop = 9 never enters)
    { "effective_inst_block", true, RZ_GET(n.k.block) }, { "effective_subsets", true, RZ_GET(n.k.sub ? 1 : 0) },
    { "effective_inst_morphs", true, RZ_GET(n.k.morph ? 1 : 0) },     // the frame walks sparse morph rows in a crowd kernel
    { "effective_fuse_fk", true, RZ_GET(n.k.solve ? 1 : 0) },
    { "effective_poses_per_wg", true, RZ_GET(n.k.poses_per_wg) }, { "effective_inst_group", true, RZ_GET(n.k.group) },
    // ---- the next frame's launch shape, parameter block and front ----
    { "effective_fk_kind", true, RZ_GET(n.dp.fk_kind) }, { "effective_morph_storage", true, RZ_GET(c->morphs.mode == 1 ? c->morphs.storage : 0) },
    { "effective_prep", true, RZ_GET(has_front(c, n.pl) ? 1 : 0) }, { "effective_overlap", true, RZ_GET(want_overlap(c, n.pl) ? 1 : 0) },
    { "effective_closure_bones", true, RZ_GET(n.pl.subfk ? c->subfk_stride : 0) },
    { "effective_closure_rounds", true, RZ_GET(n.pl.subfk ? c->subfk_rounds : 0) },      // radix-4 doubling rounds of that front (0 .. 3)
    { "effective_out_cap", true, RZ_GET(n.pl.out_cap) }, { "effective_grid", true, RZ_GET(n.pl.grid_x) },
    { "effective_sparse_piece", true, RZ_GET(n.pl.sp_cap) },      // 0 without resident sparse targets (make_plan sizes it for MODE 2 only)
    { "effective_subset_bones", true, RZ_GET(n.pl.sub_bones) }, { "effective_inst_lds", true, RZ_GET(n.pl.inst_lds) },
};
#undef RZ_GET
}  // namespace

extern "C" {

int rz_get_tuning(rz_ctx *c, const char *key, int *value)
{
    if (!c || !key || !value) return fail(RZ_ERR_INVALID, "null argument");
    if (const TuneKey *k = find_key(key)) { *value = c->*k->field; return RZ_OK; }
    const ReadKey *row = nullptr;
    for (const ReadKey &k : kReadKeys)
        if (!strcmp(key, k.name)) row = &k;
    if (!row) return fail(RZ_ERR_INVALID, "unknown tuning key '%s'", key);
    Next n;     // resolved for a key of the next frame only; the other getters do not read it
    if (row->next) {
        // what the NEXT frame will launch: a crowd's plan depends on the run lists of its launch shape, so bring them up to
        // date first (as every entry point that launches frames does) instead of describing the whole-palette fallback
        if (int r = use(c)) return r;
        if (c->mesh.V && c->skel.B) {
            if (int r = ensure_run_subsets(c)) return r;
            if (int r = ensure_subfk(c)) return r;
        }
        n.pl = make_plan(c);
        n.dp = deform_params(c, n.pl);
        n.k = frame_kernel(n.pl, n.dp);
    }
    return row->get(c, n, value);
}

}  // extern "C"
