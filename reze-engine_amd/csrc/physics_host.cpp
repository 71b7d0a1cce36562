// physics_host.cpp — rigid-body physics for PMX bodies and joints: the table's upload (physics_table.h checks, colours and derives it, and keeps
// the columns the contact stage and the linear springs derive from later), the two stages' switches, stepping, reset and readback. All of its
// state is one member of the context, RzPhysics ph (ctx.h), whose device arrays free themselves: a stage is released by resetting its part,
// the table by resetting ph, and a replacement is built in a local part that takes the old one's place only after drain(). The solver itself
// is rz_physics_kernel (kernels/physics.hip); this unit owns the hierarchy solve's override table while a physics table is resident.
#include "ctx.h"
#include "contact_table.h"

using namespace rzi;

namespace rzi {

void free_physics(rz_ctx *c)
{
    if (!c->ph.nb) return;
    drop_graph(c);
    c->ph = {};                         // every array, list and record with its counts and flags; the next table starts from a reset
    c->ovr_count = 0;                   // the overrides were physics' own
}

// per-instance buffers for the current crowd: body state, and the override table's offsets and bones (written here, once; the matrices are
// the kernel's). The table's buffers only ever grow, and only here: across steps they keep their addresses.
static int ensure_instances(rz_ctx *c)
{
    RzPhysics &ph = c->ph;
    if (ph.I == c->I && ph.state) return RZ_OK;
    if (int r = drain(c)) return r;
    drop_graph(c);
    c->ovr_count = 0;
    ph.I = 0;
    ph.state = {};
    const size_t I = c->I, nd = ph.nd, n = I * nd;
    HIP_TRY(ph.state.alloc(I * ph.nb * 4));
    HIP_TRY(hipMemset(ph.state, 0, I * ph.nb * 4 * sizeof(float4)));
    if (int r = reserve_overrides(c, n, I + 1)) return r;
    std::vector<int> off(I + 1), bones(std::max<size_t>(n, 1));
    for (size_t i = 0; i <= I; ++i) off[i] = (int)(i * nd);
    for (size_t i = 0; i < I; ++i)
        for (size_t k = 0; k < nd; ++k) bones[i * nd + k] = ph.dyn_bone[k];
    HIP_TRY(hipMemcpy(c->ovr_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    if (n) HIP_TRY(hipMemcpy(c->ovr_bone, bones.data(), n * sizeof(int), hipMemcpyHostToDevice));
    c->fol_count = 0;
    if (c->ovr_follow) {                // rz_override_follow: the bones below the dynamic bodies' bones, with the set they follow
        bones.resize(n);
        if (int r = upload_followers(c, off, bones)) return r;
    }
    ph.I = c->I;
    ph.reset = true;
    return RZ_OK;
}

static int physics_usable(rz_ctx *c, const char *what)
{
    if (!c->ph.nb) return fail(RZ_ERR_INVALID, "%s: no physics table is resident (rz_upload_physics)", what);
    if (c->lender || c->n_forks) return fail(RZ_ERR_INVALID, "%s while forks exist: physics owns the override table of one context", what);
    return RZ_OK;
}

// the solver's arguments for the resident table; a stage that is off has left its part empty, so its pointers and counts are null and 0
static RzPhysicsParams physics_params(const rz_ctx *c, uint32_t substeps, bool reset)
{
    const RzPhysics &ph = c->ph;
    const RzPhysics::Contacts &k = ph.contacts;
    RzPhysicsParams p;
    memset(&p, 0, sizeof p);
    p.body = ph.body; p.joint = ph.joint; p.colour_off = ph.colour_off; p.state = ph.state;
    p.world = c->world; p.ovr_world = c->ovr_world;
    p.nb = (int)ph.nb; p.nj = (int)ph.nj; p.ncol = (int)ph.ncol; p.nd = (int)ph.nd; p.B = (int)c->skel.B;
    p.iterations = ph.iterations; p.substeps = (int)substeps; p.reset = (reset || ph.reset) ? 1 : 0; p.block = ph.block;
    p.h = ph.h; p.gx = ph.g[0]; p.gy = ph.g[1]; p.gz = ph.g[2];
    p.c_shape = k.shape; p.c_follow_off = k.follow_off; p.c_follow_idx = k.follow_idx; p.c_pair = k.pair;
    p.c_colour_off = k.colour_off; p.c_ncol = (int)k.ncol; p.contacts = k.mode; p.c_box = k.box;
    p.lin = ph.springs.lin;
    return p;
}

// the hierarchy solve of the resident pose without overrides, then the solver: both on the stream the frame's front runs on
static int step(rz_ctx *c, uint32_t substeps, bool reset)
{
    if (!c->pl.cur.set) return fail(RZ_ERR_INVALID, "rz_physics_step: no pose set");
    if (!c->pl.cur.local || !c->fk.has_topology)
        return fail(RZ_ERR_INVALID, "rz_physics_step acts on device-solved poses (rz_set_pose_local, rz_set_pose_sampled, rz_set_pose_blended): with rz_set_pose the host owns the world matrices");
    if (int r = ensure_instances(c)) return r;
    hipStream_t st = front_stream(c);
    // overlapped crowd frames: the hierarchy solve below rewrites the current ring slot's palettes, which the last frame's skin kernel and
    // SDEF / QDEF passes may still be reading on the compute stream (run_frame moves on to the other slot; this solve does not)
    if (c->overlap_on && c->skin_recorded[c->ring_slot]) HIP_TRY(hipStreamWaitEvent(c->up_stream, c->ev_skin[c->ring_slot], 0));
    if (int r = launch_fk(c, st, false)) return r;      // without overrides: bodies follow (and are reset onto) the SOLVED pose
    HIP_TRY(rz_launch_physics(physics_params(c, substeps, reset), c->I, st, c->ph.aligned.n != 0));
    c->ph.reset = false;
    c->ovr_count = c->I * c->ph.nd;
    if (c->ovr_count) c->fk_stale = true;       // world matrices and palettes in memory are the un-overridden solve's: rz_read_world / rz_read_palette solve again
    return RZ_OK;
}

// A table's way into the context, for rz_upload_physics and rz_physics_aligned alike: checked, coloured and built first (physics_table.h:
// derive) — a refusal leaves the context as it was — then the old table goes and the new one moves in with contacts and linear springs off
// and a reset pending. aligned: the table's type-2 bodies with a mass are read as dynamic, those with a bone flagged; `kept` stays the
// table as the caller gave it. `given` may point into c->ph.kept: it is copied before the old table goes.
static int install(rz_ctx *c, const rz_physics *given, bool aligned)
{
    std::vector<int32_t> parents(c->skel.B);
    std::vector<float> bind((size_t)c->skel.B * 3);
    for (uint32_t b = 0; b < c->skel.B; ++b) {
        parents[b] = (int32_t)c->fk.host[4 * b].x;
        memcpy(&bind[(size_t)b * 3], &c->fk.host[4 * b + 1], 12);
    }
    rzphys::Derived d;
    std::string bad;
    if (int r = rzphys::derive(given, c->skel.B, parents.data(), bind.data(), aligned, d, bad)) return fail(r, "%s", bad.c_str());
    const rzphys::Built &o = d.built;
    RzPhysics::Aligned al;
    al.on = aligned ? 1 : 0;
    al.n = d.n_aligned;
    al.types = std::move(d.types);
    rzphys::Kept kept;
    kept.keep(given);
    if (int r = drain(c)) return r;
    free_physics(c);
    drop_graph(c);
    c->ovr_count = 0;                   // hand-fed overrides end here: the table is physics' own from now on
    // (the old table has gone, as it always had by here: a failed allocation leaves the context without one)
    RzPhysics ph;
    if (int r = to_device(ph.body, o.body.data(), (size_t)o.nb * 4)) return r;
    if (int r = to_device(ph.joint, o.joint.data(), (size_t)o.nj * 8)) return r;
    if (int r = to_device(ph.colour_off, o.colour_off.data(), o.colour_off.size())) return r;
    ph.nb = (uint32_t)o.nb; ph.nj = (uint32_t)o.nj; ph.ncol = (uint32_t)o.ncol; ph.nd = (uint32_t)o.nd;
    ph.iterations = o.iterations; ph.h = o.h; ph.hd = o.hd;
    for (int k = 0; k < 3; ++k) ph.g[k] = o.g[k];
    ph.block = rzphys::block_for(o.nb, o.widest);
    ph.dyn_bone = o.dyn_bone;
    ph.order = o.order;
    ph.kept = std::move(kept);
    ph.aligned = std::move(al);
    c->ph = std::move(ph);
    return RZ_OK;
}

}  // namespace rzi

extern "C" {

int rz_upload_physics(rz_ctx *c, const rz_physics *t)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_physics")) return r;
    if (!t || t->n_bodies == 0) {
        if (c->ph.nb)
            if (int r = drain(c)) return r;
        free_physics(c);
        return RZ_OK;
    }
    if (!c->fk.has_topology || c->fk.host.size() != (size_t)c->skel.B * 4)
        return fail(RZ_ERR_INVALID, "rz_upload_physics needs the hierarchy: call rz_upload_skeleton_topology first");
    return install(c, t, false);
}

int rz_physics_aligned(rz_ctx *c, uint32_t on)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_aligned")) return r;
    if (int r = static_unlocked(c, "rz_physics_aligned")) return r;
    if (!c->fk.has_topology || c->fk.host.size() != (size_t)c->skel.B * 4)
        return fail(RZ_ERR_INVALID, "rz_physics_aligned needs the hierarchy: call rz_upload_skeleton_topology first");
    const rz_physics t = c->ph.kept.view();
    return install(c, &t, on != 0);
}

int rz_physics_step(rz_ctx *c, uint32_t substeps)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_step")) return r;
    if (substeps > 1000) return fail(RZ_ERR_INVALID, "rz_physics_step: %u substeps in one call (at most 1000)", substeps);
    return step(c, substeps, false);
}

int rz_physics_contacts(rz_ctx *c, uint32_t on)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_contacts")) return r;
    if (!on) {
        if (!c->ph.contacts.mode) return RZ_OK;
        if (int r = drain(c)) return r;
        drop_graph(c);
        c->ph.contacts = {};
        return RZ_OK;
    }
    const int mode = on == 2 || on == 3 ? (int)on : 1;    // (every other nonzero value is 1, as it always was)
    rz_physics t = c->ph.kept.view();
    if (c->ph.aligned.on) t.type = c->ph.aligned.types.data();       // rz_physics_aligned: the aligned bodies are dynamic to the lists too
    if (!t.group || !t.mask || !t.friction || !t.size3)
        return fail(RZ_ERR_INVALID, "rz_physics_contacts: the resident table was uploaded without%s%s%s%s: contacts need group, mask, friction and size3",
                    !t.group ? " group" : "", !t.mask ? " mask" : "", !t.friction ? " friction" : "", !t.size3 ? " size3" : "");
    rzphys::Contacts o;
    rzphys::build_contacts(&t, o, mode);
    if (o.too_many) return fail(RZ_ERR_UNSUPPORTED, "%s", rzphys::contacts_refusal(o).c_str());
    // the new lists first, in a part of their own: a failed allocation leaves the context as it was
    RzPhysics::Contacts k;
    if (int r = to_device(k.shape, o.shape.data(), t.n_bodies)) return r;
    if (mode >= 2)
        if (int r = to_device(k.box, o.box.data(), t.n_bodies)) return r;
    if (int r = to_device(k.follow_off, o.follow_off.data(), o.follow_off.size())) return r;
    if (int r = to_device(k.follow_idx, o.follow_idx.data(), o.follow_idx.size())) return r;
    if (int r = to_device(k.pair, o.pair.data(), o.pair.size() / 2)) return r;
    if (int r = to_device(k.colour_off, o.colour_off.data(), o.colour_off.size())) return r;
    k.follow = (uint32_t)o.n_follow; k.pairs = (uint32_t)o.n_pairs; k.ncol = (uint32_t)o.ncol; k.boxes = (uint32_t)o.boxes;
    k.box_pairs = (uint32_t)o.box_pairs; k.box_box = (uint32_t)o.n_box_box;
    k.mode = mode;
    if (int r = drain(c)) return r;
    drop_graph(c);
    c->ph.contacts = std::move(k);      // (k leaves with the old lists)
    return RZ_OK;
}

int rz_physics_springs(rz_ctx *c, uint32_t on)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_springs")) return r;
    if (!on) {
        if (!c->ph.springs.on) return RZ_OK;
        if (int r = drain(c)) return r;
        drop_graph(c);
        c->ph.springs = {};
        return RZ_OK;
    }
    const float *column = c->ph.kept.view().spring_position3;
    rzphys::Linear o;
    if (column) rzphys::build_linear(column, c->ph.order, c->ph.hd, o);
    bool invalid = false;
    const std::string bad = rzphys::springs_refusal((int)c->ph.nb, (int)c->ph.nj, c->ph.block, column != nullptr, o.axes, invalid);
    if (!bad.empty()) return fail(invalid ? RZ_ERR_INVALID : RZ_ERR_UNSUPPORTED, "%s", bad.c_str());
    // the new records first, in a part of their own: a failed allocation leaves the context as it was. A table without a spring axis keeps
    // the old kernels
    RzPhysics::Springs s;
    if (o.axes)
        if (int r = to_device(s.lin, o.rec.data(), c->ph.nj)) return r;
    s.axes = (uint32_t)o.axes;
    s.on = 1;
    if (int r = drain(c)) return r;
    drop_graph(c);
    c->ph.springs = std::move(s);
    return RZ_OK;
}

int rz_physics_reset(rz_ctx *c)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_reset")) return r;
    if (!c->pl.cur.set || !c->pl.cur.local || !c->fk.has_topology) {       // nothing to stand the bodies on yet: the next step does it
        c->ph.reset = true;
        c->ovr_count = 0;
        return RZ_OK;
    }
    return step(c, 0, true);
}

int rz_read_physics(rz_ctx *c, uint32_t instance, float *state13)
{
    if (int r = use(c)) return r;
    const RzPhysics &ph = c->ph;
    if (!ph.nb) return fail(RZ_ERR_INVALID, "rz_read_physics: no physics table is resident (rz_upload_physics)");
    if (!state13) return fail(RZ_ERR_INVALID, "rz_read_physics: null output");
    if (!ph.state || ph.reset || instance >= ph.I)
        return fail(RZ_ERR_INVALID, "rz_read_physics: instance %u has no state (%u instance(s) stepped; rz_physics_step or rz_physics_reset first)", instance, ph.reset ? 0u : ph.I);
    if (int r = drain(c)) return r;
    std::vector<float> rec((size_t)ph.nb * 16);
    HIP_TRY(hipMemcpy(rec.data(), ph.state.p + (size_t)instance * ph.nb * 4, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < ph.nb; ++b) {
        const float *r = rec.data() + (size_t)b * 16;
        float *o = state13 + (size_t)b * 13;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
        o[3] = r[4]; o[4] = r[5]; o[5] = r[6]; o[6] = r[7];
        o[7] = r[8]; o[8] = r[9]; o[9] = r[10];
        o[10] = r[12]; o[11] = r[13]; o[12] = r[14];
    }
    return RZ_OK;
}

}  // extern "C"
