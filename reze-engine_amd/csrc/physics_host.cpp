// physics_host.cpp — rigid-body physics for PMX bodies and joints (ctx.h): the table's upload (physics_table.h checks, colours and derives it),
// stepping, reset and readback. The solver itself is rz_physics_kernel (kernels/physics.hip); this unit owns the hierarchy solve's override
// table while a physics table is resident.
#include "ctx.h"
#include "contact_table.h"

using namespace rzi;

namespace rzi {

// the contact stage's lists: contacts are off afterwards
void free_contacts(rz_ctx *c)
{
    dfree(c->ph_c_shape); dfree(c->ph_c_box); dfree(c->ph_c_follow_off); dfree(c->ph_c_follow_idx); dfree(c->ph_c_pair); dfree(c->ph_c_colour_off);
    c->ph_contacts = 0;
    c->ph_c_follow = c->ph_c_pairs = c->ph_c_ncol = c->ph_c_boxes = c->ph_c_box_pairs = c->ph_c_box_box = 0;
}

// the linear springs' records: the stage is off afterwards
void free_springs(rz_ctx *c)
{
    dfree(c->ph_lin);
    c->ph_springs = 0;
    c->ph_spring_axes = 0;
}

void free_physics(rz_ctx *c)
{
    if (!c->ph_nb) return;
    drop_graph(c);
    free_contacts(c);
    free_springs(c);
    dfree(c->ph_body); dfree(c->ph_joint); dfree(c->ph_state); dfree(c->ph_colour_off);
    c->ph_nb = c->ph_nj = c->ph_ncol = c->ph_nd = c->ph_I = 0;
    c->ph_dyn_bone.clear(); c->ph_group.clear(); c->ph_mask.clear(); c->ph_shape.clear(); c->ph_type.clear();
    c->ph_size.clear(); c->ph_friction.clear(); c->ph_mass.clear(); c->ph_spring_pos.clear(); c->ph_order.clear();
    c->ph_reset = true;
    c->ovr_count = 0;                   // the overrides were physics' own
}

// per-instance buffers for the current crowd: body state, and the override table's offsets and bones (written here, once; the matrices are
// the kernel's). The table's buffers only ever grow, and only here: across steps they keep their addresses.
static int ensure_instances(rz_ctx *c)
{
    if (c->ph_I == c->I && c->ph_state) return RZ_OK;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    c->ovr_count = 0;
    c->ph_I = 0;
    dfree(c->ph_state);
    const size_t I = c->I, nd = c->ph_nd, n = I * nd;
    HIP_TRY(hipMalloc(&c->ph_state, I * c->ph_nb * 4 * sizeof(float4)));
    HIP_TRY(hipMemset(c->ph_state, 0, I * c->ph_nb * 4 * sizeof(float4)));
    if (n > c->ovr_alloc || I + 1 > c->ovr_off_alloc) {
        dfree(c->ovr_off); dfree(c->ovr_bone); dfree(c->ovr_world);
        c->ovr_alloc = c->ovr_off_alloc = 0;
        const size_t cap = std::max<size_t>(n, 64);
        HIP_TRY(hipMalloc(&c->ovr_off, (I + 1) * sizeof(int)));
        HIP_TRY(hipMalloc(&c->ovr_bone, cap * sizeof(int)));
        HIP_TRY(hipMalloc(&c->ovr_world, cap * 16 * sizeof(float)));
        c->ovr_alloc = cap; c->ovr_off_alloc = I + 1;
    }
    std::vector<int> off(I + 1), bones(std::max<size_t>(n, 1));
    for (size_t i = 0; i <= I; ++i) off[i] = (int)(i * nd);
    for (size_t i = 0; i < I; ++i)
        for (size_t k = 0; k < nd; ++k) bones[i * nd + k] = c->ph_dyn_bone[k];
    HIP_TRY(hipMemcpy(c->ovr_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    if (n) HIP_TRY(hipMemcpy(c->ovr_bone, bones.data(), n * sizeof(int), hipMemcpyHostToDevice));
    c->ph_I = c->I;
    c->ph_reset = true;
    return RZ_OK;
}

static int physics_usable(rz_ctx *c, const char *what)
{
    if (!c->ph_nb) return fail(RZ_ERR_INVALID, "%s: no physics table is resident (rz_upload_physics)", what);
    if (c->lender || c->n_forks) return fail(RZ_ERR_INVALID, "%s while forks exist: physics owns the override table of one context", what);
    return RZ_OK;
}

// the hierarchy solve of the resident pose without overrides, then the solver: both on the stream the frame's front runs on
static int step(rz_ctx *c, uint32_t substeps, bool reset)
{
    if (!c->pose_set) return fail(RZ_ERR_INVALID, "rz_physics_step: no pose set");
    if (!c->pose_local || !c->has_topology)
        return fail(RZ_ERR_INVALID, "rz_physics_step acts on device-solved poses (rz_set_pose_local, rz_set_pose_sampled, rz_set_pose_blended): with rz_set_pose the host owns the world matrices");
    if (int r = ensure_instances(c)) return r;
    hipStream_t st = front_stream(c);
    // overlapped crowd frames: the hierarchy solve below rewrites the current ring slot's palettes, which the last frame's skin kernel and
    // SDEF / QDEF passes may still be reading on the compute stream (run_frame moves on to the other slot; this solve does not)
    if (c->overlap_on && c->skin_recorded[c->ring_slot]) HIP_TRY(hipStreamWaitEvent(c->up_stream, c->ev_skin[c->ring_slot], 0));
    const uint32_t saved = c->ovr_count;
    c->ovr_count = 0;                   // bodies follow (and are reset onto) the SOLVED pose
    const int r = launch_fk(c, st);
    c->ovr_count = saved;
    if (r) return r;
    RzPhysicsParams p;
    memset(&p, 0, sizeof p);
    p.body = c->ph_body; p.joint = c->ph_joint; p.colour_off = c->ph_colour_off; p.state = c->ph_state;
    p.world = c->world; p.ovr_world = c->ovr_world;
    p.nb = (int)c->ph_nb; p.nj = (int)c->ph_nj; p.ncol = (int)c->ph_ncol; p.nd = (int)c->ph_nd; p.B = (int)c->B;
    p.iterations = c->ph_iterations; p.substeps = (int)substeps; p.reset = (reset || c->ph_reset) ? 1 : 0; p.block = c->ph_block;
    p.h = c->ph_h; p.gx = c->ph_g[0]; p.gy = c->ph_g[1]; p.gz = c->ph_g[2];
    if (c->ph_contacts) {
        p.c_shape = c->ph_c_shape; p.c_follow_off = c->ph_c_follow_off; p.c_follow_idx = c->ph_c_follow_idx; p.c_pair = c->ph_c_pair;
        p.c_colour_off = c->ph_c_colour_off; p.c_ncol = (int)c->ph_c_ncol; p.contacts = c->ph_contacts; p.c_box = c->ph_c_box;
    }
    p.lin = c->ph_lin;
    HIP_TRY(rz_launch_physics(p, c->I, st));
    c->ph_reset = false;
    c->ovr_count = c->I * c->ph_nd;
    if (c->ovr_count) c->fk_stale = true;       // world matrices and palettes in memory are the un-overridden solve's: rz_read_world / rz_read_palette solve again
    return RZ_OK;
}

}  // namespace rzi

extern "C" {

int rz_upload_physics(rz_ctx *c, const rz_physics *t)
{
    if (int r = use(c)) return r;
    if (int r = static_unlocked(c, "rz_upload_physics")) return r;
    if (!t || t->n_bodies == 0) {
        if (c->ph_nb) {
            HIP_TRY(hipStreamSynchronize(c->up_stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        free_physics(c);
        return RZ_OK;
    }
    if (!c->has_topology || c->fk_host.size() != (size_t)c->B * 4)
        return fail(RZ_ERR_INVALID, "rz_upload_physics needs the hierarchy: call rz_upload_skeleton_topology first");
    const std::string bad = rzphys::validate(t, c->B);
    if (!bad.empty()) return fail(RZ_ERR_INVALID, "%s", bad.c_str());
    if (t->n_bodies > (1u << 20) || t->n_joints > (1u << 20))
        return fail(RZ_ERR_UNSUPPORTED, "physics table too large for the device solver: %u bodies and %u joints (96 B of LDS per body, + 12 B per joint once the joints outnumber the lanes; the limit is 160 KB)", t->n_bodies, t->n_joints);
    std::vector<int32_t> parents(c->B);
    std::vector<float> bind((size_t)c->B * 3);
    for (uint32_t b = 0; b < c->B; ++b) {
        parents[b] = (int32_t)c->fk_host[4 * b].x;
        memcpy(&bind[(size_t)b * 3], &c->fk_host[4 * b + 1], 12);
    }
    rzphys::Built o;
    rzphys::build(t, c->B, parents.data(), bind.data(), o);
    const int block = rzphys::block_for(o.nb, o.widest);
    const size_t lds = rz_physics_lds_bytes(o.nb, o.nj, block, 0);
    if (lds > 160 * 1024)
        return fail(RZ_ERR_UNSUPPORTED, "physics table too large for the device solver: %u bodies and %u joints need %zu B of LDS (96 B per body, + 12 B per joint once the joints outnumber the %d lanes; the limit is 160 KB)",
                    t->n_bodies, t->n_joints, lds, block);
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_physics(c);
    drop_graph(c);
    c->ovr_count = 0;                   // hand-fed overrides end here: the table is physics' own from now on
    if (int r = to_device(&c->ph_body, o.body.data(), (size_t)o.nb * 4)) return r;
    if (int r = to_device(&c->ph_joint, o.joint.data(), (size_t)o.nj * 8)) { dfree(c->ph_body); return r; }
    if (int r = to_device(&c->ph_colour_off, o.colour_off.data(), o.colour_off.size())) { dfree(c->ph_body); dfree(c->ph_joint); return r; }
    c->ph_nb = (uint32_t)o.nb; c->ph_nj = (uint32_t)o.nj; c->ph_ncol = (uint32_t)o.ncol; c->ph_nd = (uint32_t)o.nd;
    c->ph_iterations = o.iterations; c->ph_h = o.h;
    for (int k = 0; k < 3; ++k) c->ph_g[k] = o.g[k];
    c->ph_block = block;
    c->ph_dyn_bone = o.dyn_bone;
    if (t->group) c->ph_group.assign(t->group, t->group + t->n_bodies);
    if (t->mask) c->ph_mask.assign(t->mask, t->mask + t->n_bodies);
    if (t->friction) c->ph_friction.assign(t->friction, t->friction + t->n_bodies);
    c->ph_shape.assign(t->shape, t->shape + t->n_bodies);
    c->ph_type.assign(t->type, t->type + t->n_bodies);
    c->ph_size.assign(t->size3, t->size3 + (size_t)t->n_bodies * 3);
    c->ph_mass.assign(t->mass, t->mass + t->n_bodies);
    if (t->spring_position3) c->ph_spring_pos.assign(t->spring_position3, t->spring_position3 + (size_t)t->n_joints * 3);
    c->ph_order = o.order;
    c->ph_hd = o.hd;
    c->ph_I = 0;
    c->ph_reset = true;
    return RZ_OK;
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
        if (!c->ph_contacts) return RZ_OK;
        HIP_TRY(hipStreamSynchronize(c->up_stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        drop_graph(c);
        free_contacts(c);
        return RZ_OK;
    }
    const int mode = on == 2 || on == 3 ? (int)on : 1;    // (every other nonzero value is 1, as it always was)
    const size_t nb = c->ph_nb;
    if (c->ph_group.size() != nb || c->ph_mask.size() != nb || c->ph_friction.size() != nb || c->ph_size.size() != nb * 3)
        return fail(RZ_ERR_INVALID, "rz_physics_contacts: the resident table was uploaded without%s%s%s%s: contacts need group, mask, friction and size3",
                    c->ph_group.size() != nb ? " group" : "", c->ph_mask.size() != nb ? " mask" : "", c->ph_friction.size() != nb ? " friction" : "",
                    c->ph_size.size() != nb * 3 ? " size3" : "");
    rz_physics t;
    memset(&t, 0, sizeof t);
    t.n_bodies = c->ph_nb; t.type = c->ph_type.data(); t.shape = c->ph_shape.data(); t.group = c->ph_group.data(); t.mask = c->ph_mask.data();
    t.size3 = c->ph_size.data(); t.mass = c->ph_mass.data(); t.friction = c->ph_friction.data();
    rzphys::Contacts o;
    rzphys::build_contacts(&t, o, mode);
    if (o.too_many) return fail(RZ_ERR_UNSUPPORTED, "%s", rzphys::contacts_refusal(o).c_str());
    // the new lists first: a failed allocation leaves the context as it was
    float4 *shape = nullptr, *box = nullptr;
    int *foff = nullptr, *fidx = nullptr, *coff = nullptr;
    int2 *pair = nullptr;
    int r = to_device(&shape, o.shape.data(), nb);
    if (!r && mode >= 2) r = to_device(&box, o.box.data(), nb);
    if (!r) r = to_device(&foff, o.follow_off.data(), o.follow_off.size());
    if (!r) r = to_device(&fidx, o.follow_idx.data(), o.follow_idx.size());
    if (!r) r = to_device(&pair, o.pair.data(), o.pair.size() / 2);
    if (!r) r = to_device(&coff, o.colour_off.data(), o.colour_off.size());
    if (r) { dfree(shape); dfree(box); dfree(foff); dfree(fidx); dfree(pair); dfree(coff); return r; }
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    free_contacts(c);
    c->ph_c_shape = shape; c->ph_c_box = box; c->ph_c_follow_off = foff; c->ph_c_follow_idx = fidx; c->ph_c_pair = pair; c->ph_c_colour_off = coff;
    c->ph_c_follow = (uint32_t)o.n_follow; c->ph_c_pairs = (uint32_t)o.n_pairs; c->ph_c_ncol = (uint32_t)o.ncol; c->ph_c_boxes = (uint32_t)o.boxes;
    c->ph_c_box_pairs = (uint32_t)o.box_pairs; c->ph_c_box_box = (uint32_t)o.n_box_box;
    c->ph_contacts = mode;
    return RZ_OK;
}

int rz_physics_springs(rz_ctx *c, uint32_t on)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_springs")) return r;
    if (!on) {
        if (!c->ph_springs) return RZ_OK;
        HIP_TRY(hipStreamSynchronize(c->up_stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        drop_graph(c);
        free_springs(c);
        return RZ_OK;
    }
    const size_t nj = c->ph_nj;
    const bool have = c->ph_spring_pos.size() == nj * 3;          // (empty: the column was NULL)
    rzphys::Linear o;
    if (have) rzphys::build_linear(c->ph_spring_pos.data(), c->ph_order, c->ph_hd, o);
    bool invalid = false;
    const std::string bad = rzphys::springs_refusal((int)c->ph_nb, (int)nj, c->ph_block, have, o.axes, invalid);
    if (!bad.empty()) return fail(invalid ? RZ_ERR_INVALID : RZ_ERR_UNSUPPORTED, "%s", bad.c_str());
    // the new records first: a failed allocation leaves the context as it was. A table without a spring axis keeps the old kernels
    float4 *lin = nullptr;
    if (o.axes)
        if (int r = to_device(&lin, o.rec.data(), nj)) return r;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    free_springs(c);
    c->ph_lin = lin;
    c->ph_spring_axes = (uint32_t)o.axes;
    c->ph_springs = 1;
    return RZ_OK;
}

int rz_physics_reset(rz_ctx *c)
{
    if (int r = use(c)) return r;
    if (int r = physics_usable(c, "rz_physics_reset")) return r;
    if (!c->pose_set || !c->pose_local || !c->has_topology) {       // nothing to stand the bodies on yet: the next step does it
        c->ph_reset = true;
        c->ovr_count = 0;
        return RZ_OK;
    }
    return step(c, 0, true);
}

int rz_read_physics(rz_ctx *c, uint32_t instance, float *state13)
{
    if (int r = use(c)) return r;
    if (!c->ph_nb) return fail(RZ_ERR_INVALID, "rz_read_physics: no physics table is resident (rz_upload_physics)");
    if (!state13) return fail(RZ_ERR_INVALID, "rz_read_physics: null output");
    if (!c->ph_state || c->ph_reset || instance >= c->ph_I)
        return fail(RZ_ERR_INVALID, "rz_read_physics: instance %u has no state (%u instance(s) stepped; rz_physics_step or rz_physics_reset first)", instance, c->ph_reset ? 0u : c->ph_I);
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<float> rec((size_t)c->ph_nb * 16);
    HIP_TRY(hipMemcpy(rec.data(), c->ph_state + (size_t)instance * c->ph_nb * 4, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < c->ph_nb; ++b) {
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
