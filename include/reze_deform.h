/*
 * reze_deform.h — C ABI of libreze_deform.so: the MI355X-native replacement for the reference's
 * per-frame PMX morph + skin GPU path.
 *
 * The reference (AmyangXYZ/reze-engine, TypeScript + WGSL) has no FFI; its de-facto boundary is
 * the set of WebGPU calls class Engine makes for this path. Every entry point below names the
 * reference call site it replaces (paths relative to the reference repo root). The N-API addon
 * (reze-engine_amd/csrc/napi_addon.c) and the Python ctypes binding (reze-engine_amd/capi.py) are
 * thin shims over exactly these symbols — see INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative rz_status;
 *     rz_last_error() returns a thread-local human-readable message for the last failure.
 *   - "host" pointers are caller-owned and are copied (or fully consumed) before the call returns.
 *   - one rz_ctx drives ONE GPU (one process — or one context — per GPU); calls on a context are
 *     serialised by the caller (Node's main thread). Work is enqueued on the context's own HIP
 *     streams (compute, plus an upload stream for large per-frame inputs) and is asynchronous
 *     unless stated; rz_sync() drains it.
 *   - matrices are column-major float[16] exactly as engine/src/math.ts stores them.
 *   - a context owns a contiguous vertex shard [v_begin, v_begin + V) of a mesh of v_total
 *     vertices (v_begin = 0, v_total = V on a single GPU).
 */
#ifndef REZE_DEFORM_H
#define REZE_DEFORM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 5): shards are cut at 256 vertices (4: 1 024 before round 4's change, which should have bumped this), so the chunk stride of the
 *    gathered buffer changed; rz_gather_chunk exports it instead of making callers re-derive it.
 * 6 (round 5): + rz_device_numa_node.
 * 7 (round 6): + rz_map_pose / rz_commit_pose (caller-written poses), rz_time_span (event-timed K-step span), rz_instance_range
 *    (crowds sharded along the instance axis). Nothing removed or changed: a binding written against 5 or 6 keeps working.
 * 8: + rz_upload_sdef, nothing removed.
 *    rz_upload_ik came later and is an addition too: the version stays 8, a binding detects the feature by the symbol. */
#define RZ_ABI_VERSION 8

typedef struct rz_ctx rz_ctx;

typedef enum rz_status {
    RZ_OK = 0,
    RZ_ERR_INVALID = -1,      /* bad argument / call order                       */
    RZ_ERR_HIP = -2,          /* a HIP runtime call failed (message has details) */
    RZ_ERR_NO_DEVICE = -3,    /* no usable gfx950 device                         */
    RZ_ERR_RCCL = -4,         /* an RCCL call failed                             */
    RZ_ERR_OOM = -5,
    RZ_ERR_UNSUPPORTED = -6
} rz_status;

/* Timing of the most recent rz_time_frames() / per-frame statistics (getStats() additions). */
typedef struct rz_timing {
    double frame_ms;          /* average wall ms per frame over the timed run (HIP events)     */
    double deform_kernel_ms;  /* average ms of the fused morph+skin kernel alone               */
    double prep_kernel_ms;    /* average ms of the palette / active-morph prep kernel          */
    uint64_t verts_per_frame; /* instances x vertices of this shard                            */
    uint64_t algorithmic_bytes_per_frame; /* SURVEY §8d formula for this shard                 */
    uint32_t frames;
    uint32_t reserved;
} rz_timing;

const char *rz_last_error(void);
int rz_abi_version(void);

/* Number of visible HIP devices. */
int rz_device_count(int *count);
/* The NUMA node of the host the device hangs off, from its PCI address (sysfs); *node = -1 when the system does not say (one socket,
 * no sysfs). No reference counterpart (a browser tab has no say in where it runs). Per-frame inputs cross the host link: a thread
 * that feeds a GPU from the OTHER socket pays for it twice — every doorbell / queue write / signal read of a HIP call crosses the
 * socket link (+14 us of host time per rz_set_pose of a 256-character crowd on 2 x EPYC 9575F), and so does every byte the GPU pulls
 * out of pinned memory that thread first touched (2.5 MB: 57 -> 77 us). The library never moves the caller's threads; bench.py binds
 * each rank to its GPU's node with this (profiles/r5_crowd_upload_numa.txt), a Node host would be started under numactl. */
int rz_device_numa_node(int device, int *node);

/* Engine.init()  engine/src/engine.ts:157-185 (requestAdapter/requestDevice): bind to one GPU,
 * create the stream, events and staging memory. */
int rz_create(int device, rz_ctx **out);
/* Engine.dispose()  engine/src/engine.ts:1692-1701. */
int rz_destroy(rz_ctx *ctx);

/* Pure helper: contiguous shard of rank `rank` of `nranks` over v_total vertices.
 * Shards are equal-sized (a multiple of 256 vertices) except the last; *count may be 0. */
int rz_shard_range(uint32_t v_total, int nranks, int rank, uint32_t *begin, uint32_t *count);
/* The uniform stride, in vertices, between two ranks' blocks of the gathered buffers (rz_allgather / rz_gather_direct /
 * rz_read_gathered): rank r's vertices land at [r * chunk, r * chunk + count_r). It is rank 0's shard size rounded up to the shard
 * grain — ask for it here rather than re-deriving the rule (the grain changed from 1 024 to 256 vertices with ABI 5). */
int rz_gather_chunk(uint32_t v_total, int nranks, uint32_t *chunk);

/* Crowds shard along the INSTANCE axis (last sentence): rank `rank` of `nranks` poses instances [begin, begin + count)
 * of a crowd of `instances` characters — equal contiguous ranges of ceil(I / N), the last may be shorter, *count may be 0. Every rank
 * holds the whole static mesh (rz_upload_mesh of all V vertices) and calls rz_set_instances(count); there is no collective at all,
 * and no communicator (rz_comm_init refuses a crowd). The reference draws one model per engine (engine/src/engine.ts:1704-1721). */
int rz_instance_range(uint32_t instances, int nranks, int rank, uint32_t *begin, uint32_t *count);

/* setupModelBuffers()  engine/src/engine.ts:1734-1765: vertex buffer in the reference's
 * interleaved layout (8 floats/vertex: pos3 nrm3 uv2, engine.ts:340-347), joints Uint16x4
 * (:348-352), weights Unorm8x4 (:353-356). De-interleaved to planar SoA on upload.
 * The arrays describe ONLY this context's shard (V vertices). */
int rz_upload_mesh(rz_ctx *ctx, uint32_t V, const float *interleaved8, const uint16_t *joints4,
                   const uint8_t *weights4);
/* Same, from separate packed position / normal arrays ([V][3] each). */
int rz_upload_mesh_soa(rz_ctx *ctx, uint32_t V, const float *pos3, const float *nrm3,
                       const uint16_t *joints4, const uint8_t *weights4);

/* inverseBindMatrixBuffer + boneCountBuffer  engine/src/engine.ts:1767-1804. */
int rz_upload_skeleton(rz_ctx *ctx, uint32_t B, const float *inverse_bind16);

/* Vertex-morph targets — NEW capability, no reference counterpart (the reference skips the PMX
 * morph section, engine/src/pmx-loader.ts:450-553). Dense: deltas[M][V][3] for this shard.
 * Sparse: PMX on-disk form (pmx-loader.ts:483-488) — morph m owns entries
 * [morph_off[m], morph_off[m+1]) of (vert_idx relative to this shard, delta xyz).
 * Passing M = 0 removes morphs.
 * Dense STORAGE: by default each delta is kept as a signed 24-bit integer times one power-of-two scale per morph (9 B per vertex and
 * morph instead of 12 — the dense frame is bound by exactly this stream). Per morph E = the binary exponent of its largest |delta| over
 * this shard, s = 2^(E - 22), q = rint(d / s) (E + 1 when the maximum would round to 2^23; an all-zero morph: s = 1): the stored value
 * q * s differs from d by at most 2^(E - 23), that is max|d| * 2^-23 (a hair more, 1 + 2^-24 of it, for a raised E), below what one fmaf into the position rounds away. Four values take three
 * dwords (d0 = q0 | q1[7:0] << 24, d1 = q1[23:8] | q2[15:0] << 16, d2 = q2[23:16] | q3 << 8). The scale belongs to the context: two
 * shards may scale one morph differently, which is harmless — a vertex lives in one shard. A set with a non-finite delta, or an exponent
 * outside [-64, 64], is stored as fp32 planes, whole. rz_upload_morphs_dense_ex(.., RZ_MORPH_F32) asks for fp32 planes: the frames then
 * compute what they computed before 24-bit storage existed, bit for bit. rz_get_tuning("effective_morph_storage") = 24 or 32.
 * rz_read_morph_dense: the resident (decoded) deltas of morph m as three planes [3][V] — for tests.
 * rz_morph_encode24: the encoder alone, on the host, no device involved: scales[M] and, when packed is not NULL, the planes
 * [M][3][ceil(V / 4) * 12 bytes]; *storage = 24, or 32 when the set would stay fp32 (nothing else is written then). */
#define RZ_MORPH_F32 1u
int rz_upload_morphs_dense(rz_ctx *ctx, uint32_t M, const float *deltas);
int rz_upload_morphs_dense_ex(rz_ctx *ctx, uint32_t M, const float *deltas, uint32_t flags);
int rz_read_morph_dense(rz_ctx *ctx, uint32_t m, float *planes3);
int rz_morph_encode24(const float *deltas, uint32_t M, uint32_t V, uint8_t *packed, float *scales, int *storage);
int rz_upload_morphs_sparse(rz_ctx *ctx, uint32_t M, const uint32_t *morph_off,
                            const uint32_t *vert_idx, const float *delta3);

/* SDEF skinning (PMX weight type 3) — opt-in; the reference folds SDEF vertices into BDEF2 and so does every frame without a table.
 * The listed vertices of this shard are skinned as MMD does it (saba's PMXModel, PMX coordinates as they are): joints / weights of slots
 * 0 and 1 (weights renormalised over those two; slots 2 and 3 are ignored — the loader writes zeros there), the morphed rest position
 * rotated about C by the slerp of the two bones' palette rotations, plus the weighted palette transforms of the corrected centres
 * C + (R0 - rw) / 2 and C + (R1 - rw) / 2 with rw = w0 R0 + w1 R1; normals by the slerped rotation. vert_idx[n] are relative to this shard
 * (like sparse morph indices), strictly ascending and < V; c3 / r0_3 / r1_3 are [n][3] in model space. n = 0 / NULL removes the table.
 * Every frame then runs one extra pass (rz_sdef_kernel) behind the deform / skin kernel for the listed vertices, writing positions,
 * normals and, when on, the outline hull; rz_get_tuning("sdef_verts") says how many (0 = no pass). Crowd frames that keep their palettes
 * in LDS only (the bone-subset skin kernel, the one-launch device-animated crowd) also run the palette kernel (rz_prep_kernel /
 * rz_fk_kernel) in front of the pass. Like every static upload it is refused while forks exist (they borrow the table);
 * rz_upload_mesh* drops it; it drops a captured graph. */
int rz_upload_sdef(rz_ctx *ctx, uint32_t n, const uint32_t *vert_idx, const float *c3, const float *r0_3, const float *r1_3);

/* QDEF skinning (PMX 2.1 weight type 4, dual-quaternion blending) — opt-in; the reference folds QDEF vertices into BDEF4 and so does every
 * frame without a table. For a listed vertex of this shard: joints j0..j3 (clamped to B - 1) and weights w_i = u8_i / isum exactly as
 * the linear path decodes them (isum == 0: (1, 0, 0, 0)); slots of weight zero contribute nothing; p~ the morphed rest position (this
 * frame's weights, ascending morph order, zero weights skipped), n the rest normal.
 *   per bone j:  S_j = palette rows (world x inverseBind, 3 x 4); q_j = the unit quaternion of its upper 3 x 3 (Shepperd's method);
 *                t_j = its fourth column; d_j = 1/2 (t_j, 0) (x) q_j:  d.xyz = 1/2 (q.w t + t x q.xyz),  d.w = -1/2 t . q.xyz.
 *                A palette that is not rigid (scale, shear) loses its non-rigid part here. PMX poses are rigid.
 *   blend (Kavan et al., dual-quaternion linear blending): pivot = the slot with the largest u8 weight, the lowest slot on ties;
 *                s_i = -1 if dot(q_pivot, q_ji) < 0 else +1;  b_r = sum w_i s_i q_ji,  b_d = sum w_i s_i d_ji (slots ascending);
 *                n_b = |b_r| (>= w_pivot >= 1/4);  c_r = b_r / n_b,  c_d = b_d / n_b
 *   P' = R(c_r) p~ + 2 (c_r.w c_d.xyz - c_d.w c_r.xyz + c_r.xyz x c_d.xyz);  N' = normalize(R(c_r) n) (zero or non-finite: the rest
 *   normal);  hull = P' + N' edge 0.01.   (tests/qdef_ref.py restates this in float64.)
 * vert_idx[n] are relative to this shard, strictly ascending and < V; n = 0 / NULL removes the table. A vertex listed in the SDEF table
 * too is refused (RZ_ERR_INVALID) by whichever of the two uploads comes second: a PMX vertex has one weight type. Every frame then runs
 * one extra pass (rz_qdef_kernel) behind the deform / skin kernel (and behind the SDEF pass) for the listed vertices, writing positions,
 * normals and, when on, the outline hull, and extending the bounding box as the SDEF pass does; rz_get_tuning("qdef_verts") says how
 * many (0 = no pass). Crowd frames that keep their palettes in LDS only also run the palette kernel in front of the pass, once for both
 * passes. Refused while forks exist (they borrow the table); rz_upload_mesh* drops it; it drops a captured graph. The ABI version stays
 * 8: bindings detect the symbol. */
int rz_upload_qdef(rz_ctx *ctx, uint32_t n, const uint32_t *vert_idx);

/* PMX inverse kinematics — NEW (the reference's loader skips the IK block, engine/src/pmx-loader.ts). Opt-in: without a table every
 * frame launches what it launched before. n_chains IK bones; chain k: goal[k] = the IK bone itself, effector[k] = the bone that is moved
 * onto it (PMX: "target"), loops[k] iterations, limit_angle[k] radians per step, links link_off[k] .. link_off[k + 1] ordered from the
 * effector outwards (knee, then leg); link e turns bone link_bone[e] and, if link_limited[e], is clamped to the Euler limits link_min3 /
 * link_max3 (radians, three.js 'XYZ' order R = Rx * Ry * Rz; an axis with min > max is swapped). The solver is CCD in the clamp form
 * (tests/ik_ref.py is the definition): chains in ascending order of the goal's bone index; per iteration, per link L in file order:
 *     a = Rw[L]^T (pos[E] - pos[L]), b = Rw[L]^T (pos[G] - pos[L]), both normalised (a link with |a| or |b| < 1e-6 or |a x b| < 1e-7 is skipped)
 *     q[L] = normalize(clamp(q[L] * quat(axis a x b, angle min(atan2(|a x b|, a . b), limit_angle))))        then the hierarchy is re-solved
 * until |pos[G] - pos[E]| < 1e-4, no link turned, or `loops` iterations ran (0 = the chain does nothing). World matrices are those of the
 * hierarchy solve after bone morphs; a chain sees what all earlier chains left. The final pose is the hierarchy solve of the solved local
 * rotations, so append children of a link follow; rz_override_world lands after IK. Order of a frame: sample -> bone morphs -> hierarchy ->
 * IK -> hierarchy of the solved locals -> overrides -> palette. It acts on device-solved poses only (rz_set_pose_local, rz_set_pose_sampled);
 * with rz_set_pose the host owns the world matrices and has solved IK itself — the rule bone morphs follow.
 * Valid: every index < B, effector != goal, every link a proper ancestor of the effector and of the link before it (bones between two
 * links stay rigid), loops >= 0, at most 65535 chains with distinct goals and 255 links per chain. Refused with RZ_ERR_UNSUPPORTED: a bone
 * on a chain's path that takes its append rotation from a link of any chain, or an ancestor of the effector or of the goal that takes it
 * from a link of the same chain (either would force the whole solve into every step); a goal below one of its own chain's links; a path (outermost
 * link ... effector) of more than 64 bones. With a table the solve runs as rz_fk_kernel<RzIkParams> in front of the deform / skin kernel: the
 * one-launch forms ("effective_fuse_fk") are not taken, and the skeleton must fit 156 B of LDS per bone. rz_get_tuning("ik_chains") = the
 * count, ("ik_stages") = the number of stages the chains were grouped into (the chains of a stage are solved at once). n_chains = 0 removes the table. Needs rz_upload_skeleton_topology first; a new skeleton or topology drops it; refused while
 * forks exist; drops a captured graph. */
int rz_upload_ik(rz_ctx *ctx, uint32_t n_chains, const uint32_t *goal, const uint32_t *effector, const uint32_t *loops, const float *limit_angle,
                 const uint32_t *link_off, const uint32_t *link_bone, const uint8_t *link_limited, const float *link_min3, const float *link_max3);

/* Chain switches of the IK stage — the VMD show / IK keys, which turn single chains off and on over a motion (a motion traced from motion
 * capture keys the legs by FK and switches leg and toe IK off at frame 0). An addition: the version stays 8, a binding detects it by these
 * symbols. Opt-in: without a call below every frame launches what it launched before. tests/ik_switch_ref.py is the definition:
 *   state_at(keys, frame)   the row of the LAST key with key_frame <= frame, compared as floats (among keys on one frame the last wins);
 *                           before the first key the first key's row; no keys: every chain on. A pure comparison: matched exactly.
 *   choose(state)           clip A's row at frame_a when clip_b == RZ_NO_CLIP or blend < 0.5, else clip B's row at frame_b; a chosen clip
 *                           without keys is all on. A switch does not cross-fade, and layers never switch IK.
 *   solve                   the IK stage over the chains whose switch is on, in the same order; a chain that is off does nothing: its links
 *                           keep the sampled or uploaded rotations, as a chain with loops == 0 does.
 * The context holds one mask, [I][n_chains] in rz_upload_ik's chain order, all on at first. The last writer wins:
 *   rz_set_ik_enabled                              writes it (non-zero = on; NULL = all on)
 *   rz_set_pose_sampled                            while keys for RZ_NO_CLIP are resident: mask[i] = state_at(keys, frames[i])
 *   rz_set_pose_blended / rz_set_pose_layered      while any clip of the library holds keys: mask[i] = choose(states[i])
 *   rz_set_pose_local, rz_set_pose, and a sampling call without keys for its source, leave it alone.
 * The switches are evaluated on the host, which is handed every frame and state anyway; only bits travel — one character's in the kernel
 * arguments, a crowd's in one small copy, and only when they differ from the bits the device holds. While at least one bit is off
 * (rz_get_tuning("ik_switched") = their number) the solve runs as rz_fk_kernel<RzIkParams, RzIkSwitchParams>, whose waves skip the chains that are off, whose
 * workgroup skips the whole-skeleton re-solve of a stage with no chain on, and the stage loop of an instance with none; a mask of all
 * ones launches rz_fk_kernel<RzIkParams> as ever. rz_physics_step's first solve uses the same mask.
 * Keys (rz_get_tuning("ik_key_sets") = resident sets): key_enabled is [n_keys][n_chains] in rz_upload_ik's order, a chain a VMD key does
 * not name already filled in by the caller (tests/ik_switch_ref.py: flatten). clip = RZ_NO_CLIP: the motion of rz_upload_animation; else a
 * clip of the library. keys == NULL removes the set; a set of 0 keys is resident and says "all on". Static data: refused while forks exist,
 * and forks see them. The mask is pose state: a fork owns its own. rz_upload_ik (a new table or none) resets the mask and drops every key
 * set; rz_upload_animation drops the RZ_NO_CLIP keys, rz_upload_motions the library's; a new skeleton or topology drops everything.
 * rz_set_instances: shrinking keeps the mask, members that appear are all on. rz_read_ik_enabled: what the next frame's solve uses (the
 * host's mirror: no synchronisation). Refused with RZ_ERR_INVALID, nothing resident changed: no IK table; a clip index >= the library's
 * count; a key frame that is not finite; descending key frames; null arrays with n_keys > 0.
 * Not covered: the keys' `show` flag; switches inside the one-launch forms (with a table they are not taken); a cross-faded switch. */
typedef struct rz_ik_keys {
    uint32_t n_keys;
    const float *key_frame;             /* [n_keys] non-descending */
    const uint8_t *key_enabled;         /* [n_keys][n_chains] */
} rz_ik_keys;
int rz_set_ik_enabled(rz_ctx *ctx, const uint8_t *enabled);
int rz_upload_ik_keys(rz_ctx *ctx, uint32_t clip, const rz_ik_keys *keys);
int rz_read_ik_enabled(rz_ctx *ctx, uint8_t *out);

/* Instancing — NEW (the reference draws one model): I poses of the same static mesh. Shrinking the crowd keeps the
 * resident pose (instances 0 .. I-1 of it); growing it beyond the count the pose was set for needs a new rz_set_pose*. */
int rz_set_instances(rz_ctx *ctx, uint32_t I);

/* updateModelPose()  engine/src/engine.ts:2383-2389: queue.writeBuffer(worldMatrixBuffer).
 * world = I x B x 16 floats; morph_weights = I x M floats or NULL (all zero). Asynchronous H2D
 * through pinned staging; the data is consumed by the next rz_deform(). */
int rz_set_pose(rz_ctx *ctx, const float *world, const float *morph_weights);

/* Caller-written poses (ABI 7). updateModelPose()  engine/src/engine.ts:2383-2389 is ONE queue.writeBuffer of the matrices the pose
 * solve left in Model's own Float32Array. rz_set_pose costs a crowd a copy on top of that: one host thread lays 3.3 MB out in the
 * pinned ring (44 us for 256 x 200 bones) before the GPU can pull it. rz_map_pose hands the ring slot itself to the caller — *matrices
 * points at room for I x B matrices in `layout`, *morph_weights (may be passed as NULL) at I x M floats, zero-filled — the caller (its
 * pose solve, its worker threads) writes them in place, and rz_commit_pose does what is left of rz_set_pose: no pack, no copy.
 *   RZ_POSE_WORLD16  64 B per bone: column-major float[16], math.ts's layout — what rz_set_pose takes
 *   RZ_POSE_ROWS12   48 B per bone: the four columns' x y z (c0.xyz c1.xyz c2.xyz c3.xyz), i.e. the matrix without its bottom row, which
 *                    for the affine matrices a pose solve produces is 0 0 0 1 and is written back as such on the device. Only for
 *                    poses of more than 256 KB (a crowd's: rz_pull_pose_kernel expands them); a smaller pose is read in place by its
 *                    frame and must be mapped as WORLD16 (RZ_ERR_UNSUPPORTED otherwise).
 * The pointers are valid until rz_commit_pose or the next pose call on the context (rz_set_pose* cancels a mapping); the memory is
 * pinned, cacheable host memory — plain stores. One mapping at a time per context (a fork has its own ring: two frames in flight map
 * alternately). A slot comes back to the caller kStageSlots (8) / 32 commits later, after the GPU is done reading it (polled here). */
enum { RZ_POSE_WORLD16 = 0, RZ_POSE_ROWS12 = 1 };
int rz_map_pose(rz_ctx *ctx, int layout, float **matrices, float **morph_weights);
int rz_commit_pose(rz_ctx *ctx);

/* ---- forward kinematics on the device (optional) ----
 * rz_upload_skeleton_topology hands over what Model.computeWorldMatrices (engine/src/model.ts:330-420) reads from
 * the skeleton: parents[B] (-1 = root), bind_translation[B*3] (Bone.bindTranslation), and the append data of
 * model.ts:355-393: append_parent[B] (-1 or NULL = no append rotation), append_ratio[B] (NULL = all 1) and
 * append_move[B] (NULL = none; non-zero = the append parent's local translation * ratio is appended as well).
 * rz_set_pose_local then replaces rz_set_pose: it uploads local rotations (I x B x 4, x y z w — the
 * SkeletonRuntime.localRotations array, model.ts:55) and, optionally, local translations (I x B x 3 —
 * SkeletonRuntime.localTranslations, model.ts:56; NULL = all zero, which is all the reference ever has: nothing
 * writes that array there, VMD bone translations are this build's row f2) instead of world matrices, and the frame
 * computes L = T(bind + t) * R * T(add), W = W_parent * L and the palette on the GPU (f32; the host solves in
 * doubles with f32 stores, so results agree to ~1e-6, not bit for bit; the device resolves the parent chains by pointer
 * doubling, so products are associated as (L0 L1)(L2 L3) rather than ((L0 L1) L2) L3). 4x less per-frame upload; hierarchy
 * solve for all instances in one launch; one character's local pose is zero-copy like a world pose (resident after its first
 * frame, prefetched by the helper workgroup). */
int rz_upload_skeleton_topology(rz_ctx *ctx, uint32_t B, const int32_t *parents, const float *bind_translation3,
                                const int32_t *append_parent, const float *append_ratio, const uint8_t *append_move);
int rz_set_pose_local(rz_ctx *ctx, const float *local_rotations4, const float *local_translations3, const float *morph_weights);
/* PMX bone morphs (morph type 2; SURVEY §8f rank 3 "then 2 bone-morph"). The reference's loader only skips the section
 * (engine/src/pmx-loader.ts:489-497), so the semantics are this build's, the usual MMD ones: a morph with weight w adds
 * w * translation to the bone's local translation and right-multiplies its local rotation by slerp(identity, rotation, w)
 * (Quat.slerp math.ts:156-189, Quat.multiply math.ts:77-85), entries of one bone folded in ascending morph order, BEFORE
 * append rotation / the hierarchy solve (so an append child follows a morphed append parent). n entries, each naming a morph
 * of the uploaded morph set (rz_upload_morphs_* first; a model whose only morphs are bone morphs uploads an empty sparse
 * set) and a bone; the weights are the pose's morph weights (rz_set_pose_local's morph_weights, or the sampled tracks of
 * rz_set_pose_sampled — group morphs feed bone morphs like vertex morphs). Acts on device-solved poses only: with
 * rz_set_pose the host owns the world matrices and folds bone morphs itself (host/model.js). n = 0 clears. Dropped by a
 * new skeleton or morph set. */
int rz_upload_bone_morphs(rz_ctx *ctx, uint32_t n, const uint32_t *morph, const uint32_t *bone, const float *translation3,
                          const float *rotation4);

/* ---- motion sampling on the device (SURVEY §8f ranks 1 + 2 combined; optional) ----
 * The caller of the path in the reference is Engine.playAnimation (engine/src/engine.ts:1515-1553) fed by
 * VMDLoader (engine/src/vmd-loader.ts:95-160, which drops the key's position and interpolation bytes, :129-140).
 * rz_upload_animation hands a whole flattened motion to the GPU once; rz_set_pose_sampled then replaces
 * rz_set_pose_local: per frame the host sends ONE float per instance — the (fractional, 30 fps) frame that instance
 * is posed at — and the frame samples every bone (slerp warped by the later key's R Bezier curve, per-axis lerp
 * warped by the X / Y / Z curves) and every vertex morph (linear keys; group-morph tracks feed their children by
 * ratio) on the device, then solves the hierarchy (needs rz_upload_skeleton_topology) and deforms. Bones and morphs
 * the motion does not key are at rest. Same arithmetic as host/vmd-sampler.js in f32.
 *   bone tracks : track_bone[n] (bone index, each bone at most once), key_off[n+1], and per key (ascending frame
 *                 inside a track) key_frame, key_rot4 (x y z w), key_pos3, key_interp16 (the first 16 of the 64
 *                 interpolation bytes: X_x1 Y_x1 Z_x1 R_x1 | ..y1 | ..x2 | ..y2; NULL = linear)
 *   morph tracks: mkey_off[m+1], mkey_frame, mkey_weight; feeds per VERTEX MORPH of the uploaded morph set:
 *                 feed_off[M+1], feed_track, feed_ratio — its own track (ratio 1) first, then the group-morph
 *                 tracks that include it, ascending (the order Model.getEffectiveMorphWeights adds them in).
 * Refused (RZ_ERR_INVALID, nothing resident changes): a key that is not finite — frame, rotation, position or morph weight — in a track
 * that drives a bone or feeds a vertex morph of this model, with the track and the key named ("track 3 key 17: the rotation is not
 * finite"; rz_upload_motions puts "clip k: " in front); keys of tracks that drive nothing of this model are not looked at.
 * rz_set_pose_sampled refuses a frame that is NaN or infinite ("instance i: a frame that would be sampled is not finite", the wording of
 * rz_set_pose_blended) and leaves the resident pose as it was. */
typedef struct rz_animation {
    uint32_t n_bone_tracks;
    const int32_t *track_bone;
    const uint32_t *key_off;
    const float *key_frame;
    const float *key_rot4;
    const float *key_pos3;
    const uint8_t *key_interp16;
    uint32_t n_morph_tracks;
    const uint32_t *mkey_off;
    const float *mkey_frame;
    const float *mkey_weight;
    const uint32_t *feed_off;
    const int32_t *feed_track;
    const float *feed_ratio;
} rz_animation;
int rz_upload_animation(rz_ctx *ctx, const rz_animation *anim);
int rz_set_pose_sampled(rz_ctx *ctx, const float *frames);
/* ---- a motion library on the device: per-instance clips and cross-fades — NEW (optional) ----
 * rz_upload_animation holds ONE motion and rz_set_pose_sampled sends one frame number per instance, so a crowd dances one dance and a
 * character can only hard-cut between motions. rz_upload_motions makes n_clips motions resident at once — each an rz_animation, checked
 * exactly as rz_upload_animation checks it (offsets non-decreasing, key frames not descending, a bone driven by at most one track per
 * clip, feed tracks in range; bones the model lacks are skipped), their keys concatenated on the device — and rz_set_pose_blended poses
 * instance i from states[i] = (clip_a, frame_a, clip_b, frame_b, blend) (tests/motion_ref.py is the definition):
 *     A = sample(clip_a, frame_a), B = sample(clip_b, frame_b)      what host/vmd-sampler.js defines, in f32 (rz_set_pose_sampled's sampler);
 *                                                                   a bone / morph a clip does not key: identity, zero translation, weight 0
 *     clip_b == RZ_NO_CLIP or blend == 0: exactly A (B is not evaluated, its fields are not read);  blend == 1: exactly B
 *     otherwise per bone  q = Quat.slerp(qa, qb, blend)  (math.ts:156-189: qb negated when the dot product is negative, normalised lerp
 *     above 0.9995, sine form otherwise),  t = ta + (tb - ta) * blend;  per vertex morph  w = wa + (wb - wa) * blend  on the effective
 *     weights (own track, then group feeds). clip_a == clip_b is legal: two times of one motion.
 * The result is a device-resident local pose with translations; from there the frame is an rz_set_pose_local frame: bone morphs ->
 * hierarchy -> IK (with a table) -> overrides -> palette -> deform / skin -> the SDEF and QDEF passes. rz_motion_kernel runs ONCE per
 * call, in front of the frame, on the stream a copied pose of the same size would have travelled on, into the pose block that copy would
 * have taken; rz_deform_n, graph replays and rz_time_span replay the resident pose. No host synchronisation; one character's state rides
 * in the kernel arguments, a crowd's states go through a slot of the pinned ring.
 * rz_upload_motions: independent of rz_upload_animation (both may be resident); n_clips = 0 removes the library; refused while forks exist
 * (they borrow it); a new skeleton drops it; rz_get_tuning("motion_clips") = the count. rz_set_pose_blended needs the library and
 * rz_upload_skeleton_topology; it refuses (RZ_ERR_INVALID, the resident pose untouched) a clip index >= n_clips (other than RZ_NO_CLIP in
 * clip_b), a non-finite frame that would be sampled, a blend that is not in [0, 1], and a morph set of another size than the one the
 * feeds were built for (upload the library again); a device error behind those checks leaves the context without a pose, as in
 * rz_upload_pose. It cancels an outstanding rz_map_pose mapping. The ABI version stays 8: bindings
 * detect the symbols. */
#define RZ_NO_CLIP 0xffffffffu
typedef struct rz_motion_state { uint32_t clip_a; float frame_a; uint32_t clip_b; float frame_b; float blend; } rz_motion_state;
int rz_upload_motions(rz_ctx *ctx, uint32_t n_clips, const rz_animation *clips);
int rz_set_pose_blended(rz_ctx *ctx, const rz_motion_state *states);
/* ---- layers on top of the cross-fade: bone / morph masks, additive clips — NEW (optional) ----
 * rz_set_pose_layered poses instance i from base[i] exactly as rz_set_pose_blended does, then applies layers[i][0 .. n_layers) in order
 * (n_layers <= RZ_MAX_MOTION_LAYERS), each one clip of the library at its own frame with a weight, an optional mask and a mode
 * (tests/layer_ref.py is the definition):
 *   1. (q, t, w) is what rz_set_pose_blended defines for base[i].
 *   2. A layer with clip == RZ_NO_CLIP or weight == 0 is skipped as a whole: its other fields are not read (a non-finite frame is legal).
 *   3. Otherwise L = sample(clip, frame), the library's sampler. The layer acts on bone b only when the clip keys b (a track with at least
 *      one key) AND the mask includes b (RZ_NO_MASK includes everything):
 *        RZ_LAYER_OVERRIDE   q = Quat.slerp(q, qL, weight),  t = t + (tL - t) * weight;  at weight == 1 q and t ARE qL and tL
 *        RZ_LAYER_ADDITIVE   q = Quat.multiply(q, Quat.slerp(identity, qL, weight)),  t = t + tL * weight   (the forms bone morphs use;
 *                            nothing is renormalised beyond what those forms do)
 *   4. The layer acts on vertex morph m only when at least one of m's feeds in that clip holds a key AND the mask includes m (masks
 *      uploaded without morph masks include every morph); wL = the effective weight (own track, then group feeds):
 *        OVERRIDE   w = w + (wL - w) * weight, at weight == 1 w IS wL;   ADDITIVE   w = w + wL * weight
 *   5. n_layers == 0, or every layer skipped, gives the bits of rz_set_pose_blended(base).
 * The result is written where rz_set_pose_blended writes it (rz_motion_kernel with layers, once per call, same pose block, stream and event);
 * every frame behind it is an rz_set_pose_local frame and replays do not sample again. One character's state and layers ride in the
 * kernel arguments (100 bytes), a crowd's I x (20 + 20 n_layers) bytes go through a slot of the pinned ring.
 * rz_upload_motion_masks: n_masks masks, one byte per bone (non-zero = included), and optionally one byte per vertex morph; static data
 * like the library (forks see it; refused while forks exist; a new skeleton drops it; n_masks = 0 removes it;
 * rz_get_tuning("motion_masks") = the count). The masks are built for the morph set resident at upload: with a set of another size
 * rz_set_pose_layered refuses masked layers until they are uploaded again.
 * rz_set_pose_layered refuses (RZ_ERR_INVALID, the resident pose untouched, instance and layer named) whatever rz_set_pose_blended refuses
 * of base, n_layers > RZ_MAX_MOTION_LAYERS, layers == NULL with n_layers > 0, and a layer that is not skipped with a clip >= n_clips, a
 * mask >= n_masks (other than RZ_NO_MASK), a mode > 1, a weight that is not finite or not in [0, 1], or a non-finite frame. It cancels an
 * outstanding rz_map_pose mapping. The ABI version stays 8: bindings detect the symbols. */
#define RZ_MAX_MOTION_LAYERS 4
#define RZ_NO_MASK 0xffffffffu
enum { RZ_LAYER_OVERRIDE = 0, RZ_LAYER_ADDITIVE = 1 };
typedef struct rz_motion_layer { uint32_t clip; float frame; float weight; uint32_t mask; uint32_t mode; } rz_motion_layer; /* 20 B */
int rz_upload_motion_masks(rz_ctx *ctx, uint32_t n_masks, const uint8_t *bone_mask /* [n_masks][B] */, const uint8_t *morph_mask /* [n_masks][M] or NULL */);
int rz_set_pose_layered(rz_ctx *ctx, const rz_motion_state *base /* [I] */, uint32_t n_layers, const rz_motion_layer *layers /* [I][n_layers] */);
/* ---- physics hand-off for device-solved poses ----
 * updateModelPose()  engine/src/engine.ts:2375-2381: between evaluatePose() and the world-matrix upload the reference
 * lets physics overwrite the world matrices of rigid-body-driven bones IN PLACE (physics.ts:715-751,
 * boneWorldMatrices.set(values, boneIndex * 16)): children keep the matrices solved from the un-overridden parent.
 * With rz_set_pose the host owns the world matrices and does exactly that before the call. When the hierarchy is
 * solved on the GPU (rz_set_pose_local / rz_set_pose_sampled) this entry point is the same hook: `n` world matrices
 * (column-major 4x4, affine) replace the solved ones of (instance[k], bone[k]) after the hierarchy solve and before
 * the palette product, in every following frame until the next call; n = 0 clears. instance = NULL means instance 0.
 * Several entries for one bone: the last wins (successive set() calls). Asynchronous H2D through pinned staging.
 * Physics itself (Bullet via @fred3d/ammo) stays out of scope: this only carries its result.
 * ---- bones below an overridden bone follow it — NEW (optional, off by default) ----
 * The seam above leaves every bone BELOW an overridden one where the un-overridden solve put it: a strand's tip bone without a body,
 * an ornament hanging off a hair bone, the sub-bone of a skirt plate stay with the animation while the physics bone swings away.
 * rz_override_follow(ctx, 1) adds one stage to the device hierarchy solve, defined by tests/follow_ref.py:
 *   S   the solved world matrices of an instance — hierarchy, bone morphs and IK, exactly what is solved without the flag;
 *   O   the set of that instance's overridden bones, with matrices O_a (hand-fed here, or written by rz_physics_step);
 *   every bone b outside O with an ancestor in O takes, with a = the NEAREST such ancestor along `parents`,
 *       W_b = O_a (S_a^-1 S_b),   S_a^-1 the rigid inverse (R^T, -R^T p: world matrices carry no scale);
 *   bones of O take O_a, all others keep S_b. So an override below another override is absolute: the bones between the two follow the
 *   upper one, the bones below the lower one the lower one.
 * Order of a frame: sample -> bone morphs -> hierarchy -> IK -> followers -> overrides -> palette. NOT covered — nothing is evaluated again
 * on the followed pose: append rotation / move whose append parent is overridden or follows; IK chains below an overridden bone; following
 * (type 0 / 2) bodies on follower bones (the first solve of rz_physics_step runs without overrides as before, so bodies are placed on the
 * un-followed pose). PMX after-physics bones are a stage of their own behind the overrides (rz_upload_after_physics below), which
 * re-evaluates the listed bones; transform levels among before-physics bones stay unread (the first solve reads pose quaternions, which
 * adds no ordering dependency).
 * A flag of the context, off by default. It needs a resident topology (RZ_ERR_INVALID without), persists across rz_override_world calls,
 * physics uploads / removals and rz_set_instances, and is cleared by a new skeleton or topology. A fork inherits it at rz_fork and may set
 * it like its lender. A change drops the captured graph. on > 1: RZ_ERR_INVALID, context untouched. The follower lists — per instance the
 * followers ascending by bone, each with its ancestor's entry in the override table — are built on the host from `parents` wherever the
 * override set is built: here (they travel in the same pinned slot down the same stream), with a physics table's per-instance buffers,
 * and when the flag flips while a set is resident. With the flag off, or with a set nothing hangs below, nothing is built, uploaded or
 * passed and every frame launches what it launched before; with follower entries resident the solve is rz_fk_kernel<RzFollowParams> /
 * rz_fk_kernel<RzIkParams, RzFollowParams>, and a single character's frame keeps the solve in that kernel instead of its own prologue.
 * rz_get_tuning("override_follow") = 0 / 1, ("override_followers") = the follower entries resident over all instances (0 while off).
 * The ABI version stays 8: bindings detect the symbol. Host twin for host-solved poses: Model.followOverrides (host/model.js). */
int rz_override_world(rz_ctx *ctx, uint32_t n, const uint32_t *instance, const uint32_t *bone, const float *world16);
int rz_override_follow(rz_ctx *ctx, uint32_t on);
/* ---- PMX after-physics bones: solved again behind the overrides — NEW (optional) ----
 * PMX flag 0x1000 ("deform after physics") marks helper bones that must see the simulated pose: a skirt or sleeve aid that takes half the
 * rotation of the physics bone beside it, a chest support that appends from a sprung body's bone, a twist bone under a physics-driven arm.
 * Solved once before the physics step, such a bone stays with the animation while the bone it copies swings away. rz_upload_after_physics
 * hands over the ordered list A of those bones (ascending transform level, then index: Model.afterPhysicsOrder in host/model.js); a
 * frame then runs sample -> bone morphs -> hierarchy -> IK -> followers -> overrides -> AFTER-PHYSICS BONES -> palette. The stage is defined
 * by tests/after_ref.py. With F the world matrices as the frame leaves them today and O the instance's overridden bones, for b in A, in
 * list order:
 *   b in O: skipped — an overridden bone is never re-evaluated;
 *   P = F[parent(b)] (identity for a root); with an append parent a in effect, a's local transform AS FINALLY POSED is read from F:
 *   R_a = rot(F[parent(a)])^T rot(F[a]), t_a = rot(F[parent(a)])^T (pos(F[a]) - pos(F[parent(a)])) - bind_a (a root a: F[a] itself),
 *   q_a = quat(R_a) by the branch on the largest of trace, m00, m11, m22, normalised; then the local matrix exactly as the first solve forms
 *   it from q_a and t_a (ratio clamped to [-1, 1] for the rotation, conjugate for a negative ratio, the shorter arc, |ratio| <= 1e-6 = no
 *   append, the unclamped ratio for append move): L = T(bind_b + t_b) R(A) R(q_b) T(add), with q_b, t_b the local pose after bone morphs;
 *   F[b] = P L, and later entries read the new F[b].
 * So a listed bone below an overridden bone follows it through its own local transform, not rigidly, and a helper that appends from an
 * overridden bone, a follower, an IK link or an earlier listed bone sees where that bone really is. Where the append parent itself takes
 * append, this stage sees its full local rotation, while the first solve, like the reference, leaves the parent's own append out: the one
 * place where the two passes differ by more than rounding. The stage runs only while the override table holds at least one entry (hand-fed
 * or physics'); without overrides the first solve is the answer already and every frame launches what it launched before, bit for bit.
 * NOT covered: non-listed bones below a listed bone keep their matrices (as in MMD); IK chains whose bones are listed are not solved again;
 * following bodies on listed bones are placed on the first solve; transform levels among before-physics bones; an append parent whose
 * final local rotation lies near 180 degrees (the shorter-arc choice flips there, exactly as in the first solve).
 * `bones` [n] is in evaluation order; n = 0 removes the list. RZ_ERR_INVALID, naming the bone: no topology resident, an index >= B, a bone
 * listed twice, a listed bone whose parent, append parent or append parent's parent is listed LATER (the authoring error PMX editors warn
 * about; level-parallel evaluation would not reproduce MMD's one-frame lag). RZ_ERR_UNSUPPORTED: a listed bone that is a link or the
 * effector of a resident IK chain or lies on its path (outermost link ... effector) — in whichever order the two tables arrive:
 * rz_upload_ik checks the resident list too; a goal may be listed — and a skeleton whose 48 B per bone + 1 B per entry exceed 160 KB of LDS.
 * Static data: a new skeleton or topology clears the list, rz_fork lends it, and it is refused while forks exist like every static upload.
 * The host derives dependency levels (level = 1 + the largest level over EARLIER entries that are the bone's parent, append parent or append
 * parent's parent) and rz_fk_after_kernel (kernels/after.hip), a kernel of its own behind whichever hierarchy kernel ran, evaluates a
 * level in parallel. A single character's frame keeps its solve out of the deform kernel's prologue while the stage runs.
 * rz_get_tuning("after_physics") = entries resident, ("after_physics_levels") = their levels. ABI stays 8: bindings detect the symbol.
 * Host twin for host-solved poses: Model.solveAfterPhysics (host/model.js). */
int rz_upload_after_physics(rz_ctx *ctx, uint32_t n, const uint32_t *bones);
/* ---- rigid-body physics on the device for PMX bodies and joints — NEW (optional) ----
 * The reference runs Bullet (Ammo, loaded at run time: engine/src/physics.ts) on the host around the seam above. rz_upload_physics /
 * rz_physics_step keep the seam (physics.ts:534-569) and replace the solver by one of this build's own, defined in float64 by
 * tests/physics_ref.py and run in float32 by rz_physics_kernel (kernels/physics.hip), which WRITES THE OVERRIDE TABLE on the device: no
 * frame kernel changes, and without a table every frame launches what it launched before. The ABI version stays 8: bindings detect the symbols.
 * One rz_physics_step(substeps):
 *   1. the hierarchy solve of the resident pose runs without overrides (with IK when a table is resident); a body of type 0 or 2, or of mass
 *      0, is placed at boneWorld x offset with zero velocity (physics.ts:663-667 treats types 0 and 2 alike); bone -1: at offset itself.
 *      offset = inverseBind x T(shapePosition) R(shapeRotation) (physics.ts:572-596), computed by the caller, as position3 + quaternion4.
 *   2. `substeps` fixed steps of h (default 1/75 s, the reference's fixedTimeStep; callers cap at 10 per call, its maxSubSteps). XPBD rigid
 *      bodies (Mueller et al. 2020) in the smallest form that covers PMX joints. Per substep:
 *        integrate the dynamic bodies (type 1, mass > 0):  v += h g  (g default (0, -98, 0), physics.ts:56);  v *= (1 - linear_damping)^h;
 *          w *= (1 - angular_damping)^h;  keep x_prev, q_prev;  x += h v;  q = normalize(q + (h/2) [w, 0] (x) q)   (no gyroscopic term)
 *        `iterations` passes (default 4) over the joints in colour order — colours assigned at upload, greedily in file order, so that no
 *          two joints of a colour share a dynamic body; per joint, with p = x + q r the world anchors, Q_A = q_A j_A the joint frame carried
 *          by body A (anchors r and frames j taken once in the bind pose: the body at T(sum of bind translations up its bone's chain) x offset,
 *          the joint at position3 / Quat.fromEuler(rotation3)):
 *            position         d = Q_A^-1 (p_B - p_A);  e = d - clamp(d, position_min, position_max);  c = Q_A e is removed as a rigid
 *                             positional constraint (compliance 0) with the 3 x 3 generalised inverse mass of the anchor pair:
 *                             K p = c,  K = (1/m_A + 1/m_B) 1 - [r_A]x I_A^-1 [r_A]x - [r_B]x I_B^-1 [r_B]x;  A gets +p at r_A, B -p
 *                             at r_B. (The scalar split 1/m + (r x n)^T I^-1 (r x n) along n = c / |c| moves the anchor off n whenever
 *                             the body is not a ball around it: its residual rose between iterations and the bodies jittered.)
 *                             Skipped when |c| <= 1e-9 or det K <= 0
 *            rotation limits  the Euler angles ('XYZ', R = Rx Ry Rz, the IK limits' convention) of q_rel = Q_A^-1 Q_B clamped to
 *                             [rotation_min, rotation_max]; when any changed, the rotation Q_A q_clamped q_rel^-1 Q_A^-1 — angle
 *                             theta = 2 atan2(|xyz|, w) about n — is removed as a rigid angular constraint with the 3 x 3 inverse inertia
 *                             of the pair: K l = theta n, K = I_A^-1 + I_B^-1 in world space; A turns by -I_A^-1 l, B by +I_B^-1 l (the
 *                             scalar split n^T I^-1 n turns a body about I^-1 n, not n: a welded joint then only converges linearly).
 *                             Skipped when |xyz| <= 1e-9 or det K <= 0
 *            angular springs  Euler angles (ex, ey, ez), Q_A and Q_B taken once, after the limits; per axis with spring_rotation k > 0:
 *                             C = that angle, about its gimbal axis n (x: Q_A e_x, y: Q_A (0, cos ex, sin ex), z: Q_B e_z — a rotation
 *                             about which changes that angle alone), alpha~ = 1 / (k h^2),
 *                             d_lambda = (-C - alpha~ lambda) / (w_A + w_B + alpha~); lambda is accumulated over the iterations of a
 *                             substep and zero at its start
 *            linear springs   only under rz_physics_springs (below): the last stage of the joint, per axis with spring_position k > 0
 *          a rotation correction d_phi is applied as q = normalize(q + (1/2) [d_phi, 0] (x) q); a min > max pair of limits is swapped
 *        velocities from the pose change:  v = (x - x_prev) / h;  w = 2 (q (x) q_prev^-1).xyz / h, negated when .w < 0
 *      Inverse inertia, diagonal in the body frame: sphere 2/5 m r^2 (r = size.x); box m/3 (b^2 + c^2) with half extents = size; capsule the
 *      box of half extents (r, r + height/2, r) (r = size.x, height = size.y).
 *   3. every dynamic body with a bone gives boneWorld = bodyWorld x offset^-1: that bone's override, in every following frame until the
 *      next step. Children of an overridden bone keep the matrices solved from the un-overridden parent, as rz_override_world documents
 *      (unless rz_override_follow is on: then they follow it, as stated there).
 * NOT covered: contacts unless rz_physics_contacts enables them (below; boxes only under on = 2 and 3); linear springs (spring_position)
 * unless rz_physics_springs enables them (below); restitution. A welded joint (all limits equal) whose
 * anchor is off the body's centre converges only linearly in `iterations` (the position and the rotation stage each undo part of the
 * other): about 0.3 of a parent's jump is left at 4 iterations, 1e-5 of it at 32. Without contacts shapes feed the inertia only; group, mask
 * and friction are kept for the contact stage and spring_position for the linear springs; restitution is unused (group, mask, friction,
 * restitution and spring_position may be NULL; contacts need the first three, the linear springs the last). There is no host-side twin of the solver.
 * rz_upload_physics: needs rz_upload_skeleton_topology first; NULL or n_bodies = 0 removes the table; gravity3 NULL, h = 0, iterations = 0 =
 *   the defaults. RZ_ERR_INVALID (context untouched): a body, bone or joint index out of range, body_a == body_b, a value that is not finite,
 *   mass < 0, a damping outside [0, 1], h < 0, a type or shape above 2, two dynamic bodies on one bone. RZ_ERR_UNSUPPORTED: a table whose state does not fit the
 *   kernel's LDS (96 B per body, + 12 B per joint once the joints outnumber the 256 lanes; the limit is 160 KB). A new skeleton or
 *   topology drops the table. With a table resident physics owns the override table — the dynamic bodies' bones of instance i at
 *   [i nd, (i + 1) nd) — and rz_override_world is refused.
 * rz_physics_step: enqueues on the frame's stream, no host synchronisation: the hierarchy solve, then rz_physics_kernel (one workgroup per
 *   instance, state in LDS across all substeps). substeps = 0 only re-places the following bodies and re-emits the overrides; more than 1000 in one call is RZ_ERR_INVALID. Acts on
 *   device-solved poses only (rz_set_pose_local / _sampled / _blended; with rz_set_pose the host owns the world matrices: refused). The
 *   first step after an upload, after rz_physics_reset, or after rz_set_instances changed the count behaves as a reset followed by the step.
 *   rz_deform_n, graph replays and rz_time_span replay the resident overrides and do not advance the simulation; the override buffers keep
 *   their addresses across steps. The one-launch crowd form is not taken while overrides are resident (as with rz_override_world).
 * rz_physics_reset: every body onto its bone's SOLVED (un-overridden) pose, zero velocities (without a device-solved pose: at the next step).
 * All three are refused while forks exist. rz_read_physics: per body x3 q4 v3 w3 of one instance; blocking; for tests and tools.
 * rz_get_tuning("physics_bodies") / ("physics_joints") / ("physics_colours") = the counts; ("physics_block") = the lanes per workgroup the
 * resident table is solved with (64 when the bodies and the widest colour fit one wave, else 256), ("physics_own") = 1 when every lane keeps
 * its joint in registers (no more joints than lanes), 0 when lanes stride over a colour, ("physics_lds") = the bytes of LDS per workgroup;
 * all read-only, 0 without a table.
 * ---- contacts between rigid bodies — NEW (optional, off by default) ----
 * rz_physics_contacts(ctx, 1) adds a contact stage to rz_physics_kernel for the resident table (the reference registers every body with
 * 1 << group and its mask, physics.ts:257-269, and joints do not exempt their bodies); 2 adds it with the table's boxes taking part (`boxes`
 * below); 3 with pairs of two boxes as well (`box pairs` below); 0 drops it. Defined in float64 by tests/contact_ref.py.
 *   shapes      a sphere is the point x with radius size.x; a capsule the segment x +- q (0, size.y / 2, 0) with radius size.x (axis Y).
 *   candidates  fixed when the stage is enabled: all a < b with at least one dynamic body, both spheres or capsules with radius > 0, both
 *               masks nonzero, (1 << group[a]) & mask[b] and (1 << group[b]) & mask[a] both nonzero. follow pairs (one dynamic body):
 *               per dynamic body the list of its following partners, ascending; dynamic pairs: coloured greedily in lexicographic (a, b)
 *               order so that no two pairs of a colour share a body, solved in (colour, a, b) order.
 *   where       in every iteration of a substep, after the last joint colour: pass F, every dynamic body on itself alone against its
 *               following partners in list order; then pass D, the dynamic pairs colour by colour.
 *   one contact (A the lower index)
 *     1. closest points cA, cB of the segments P + s d, s in [0, 1], P = x - u, d = u + u, u = q (0, size.y / 2, 0): with r = P_A - P_B,
 *        a = d_A.d_A, e = d_B.d_B, f = d_B.r, c = d_A.r, b = d_A.d_B and clamp to [0, 1]: a <= 1e-9 and e <= 1e-9: s = t = 0; a <= 1e-9:
 *        s = 0, t = clamp(f / e); e <= 1e-9: t = 0, s = clamp(-c / a); else s = clamp((b f - c e) / (a e - b b)) when a e - b b > 1e-9, else 0;
 *        t = (b s + f) / e; t < 0: t = 0, s = clamp(-c / a); t > 1: t = 1, s = clamp((b - c) / a)
 *     2. d = cB - cA, dist = |d|, pen = (rA + rB) - dist; skipped unless pen > 0 and dist > 1e-9
 *     3. n = d / dist; arms ra = (cA + n rA) - x_A, rb = (cB - n rB) - x_B
 *     4. w = w_A + w_B, w_X = 1/m_X + (r_X x n)^T I_X^-1 (r_X x n), 0 for a following body; skipped unless w > 0
 *     5. d_lambda = pen / w, p = n d_lambda: x_A -= p / m_A, q_A turned by -I_A^-1 (ra x p); x_B += p / m_B, q_B by +I_B^-1 (rb x p)
 *     6. friction, mu = friction[A] friction[B] (Bullet's combination), when mu > 0: the arms are carried in the body frames from before 5
 *        (la = q_A^-1 ra, lb likewise) and re-expressed in the corrected pose; the contact point's slip over this substep
 *        D = [(x_A + ra) - (x_A,prev + q_A,prev la)] - [the same for B], its tangential part Dt = D - n (D.n); when |Dt| > 1e-9 an impulse
 *        of min(|Dt| / w_t, mu d_lambda) along Dt / |Dt| (w_t the generalised inverse mass along it, skipped unless > 0), A -, B +. A
 *        following body's previous pose is its current pose (it is placed once per call).
 *     7. only dynamic bodies are corrected and written.
 *   boxes       on = 1: no contact involves a box (those with a nonzero mask are counted in "physics_contact_boxes"). on = 2: a box (shape 1,
 *               the set |y_i| <= e_i in its own frame, e = size3, the three half extents the inertia reads) takes part when all three are
 *               > 0 and its mask is nonzero, against spheres and capsules in either index order, following or dynamic, as a shape of
 *               radius 0. A pair of two boxes is no candidate; those the rule would pair are counted in "physics_contact_box_pairs".
 *               Defined in float64 by tests/contact_box_ref.py. With a box X and a round shape R (segment P + s d, radius r; a sphere:
 *               d = 0) step 1 becomes:
 *     1a. the segment in the box frame: P' = q_X^-1 (P - x_X), d' = q_X^-1 d
 *     1b. c(s) = P' + s d', g(s) = c - clamp(c, -e, e), f(s) = g(s).d' (half the derivative of the squared distance, monotone):
 *         f(0) >= 0: s = 0; else f(1) <= 0: s = 1; else 24 bisection steps on [lo, hi] = [0, 1] — m = (lo + hi) / 2, f(m) > 0: hi = m,
 *         else lo = m — and s = (lo + hi) / 2
 *     1c. b' = clamp(c(s), -e, e); the round shape's point is P + s d in world space, the box's x_X + q_X b'
 *     1d. shallow, |c(s) - b'| > 1e-9: steps 2 - 7 unchanged (A the lower index, n from cA to cB, the box's radius 0)
 *     1e. deep, |c(s) - b'| <= 1e-9 (the centre line is inside the box): the axis i with the smallest e_i - |c_i| (the first of x, y, z
 *         wins a tie), sg = +1 when c_i >= 0, else -1; outward normal N = sg q_X axis_i; the box's point is c with component i set to
 *         sg e_i; pen = r + (e_i - |c_i|); n = N when the box is A, -N when it is B; steps 3 - 7 with this n and pen, without the
 *         dist > 1e-9 test.
 *         A pair without a box runs steps 1 - 7 as they are.
 *   box pairs   on = 3: everything on = 2 does, and a pair of two boxes that the rule pairs is a candidate like any other — it enters the
 *               follow lists and the coloured dynamic pairs, counts toward the 65 536 candidates and is counted in
 *               "physics_contact_box_box"; "physics_contact_box_pairs" is then 0. Defined in float64 by tests/contact_boxbox_ref.py. For
 *               two boxes, A the lower index, with a_i = q_A axis_i, b_j = q_B axis_j, half extents eA and eB, t = x_B - x_A,
 *               C_ij = a_i.b_j, tA_i = a_i.t, tB_j = b_j.t, step 1 becomes:
 *     1a. the overlaps of the 15 axes. Face A_i: o = eA_i + sum_j eB_j |C_ij| - |tA_i|. Face B_j: o = sum_i eA_i |C_ij| + eB_j - |tB_j|.
 *         Edge (i, j), with i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1, j2 likewise and l2 = 1 - C_ij^2, considered only when l2 > 1e-6:
 *         o = (eA_i1 |C_i2,j| + eA_i2 |C_i1,j| + eB_j1 |C_i,j2| + eB_j2 |C_i,j1| - |tA_i2 C_i1,j - tA_i1 C_i2,j|) / sqrt(l2).
 *         Any considered o <= 0: no contact.
 *     1b. the face axis is the first smallest in the order A0 A1 A2 B0 B1 B2, the edge axis the first smallest in the order (0,0), (0,1)
 *         .. (2,2); the edge wins only when o_edge < 0.95 o_face; pen is the chosen o.
 *     1c. a face axis i of the reference box X, the other box Y incident: sg = +1 when the component along the axis of the vector from
 *         x_X to x_Y is >= 0, else -1; N = sg axis. Y's point p = x_Y - sum_k clamp((N.y_k) / 0.05, -1, 1) eY_k y_k: a vertex, sliding
 *         continuously to an edge midpoint or the face centre as Y's face becomes parallel to X's. p' = q_X^-1 (p - x_X) clamped to
 *         [-eX, eX], its component i then set to sg eX_i; cX = x_X + q_X p', cY = cX - N pen; n = N when X is A, else -N.
 *     1d. an edge axis (i, j): L = (a_i x b_j) / |a_i x b_j|, n = L when t.L >= 0, else -L. A's edge has its centre at
 *         x_A + sum_{k != i} s_k eA_k a_k, s_k = +1 when a_k.n >= 0, else -1, and half length eA_i along a_i; B's at
 *         x_B - sum_{k != j} s'_k eB_k b_k, s'_k from b_k.n likewise, half length eB_j along b_j. cA, cB are the closest points of the
 *         two segments by the clamped solve of step 1 above.
 *         Then steps 3 - 7 with both radii 0, without the dist > 1e-9 test. One point per pair and iteration: no manifold.
 *         At rest a face on a face is the tie of 1b between A_i and B_i; the first in the order wins it. A thin plate lying flat is
 *         turned back by about 60 g h^2 / e times its tilt per contact (e its larger half extent): at the default step and gravity
 *         a plate with e of 0.6 and less rattles at rest by some 0.007 rad, one of 0.8 rests.
 *   NOT covered: restitution, a velocity pass (a penetration removed in one substep arrives as velocity, as in plain XPBD), a broad
 *   phase, a manifold of several points; under on = 2 box against box (left out, counted in "physics_contact_box_pairs").
 * rz_physics_contacts: on = 1 (and every value but 0, 2 and 3) builds and uploads the lists for the resident table, on = 2 the lists with
 *   the boxes taking part, on = 3 those with pairs of two boxes as well, on = 0 drops them; switching among 1, 2 and 3 rebuilds them; none resets the simulation; all
 *   drop a captured graph (replays still do not advance the simulation). A new rz_upload_physics, a table removal, a new skeleton or a
 *   new topology turns contacts off. RZ_ERR_INVALID: no resident table; a table uploaded with group, mask, friction or size3 NULL; forks
 *   exist. RZ_ERR_UNSUPPORTED (the context keeps its state): more than 65 536 candidates, follow entries + dynamic pairs — every pair of
 *   the table is tested, a broad phase does not exist yet. The stage adds no LDS: "physics_lds" and the 160 KB limit are unchanged.
 * rz_get_tuning("physics_contacts") = 0 / 1 / 2 / 3, ("physics_contact_follow") = the follow entries, ("physics_contact_pairs") = the dynamic
 * pairs, ("physics_contact_colours") = their colours, ("physics_contact_boxes") = the boxes with a nonzero mask that take no part (on = 1:
 * all of them; on = 2 and 3: those with an extent of 0), ("physics_contact_box_pairs") = the pairs of two boxes left out under on = 2 (a build
 * without box contacts does not know this key: that is how a binding detects them), ("physics_contact_box_box") = the pairs of two boxes
 * taking part under on = 3, 0 in every other mode (a build without on = 3 does not know this key, the ABI version stayed 8: that is how a
 * binding detects it); all read-only, 0 without contacts.
 * ---- linear joint springs — NEW (optional, off by default) ----
 * rz_physics_springs(ctx, 1) adds the linear springs of the resident table's joints (PMX spring_position: a joint with play along an axis
 * and a spring on it then swings about its rest point instead of hanging at the end of its play); 0 drops them. Defined in float64 by
 * tests/spring_ref.py. The stage is the last of a joint's solve, behind the angular springs, in every iteration; per axis ax = x, y, z in
 * that order with spring_position[ax] = k > 0, each axis from the pose the one before left:
 *     r_A = q_A r_a, r_B = q_B r_b, n = Q_A e_ax (Q_A = q_A j_A; n is taken as fixed for this correction)
 *     C = n . ((x_B + r_B) - (x_A + r_A)) — the component of d the position stage computes; the rest point is 0
 *     w = 1/m_A + 1/m_B + (r_A x n)^T I_A^-1 (r_A x n) + (r_B x n)^T I_B^-1 (r_B x n)
 *     alpha~ = 1 / (k h^2), d_lambda = (-C - alpha~ lambda) / (w + alpha~), lambda += d_lambda (three more multipliers per joint, zero at
 *     the start of a substep);  x_A -= n d_lambda / m_A, q_A turned by -I_A^-1 (r_A x n) d_lambda;  x_B += n d_lambda / m_B, q_B by
 *     +I_B^-1 (r_B x n) d_lambda. Only dynamic bodies are written; k <= 0: no spring on that axis.
 *   One body on one spring is backward Euler's oscillator: period 2 pi h / atan(omega h) with omega^2 = k / m, amplitude falling by
 *   (1 + (omega h)^2)^(-1/2) per substep, whatever `iterations` is. The rest point is always 0 (the joint's own position).
 * rz_physics_springs: on != 0 derives one record per joint (alpha~ per axis in double, rounded once, and the axes' bits) from the
 *   spring_position3 kept at upload and selects the LSPRING instantiations of rz_physics_kernel; a table without any k > 0 is taken and
 *   goes on through the kernels and the LDS it had. Neither value resets or touches the simulation; both drop a captured graph. A new
 *   rz_upload_physics, a table removal, a new skeleton or a new topology turns the springs off. Without the call a table steps through
 *   exactly the kernels, and to exactly the bits, it did before this entry point existed. RZ_ERR_INVALID: no resident table; forks exist;
 *   a table with joints uploaded with spring_position3 NULL. RZ_ERR_UNSUPPORTED: in the striding form (more joints than lanes) the
 *   multipliers in LDS cost 24 B per joint instead of 12, and 96 B per body + 24 B per joint exceeds 160 KB. The context keeps its state
 *   in every case. The block size chosen at upload does not change.
 * rz_get_tuning("physics_springs") = 0 / 1, ("physics_spring_axes") = the (joint, axis) pairs with k > 0 while enabled, else 0;
 * ("physics_lds") reports the size actually launched. A build without the symbol has no linear springs (the ABI version stayed 8).
 * ---- PMX type-2 bodies, "physics + bone position alignment" — NEW (optional, off by default) ----
 * Without rz_physics_aligned a body of type 2 follows its bone, as in the engine this one was modelled on. MMD simulates it like a dynamic
 * body and gives its bone the rotation only; rz_physics_aligned(ctx, 1) does the same. Defined in float64 by tests/align_ref.py. A body is
 * ALIGNED when the feature is on, its type is 2, its mass is > 0 and it has a bone. A type-2 body with a mass and no bone becomes a plain
 * dynamic body; a type-2 body of mass 0 keeps following its bone. The table is then the same table with those bodies' type read as 1 —
 * integration, joints in colour order, every spring, every contact mode, velocities, all as stated above — and two rules:
 *   1. at the start of every rz_physics_step call — once per call, not per substep — an aligned body keeps q, v and w and is put back onto
 *      its bone: x = p_bone + rot(q (x) offset_q^-1) offset_p, p_bone the translation of the bone's matrix in the un-overridden solve the
 *      call has just run. On a reset (the implicit one of the first step too) every body is placed on its bone as ever, which satisfies it.
 *   2. the override of an aligned body's bone takes its rotation from the body, q (x) offset_q^-1, and its translation column is the solved
 *      matrix's own, the same float32 bits. The state (rz_read_physics) keeps the simulated x.
 *   There is no pin inside the solve: joints hold the body, as in MMD; an aligned body without a joint drifts during a call and is back on
 *   its bone at the next. substeps = 0 re-pins and re-emits with the new bone position. rz_physics_step(n) is therefore NOT n calls of
 *   rz_physics_step(1) for a table with aligned bodies; it stays so, bit for bit, for every other table.
 * rz_physics_aligned: on != 0 derives again, from the table kept at upload, everything rz_upload_physics derives — validation, the joints'
 *   colours and order, inverse mass and inertia, the overridden bones and their slots, the block size — with those bodies dynamic, and
 *   flags the aligned ones; 0 derives it as uploaded. Like a new upload both values turn contacts and linear springs off, reset the
 *   simulation, drop a captured graph and rebuild rz_override_follow's lists: call it right behind rz_upload_physics, ahead of
 *   rz_physics_springs and rz_physics_contacts. A new rz_upload_physics, a table removal, a new skeleton or a new topology turns it off.
 *   With on = 1 and no aligned body the table steps through the kernels, and to the bits, of a plain upload; the ALIGN instantiations of
 *   rz_physics_kernel run only for a table that has one. RZ_ERR_INVALID: no resident table; forks exist; two bodies that are dynamic now
 *   drive one bone (the message names both). RZ_ERR_UNSUPPORTED: the LDS of the launch form the new colouring selects exceeds 160 KB —
 *   the upload's own check on the new block size; with 96 B per body and 12 B per joint it cannot fail for a table the upload took (the
 *   block differs only below 65 bodies, where both forms fit). The context keeps its state in every one of them.
 * rz_get_tuning("physics_aligned") = 0 / 1, ("physics_aligned_bodies") = the aligned bodies while on, else 0. A build without the symbol
 * has no aligned bodies (the ABI version stayed 8). */
typedef struct rz_physics {
    uint32_t n_bodies;
    const int32_t *bone;                /* [n_bodies] -1 = none */
    const uint8_t *type, *shape;        /* type 0 follows its bone, 1 dynamic, 2 dynamic + bone (follows like 0 unless rz_physics_aligned); shape 0 sphere, 1 box, 2 capsule */
    const float *size3, *offset_pos3, *offset_rot4;
    const float *mass, *linear_damping, *angular_damping, *restitution, *friction;
    const uint8_t *group;
    const uint16_t *mask;
    uint32_t n_joints;
    const uint32_t *body_a, *body_b;
    const float *position3, *rotation3;                 /* model space, bind pose; rotation as the loader's Euler angles */
    const float *position_min3, *position_max3, *rotation_min3, *rotation_max3, *spring_position3, *spring_rotation3;
    const float *gravity3;              /* NULL = (0, -98, 0) */
    float h;                            /* 0 = 1/75 s */
    uint32_t iterations;                /* 0 = 4 */
} rz_physics;
int rz_upload_physics(rz_ctx *ctx, const rz_physics *tab);
int rz_physics_step(rz_ctx *ctx, uint32_t substeps);
int rz_physics_reset(rz_ctx *ctx);
int rz_physics_contacts(rz_ctx *ctx, uint32_t on);
int rz_physics_springs(rz_ctx *ctx, uint32_t on);
int rz_physics_aligned(rz_ctx *ctx, uint32_t on);
int rz_read_physics(rz_ctx *ctx, uint32_t instance, float *state13);
/* Blocking readback of one instance's world matrices (B x 16, column-major) as the frame used them. */
int rz_read_world(rz_ctx *ctx, uint32_t instance, float *world16);

/* computeSkinMatrices() dispatch  engine/src/engine.ts:2393-2402 (WGSL :906-930) followed by the
 * per-vertex body of vs()  engine/src/engine.ts:253-272 (copies :440-443/:700-703), executed
 * once per frame instead of once per draw pass. Enqueues the frame; asynchronous. */
int rz_deform(rz_ctx *ctx);
/* Enqueue `frames` consecutive frames of the resident pose without returning to the host
 * in between (steady-state replay; same kernels as rz_deform). Asynchronous. */
int rz_deform_n(rz_ctx *ctx, uint32_t frames);

/* ---- frames in flight ----
 * WebGPU queues frames: while the GPU drains frame f the application is already encoding frame f + 1 into its own command
 * buffer and the renderer reads frame f's output. A context has ONE compute stream and ONE set of output buffers, so its
 * frames run strictly one after the other and every frame pays its own launch ramp and tail — 1 us of a 16 us frame on a
 * 1/8 shard of C5, 2 us of a 6 us frame on a 30 k-vertex character. rz_fork makes a second context on the same GPU that
 * BORROWS every static device buffer of `ctx` (mesh, skeleton, topology, morph targets, bone morphs, motion, motion library, edge scale — no
 * copy, no extra HBM) and owns everything per-frame (streams, pose slots, palettes, outputs, tuning state copied from `ctx`
 * at fork time). Alternate frames between the two (rz_set_pose* + rz_deform on one while the other's frame is in flight, or
 * rz_deform_pair for a replay) and the tail of frame f overlaps the ramp of frame f + 1: measured 16.3 -> 15.2 us per frame
 * on the 1/8 shard, 6.3 -> 4.4 us on the character (tools/archive/shard_two_streams.py). While forks exist, static uploads fail on
 * both sides with RZ_ERR_INVALID; destroy the forks before the context they were forked from (rz_destroy refuses otherwise).
 * A fork cannot be forked and takes no part in gathers. */
int rz_fork(rz_ctx *ctx, rz_ctx **fork_out);
/* `frames` frames of the resident poses, alternating a, b, a, b ... (each on its own stream, into its own outputs). */
int rz_deform_pair(rz_ctx *a, rz_ctx *b, uint32_t frames);

int rz_sync(rz_ctx *ctx);

/* Blocking readback of deformed positions / normals of instance `instance`, vertices
 * [v0, v0+n) of this shard, packed [n][3]. Either pointer may be NULL. (getDeformed()) */
int rz_read(rz_ctx *ctx, uint32_t instance, uint32_t v0, uint32_t n, float *pos3, float *nrm3);
/* Blocking readback of the skin-matrix palette of one instance as B x 12 floats (rows 0..2 of
 * world*inverseBind, row-major 3x4) — the skinMatrixBuffer of engine.ts:1770-1774. */
int rz_read_palette(rz_ctx *ctx, uint32_t instance, float *rows3x4);

/* ---- fused consumers of the deformed mesh (optional) ----
 * rz_upload_edge_scale: per-vertex outline edge size (the material's edgeSize of the draw call that owns the
 * vertex, engine/src/engine.ts:415-421). Once set, every frame also writes the outline pass's inverted hull
 * expandedPos = worldPos + worldNormal * edgeSize * 0.01 (engine.ts:458-461, vertex shader :431-463) so the
 * outline pipeline no longer re-skins; NULL turns it off. rz_read_hull reads it back.
 * rz_enable_aabb: every frame also reduces the axis-aligned bounding box of the deformed positions of each
 * instance inside the skin kernel (no extra pass over the mesh); rz_read_aabb returns min xyz, max xyz of the
 * most recent frame. With an SDEF table (rz_upload_sdef; the same holds for a QDEF table, rz_upload_qdef) the pass extends that box by the listed vertices' final positions, so the
 * box is that of all final positions together with the BDEF2 positions the skin kernel computed for the SDEF vertices first: a
 * conservative bound (it contains every final position), not always the tightest one. */
int rz_upload_edge_scale(rz_ctx *ctx, uint32_t V, const float *edge_size);
int rz_read_hull(rz_ctx *ctx, uint32_t instance, uint32_t v0, uint32_t n, float *pos3);
int rz_enable_aabb(rz_ctx *ctx, int enable);
int rz_read_aabb(rz_ctx *ctx, uint32_t instance, float min_max6[6]);

/* Benchmark helper: enqueue `frames` back-to-back frames of the resident pose between two HIP
 * events on the context's stream, then (mode 1) time the deform kernel alone and (mode 2) the
 * prep kernel alone the same way. Blocking. */
int rz_time_frames(rz_ctx *ctx, uint32_t frames, rz_timing *out);

/* Benchmark helper ("hipEvent pairs around >= 200 back-to-back frames after 20 warm-up frames"): `lead` untimed frames, then
 * `frames` timed frames of the resident pose exactly as rz_deform_n enqueues them — or, with a fork in `b`, as rz_deform_pair alternates
 * them — the timed ones between two events on the context's stream; blocks until they have drained and returns the span between the
 * events in ms. The lead frames sit in front of the opening event in the SAME call, so the timed frames are enqueued behind a busy GPU and
 * run back to back from the first one (lead = 0: the first timed frame starts on an idle GPU and waits ~5 us for its own launch). The
 * host's clock around the same calls adds a fixed ~30 us per timed region (first launch + waking up from the wait): 9 % of 20 steps of a
 * 16.6 us frame. b = NULL: one stream. */
int rz_time_span(rz_ctx *a, rz_ctx *b, uint32_t lead, uint32_t frames, double *span_ms);

/* Tuning knobs (bench sweeps / tests); 0 / -1 = automatic. Keys: "morph_split" (0,1,2,4,8 lanes
 * per vertex quad; without dense targets it only sets the wave step: 1 -> 256 vertices, >= 4 -> 64), "unroll" (0,4,8 morphs in flight per lane), "grid_cap" (total workgroups),
 * "geo_lds" (0/1: rest geometry transposed through LDS vs 4-byte loads), "nontemporal" (0/1,
 * morph-stream loads), "nt_store" (0/1, output stores), "fast" (-1 auto, 0 always run the
 * separate prep kernel, 1 one-launch frame when possible), "out_cap" (-1 auto, 0 off, else vertices a wave
 * parks in LDS before writing them out in one burst), "inst_loop" (-1 auto, 0 off, 2..8 / 10..64 poses
 * per workgroup in instanced morph-free frames, 9 = the register-resident form), "pose_prefetch" (-1 auto / 1: the first frame of a zero-copy pose — world matrices, or local rotations
 * [+ translations] of a single character whose hierarchy is solved inside the deform kernel — carries a helper workgroup that stages the
 * NEXT pose into device memory when the host has already written it — a per-frame loop whose host runs ahead of the GPU then never
 * pays the PCIe round trip; a staged pose is only ever taken by a frame of the same pose kind;
 * 0: off; rz_get_tuning("pose_staged") tells whether the current pose was staged that way),
 * "inst_subsets" (-1 auto / 1: a crowd workgroup stages
 * only the bones its vertex run names when that list is shorter than the skeleton — same bits, a fraction of the LDS and of the
 * per-workgroup front; 0: always the whole palette), "inst_block" (0 auto, 256 / 512 / 1024 threads per
 * workgroup of the instanced kernel; for crowds "fast" -1 / 1 = palettes formed inside the skin kernel, one launch per frame, 0 =
 * rz_prep_kernel in front), "inst_order" (1 default / 0: which workgroups of the instanced kernel an XCD gets — 1: every vertex run
 * of ITS pose groups, so an XCD's L2 pulls one eighth of the poses' matrices; 0: one vertex run of every pose group), "graph" (0/1: rz_deform_n replays hipGraphs of 16 captured frames instead of launching every kernel —
 * for launch-bound replay of small frames), "zero_copy" (-1 auto = on, 0: every pose is copied to the device; one character's
 * per-frame inputs are otherwise read by the frame's kernels straight from a pinned, device-mapped slot), "fuse_fk" (-1 auto, 0, 1:
 * a device-animated single character solves its bone hierarchy inside the deform kernel — one launch per frame — instead of
 * rz_fk_kernel [+ rz_prep_kernel] in front), "fuse_fk_plain" (-1 auto / 1: the fused frame of a PLAIN pose — no physics overrides, <= 512 bones, <= 256 morphs —
 * runs a kernel variant whose hierarchy solve is specialised for an uploaded / a sampled pose; 0: always the generic solve; same bits;
 * rz_get_tuning("effective_fk_kind") says which: 0 generic, 1 uploaded, 2 sampled),
 * "pose_pull" (-1 auto: the world matrices of a pose of more than 256 KB — a crowd's — are pulled out of their pinned ring slot by a
 * kernel on the upload stream, as the upper three rows of every affine matrix [a pose with any other bottom row travels whole]; local
 * rotations, a quarter of the bytes, stay with the copy engine, which does not disturb the frame they run under; 1: every such pose
 * is pulled; 0: the runtime copies every pose as it was handed over; rz_get_tuning("pose_pulled") / ("pose_rows") tell what the
 * last upload did),
 * "qdef_chunks" (0 auto = 1, 1..64: how many 256-vertex chunks of the QDEF table one workgroup of rz_qdef_kernel takes behind one
 * conversion of the skeleton to dual quaternions; same bits),
 * "sparse_piece" (0 auto, else a multiple of 16 in 16..2048: how many entries of the sparse targets' per-vertex CSR a wave stages in LDS
 * at a time — a test and diagnosis handle, same bits at every size; a piece the LDS does not hold next to the palette is lowered to what
 * fits; rz_get_tuning("effective_sparse_piece") gives the piece of the next frame, 0 without resident sparse targets),
 * "inst_morphs" (-1 auto = off, 0, 1: a crowd — rz_set_instances(n > 1) — with SPARSE morph targets takes the crowd skin kernels: a
 * workgroup decodes each vertex once for its group of "inst_loop" poses and walks the vertex's row of the CSR once per pose, the group's
 * per-instance morph weights parked in LDS behind its palettes, instead of the single-mesh kernel run once per instance. The same bits as
 * with the key off, on every instance. It applies where the morph-free crowd kernels apply — no outline hull, no bounding box,
 * "inst_loop" neither 0 nor 9, a group of at least two poses — and where the group's inst_loop x (morphs + 8, rounded up to 4) x 4 B of
 * weights fit the LDS beside its palettes [80 KB per workgroup at 256 threads, 156 KB otherwise]; otherwise, and for dense targets,
 * the frame is the one launched with the key off, never an error. A device-animated crowd solves its hierarchy in the same launch only
 * while the pose's morph weights are in device memory before the frame [rz_set_pose_local, rz_set_pose_blended, rz_set_pose_layered;
 * not at 1024 threads]: behind rz_set_pose_sampled rz_fk_kernel stays in front, which writes them.
 * rz_get_tuning("effective_inst_morphs") is 1 when the next frame walks morph rows in a crowd kernel),
 * "overlap" (-1 / 0 off, 1: crowds run their front kernels on the upload stream under
 * the previous frame's skin kernel — measured slower on this runtime, kept for experiments). There is no key that makes a frame
 * emit anything but the deformed mesh: ablation switches exist only in a tools-only build and "dbg" is rejected here.
 * rz_get_tuning also answers "effective_split" / "effective_unroll" / "effective_grid" / "effective_fast" / "effective_out_cap" /
 * "effective_inst_group" / "effective_inst_block" / "effective_fuse_fk" / "effective_overlap" / "pose_resident" /
 * "effective_subsets" / "effective_subset_bones" / "effective_inst_lds" / "effective_fk_kind" / "effective_variant" (the last template
 * argument of the single-mesh frame kernel: 0 everything compiled in, 3 without the fused consumers, 1 / 2 also with the specialised
 * hierarchy solve), "effective_closure_bones" / "effective_closure_rounds" (a device-animated crowd whose next frame solves the
 * hierarchy in the front of the crowd kernel: closure records per vertex run — the longest run's, shorter ones are padded — and the
 * radix-4 doubling rounds over them, 0 .. 3 for a longest chain of 1 / 2-4 / 5-16 / 17-64 bones; both 0 when rz_fk_kernel runs in front) and the counts
 * "verts" / "bones" / "morphs" / "instances" / "sdef_verts" (SDEF vertices the next frame fixes, 0 = no SDEF pass) / "qdef_verts" (likewise for QDEF). Unknown keys return RZ_ERR_INVALID.
 * NOT a pure getter for crowds: an "effective_*" key describes the frame the NEXT rz_deform will launch, and a crowd's plan depends on
 * the per-run bone lists of its launch shape — when the shape, the mesh or the skeleton changed since the last frame the call brings
 * them up to date first, exactly as the next frame would (stream drained, one small kernel, one readback, a captured graph dropped).
 * Poll these keys at setup time or after a frame, not between a shape change and the frame in a latency-critical loop. (An unknown
 * "effective_*" key is refused before any of that work.) */
int rz_set_tuning(rz_ctx *ctx, const char *key, int value);
int rz_get_tuning(rz_ctx *ctx, const char *key, int *value);

/* Setup-time search over launch shapes (like a GEMM library's "find" mode; no reference counterpart — WebGPU hides
 * the dispatch shape, engine.ts:2393-2402). Candidates: the built-in heuristic plan (entry 0) and every distinct plan among morph
 * split {1,2,4,8} x {1,2,4} workgroups per CU (instanced frames: poses per workgroup x workgroups per CU), timed with the
 * CURRENT mesh / morphs / pose on this GPU: `frames` frames per round (0 = 100, at most 1000) after ~0.25 s of untimed frames (clocks), 5 rounds dealt round-robin over
 * the candidates (so clock / thermal drift hits all of them alike), the MEDIAN round of each is its time.
 *   rz_autotune_measure  fills `table` (at most `cap` entries, *count = how many) and changes nothing;
 *   rz_autotune_apply    adopts one entry as the "morph_split" / "grid_cap" / "inst_loop" tuning values;
 *   rz_autotune          = measure + rz_autotune_pick + apply. The heuristic plan is KEPT unless a candidate is clearly faster — median
 *                        >= 2 % lower and its slowest round under the heuristic's fastest round: the landscape is flat near the
 *                        optimum and a search that follows noise returns a different plan on every run.
 * Several GPUs deforming shards of one mesh (one process per GPU) take the element-wise MAX of their tables' `ms` over the
 * ranks, then every rank picks from that one table with rz_autotune_pick and applies the same entry — one plan on all ranks,
 * judged by the slowest GPU, which is what the frame time is (bench.py does this over torch.distributed).
 * Every candidate is a plan the parity tests cover. The result belongs to the workload it was timed on: uploading
 * another mesh or other morph targets, or changing the instance count, returns the three keys to their heuristics, and
 * so does rz_set_tuning(key, 0 / -1). */
typedef struct rz_tune_entry {
    int morph_split, grid_cap, inst_loop;   /* the request (rz_set_tuning values; 0 / 0 / -1 = the heuristics) */
    int eff_split, eff_grid, eff_inst_group;/* what it resolves to on this context */
    int same_as;                            /* index of an earlier entry that resolves to the same launch (its time is shared), or -1 */
    float ms;                               /* median round, ms per frame */
    float ms_min, ms_max;                   /* fastest / slowest round */
} rz_tune_entry;
int rz_autotune_measure(rz_ctx *ctx, uint32_t frames, rz_tune_entry *table, int cap, int *count);
/* index of the entry to adopt under the stability rule above (entry 0 unless some entry's ms < 0.98 x entry 0's and, when the
 * spreads are filled in, its ms_max < entry 0's ms_min; ranks that MAX-reduce `ms` reduce ms_max by MAX and ms_min by MIN) */
int rz_autotune_pick(const rz_tune_entry *table, int count);
int rz_autotune_apply(rz_ctx *ctx, const rz_tune_entry *entry);
int rz_autotune(rz_ctx *ctx, uint32_t frames);

/* Device pointers of the output buffers ([I][Vpad][3] floats each) and the padded vertex count,
 * so a host framework can wrap them without a copy. */
int rz_output_ptrs(rz_ctx *ctx, void **pos, void **nrm, uint32_t *v_padded);

/* ---- multi-GPU: vertex shards + optional all-gather of deformed positions ----
 * One context per GPU / process. rz_comm_unique_id() is called by rank 0 and the 128 bytes are
 * broadcast by the host (IPC, torch.distributed, files ...); every rank then calls
 * rz_comm_init() with the same id. rz_allgather() runs ncclAllGather over xGMI on the
 * context's stream: every rank ends up with the full [v_total_padded][3] position (and, when
 * with_normals != 0, normal) arrays of instance 0. */
int rz_comm_unique_id(char id[128]);
/* Which RCCL this library is bound to (lazily, on the first multi-GPU call): the file it came from, ncclGetVersion(),
 * and whether it is a copy the process had ALREADY loaded (PyTorch ships its own librccl.so with the same soname): the
 * library looks for one with RTLD_NOLOAD first, so that a process never runs two RCCL runtimes side by side. */
int rz_rccl_info(char *path, size_t path_bytes, int *version, int *reused);
/* What the communicator itself says after rz_comm_init / rz_comm_init_all: ncclCommCount and ncclCommUserRank
 * (evidence that RCCL really spans `nranks` ranks — bench.py prints it per rank). */
int rz_comm_info(rz_ctx *ctx, int *comm_count, int *comm_user_rank);
int rz_comm_init(rz_ctx *ctx, int nranks, int rank, const char id[128], uint32_t v_total);
int rz_allgather(rz_ctx *ctx, int with_normals);
int rz_read_gathered(rz_ctx *ctx, uint32_t v0, uint32_t n, float *pos3, float *nrm3);

/* Single-process form (one Node process driving several GPUs, one context each): ctxs[r] is rank r and
 * must hold shard r of rz_shard_range(v_total, n, r). rz_comm_init_all = ncclCommInitAll; rz_allgather_all
 * issues every rank's ncclAllGather inside one ncclGroupStart/End. */
int rz_comm_init_all(rz_ctx **ctxs, int n, uint32_t v_total);
int rz_allgather_all(rz_ctx **ctxs, int n, int with_normals);

/* Peer-direct gather ("peer-direct stores replacing the all-gather"), single-process form.
 * The reference has one consumer of the deformed mesh — the rasteriser behind vs() (engine.ts:245-276) — so only ONE
 * GPU (`root`, an index into ctxs) needs the whole mesh. rz_gather_direct allocates the [n x chunk][3] position and
 * normal arrays on the root's GPU, enables peer access and re-points every context's output at its own slice of
 * them: from then on each rz_deform stores its shard straight into the root's memory over xGMI while it computes —
 * no collective, no second pass over the output, no RCCL. ctxs[r] must hold shard r of rz_shard_range(v_total, n, r);
 * contexts may share a GPU (then no peer mapping is involved). rz_read() on a contributor still returns its shard.
 * rz_gather_fence(root) makes the root's stream wait (hipStreamWaitEvent, nothing blocks on the host) for
 * everything the other contexts have enqueued so far, so a consumer enqueued on the root's stream sees the whole
 * frame; rz_read_gathered(root, ...) fences, synchronises and copies to the host. Uploading a new mesh to a
 * contributor returns that context to its private output buffers; uploading one to the root, or destroying the
 * root, returns all of them. */
int rz_gather_direct(rz_ctx **ctxs, int n, uint32_t v_total, int root);
int rz_gather_fence(rz_ctx *root);

#ifdef __cplusplus
}
#endif
#endif /* REZE_DEFORM_H */
