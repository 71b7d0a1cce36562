// deform_kernels.h — parameter blocks and launchers shared by the kernel files (kernels/*.hip) and the host side (ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "frame_kernel.h"
#include "lds_layout.h"

// rz_prep_kernel: palette = rows 0..2 of world * inverseBind (engine/src/engine.ts:926-928) and the
// ordered list of morphs with a non-zero weight.
struct RzPrepParams {
    const float *world;      // [I][B][16] column-major
    const float *inv_bind;   // [B][16]
    float4 *palette;         // [I][B][3]  row-major 3x4
    const float *morph_w;    // [I][M]
    const float *dense_fold; // [M] 24-bit dense storage: the factor folded into every listed weight (RzDeformParams); null = none
    uint32_t *act_idx;       // [I][Mpad]
    float *act_w;            // [I][Mpad]
    int *act_count;          // [I]
    int B;
    int M;
    int Mpad;
};

// rz_fk_kernel: forward kinematics + palette on the device (engine/src/model.ts:330-420, engine.ts:926-928).
// motion sampling inside rz_fk_kernel: frame-indexed VMD sampling on the device (the GPU twin of host/vmd-sampler.js; the reference has no
// counterpart — its loader drops positions and interpolation bytes, engine/src/vmd-loader.ts:129-140).
struct RzSampleParams {
    const float *frames;          // [I] fractional frame (30 fps) each instance is posed at; nullptr = no sampling
                                  // (the track record of every bone is word 2 of its bone record: RzFkParams::bone_rec)
    const float *key_frame;       // [K] ascending inside a track
    const float4 *key_rot;        // [K]
    const float *key_pos;         // [K][3]
    const uint4 *key_interp;      // [K] first 16 interpolation bytes of each key (nullptr = linear)

    const float *mkey_frame;      // [Km]
    const float *mkey_weight;     // [Km]
    const uint32_t *feed_off;     // [M + 1] per vertex morph: the tracks that feed it ...
    const uint4 *feed_range;      //   ... as (first key, end, bits(first frame), bits(last frame)) into mkey_*: own track first, then group-morph tracks ascending
    const float *feed_ratio;
    float *morph_w;               // [I][M] out
    int M;
    int frames_inline;            // 1: every instance is posed at `frame0` (one character: the frame rides in the kernel arguments)
    float frame0;
};

struct RzFkParams {
    const float4 *local_q;      // [I][B] local rotations (x,y,z,w)
    const float *local_t;       // [I][B][3] local translations (SkeletonRuntime.localTranslations) or nullptr = all zero
    // static data of the solve, ONE block per skeleton (kernels/fk.hip.h): 64-byte bone records
    //   w0: parent (-1 = root) | append parent (-1 = no append rotation) | bits(append ratio) | flags (bit 0: append-move —
    //       the append parent's local translation * ratio is appended too, model.ts:388-393)
    //   w1: bits of the parent-relative bind translation x y z | 0
    //   w2: the motion's track of the bone (first key, end, bits(first frame), bits(last frame)); zeros without a motion
    //   w3: ancestors for the radix-4 doubling rounds 0 and 1 (a1 | a2 << 16, a3, a4 | a8 << 16, a12; 0xffff = above the root)
    // followed by [sample.M] 32-byte vertex-morph records (first feed's key range | first feed, end of feeds, bits(ratio), 0)
    const uint4 *bone_rec;      // [B][4] (+ [M][2])
    const uint2 *anc_more;      // [n_rounds - 2][B] (a1 | a2 << 16, a3) for the doubling rounds beyond the second (hierarchies deeper than 16), or null
    const float *inv_bind;      // [B][16]
    float *world;               // [I][B][16] out
    float4 *palette;            // [I][B][3] out
    int B;
    int n_rounds;               // radix-4 doubling rounds = ceil(log4(depth of the hierarchy)); 0 = roots only
    // physics hand-off (engine.ts:2379-2381, physics.ts:715-751): world matrices that replace the solved ones AFTER the
    // hierarchy solve — children keep the matrices solved from the un-overridden parent, exactly like the reference's
    // in-place boneWorldMatrices.set() (the entry points with the follow stage let them follow it: RzFollowParams). Entries sorted by
    // instance; ovr_off[i]..ovr_off[i+1] are instance i's.
    const int *ovr_off;         // [I + 1] or nullptr
    const int *ovr_bone;        // [n]
    const float *ovr_world;     // [n][16] column-major
    // PMX bone morphs (morph type 2: a weight-scaled translation + rotation offset on a bone's LOCAL pose; the reference's
    // loader skips the section, engine/src/pmx-loader.ts:489-497). Stored per bone; applied after the pose is staged /
    // sampled and before the local matrices are formed:  t += w * t_e ;  q = q * slerp(I, q_e, w)  for its entries in
    // ascending morph order (host twin: host/model.js posedLocals()).
    const uint32_t *bm_off;     // [B + 1] or nullptr = the model has no bone morphs
    const uint32_t *bm_morph;   // [n] morph index of each entry, ascending inside a bone
    const float4 *bm_rot;       // [n] x y z w
    const float4 *bm_tr;        // [n] x y z (w unused)
    const float *bm_w;          // [I][bm_M] morph weights of an uploaded (not sampled) pose
    int bm_M;
    RzSampleParams sample;      // sample.frames != nullptr: local_q / local_t are ignored, the pose is sampled in the kernel
    // FUSED frame of a zero-copy local pose (one character; RzDeformParams: pf_* / st_tag): `local_q` / `local_t` name the pinned slot.
    float4 *copy_q;             // device pose block: workgroup 0 leaves the pose there for the frames that replay it, or null
    float *copy_t;
    const float4 *st_local_q;   // where the previous frame's helper staged this pose if RzDeformParams::st_tag holds st_expect, or null
    const float *st_local_t;
    uint64_t st_expect;
};

// PMX inverse kinematics (rz_upload_ik; kernels/ik.hip.h): the stage the solve runs between the doubling rounds and the override pass.
// A block of its own, an argument of the rz_fk_kernel instantiations with the stage only (RzFkStages below): RzFkParams — embedded in
// the fused kernels' arguments — does not change.
struct RzIkParams {
    const uint4 *chain;         // [n_chains][2], sorted by (stage, IK bone): (goal, first path entry, path length, parent of the path's first bone or -1)
                                //                                            (loops, bits(per-step angle limit), first link, links)
    const uint32_t *path;       // per chain its path, outermost link ... effector, parents first: bone | bit 31 = the bone is a link of the chain
    const float4 *link;         // [links][2] in file order: (min xyz | position on the path), (max xyz | 1 = limited)
    const uint32_t *stage_off;  // [n_stages + 1] chains of each stage: chains of one stage do not read what another one of it writes
    int n_stages;
    int n_chains;
};

// Followers of overridden bones (rz_override_follow; kernels/fk.hip.h: FOLLOW): per instance the bones below an overridden bone, each with
// the entry of its NEAREST overridden ancestor in the override table, ascending by bone. A block of its own like RzIkParams, an argument of the
// rz_fk_kernel instantiations with the stage only, which are launched only while entries exist: RzFkParams — embedded in the fused kernels'
// arguments — does not change, and with the flag off (or nothing to follow) both pointers are null and every frame launches what it launched before.
struct RzFollowParams {
    const int *off;             // [I + 1] or nullptr
    const uint2 *ent;           // [n] (follower bone, index into ovr_bone / ovr_world)
};

// PMX after-physics bones (rz_upload_after_physics; kernels/after.hip: rz_fk_after_kernel; defined by tests/after_ref.py): the listed bones
// are evaluated again behind the override write, level by level, on the world matrices the solve left in memory. Static data built on the
// host (after_table.h). A block of its own, handed to a kernel of its own that is launched only while the list AND a non-empty override
// table are resident: RzFkParams — embedded in the fused kernels' arguments — does not change.
struct RzAfterParams {
    const uint4 *rec;           // [n][3], sorted by (level, bone): (parent, append parent or -1, bits(append ratio), flags) — the bone record's word 0 —
                                //         (bits(bind translation) x y z, the bone), (bits(the append parent's bind translation) x y z, its parent or -1)
    const int *level_off;       // [n_levels + 1] entries of each level
    const int *index;           // [B] entry of a bone, -1 = not listed
    int n;
    int n_levels;
};

// Per-instance switches of the IK chains (rz_set_ik_enabled / rz_upload_ik_keys; kernels/ik.hip.h: SW; defined by tests/ik_switch_ref.py):
// one bit per chain in the DEVICE's chain order (RzIkParams::chain: sorted by stage, so a stage is a contiguous bit range), bit c of word
// c / 32, set = the chain is solved. The host evaluates the switches (it knows every frame and state it hands over) and only the bits
// travel: one character's few words in the kernel arguments, a crowd's in a device array. A block of its own like RzFollowParams, an argument of
// the rz_fk_kernel instantiations with the switches only, which are launched only while at least one bit is clear: RzFkParams and RzIkParams do not change.
constexpr int kRzIkSwInline = 4;
struct RzIkSwitchParams {
    const uint32_t *mask;       // [I][words], or nullptr: one instance, its words are w0 below
    uint32_t w0[kRzIkSwInline];
    int words;                  // words per instance = ceil(n_chains / 32)
};

// Which stages the next hierarchy solve runs: the four blocks above, each the empty one its builder returns (null pointers, n_chains == 0,
// words == 0, n == 0) while its stage is off. The one description rz_launch_fk picks its instantiation from, rz_fk_lds_bytes sizes the
// LDS from and the host asks (plan.cpp: solve_stages). ik / fo / sw are arguments of the solve; af is the launch behind it.
struct RzFkStages {
    RzIkParams ik;
    RzIkSwitchParams sw;
    RzFollowParams fo;
    RzAfterParams af;
    bool plain() const { return !ik.n_chains && !sw.words && !fo.off && !af.n; }       // no stage: what the fused kernels' embedded solve can stand in for
};

// rz_deform_kernel: fused morph + 4-bone LBS (engine/src/engine.ts:253-272).
struct RzDeformParams {
    const float *geom;          // 6 planes of Vp floats: x y z nx ny nz
    const uint32_t *joints01;   // [Vp] j0 | j1 << 16
    const uint32_t *joints23;   // [Vp] j2 | j3 << 16
    const uint32_t *weights;    // [Vp] 4 x unorm8
    float4 *palette;            // [I][B][3]  (read by !FAST, written once per frame by FAST)
    const float *world;         // [I][B][16] (FAST)
    const float *inv_bind;      // [B][16]    (FAST)
    const float *dense;         // [M][3][Vp] planes (MODE 1): fp32, or 24-bit integers, 3 * Vp bytes a plane (dense_fold != null)
    const float *dense_fold;    // [M] 24-bit storage: s_m * 2^-8 per morph, folded into the weights of the active list; null = fp32 planes
    const uint32_t *act_idx;    // [I][Mpad]
    const float *act_w;         // [I][Mpad]
    const int *act_count;       // [I]
    const float *morph_w;       // [I][M]   (MODE 2)
    // Zero-copy first frame (single character): `world` / `morph_w` point into PINNED HOST memory (the staging slot the
    // host has just written) and workgroup 0 of the FAST kernel leaves a copy in device memory for the frames that replay
    // this pose. null = the pose is already resident and `world` / `morph_w` are device pointers.
    float *world_copy;          // [B][16] device destination, or null
    float *morph_w_copy;        // [M]     device destination (MODE 2), or null
    // Pose PREFETCH of zero-copy frames (FAST, one character). A frame whose pose still sits in its pinned slot
    // pays one PCIe round trip (2-3 us) that a 16 us shard frame cannot hide. So the frame of pose u also carries ONE helper
    // workgroup (blockIdx.x == 0; the workers shift by one) that looks at the ring slot the NEXT upload will use: if the host
    // has already written pose u + 1 there — it runs several frames ahead of the GPU in a per-frame loop — the helper copies
    // it into the device pose block that upload will name and tags it with the upload's sequence number. The frame of pose
    // u + 1 checks the tag (one scalar load): staged -> it reads HBM like a resident pose; not staged (the host was late, the
    // slot was not written yet, another pose kind came) -> it reads the pinned slot exactly as before. No event, no wait,
    // nothing on the host; a miss costs nothing but the helper's slot.
    const float *pf_src;            // pinned slot of the next upload (device-mapped), or null = no helper in this launch
    const uint64_t *pf_src_seq;     // its header: the sequence number of the pose it holds, written by the host AFTER the pose
    float *pf_dst;                  // device pose block the next upload will name ([world | weights], the slot's layout)
    uint64_t *pf_tag;               // device: sequence number of the pose staged in pf_dst
    uint64_t pf_expect;             // header value of the completely written next pose
    uint32_t pf_bytes;              // bytes to stage (multiple of 16)
    const uint64_t *st_tag;         // THIS frame's pose: staged in the device block when *st_tag == st_expect, else in the pinned slot
    uint64_t st_expect;
    const float *st_world;          // [B][16] staged copy
    const float *st_morph_w;        // [M]     staged copy (MODE 2; fused-hierarchy frames: every mode)
    // FUSED single-character frame (fk_on): every workgroup of the (!FAST) kernel first solves the bone hierarchy itself —
    // motion sampling included when the pose is sampled — straight into its LDS palette, and compacts the morph weights
    // into its LDS list: no rz_fk_kernel, no rz_prep_kernel, ONE launch per device-animated frame. Workgroup 0 also
    // leaves world matrices, palette and sampled weights in memory (rz_read_world / rz_read_palette).
    RzFkParams fk;
    int fk_on;
    int fk_kind;                // 0: the generic solve; 1 / 2: the kernel variant specialised for a PLAIN uploaded / sampled pose (kernels/fk.hip.h: fk_solve<FUSED, KIND>)
    const uint32_t *sp_ptr;     // [Vp+1]   (MODE 2) per-vertex CSR row pointers
    const float4 *sp_entries;   // [E]      (dx,dy,dz,bits(morph))
    float *out_pos;             // [I][Vp][3]
    float *out_nrm;             // [I][Vp][3]
    const float *edge;          // [Vp] per-vertex outline edge size, or null (hull epilogue off)
    float *out_hull;            // [I][Vp][3] worldPos + worldNormal * edge * 0.01   (engine.ts:458-461)
    uint32_t *aabb;             // [I][2 slots][6] order-preserving keys of min xyz / max xyz, or null
    int aabb_slot;              // slot this launch accumulates into (the other one is re-armed)
    uint32_t Vp;                // padded vertex count (multiple of 1024)
    uint32_t n_verts;           // real vertex count V
    uint32_t n_quads;           // ceil(V / 4)
    uint32_t quads_per_wave;    // contiguous run owned by each wave of the grid (multiple of 8)
    uint32_t out_cap;           // vertices buffered in LDS per wave before a 16-B/lane flush (0 = store directly)
    uint32_t sp_cap;            // MODE 2: CSR entries a wave stages in LDS at a time (multiple of 64 = whole 1 KiB bursts)
#ifdef RZ_ABLATE
    int dbg;                    // ablation switch — tools-only build (see RZ_DBG in deform_kernels.hip); absent from the product
    unsigned long long *tl;     // tools-only build, dbg = 100: per-wave timeline, 8 x u64 per wave (RZ_STAMP in deform_kernels.hip)
#endif
    int inst_order;             // instanced skin: 0 = an XCD takes one vertex run of every pose group, 1 = every vertex run of its pose groups
    // Instanced skin, BONE-SUBSET form: a vertex run only references a few of the skeleton's bones (PMX meshes are bone-local),
    // so its workgroups stage just those — rz_run_subsets_kernel lists, per vertex run, the sorted set of bones its vertices
    // name and rewrites the joints as slots of that list. null = the whole palette is staged and joints01 / joints23 are used.
    const uint32_t *rj01;       // [Vp] slot(j0) | slot(j1) << 16   (joints already clamped to B - 1)
    const uint32_t *rj23;       // [Vp] slot(j2) | slot(j3) << 16
    const uint16_t *sub_list;   // [runs][sub_stride] ascending bone indices of each run's subset
    const uint32_t *sub_count;  // [runs]
    int sub_stride;
    int sub_max;                // longest list of the launch shape: every list is padded to it with bone 0
    int dma;                    // FAST: stage raw matrices by LDS-DMA (else plain loads after the first morph phase)
    int B;
    int M;
    int Mpad;
};

// Active-morph list of a single-instance frame, passed BY VALUE in the kernel arguments (FAST path):
// compacted on the host by rz_set_pose, so the frame needs no prep kernel and no dependent load
// before the morph stream starts.
constexpr int kKargMorphs = 128;
constexpr int kKargPad = 8;          // the remainder loop may peek up to S-1 entries past `count`
struct RzMorphList {
    int count;
    uint32_t idx[kKargMorphs + kKargPad];
    float w[kKargMorphs + kKargPad];
};

// rz_sdef_kernel (kernels/sdef.hip): SDEF skinning of the vertices listed by rz_upload_sdef, a pass of its own behind the frame kernel.
// One lane per (table entry, instance); it reads what the frame kernel read and overwrites that kernel's output for the listed vertices.
struct RzSdefParams {
    const uint32_t *tab;        // [10][n] SoA planes, 40 B per entry: vertex index (ascending, < V) | C xyz | R0 xyz | R1 xyz
    const float *geom;          // 6 planes of Vp floats
    const uint32_t *joints01;   // [Vp] j0 | j1 << 16 (slots 2 / 3 of an SDEF vertex are ignored)
    const uint32_t *weights;    // [Vp] 4 x unorm8
    const float4 *palette;      // [I][B][3] this frame's palette rows
    const float *dense;         // [M][3][Vp] (mode 1)
    const float *dense_fold;    // [M] or null: as in RzDeformParams
    const uint32_t *sp_ptr;     // [Vp + 1]   (mode 2)
    const float4 *sp_entries;
    const float *morph_w;       // [I][M] this frame's weights (sparse targets; dense with wsrc 2): the device copy the frame read or left
    const uint32_t *act_idx;    // [I][Mpad] the ring slot's ordered active list, written by rz_prep_kernel in front of the frame (wsrc 1)
    const float *act_w;         // [I][Mpad]
    const int *act_count;       // [I]
    float *out_pos, *out_nrm;   // [I][Vp][3] where the frame kernel wrote (its own buffers or the gathered ones)
    const float *edge;          // [Vp] or null: also the outline hull
    float *out_hull;
    uint32_t *aabb;             // [I][2][6] or null: extend slot `aabb_slot`, the one the frame kernel accumulated into
    uint32_t n;                 // entries
    int mode, M, Mpad;          // morph mode of the frame (0 when it has no weights to apply)
    int wsrc;                   // mode 1: 0 = the one-launch frame's kernel-argument list (RzMorphList), 1 = act_*, 2 = morph_w compacted in the pass
    int aabb_slot;
    uint32_t Vp;
    int B;
};                              // (no padding: frame_signature() hashes the struct)
struct RzMorphList;
hipError_t rz_launch_sdef(const RzSdefParams &p, const RzMorphList &ml, uint32_t instances, hipStream_t st);

// rz_qdef_kernel (kernels/qdef.hip): dual-quaternion skinning of the vertices listed by rz_upload_qdef, the same kind of pass. The frame
// fields carry the names they have in RzSdefParams (kernels/pass_parts.hip.h reads either struct).
struct RzQdefParams {
    const uint32_t *tab;        // [n] vertex indices (ascending, < V)
    const float *geom;          // 6 planes of Vp floats
    const uint32_t *joints01;   // [Vp] j0 | j1 << 16
    const uint32_t *joints23;   // [Vp] j2 | j3 << 16
    const uint32_t *weights;    // [Vp] 4 x unorm8
    const float4 *palette;      // [I][B][3] this frame's palette rows
    const float *dense;
    const float *dense_fold;
    const uint32_t *sp_ptr;
    const float4 *sp_entries;
    const float *morph_w;
    const uint32_t *act_idx;
    const float *act_w;
    const int *act_count;
    float *out_pos, *out_nrm;
    const float *edge;
    float *out_hull;
    uint32_t *aabb;
    uint32_t n;
    int mode, M, Mpad;
    int wsrc;
    int aabb_slot;
    uint32_t Vp;
    int B;
    int chunks;                 // 256-vertex chunks of the table one workgroup takes behind one conversion of the skeleton (>= 1)
    int pad_;
};                              // (no padding: frame_signature() hashes the struct)
hipError_t rz_launch_qdef(const RzQdefParams &p, const RzMorphList &ml, uint32_t instances, hipStream_t st);

// rz_motion_kernel<P> (kernels/motion.hip): the local pose of every instance from a library of resident motions, in front of the frame. One
// entry, instantiated for the two parameter blocks below: RzMotionParams, the cross-fade alone (rz_upload_motions / rz_set_pose_blended),
// and RzLayerParams, the cross-fade with layers on top. A kernel of its own: the frame kernels and rz_fk_kernel see a resident local pose.
struct RzMotionState {          // = rz_motion_state of the C ABI (pose.cpp asserts the layout)
    uint32_t clip_a; float frame_a;
    uint32_t clip_b; float frame_b;     // clip_b = kRzNoClip: there is no second clip
    float blend;                        // 0 = all of clip_a ... 1 = all of clip_b
};
constexpr uint32_t kRzNoClip = 0xffffffffu;
struct RzMotionParams {
    const RzMotionState *states;    // [I] on the device, or null: one character, the state rides in the kernel arguments (state0)
    RzMotionState state0;
    const uint4 *bone_rec;          // [n_clips][B] track of each bone in each clip: word 2 of the hierarchy's bone record (first key, end, bits(first
                                    //              frame), bits(last frame)), key indices absolute in the concatenated key arrays
    const uint32_t *feed_off;       // [n_clips][M + 1] per clip and vertex morph: its feeds in the concatenated feed arrays
    RzSampleParams sample;          // the concatenated keys / morph keys / feeds of all clips (frames, morph_w, M unused; feed_off = the array above)
    float4 *local_q;                // [I][B] out: the local-pose part of a pose block ...
    float *local_t;                 // [I][B][3]
    float *morph_w;                 // [I][M]
    int B;
    int M;
};

// The cross-fade above, then up to kRzMaxLayers layers per instance — one clip each at its own frame with a weight, an optional bone / morph
// mask and a mode (rz_upload_motion_masks / rz_set_pose_layered). With no live layer it writes what the instantiation without layers
// writes, bit for bit, where that writes it; rz_set_pose_blended keeps launching the one without.
constexpr int kRzMaxLayers = 4;
constexpr uint32_t kRzNoMask = 0xffffffffu;
struct RzMotionLayer {          // = rz_motion_layer of the C ABI (pose.cpp asserts the layout)
    uint32_t clip; float frame;         // clip = kRzNoClip or weight = 0: the layer is skipped, nothing else of it is read
    float weight;
    uint32_t mask;                      // kRzNoMask: every bone and morph
    uint32_t mode;                      // 0 override, 1 additive
};
struct RzLayerParams {
    RzMotionParams m;               // the library, the base states ([I] or state0) and the output, as the instantiation without layers takes them
    const RzMotionLayer *layers;    // [I][n_layers] on the device, or null: one character, the layers ride in the kernel arguments (layers0)
    RzMotionLayer layers0[kRzMaxLayers];
    int n_layers;
    const uint32_t *bone_bits;      // [n_masks][bone_words] bit sets: bit (b & 31) of word b >> 5 = the mask includes bone b
    const uint32_t *morph_bits;     // [n_masks][morph_words], or null: every mask includes every morph
    int bone_words, morph_words;
};
hipError_t rz_launch_motion(const RzMotionParams &p, uint32_t instances, hipStream_t st);      // rz_motion_kernel<RzMotionParams>
hipError_t rz_launch_motion(const RzLayerParams &p, uint32_t instances, hipStream_t st);       // rz_motion_kernel<RzLayerParams>

// rz_physics_kernel (kernels/physics.hip): rigid bodies and joints of every instance advanced by `substeps` fixed steps, one workgroup per
// instance, in front of the frame (rz_upload_physics / rz_physics_step). It reads the world matrices the hierarchy solve left in memory and
// writes the solve's override table; the frame kernels see overrides, nothing else.
struct RzPhysicsParams {
    const float4 *body;         // [nb][4]  offset position | inverse mass (0 = follows its bone);  offset rotation;  inverse inertia (body frame) |
                                //          (1 - linear damping)^h;  (1 - angular damping)^h | bits(bone, -1 = none) | bits(override slot, -1 = none) | 0
    const float4 *joint;        // [nj][8]  in solve order (colour, file index): anchor in A | bits(body A);  anchor in B | bits(body B);  joint frame in A;
                                //          joint frame in B;  position min | alpha~ x;  position max | alpha~ y;  rotation min | alpha~ z;  rotation max | bits(spring axes)
    const int *colour_off;      // [ncol + 1] joints of colour k: colour_off[k] .. colour_off[k + 1]
    float4 *state;              // [I][nb][4] x | q | v | w
    const float *world;         // [I][B][16] the un-overridden hierarchy solve (after IK)
    float *ovr_world;           // [I][nd][16] out: the override table's matrices
    int nb, nj, ncol, nd, B;
    int iterations, substeps;
    int reset;                  // every body (not only the following ones) is placed on its bone first
    int block;                  // 64 or 256 lanes
    float h, gx, gy, gz;
    // the contact stage (rz_physics_contacts; contact_table.h derives the lists): null / 0 unless contacts is 1, 2 or 3
    const float4 *c_shape;      // [nb]     radius | half length of the segment (0: a sphere) | friction | bits(1 = takes part, 4 = a box)
    const int *c_follow_off;    // [nb + 1] a dynamic body's following partners: c_follow_idx[c_follow_off[b] .. c_follow_off[b + 1]), ascending
    const int *c_follow_idx;
    const int2 *c_pair;         // [pairs]  dynamic pairs (a < b) in solve order (colour, a, b)
    const int *c_colour_off;    // [c_ncol + 1]
    int c_ncol;
    int contacts;               // the CONTACT instantiations: 1 spheres and capsules | 2 boxes take part as well | 3 and box against box
    const float4 *c_box;        // [nb]     contacts = 2 and 3 only: a box's half extents | 0, zeros for every other body (behind the rest:
                                //          the arguments of the other instantiations stay where they were)
    // the linear springs (rz_physics_springs; physics_table.h derives the records): null = off, the LSPRING instantiations otherwise
    const float4 *lin;          // [nj]     in solve order: alpha~ x | alpha~ y | alpha~ z | bits(axes with spring_position > 0) (behind the rest, as c_box is)
};
// (its LDS: physics_table.h, rzphys::lds_bytes and kLdsLimit)
hipError_t rz_launch_physics(const RzPhysicsParams &p, uint32_t instances, hipStream_t st, bool aligned = false);   // aligned: the ALIGN instantiations (rz_physics_aligned)

// Every kernel's dynamic LDS is laid out in lds_layout.h (rzlds); what follows maps parameter blocks onto its scalars.
// the pose's morph weights the solve keeps in LDS for the bone morphs (rzlds::solve: n_weights): none without bone morphs
__host__ __device__ inline int rz_fk_mw_count(const RzFkParams &p)
{
    if (!p.bm_off) return 0;
    const int m = p.bm_M > p.sample.M ? p.bm_M : p.sample.M;
    return m > 1 ? m : 1;
}
// the generic frame's layout for a variant: the lists are in LDS for sparse targets and for a dense frame behind rz_prep_kernel / the fused
// solve; a wave step is 256 / S vertices of 3 planes (9 with the rest geometry through LDS); pieces are staged for sparse targets only
inline rzlds::Frame rz_deform_layout(int B, int M, int Mpad, uint32_t out_cap, uint32_t sp_cap, bool fused, const RzVariant &v)
{
    return rzlds::frame(B, (v.mode == 2 || (!v.fast && v.mode == 1)) ? Mpad : 0, v.geo ? 9 : 3, 256 / v.S, out_cap, v.mode == 2 ? sp_cap : 0, fused, M);
}

hipError_t rz_launch_prep(const RzPrepParams &p, uint32_t instances, hipStream_t st);
// The hierarchy solve (kernels/front.hip: rz_fk_kernel<Stage...>) with the stages `s` lists: one launcher picks the instantiation, whose
// kernel arguments carry the blocks of the stages that are on and nothing else.
hipError_t rz_launch_fk(const RzFkParams &p, const RzFkStages &s, uint32_t instances, hipStream_t st);
inline size_t rz_fk_lds_bytes(const RzFkParams &p, const RzFkStages &s) { return rzlds::solve(p.B, s.ik.n_chains != 0, rz_fk_mw_count(p)).total(); }      // its dynamic LDS
// the after-physics stage (s.af) behind the solve, on the same stream (kernels/after.hip: rz_fk_after_kernel): reads the world matrices
// the solve left in memory and writes the listed bones' world matrices and palette rows again
hipError_t rz_launch_fk_after(const RzFkParams &p, const RzAfterParams &a, uint32_t instances, hipStream_t st);
inline size_t rz_deform_lds_bytes(const RzDeformParams &p, const RzVariant &v) { return rz_deform_layout(p.B, p.M, p.Mpad, p.out_cap, p.sp_cap, p.fk_on != 0, v).total(); }
// Crowd frame with the hierarchy solved in the skin kernel's front (kernels/crowd.hip: rz_skin_instances_fk_kernel): per vertex run the
// closure of its named bones under "parent of", one 80-byte record per closure slot (plan.cpp: ensure_subfk)
struct RzSubFk {
    const uint32_t *count;      // [runs] closure slots of each run
    const uint4 *rec;           // [runs][stride][5]
    uint32_t stride;            // closure slots of the largest run
    uint32_t rounds;            // radix-4 doubling rounds the deepest closure needs (<= 3)
};
// The launch shape of a frame's kernel: grid (grid_x, n_inst) for one mesh; for a crowd grid_x vertex runs of verts_per_wg vertices by
// ceil(n_inst / G) groups (the register form: ranges) of G poses. lds = the dynamic LDS of the launch.
struct RzLaunchShape { int G, n_inst; uint32_t verts_per_wg, grid_x; size_t lds; };
// The frame's kernel (frame_kernel.h), ONE entry: the kernel file of k's family picks the instantiation k names and launches it, or refuses
// (hipErrorInvalidValue) a record this build does not carry. ml: the one-launch dense frame's list; f: the crowd fk front's records.
hipError_t rz_launch_frame(const RzFrameKernel &k, const RzDeformParams &p, const RzMorphList &ml, const RzSubFk &f, const RzLaunchShape &s, hipStream_t st);
// behind it; the MORPH half of crowd.hip (crowd_morph.hip) also walks the context's sparse CSR per pose, weights p.morph_w [I][M] staged in LDS
hipError_t rz_launch_deform_dense(const RzFrameKernel &k, const RzDeformParams &p, const RzMorphList &ml, const RzLaunchShape &s, hipStream_t st);
hipError_t rz_launch_deform_small(const RzFrameKernel &k, const RzDeformParams &p, const RzLaunchShape &s, hipStream_t st);
hipError_t rz_launch_crowd(const RzFrameKernel &k, const RzDeformParams &p, const RzSubFk &f, const RzLaunchShape &s, hipStream_t st);
hipError_t rz_launch_crowd_morph(const RzFrameKernel &k, const RzDeformParams &p, const RzSubFk &f, const RzLaunchShape &s, hipStream_t st);
// per vertex run of `per` vertices: the ascending list of bones its vertices name + the joints rewritten as slots of it
hipError_t rz_launch_run_subsets(const uint32_t *j01, const uint32_t *j23, uint32_t v_lim, uint32_t per, uint32_t runs, uint32_t B,
                                 uint16_t *list, uint32_t *count, uint32_t *rj01, uint32_t *rj23, hipStream_t st);
// a crowd's per-frame pose pulled out of a pinned, device-mapped slot (kernels/front.hip: rz_pull_pose_kernel)
hipError_t rz_launch_pull_pose(const void *src, void *dst, uint32_t bones, size_t raw_bytes, hipStream_t st);
uint32_t rz_quads_per_tile(int S);
bool rz_has_all_variants();      // false in the product: only the variants a plan can select by default are compiled in
#ifdef RZ_ALL_VARIANTS
hipError_t rz_launch_gate(const uint32_t *flag, hipStream_t st);     // test hook (tools-only build): the stream waits until *flag != 0
#endif
hipError_t rz_launch_deinterleave(const float *src, int stride, int offset, uint32_t n, float *px, float *py,
                                  float *pz, hipStream_t st);
hipError_t rz_launch_pack_skinning(const uint16_t *joints4, const uint8_t *weights4, uint32_t n, uint32_t *j01,
                                   uint32_t *j23, uint32_t *wq, hipStream_t st);
