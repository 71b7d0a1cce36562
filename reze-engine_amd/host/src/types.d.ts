/*
 * types.d.ts — the data shapes the host sources (host/src/*.ts) annotate with. Declarations only: nothing here reaches the shipped
 * JavaScript (tools/ts_erase.py drops `import type` lines with every other annotation). The shapes are the reference's
 * (engine/src/model.ts:6-68, vmd-loader.ts:4-24) plus what this build adds: morph sets, the flattened motion of the device sampler and
 * the raw N-API addon (csrc/napi_addon.c over include/reze_deform.h).
 */
import type { Mat4, Quat, Vec3 } from './math'

export type NumArray = Float32Array | number[]
export type Quad = [number, number, number, number]
export type Triple = [number, number, number]

/** model.ts:24-34 */
export interface Bone {
  name: string
  parentIndex: number
  bindTranslation: Triple
  children: number[]
  appendParentIndex?: number
  appendRatio?: number
  appendRotate?: boolean
  appendMove?: boolean
  /** PMX IK block (flag 0x0020): this bone is the goal. Links run from the effector outwards; limits are Euler angles in radians as stored. */
  ik?: IKBlock
  /** PMX flag 0x1000, "deform after physics": present (true) only on bones that carry it (Model.afterPhysicsOrder, Engine { afterPhysics }) */
  afterPhysics?: boolean
  /** the PMX transform order ("deform layer"): present only when it is not 0 */
  transformLevel?: number
}
export interface IKLink { bone: number; min?: Triple; max?: Triple }
export interface IKBlock { effector: number; loops: number; limitAngle: number; links: IKLink[] }
export interface IKChain extends IKBlock { goal: number }
/** model.ts:36-45 */
export interface Skeleton { bones: Bone[]; inverseBindMatrices: Float32Array }
export interface Skinning { joints: Uint16Array; weights: Uint8Array }
// SDEF vertices (PMX weight type 3) of a model: ascending vertex indices and their C / R0 / R1 ([n][3], model space); empty without SDEF
export interface SdefTable { index: Uint32Array; c: Float32Array; r0: Float32Array; r1: Float32Array }
/** model.ts:52-59 */
export interface SkeletonRuntime {
  nameIndex: Record<string, number>
  localRotations: Float32Array
  localTranslations: Float32Array
  worldMatrices: Float32Array
  computedBones: boolean[]
}
/** model.ts:61-68 */
export interface RotTweenState {
  active: Uint8Array
  startQuat: Float32Array
  targetQuat: Float32Array
  startTimeMs: Float32Array
  durationMs: Float32Array
}
/** PMX bone morphs (type 2) and UV morphs (type 3), flattened by the loader; ascending morph index */
export interface BoneMorphEntries { morph: Uint32Array; bone: Uint32Array; translation: Float32Array; rotation: Float32Array }
export interface UvMorphEntries { morph: Uint32Array; vertex: Uint32Array; delta: Float32Array }
/** What PmxLoader.morphs() returns and Model keeps: vertex morphs as CSR over morphs (offsets / vertexIndex / deltas), group morphs as lists */
export interface MorphSet {
  names: string[]
  types: Uint8Array
  panels: Uint8Array
  groups: Array<Array<[number, number]> | null>
  offsets: Uint32Array
  vertexIndex: Uint32Array
  deltas: Float32Array
  boneEntries: BoneMorphEntries
  uvEntries: UvMorphEntries
}
export interface PosedLocals { rot: Float32Array; tra: Float32Array; moved: boolean }
export interface Material { name: string; edgeFlag: number; edgeSize: number; vertexCount: number; [key: string]: unknown }
export interface Texture { path: string; name: string }

/** vmd-loader.ts:4-24 (+ position and interpolation, which the reference drops, and the morph block it does not read) */
export interface BoneFrame { boneName: string; frame: number; rotation: Quat; position: Vec3; interpolation: Uint8Array }
export interface MorphFrame { morphName: string; frame: number; time: number; weight: number }
export interface VMDKeyFrame { time: number; boneFrames: BoneFrame[] }
/** one key of a VMD's show / IK block: the chains it names are switched; a chain it does not name keeps its state */
export interface IKFrame { frame: number; time: number; show: boolean; ik: Array<{ name: string; enabled: boolean }> }
export type VMDKeyFrames = VMDKeyFrame[] & { morphFrames?: MorphFrame[]; ikFrames?: IKFrame[] }
export interface BoneSample { rotation: Quad; position: Triple }
/** VMDSampler.flatten(): the arrays of rz_animation (include/reze_deform.h) */
export interface FlatMotion {
  trackBone: Int32Array; keyOff: Uint32Array; keyFrame: Float32Array; keyRot: Float32Array; keyPos: Float32Array; keyInterp: Uint8Array
  mkeyOff?: Uint32Array; mkeyFrame?: Float32Array; mkeyWeight?: Float32Array
  feedOff?: Uint32Array; feedTrack?: Int32Array; feedRatio?: Float32Array
  /** the motion's IK on / off keys for the model's chains (rz_ik_keys): frames [n] non-descending, enabled [n][chains] */
  ikKeys?: { frames: Float32Array; enabled: Uint8Array }
}

/** Engine.seekMotions(): instance i is posed from motion `a` at frameA, cross-faded by `blend` (0 .. 1) into motion `b` at frameB */
export interface MotionState { a: string; frameA: number; b?: string | null; frameB?: number; blend?: number; layers?: MotionLayer[] }
/** one layer of a MotionState: motion `motion` at `frame`, applied with `weight` (default 1) where the mask `mask` (Engine.setMotionMask; none: everywhere) includes the bone or morph and the motion keys it — override (slerp / lerp towards it) or `additive` */
export interface MotionLayer { motion: string; frame: number; weight?: number; mask?: string | null; additive?: boolean }
/** Engine.setMotionMask(): the bones a layer may act on (`withDescendants`: and every bone below them) and the morphs (names, 'all' — the default — or 'none') */
export interface MotionMaskSpec { bones: string[]; withDescendants?: boolean; morphs?: string[] | 'all' | 'none' }
/** Model.applyLayeredFrame(): a mask resolved for one model, one byte per bone and per morph (morphs null: all) */
export interface HostMask { bones: Uint8Array; morphs: Uint8Array | null }
export interface LayeredBase { a: VMDSamplerLike; frameA: number; b?: VMDSamplerLike | null; frameB?: number; blend?: number }
export interface HostLayer { sampler: VMDSamplerLike | null; frame: number; weight?: number; mask?: string | null; additive?: boolean }
/** what Model.applyLayeredFrame needs of a VMDSampler */
export interface VMDSamplerLike {
  boneNames(): string[]; morphNames(): string[]
  sampleBone(name: string, frame: number): { rotation: number[]; position: number[] } | null
  sampleMorph(name: string, frame: number): number | null
  ikStateAt?(frame: number): Map<string, boolean>
}

/** opaque rz_ctx handle of the addon */
export type DeformContext = unknown
export interface Timing { frameMs: number; deformKernelMs: number; prepKernelMs: number; vertsPerFrame: number; algorithmicBytesPerFrame: number; frames: number }
/** reze_deform.node — every function throws an Error carrying rz_last_error() on failure (csrc/napi_addon.c) */
export interface DeformAddon {
  abiVersion(): number
  deviceCount(): number
  deviceNumaNode(device: number): number
  create(device: number): DeformContext
  destroy(ctx: DeformContext): void
  fork(ctx: DeformContext): DeformContext
  shardRange(vTotal: number, nranks: number, rank: number): [number, number]
  instanceRange(instances: number, nranks: number, rank: number): [number, number]
  gatherChunk(vTotal: number, nranks: number): number
  uploadMesh(ctx: DeformContext, interleaved8: Float32Array, joints4: Uint16Array, weights4: Uint8Array): void
  uploadSkeleton(ctx: DeformContext, inverseBind: Float32Array): void
  uploadSkeletonTopology(ctx: DeformContext, parents: Int32Array, bind: Float32Array, appendParent: Int32Array | null, appendRatio: Float32Array | null, appendMove: Uint8Array | null): void
  uploadMorphsDense(ctx: DeformContext, morphs: number, deltas: Float32Array | null): void
  uploadMorphsSparse(ctx: DeformContext, offsets: Uint32Array, vertexIndex: Uint32Array, deltas: Float32Array): void
  uploadBoneMorphs(ctx: DeformContext, morph: Uint32Array | null, bone: Uint32Array | null, translation3: Float32Array | null, rotation4: Float32Array | null): void
  uploadAnimation(ctx: DeformContext, motion: FlatMotion): void
  uploadMotions(ctx: DeformContext, motions: FlatMotion[]): void
  uploadEdgeScale(ctx: DeformContext, edge: Float32Array | null): void
  uploadIK(ctx: DeformContext, goal: Uint32Array | null, effector: Uint32Array | null, loops: Uint32Array | null, limitAngle: Float32Array | null, linkOff: Uint32Array | null, linkBone: Uint32Array | null, linkLimited: Uint8Array | null, linkMin3: Float32Array | null, linkMax3: Float32Array | null): void
  uploadSdef(ctx: DeformContext, index: Uint32Array | null, c3: Float32Array | null, r0_3: Float32Array | null, r1_3: Float32Array | null): void
  uploadQdef(ctx: DeformContext, index: Uint32Array | null): void
  uploadPhysics(ctx: DeformContext, tables: PhysicsTables | null, options?: { gravity?: Float32Array; h?: number; iterations?: number } | null): void
  physicsStep(ctx: DeformContext, substeps: number): void
  physicsReset(ctx: DeformContext): void
  physicsContacts(ctx: DeformContext, on: 0 | 1 | 2 | 3): void
  physicsSprings(ctx: DeformContext, on: 0 | 1): void
  physicsAligned(ctx: DeformContext, on: 0 | 1): void
  overrideFollow(ctx: DeformContext, on: 0 | 1): void
  uploadAfterPhysics(ctx: DeformContext, bones: Uint32Array): void
  uploadIKKeys(ctx: DeformContext, clip: number | null, frames: Float32Array | null, enabled?: Uint8Array | null): void
  setIKEnabled(ctx: DeformContext, mask: Uint8Array | null): void
  readIKEnabled(ctx: DeformContext): Uint8Array
  readPhysics(ctx: DeformContext, instance: number, state13: Float32Array): void
  enableAabb(ctx: DeformContext, on: boolean): void
  setInstances(ctx: DeformContext, count: number): void
  setPose(ctx: DeformContext, world: Float32Array, morphWeights: Float32Array | null): void
  setPoseLocal(ctx: DeformContext, localRotations: Float32Array, morphWeights: Float32Array | null, localTranslations?: Float32Array | null): void
  setPoseSampled(ctx: DeformContext, frames: Float32Array): void
  /** 20 bytes per instance: clipA u32 | frameA f32 | clipB u32 (0xffffffff = none) | frameB f32 | blend f32, little-endian */
  setPoseBlended(ctx: DeformContext, states: ArrayBuffer): void
  /** n masks of one byte per bone and, optionally, per morph (non-zero = included); n = 0 removes them (rz_upload_motion_masks) */
  uploadMotionMasks(ctx: DeformContext, n: number, bones: Uint8Array | null, morphs: Uint8Array | null): void
  /** setPoseBlended's states and nLayers x 20 bytes per instance: clip u32 (0xffffffff = none) | frame f32 | weight f32 | mask u32 (0xffffffff = none) | mode u32 (0 override, 1 additive), little-endian (rz_set_pose_layered) */
  setPoseLayered(ctx: DeformContext, states: ArrayBuffer, nLayers: number, layers: ArrayBuffer): void
  mapPose(ctx: DeformContext, layout?: 0 | 1): { matrices: Float32Array; morphWeights: Float32Array | null }
  commitPose(ctx: DeformContext): void
  overrideWorld(ctx: DeformContext, bones: Uint32Array, world16: Float32Array, instances: Uint32Array | null): void
  deform(ctx: DeformContext): void
  deformN(ctx: DeformContext, frames: number): void
  deformPair(ctx: DeformContext, fork: DeformContext, frames: number): void
  sync(ctx: DeformContext): void
  read(ctx: DeformContext, instance: number, v0: number, n: number, positions: Float32Array | null, normals: Float32Array | null): void
  readHull(ctx: DeformContext, instance: number, v0: number, n: number, hull: Float32Array): void
  readAabb(ctx: DeformContext, instance: number): Float32Array
  readWorld(ctx: DeformContext, instance: number, world16: Float32Array): void
  readPalette(ctx: DeformContext, instance: number, rows: Float32Array): void
  readGathered(ctx: DeformContext, v0: number, n: number, positions: Float32Array | null, normals: Float32Array | null): void
  timeFrames(ctx: DeformContext, frames: number): Timing
  timeSpan(ctx: DeformContext, fork: DeformContext | null, frames: number, lead?: number): number
  autotune(ctx: DeformContext, frames?: number): void
  setTuning(ctx: DeformContext, key: string, value: number): void
  getTuning(ctx: DeformContext, key: string): number
  commInitAll(ctxs: DeformContext[], vTotal: number): void
  allgatherAll(ctxs: DeformContext[], withNormals: boolean): void
  gatherDirect(ctxs: DeformContext[], vTotal: number, root: number): void
  gatherFence(root: DeformContext): void
}

// PMX rigid bodies and joints as the loader reads them (pmx-loader.ts: rigidbodies(), joints())
export interface Rigidbody {
  name: string; englishName: string; boneIndex: number; group: number; collisionMask: number; shape: number
  size: Vec3; shapePosition: Vec3; shapeRotation: Vec3
  mass: number; linearDamping: number; angularDamping: number; restitution: number; friction: number; type: number
  bodyOffsetMatrixInverse: Mat4
}
export interface Joint {
  name: string; englishName: string; type: number; rigidbodyIndexA: number; rigidbodyIndexB: number
  position: Vec3; rotation: Vec3; positionMin: Vec3; positionMax: Vec3; rotationMin: Vec3; rotationMax: Vec3
  springPosition: Vec3; springRotation: Vec3
}
// the flat arrays rz_upload_physics takes (Model.physicsTables()): offsets = inverseBind x T(shapePosition) R(shapeRotation)
export interface PhysicsTables {
  nBodies: number; bone: Int32Array; type: Uint8Array; shape: Uint8Array; size: Float32Array; offsetPos: Float32Array; offsetRot: Float32Array
  mass: Float32Array; linearDamping: Float32Array; angularDamping: Float32Array; restitution: Float32Array; friction: Float32Array
  group: Uint8Array; mask: Uint16Array
  nJoints: number; bodyA: Uint32Array; bodyB: Uint32Array; position: Float32Array; rotation: Float32Array
  positionMin: Float32Array; positionMax: Float32Array; rotationMin: Float32Array; rotationMax: Float32Array
  springPosition: Float32Array; springRotation: Float32Array
}
/** the reference Physics' seam (engine.ts:2379-2381): may overwrite world matrices in place */
export interface PhysicsLike { step(dt: number, worldMatrices: Float32Array, inverseBindMatrices: Float32Array): void }
export interface EngineOptions {
  ambient?: number; bloomIntensity?: number; rimLightIntensity?: number; cameraDistance?: number; cameraTarget?: Vec3
  device?: number; devices?: number[]; deviceFK?: boolean; deviceSampling?: boolean; outline?: boolean; bounds?: boolean
  gather?: boolean | 'direct'; morphLayout?: 'sparse' | 'dense'; realtime?: boolean; physics?: PhysicsLike | null
  framesInFlight?: 1 | 2; autotune?: boolean; sdef?: boolean; qdef?: boolean; ik?: boolean; devicePhysics?: boolean; physicsContacts?: boolean | 'boxes' | 'all'; physicsSprings?: boolean; physicsAligned?: boolean; followOverrides?: boolean; afterPhysics?: boolean; ikKeys?: boolean; crowdMorphs?: boolean
}
export interface EngineStats { fps: number; frameTime: number; gpuMemory: number; deformMs: number; vertsPerSec: number; hbmGBps: number }
export interface DeformedMesh { positions: Float32Array; normals: Float32Array }
export interface Bounds { min: number[]; max: number[] }
export interface Shard { ctx: DeformContext; begin: number; count: number; fork: DeformContext | null; last: DeformContext | null; flip: number }
export interface Timer { due: number; fn: () => void; id: number; handle: unknown }
