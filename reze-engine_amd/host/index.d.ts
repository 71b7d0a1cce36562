// Typings for the host package; shapes follow the reference's engine/src/index.ts:1-2 exports.
export class Vec3 {
  x: number; y: number; z: number
  constructor(x: number, y: number, z: number)
  add(o: Vec3): Vec3; subtract(o: Vec3): Vec3; scale(k: number): Vec3; dot(o: Vec3): number; cross(o: Vec3): Vec3
  length(): number; normalize(): Vec3; clone(): Vec3
}
export class Quat {
  x: number; y: number; z: number; w: number
  constructor(x: number, y: number, z: number, w: number)
  add(o: Quat): Quat; clone(): Quat; multiply(o: Quat): Quat; conjugate(): Quat; length(): number; normalize(): Quat
  rotateVec(v: Vec3): Vec3; rotate(v: Vec3): Vec3; toArray(): [number, number, number, number]; toEuler(): Vec3
  static slerp(a: Quat, b: Quat, t: number): Quat
  static fromEuler(rotX: number, rotY: number, rotZ: number): Quat
  static fromTo(from: Vec3, to: Vec3): Quat
}
export class Mat4 {
  values: Float32Array
  constructor(values: Float32Array)
  static identity(): Mat4
  static perspective(fov: number, aspect: number, near: number, far: number): Mat4
  static lookAt(eye: Vec3, target: Vec3, up: Vec3): Mat4
  static fromQuat(x: number, y: number, z: number, w: number): Mat4
  static fromPositionRotation(position: Vec3, rotation: Quat): Mat4
  static multiplyArrays(a: Float32Array, aOffset: number, b: Float32Array, bOffset: number, out: Float32Array, outOffset: number): void
  static toQuatFromArray(m: Float32Array, offset: number): Quat
  multiply(other: Mat4): Mat4; clone(): Mat4; getPosition(): Vec3; toQuat(): Quat; setIdentity(): this
  translateInPlace(tx: number, ty: number, tz: number): this; inverse(): Mat4
}
export interface EngineOptions {
  ambient?: number; bloomIntensity?: number; rimLightIntensity?: number; cameraDistance?: number; cameraTarget?: Vec3
  /** HIP device ordinal (default 0). */ device?: number
  /** Solve the bone hierarchy on the GPU (uploads local rotations instead of world matrices). */ deviceFK?: boolean
  /** Also write the outline pass's inverted hull every frame. */ outline?: boolean
  /** Also reduce the deformed mesh's bounding box every frame. */ bounds?: boolean
  /** Skin SDEF vertices (PMX weight type 3) as MMD does (default false: they are skinned as BDEF2, like the reference). */ sdef?: boolean
  /** Blend QDEF vertices (PMX 2.1 weight type 4) as dual quaternions (default false: they are skinned as BDEF4, like the reference). */ qdef?: boolean
  /** Solve PMX inverse kinematics (default false: the IK goal bones move, the legs do not follow, like the reference). With deviceFK the chains are uploaded once (rz_upload_ik) and solved on the GPU, else Model.solveIK() runs on the host. A bone with an IK block carries `ik: { effector, loops, limitAngle, links: [{ bone, min?, max? }] }` (Model.getIKChains() lists them). */ ik?: boolean
  /** One context per listed GPU; the mesh is vertex-sharded across them. */ devices?: number[]
  /** With deviceFK: seekFrame() samples the motion on the GPU (rz_upload_animation once, one float per frame). */ deviceSampling?: boolean
  /** Search launch shapes (morph split, workgroups per CU) once on the first rendered frame. */ autotune?: boolean
  /** 2: consecutive frames alternate between the context and a fork of it (own stream + outputs, shared static data), so frame f + 1 ramps up under frame f's tail. Single GPU, no gather. */ framesInFlight?: 1 | 2
  /** true: RCCL all-gather of the deformed mesh after every frame (distinct GPUs only); 'direct': every shard's kernel stores
   *  straight into the first GPU's gathered buffer over xGMI — no collective, GPUs may repeat in `devices`. */ gather?: boolean | 'direct'
  /** How PMX vertex morphs are laid out in HBM (default 'sparse'). */ morphLayout?: 'sparse' | 'dense'
  /** false: time only advances through step(timeMs). */ realtime?: boolean
  /** Physics hand-off (engine.ts:2379-2381), host-FK frames: step() may overwrite world matrices in place before they are uploaded. */
  physics?: { step(dt: number, boneWorldMatrices: Float32Array, boneInverseBindMatrices: Float32Array): void }
  /** Rigid-body physics on the GPU for the model's PMX bodies and joints (needs deviceFK; exclusive with `physics` and framesInFlight: 2). loadModel uploads Model.physicsTables() (rz_upload_physics); every frame turns the time the clock advanced since the last one into min(10, floor(accumulated / h)) fixed substeps of h = 1/75 s (rz_physics_step) before it deforms. No restitution; contacts (physicsContacts) and the joints' linear springs (physicsSprings) are opt-in. */ devicePhysics?: boolean
  /** With devicePhysics: contacts and friction between the model's sphere and capsule bodies by their PMX groups and masks (rz_physics_contacts, called on every shard right after the table's upload at loadModel). Off by default; without devicePhysics it throws. true: boxes take no part. 'boxes': the model's box bodies collide with its spheres and capsules as well (rz_physics_contacts(ctx, 2)); a pair of two boxes is still left out. 'all': pairs of two boxes collide too (rz_physics_contacts(ctx, 3)). */ physicsContacts?: boolean | 'boxes' | 'all'
  /** With devicePhysics: the model's PMX type-2 bodies ("physics + bone position alignment") are simulated instead of following their bones (rz_physics_aligned, called on every shard right after the table's upload at loadModel, ahead of physicsSprings and physicsContacts): such a body swings like a dynamic one, and its bone takes the rotation and keeps its animated position. Off by default; without devicePhysics it throws. */ physicsAligned?: boolean
  /** With devicePhysics: the linear springs of the model's joints (PMX spring_position; rz_physics_springs, called on every shard right after the table's upload at loadModel, ahead of physicsContacts): a joint with play along an axis and a spring on it swings about its rest point instead of hanging at the end of its play. Off by default; without devicePhysics it throws. */ physicsSprings?: boolean
  /** With deviceFK: bones below an overridden bone follow it (rz_override_follow, called on every shard and fork behind the topology upload) — W_b = O_a (S_a^-1 S_b) with a the nearest overridden ancestor of b, S the solved pose; for the overrides devicePhysics writes and for those of setBoneWorldOverrides. A strand's tip bone without a body, an ornament on a hair bone, the sub-bone of a skirt plate then ride the physics bone instead of staying with the animation. Not re-evaluated on the followed pose: append transforms, IK chains, following bodies. Off by default; without deviceFK it throws (host FK: call Model.followOverrides(world, bones, matrices) from the { physics } hook). */ followOverrides?: boolean
  /** With deviceFK: the model's PMX after-physics bones (flag 0x1000) are solved again behind the overrides, from the final pose of the bones they read (rz_upload_after_physics, called on every shard behind the topology upload and behind the IK table; forks borrow the list) — a skirt aid that takes half the rotation of a physics bone, a support bone that appends from a sprung body's bone then see the simulated pose. Evaluation order: Model.afterPhysicsOrder() (transform level, then index; it throws on a bone listed before a bone it reads). Off by default; without deviceFK it throws (host FK: call Model.solveAfterPhysics(world, overriddenBones) at the end of the { physics } hook). */ afterPhysics?: boolean
  /** With ik: honour the motion's VMD show / IK keys, which switch single IK chains off and on over time (a motion traced from motion capture switches leg and toe IK off at frame 0). Host path: seekFrame, playAnimation and seekMotions set the model's chain switches (Model.setIKChainEnabled) before the pose solve; a cross-fade takes clip `a`'s switches below blend 0.5 and clip `b`'s from there on, layers never switch. With { deviceFK, deviceSampling } the keys are uploaded behind the motion (rz_upload_ik_keys) and evaluated by the pose calls; host-sampled deviceFK frames send the switches with the pose (rz_set_ik_enabled). The keys' `show` flag is returned by the loader and not used. Off by default: a motion with such keys plays as before; without ik it throws. */ ikKeys?: boolean
  /** A crowd (setInstanceCount) of a model with vertex morphs takes the crowd skin kernels: each vertex is decoded once for a group of poses and its morph row walked once per pose, instead of the single-mesh kernel run once per instance (tuning key inst_morphs = 1, set on every shard behind setInstanceCount and on every fork). The frames are the same bits either way; whether it is faster depends on the model (profiles/crowd_morph_cost.txt). A group whose morph weights do not fit the LDS beside its palettes, the outline hull and the bounds keep the other kernel. Off by default. */ crowdMorphs?: boolean
}
export interface MotionState { a: string; frameA: number; b?: string | null; frameB?: number; blend?: number; layers?: MotionLayer[] }
/** one layer of a MotionState: motion `motion` at `frame`, applied with `weight` (default 1) where the mask `mask` (Engine.setMotionMask; none: everywhere) includes the bone or morph and the motion keys it — override (slerp / lerp towards it) or `additive` (q * slerp(identity, qL, weight), t + tL * weight, w + wL * weight). At most 4 per state. */
export interface MotionLayer { motion: string; frame: number; weight?: number; mask?: string | null; additive?: boolean }
export interface MotionMaskSpec { bones: string[]; withDescendants?: boolean; morphs?: string[] | 'all' | 'none' }
export interface EngineStats {
  fps: number; frameTime: number; gpuMemory: number
  deformMs: number; vertsPerSec: number; hbmGBps: number
}
export class Engine {
  constructor(canvas: unknown | null, options?: EngineOptions)
  init(): Promise<void>
  loadModel(path: string): Promise<void>
  loadAnimation(path: string): Promise<void>
  playAnimation(options?: { breathBones?: string[] | Record<string, number>; breathDuration?: number }): void
  stopAnimation(): void
  rotateBones(bones: string[], rotations: Quat[], durationMs?: number): void
  /** uv + UV morphs (PMX type 3), V x 2; a host-side sparse update — UVs never pass through the deformation kernel. */
  getMorphedUVs(): Float32Array
  /** Vertex morphs move vertices, bone morphs (PMX type 2) move bones before the hierarchy solve, group morphs feed both. */
  setMorphWeights(namesOrIndices: Array<string | number>, weights: number[]): void
  render(): void
  step(timeMs: number): void
  /** MMD-interpolated pose at a (fractional, 30 fps) frame; with a crowd (setInstanceCount) one frame per instance. */
  seekFrame(frame: number | ArrayLike<number>): void
  /** Add or replace a named motion of the motion library (loadAnimation / seekFrame are untouched). */
  loadMotion(name: string, path: string): Promise<void>
  /** Pose from the motion library: motion `a` at frameA, cross-faded by `blend` (0 .. 1) into motion `b` at frameB — slerp for rotations, lerp for translations and morph weights. With { deviceFK, deviceSampling } the library is uploaded once (rz_upload_motions) and every frame is one rz_set_pose_blended; a crowd takes one state per instance. Otherwise one character is posed on the host (Model.applyBlendedFrame). */
  seekMotions(state: MotionState | MotionState[]): void
  /** Add or replace the mask `name` for MotionState.layers: the named bones (`withDescendants`: and every bone below them in the skeleton) and morphs (names, 'all' — the default — or 'none'). With { deviceFK, deviceSampling } the masks are uploaded once per (mask set, model) (rz_upload_motion_masks) and a state with layers is one rz_set_pose_layered; otherwise one character is posed on the host (Model.applyLayeredFrame). */
  setMotionMask(name: string, spec: MotionMaskSpec): void
  /** n independently posed copies of the model (needs { deviceFK, deviceSampling }, one GPU). */
  setInstanceCount(n: number): void
  /** Physics hand-off with { deviceFK }: world matrices (column-major 4x4 each) that replace the GPU-solved ones of the listed bones until the next call. */
  setBoneWorldOverrides(boneIndices: ArrayLike<number>, worldMatrices: ArrayLike<number>, instances?: ArrayLike<number>): void
  /** With { ik }: hold one IK chain (the name of its IK bone, or its index in Model.getIKChains()) off or on by hand, for one crowd member or all; `on` null hands it back to the motion. A chain that is off does nothing: its links keep the sampled or uploaded rotations. On the device path the held switches are laid over the state the motion's keys give (all on without ikKeys) and sent behind every pose call (rz_set_ik_enabled): only the named switch changes, as on the host path. */
  setIKEnabled(nameOrIndex: string | number, on: boolean | null, instance?: number): void
  /** With { devicePhysics }: every body back onto its bone's solved pose with zero velocities (rz_physics_reset); the accumulated time is dropped. */
  resetPhysics(): void
  getDeformed(instance?: number): { positions: Float32Array; normals: Float32Array }
  getOutlineHull(): Float32Array
  getBounds(): { min: number[]; max: number[] }
  runRenderLoop(callback?: () => void): void
  stopRenderLoop(): void
  measure(frames?: number): { frameMs: number; deformKernelMs: number; prepKernelMs: number; vertsPerFrame: number; algorithmicBytesPerFrame: number; frames: number }
  getStats(): EngineStats
  dispose(): void
}
export class Model { [key: string]: any }
export class PmxLoader { static load(path: string): Promise<Model>; static loadFromBuffer(buf: ArrayBuffer | Uint8Array): Model }
export class VMDLoader { static load(path: string): Promise<any[]>; static loadFromBuffer(buf: ArrayBuffer | Uint8Array): any[] }
/** Frame-indexed MMD sampling of a loaded motion (rotation / position / morph keys); flatten() feeds the device sampler. */
export class VMDSampler {
  constructor(keyFrames: any[])
  lastFrame: number
  sampleBone(name: string, frame: number): { rotation: number[]; position: number[] } | null
  sampleMorph(name: string, frame: number): number | null
  boneNames(): string[]; morphNames(): string[]
  /** the IK switches at `frame`, name of the IK bone -> on, for every chain the motion's show / IK keys name: the state the last key with key.frame <= frame left (before the first key: the first key's); empty without such keys */
  ikStateAt(frame: number): Map<string, boolean>
  /** `ikChainNames` (Model.getIKChainNames()): a motion with show / IK keys also returns ikKeys: { frames, enabled [n][chains] } for rz_upload_ik_keys */
  flatten(boneNameIndex: Record<string, number>, morphs: { names: string[]; types: ArrayLike<number>; groups: Array<Array<[number, number]> | null> } | null, ikChainNames?: string[] | null): Record<string, Int32Array | Uint32Array | Float32Array | Uint8Array | { frames: Float32Array; enabled: Uint8Array }>
}
