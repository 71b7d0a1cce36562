'use strict'
/*
 * Source: host/src/model.ts (TypeScript). host/model.js is that file with its types erased (tools/ts_erase.py; no tsc in the image) - edit the .ts.
 * model.js — scene data + CPU pose solve (stays on the host, north star: "the PMX/VMD parsers and
 * CPU bone-hierarchy solve stay in TypeScript").
 *
 * Mirrors the reference's class Model (engine/src/model.ts:70-421): same constructor argument
 * order, same getters (getVertices / getSkinning / getSkeleton / getBoneWorldMatrices / ...),
 * same rotateBones() tween semantics (:246-315), updateRotationTweens (:158-194) and forward
 * kinematics with MMD append-rotation (:330-420), same typed-array state (SkeletonRuntime,
 * :52-59). World matrices come out bit-identical to the reference because every intermediate
 * matrix is stored to Float32Array at the same points.
 *
 * Additions the reference lacks (SURVEY §8b): an injectable clock (the reference reads
 * performance.now(), model.ts:160,249 — not reproducible frame for frame) and vertex-morph state
 * (names, sparse targets, weights, group-morph flattening) feeding the fused GPU kernel.
 */
import { Quat, easeInOut, kernels } from './math'
import type { Bone, HostLayer, HostMask, IKChain, Joint, LayeredBase, Material, MorphSet, NumArray, PhysicsTables, PosedLocals, Rigidbody, RotTweenState, SdefTable, Skeleton, SkeletonRuntime, Skinning, Texture } from './types'
import type { VMDSampler } from './vmd-sampler'
const { slerpInto, mulInto, quatToMatInto, identityInto } = kernels

const VERTEX_STRIDE = 8 // floats per vertex: x y z nx ny nz u v  (model.ts:4, :196-200)

let defaultClock: () => number
try {
  const { performance } = require('perf_hooks')
  defaultClock = () => performance.now()
} catch (e) {
  defaultClock = () => Date.now()
}

class Model {
  vertexData: Float32Array
  vertexCount: number
  indexData: Uint32Array
  textures: Texture[]
  materials: Material[]
  skeleton: Skeleton
  skinning: Skinning
  sdef: SdefTable
  qdef: Uint32Array
  rigidbodies: Rigidbody[]
  joints: Joint[]
  clock: () => number
  runtimeSkeleton: SkeletonRuntime
  rotTweenState: RotTweenState
  solveOrder: number[]
  _rot: Float32Array
  _app: Float32Array
  _tmpA: Float32Array
  _tmpB: Float32Array
  _follow: Float64Array
  _tr: Float32Array
  _q: number[]
  applyLocalTranslations: boolean
  morphs: MorphSet | null
  morphWeights: Float32Array
  effectiveMorphWeights: Float32Array
  morphNameIndex: Record<string, number>
  hasBoneMorphs: boolean
  poseRotations: Float32Array
  poseTranslations: Float32Array
  _uv?: Float32Array
  _uvWeights?: Float32Array
  ikEnabled: boolean
  ikChains: IKChain[] | null
  ikChainOn: Uint8Array | null
  ikKeys: boolean
  ikRotations: Float32Array
  ikTranslations: Float32Array
  _ikR: Float64Array
  _ikP: Float64Array
  _ikDeps: Record<number, number[]>
  /**
   * @param {Float32Array} vertexData interleaved 8 floats / vertex
   * @param {Uint32Array} indexData
   * @param {Array} textures
   * @param {Array} materials
   * @param {{bones: Array, inverseBindMatrices: Float32Array}} skeleton
   * @param {{joints: Uint16Array, weights: Uint8Array}} skinning
   * @param {Array} [rigidbodies]
   * @param {Array} [joints]
   * @param {object|null} [morphs] { names, types, offsets:Uint32Array(M+1), vertexIndex:Uint32Array,
   *                                 deltas:Float32Array(E*3), groups: Array<Array<[child, ratio]>|null> }
   */
  constructor(vertexData: Float32Array, indexData: Uint32Array, textures: Texture[], materials: Material[], skeleton: Skeleton, skinning: Skinning, rigidbodies?: Rigidbody[], joints?: Joint[], morphs?: MorphSet | null) {
    if (!skeleton || !skeleton.bones || skeleton.bones.length === 0) throw new Error('Model has no bones')
    this.vertexData = vertexData
    this.vertexCount = vertexData.length / VERTEX_STRIDE
    this.indexData = indexData
    this.textures = textures || []
    this.materials = materials || []
    this.skeleton = skeleton
    this.skinning = skinning
    // SDEF vertices (PMX weight type 3): set by the PMX loader; skinned as BDEF2 unless the engine is asked for SDEF ({ sdef: true })
    this.sdef = { index: new Uint32Array(0), c: new Float32Array(0), r0: new Float32Array(0), r1: new Float32Array(0) }
    // QDEF vertices (PMX 2.1 weight type 4), ascending: set by the PMX loader; skinned as BDEF4 unless the engine is asked for QDEF ({ qdef: true })
    this.qdef = new Uint32Array(0)
    this.rigidbodies = rigidbodies || []
    this.joints = joints || []
    this.clock = defaultClock

    const n = skeleton.bones.length
    const nameIndex = {}
    for (let i = 0; i < n; i++) nameIndex[skeleton.bones[i].name] = i
    const localRotations = new Float32Array(n * 4)
    for (let i = 0; i < n; i++) localRotations[i * 4 + 3] = 1
    this.runtimeSkeleton = {
      nameIndex,
      localRotations, // quat per bone (x,y,z,w)
      localTranslations: new Float32Array(n * 3),
      worldMatrices: new Float32Array(n * 16),
      computedBones: new Array(n).fill(false),
    }
    this.rotTweenState = {
      active: new Uint8Array(n),
      startQuat: new Float32Array(n * 4),
      targetQuat: new Float32Array(n * 4),
      startTimeMs: new Float32Array(n),
      durationMs: new Float32Array(n),
    }
    // parent-first evaluation order (the reference recurses; the result per bone is the same)
    this.solveOrder = Model.parentFirstOrder(skeleton.bones)
    // scratch matrices for the FK (no per-bone allocation)
    this._rot = new Float32Array(16)
    this._app = new Float32Array(16)
    this._tmpA = new Float32Array(16)
    this._tmpB = new Float32Array(16)
    this._follow = new Float64Array(12) // followOverrides(): S_a^-1 S_b, rows
    this._tr = new Float32Array(16)
    this._q = [0, 0, 0, 1]

    // Frame-sampled VMD playback may also move bones (センター etc.). The reference never writes localTranslations and
    // applies them only through append-move (model.ts:388-393), so this stays off unless a sampler turns it on.
    this.applyLocalTranslations = false

    this.morphs = morphs || null
    const m = this.morphs ? this.morphs.names.length : 0
    this.morphWeights = new Float32Array(m) // as set by the user / animation (includes group morphs)
    this.effectiveMorphWeights = new Float32Array(m) // group morphs flattened onto their children
    this.morphNameIndex = {}
    for (let i = 0; i < m; i++) this.morphNameIndex[this.morphs.names[i]] = i
    // PMX bone morphs (type 2): the local pose the hierarchy solve sees = the runtime's local pose with them folded in
    this.hasBoneMorphs = !!(this.morphs && this.morphs.boneEntries && this.morphs.boneEntries.morph.length > 0)
    this.poseRotations = new Float32Array(this.hasBoneMorphs ? n * 4 : 0)
    this.poseTranslations = new Float32Array(this.hasBoneMorphs ? n * 3 : 0)
    // PMX inverse kinematics: off unless the engine is asked for it ({ ik: true }); the chains come from the loader's bone.ik
    this.ikEnabled = false
    this.ikChains = null
    this.ikChainOn = null // per-chain switches of solveIK(), in getIKChains() order; null = every chain on
    this.ikKeys = false // setIKKeys(): the pose calls that sample a motion also set the switches from its show / IK keys
    this.ikRotations = new Float32Array(0)
    this.ikTranslations = new Float32Array(0)
    this._ikR = new Float64Array(0)
    this._ikP = new Float64Array(0)
    this._ikDeps = {}
  }

  static parentFirstOrder(bones: Bone[]): number[] {
    const n = bones.length
    const state = new Uint8Array(n)
    const order = []
    for (let i = 0; i < n; i++) {
      if (state[i]) continue
      const chain = []
      let b = i
      while (b >= 0 && b < n && !state[b]) { state[b] = 1; chain.push(b); b = bones[b].parentIndex }
      for (let k = chain.length - 1; k >= 0; k--) order.push(chain[k])
    }
    return order
  }

  /** Replace performance.now() (deterministic tests / offline stepping). */
  setClock(fn: (() => number) | null): void { this.clock = fn || defaultClock }

  // ---- static data getters (model.ts:196-238) ----
  getVertices(): Float32Array { return this.vertexData }
  getTextures(): Texture[] { return this.textures }
  getMaterials(): Material[] { return this.materials }
  getVertexCount(): number { return this.vertexCount }
  getIndices(): Uint32Array { return this.indexData }
  getSkeleton(): Skeleton { return this.skeleton }
  getSkinning(): Skinning { return this.skinning }
  getSdef(): SdefTable { return this.sdef }
  getQdef(): Uint32Array { return this.qdef }
  getRigidbodies(): Rigidbody[] { return this.rigidbodies }
  getJoints(): Joint[] { return this.joints }

  /*
   * The flat arrays rz_upload_physics takes. A body's frame in its bone's space is offset = inverseBind x T(shapePosition) R(shapeRotation)
   * (physics.ts:572-596), Euler angles -> quaternion with Quat.fromEuler as the reference does; the loader's inverse binds are pure
   * translations, so the rotation of the offset is the shape's. A body without a bone (-1) keeps its model-space frame.
   */
  physicsTables(): PhysicsTables {
    const rb = this.rigidbodies, jt = this.joints, nb = rb.length, nj = jt.length
    const ib = this.skeleton.inverseBindMatrices, B = this.skeleton.bones.length
    const t: PhysicsTables = {
      nBodies: nb, bone: new Int32Array(nb), type: new Uint8Array(nb), shape: new Uint8Array(nb), size: new Float32Array(nb * 3),
      offsetPos: new Float32Array(nb * 3), offsetRot: new Float32Array(nb * 4), mass: new Float32Array(nb), linearDamping: new Float32Array(nb),
      angularDamping: new Float32Array(nb), restitution: new Float32Array(nb), friction: new Float32Array(nb), group: new Uint8Array(nb),
      mask: new Uint16Array(nb), nJoints: nj, bodyA: new Uint32Array(nj), bodyB: new Uint32Array(nj), position: new Float32Array(nj * 3),
      rotation: new Float32Array(nj * 3), positionMin: new Float32Array(nj * 3), positionMax: new Float32Array(nj * 3),
      rotationMin: new Float32Array(nj * 3), rotationMax: new Float32Array(nj * 3), springPosition: new Float32Array(nj * 3),
      springRotation: new Float32Array(nj * 3),
    }
    for (let i = 0; i < nb; i++) {
      const b = rb[i]
      const bone = b.boneIndex >= 0 && b.boneIndex < B ? b.boneIndex : -1
      t.bone[i] = bone; t.type[i] = b.type; t.shape[i] = b.shape; t.group[i] = b.group; t.mask[i] = b.collisionMask
      t.size.set([b.size.x, b.size.y, b.size.z], i * 3)
      const o = bone >= 0 ? bone * 16 + 12 : -1
      t.offsetPos.set([b.shapePosition.x + (o >= 0 ? ib[o] : 0), b.shapePosition.y + (o >= 0 ? ib[o + 1] : 0), b.shapePosition.z + (o >= 0 ? ib[o + 2] : 0)], i * 3)
      const q = Quat.fromEuler(b.shapeRotation.x, b.shapeRotation.y, b.shapeRotation.z)
      t.offsetRot.set([q.x, q.y, q.z, q.w], i * 4)
      t.mass[i] = b.mass; t.linearDamping[i] = b.linearDamping; t.angularDamping[i] = b.angularDamping
      t.restitution[i] = b.restitution; t.friction[i] = b.friction
    }
    for (let j = 0; j < nj; j++) {
      const s = jt[j]
      t.bodyA[j] = s.rigidbodyIndexA; t.bodyB[j] = s.rigidbodyIndexB
      const src = [s.position, s.rotation, s.positionMin, s.positionMax, s.rotationMin, s.rotationMax, s.springPosition, s.springRotation]
      const dst = [t.position, t.rotation, t.positionMin, t.positionMax, t.rotationMin, t.rotationMax, t.springPosition, t.springRotation]
      for (let k = 0; k < 8; k++) dst[k].set([src[k].x, src[k].y, src[k].z], j * 3)
    }
    return t
  }
  getBoneNames(): string[] { return this.skeleton.bones.map((b) => b.name) }
  getBoneWorldMatrices(): Float32Array { return this.runtimeSkeleton.worldMatrices }
  getBoneInverseBindMatrices(): Float32Array { return this.skeleton.inverseBindMatrices }

  // ---- pose API ----
  _tweenValue(idx: number, now: number, out: NumArray): number {
    const st = this.rotTweenState
    const qi = idx * 4
    const dur = Math.max(1, st.durationMs[idx])
    const t = Math.max(0, Math.min(1, (now - st.startTimeMs[idx]) / dur))
    slerpInto(out, st.startQuat[qi], st.startQuat[qi + 1], st.startQuat[qi + 2], st.startQuat[qi + 3],
      st.targetQuat[qi], st.targetQuat[qi + 1], st.targetQuat[qi + 2], st.targetQuat[qi + 3], easeInOut(t))
    return t
  }

  /** model.ts:246-315 — immediate set (durationMs 0/undefined) or arm a quadratic-ease slerp tween. */
  rotateBones(names: string[], quats: Quat[], durationMs?: number): void {
    const st = this.rotTweenState
    const rot = this.runtimeSkeleton.localRotations
    const nameIndex = this.runtimeSkeleton.nameIndex
    const now = this.clock()
    const dur = durationMs && durationMs > 0 ? durationMs : 0
    const cur = this._q
    for (let i = 0; i < names.length; i++) {
      const found = nameIndex[names[i]]
      const idx = found === undefined || found === null ? -1 : found
      if (idx < 0 || idx >= this.skeleton.bones.length) continue
      const q = quats[i].normalize()
      const qi = idx * 4
      if (dur === 0) {
        rot[qi] = q.x; rot[qi + 1] = q.y; rot[qi + 2] = q.z; rot[qi + 3] = q.w
        st.active[idx] = 0
        continue
      }
      // start from where the bone is now: the running tween's interpolated value, else the stored rotation
      let sx = rot[qi], sy = rot[qi + 1], sz = rot[qi + 2], sw = rot[qi + 3]
      if (st.active[idx] === 1) {
        this._tweenValue(idx, now, cur)
        sx = cur[0]; sy = cur[1]; sz = cur[2]; sw = cur[3]
      }
      st.startQuat[qi] = sx; st.startQuat[qi + 1] = sy; st.startQuat[qi + 2] = sz; st.startQuat[qi + 3] = sw
      st.targetQuat[qi] = q.x; st.targetQuat[qi + 1] = q.y; st.targetQuat[qi + 2] = q.z; st.targetQuat[qi + 3] = q.w
      st.startTimeMs[idx] = now
      st.durationMs[idx] = dur
      st.active[idx] = 1
    }
  }

  /** model.ts:158-194 */
  updateRotationTweens(): void {
    const st = this.rotTweenState
    const rot = this.runtimeSkeleton.localRotations
    const now = this.clock()
    const cur = this._q
    for (let i = 0, n = this.skeleton.bones.length; i < n; i++) {
      if (st.active[i] !== 1) continue
      const t = this._tweenValue(i, now, cur)
      const qi = i * 4
      rot[qi] = cur[0]; rot[qi + 1] = cur[1]; rot[qi + 2] = cur[2]; rot[qi + 3] = cur[3]
      if (t >= 1) st.active[i] = 0
    }
  }

  /** model.ts:325-328 */
  evaluatePose(): void {
    this.updateRotationTweens()
    this.computeWorldMatrices()
  }

  /**
   * The local pose the hierarchy solve consumes. Without bone morphs (or with all of them at weight 0) these ARE the
   * runtime arrays (model.ts:55-56). A PMX bone morph (type 2; the reference only skips the section,
   * pmx-loader.ts:489-497, so the semantics are this build's, the usual MMD ones) with effective weight w adds
   * w * translation to its bone's local translation and right-multiplies the local rotation by
   * Quat.slerp(identity, rotation, w) (math.ts:156-189, :77-85); entries fold in ascending morph order; the runtime arrays
   * (tween / animation state) are left untouched. GPU twin: fk_solve's bone-morph pass (csrc/deform_kernels.hip).
   */
  posedLocals(): PosedLocals {
    const rs = this.runtimeSkeleton
    const raw = { rot: rs.localRotations, tra: rs.localTranslations, moved: false }
    if (!this.hasBoneMorphs) return raw
    const w = this.getEffectiveMorphWeights()
    const be = this.morphs.boneEntries
    const n = be.morph.length
    let any = false
    for (let k = 0; k < n && !any; k++) any = w[be.morph[k]] !== 0
    if (!any) return raw
    const rot = this.poseRotations, tra = this.poseTranslations
    rot.set(rs.localRotations); tra.set(rs.localTranslations)
    const s = this._q
    for (let k = 0; k < n; k++) {
      const wk = w[be.morph[k]]
      if (wk === 0) continue
      const b = be.bone[k], qi = b * 4, ti = b * 3
      tra[ti] += wk * be.translation[k * 3]; tra[ti + 1] += wk * be.translation[k * 3 + 1]; tra[ti + 2] += wk * be.translation[k * 3 + 2]
      slerpInto(s, 0, 0, 0, 1, be.rotation[k * 4], be.rotation[k * 4 + 1], be.rotation[k * 4 + 2], be.rotation[k * 4 + 3], wk)
      const x = rot[qi], y = rot[qi + 1], z = rot[qi + 2], ww = rot[qi + 3] // Hamilton product local * s
      rot[qi] = ww * s[0] + x * s[3] + y * s[2] - z * s[1]
      rot[qi + 1] = ww * s[1] - x * s[2] + y * s[3] + z * s[0]
      rot[qi + 2] = ww * s[2] + x * s[1] - y * s[0] + z * s[3]
      rot[qi + 3] = ww * s[3] - x * s[0] - y * s[1] - z * s[2]
    }
    return { rot, tra, moved: true }
  }

  /**
   * model.ts:330-420. Per bone: R = fromQuat(q); append-rotation R = fromQuat(slerp(I, +-q_append,
   * |ratio|)) * R when appendRotate && valid parent && |clamp(ratio,-1,1)| > 1e-6; append-move only
   * inside that branch; L = T(bind) * R * T(add); W = W_parent * L.
   */
  computeWorldMatrices(): void {
    const bones = this.skeleton.bones
    const n = bones.length
    const { rot, tra, moved } = this.ikEnabled ? this.solveIK() : this.posedLocals()
    const useT = this.applyLocalTranslations || moved
    const world = this.runtimeSkeleton.worldMatrices
    const R = this._rot, A = this._app, T = this._tr, X = this._tmpA, L = this._tmpB
    const q = this._q
    for (let k = 0; k < n; k++) {
      const i = this.solveOrder[k]
      const b = bones[i]
      if (b.parentIndex >= n) console.warn('[RZM] bone ' + i + ' parent out of range: ' + b.parentIndex)
      const qi = i * 4
      quatToMatInto(R, 0, rot[qi], rot[qi + 1], rot[qi + 2], rot[qi + 3])
      let ax = 0, ay = 0, az = 0
      let rotM = R
      const ap = b.appendParentIndex
      if (b.appendRotate && ap !== undefined && ap !== null && ap >= 0 && ap < n) {
        const ratio = b.appendRatio === undefined || b.appendRatio === null ? 1 : Math.max(-1, Math.min(1, b.appendRatio))
        if (Math.abs(ratio) > 1e-6) {
          const aq = ap * 4
          let qx = rot[aq], qy = rot[aq + 1], qz = rot[aq + 2]
          const qw = rot[aq + 3]
          if (ratio < 0) { qx = -qx; qy = -qy; qz = -qz }
          slerpInto(q, 0, 0, 0, 1, qx, qy, qz, qw, ratio < 0 ? -ratio : ratio)
          quatToMatInto(A, 0, q[0], q[1], q[2], q[3])
          mulInto(X, 0, A, 0, R, 0)
          rotM = X
          if (b.appendMove) {
            const r = b.appendRatio === undefined || b.appendRatio === null ? 1 : b.appendRatio
            ax = tra[ap * 3] * r; ay = tra[ap * 3 + 1] * r; az = tra[ap * 3 + 2] * r
          }
        }
      }
      // L = T(bind) * rotM * T(add), each product stored as f32 like the reference's Mat4.multiply chain
      identityInto(T, 0)
      T[12] += b.bindTranslation[0]; T[13] += b.bindTranslation[1]; T[14] += b.bindTranslation[2]
      if (useT) { T[12] += tra[i * 3]; T[13] += tra[i * 3 + 1]; T[14] += tra[i * 3 + 2] }
      mulInto(L, 0, T, 0, rotM, 0)
      identityInto(T, 0)
      T[12] += ax; T[13] += ay; T[14] += az
      const L2 = rotM === X ? R : X // a free scratch matrix
      mulInto(L2, 0, L, 0, T, 0)
      const wo = i * 16
      if (b.parentIndex >= 0) {
        mulInto(T, 0, world, b.parentIndex * 16, L2, 0)
        world.set(T, wo)
      } else {
        world.set(L2, wo)
      }
    }
    this.runtimeSkeleton.computedBones.fill(true)
  }

  /** The model's IK chains (bones the loader gave an `ik` block), ascending IK bone index: the solve order. `goal` is the IK bone itself. */
  getIKChains(): IKChain[] {
    if (!this.ikChains) {
      const out = []
      const bones = this.skeleton.bones
      for (let i = 0; i < bones.length; i++) {
        const k = bones[i].ik
        if (!k) continue
        out.push({ goal: i, effector: k.effector, loops: k.loops, limitAngle: k.limitAngle, links: k.links.map((l) => ({ bone: l.bone, min: l.min, max: l.max })) })
      }
      this.ikChains = out
    }
    return this.ikChains
  }

  /** Switch the host IK solve on or off (a model without IK bones stays off). */
  setIK(on: boolean): void { this.ikEnabled = !!on && this.getIKChains().length > 0 }

  /**
   * Switch one IK chain of solveIK() off or on: `nameOrIndex` is the name of the chain's IK bone or its index in getIKChains(). A chain
   * that is off does nothing: its links keep the posed rotations (tests/ik_switch_ref.py; device twin: rz_set_ik_enabled).
   */
  setIKChainEnabled(nameOrIndex: string | number, on: boolean): void {
    const chains = this.getIKChains()
    const k = typeof nameOrIndex === 'number' ? nameOrIndex : chains.findIndex((ch) => this.skeleton.bones[ch.goal].name === nameOrIndex)
    if (!(k >= 0 && k < chains.length) || k !== Math.floor(k)) throw new Error('setIKChainEnabled: no IK chain ' + JSON.stringify(nameOrIndex))
    if (!this.ikChainOn) this.ikChainOn = new Uint8Array(chains.length).fill(1)
    this.ikChainOn[k] = on ? 1 : 0
  }

  /** the switches of getIKChains(), in that order */
  getIKChainEnabled(): boolean[] { return this.getIKChains().map((_, k) => !this.ikChainOn || this.ikChainOn[k] !== 0) }

  /** the names of the chains' IK bones, in getIKChains() order: what a VMD's show / IK keys name */
  getIKChainNames(): string[] { return this.getIKChains().map((ch) => this.skeleton.bones[ch.goal].name) }

  /** With it on, applySampledFrame / applyBlendedFrame / applyLayeredFrame also set the chain switches from the motion's show / IK keys. Off by default. */
  setIKKeys(on: boolean): void { this.ikKeys = !!on }

  /** every chain's switch from a sampler's IK state at `frame` (VMDSampler.ikStateAt); a chain the motion never names is on, and so is every chain without a sampler */
  applyIKState(sampler: { ikStateAt?(frame: number): Map<string, boolean> } | null, frame: number): void {
    const state = sampler && sampler.ikStateAt ? sampler.ikStateAt(frame) : new Map()
    this.getIKChainNames().forEach((name, k) => this.setIKChainEnabled(k, state.get(name) !== false))
  }

  /**
   * Bones below an overridden bone follow it: the host twin of the device stage rz_override_follow (csrc/kernels/fk.hip.h: FOLLOW), the
   * definition of tests/follow_ref.py in doubles with f32 stores. `world` holds the SOLVED world matrices S (n x 16, column-major: what
   * computeWorldMatrices() left, before a physics hook wrote into it) and is rewritten in place; `bones` / `matrices` (16 floats each)
   * are the override set O, of several entries for one bone the last. Every bone b outside O with an ancestor in O takes
   * W_b = O_a (S_a^-1 S_b), a the NEAREST such ancestor along the parents and S_a^-1 the rigid inverse (R^T, -R^T p); bones of O take
   * O_a; all others keep S_b. An override below another override is absolute. Nothing is evaluated again on the followed pose (append
   * transforms, IK). For host-FK users of the { physics } hook: call it from the hook with a copy of the matrices taken on entry.
   */
  followOverrides(world: Float32Array, bones: ArrayLike<number>, matrices: ArrayLike<number>): void {
    const sk = this.skeleton.bones, n = sk.length
    if (matrices.length !== bones.length * 16) throw new Error('followOverrides: ' + bones.length + ' bones need ' + bones.length * 16 + ' matrix floats')
    if (world.length !== n * 16) throw new Error('followOverrides: world holds ' + world.length + ' floats, the skeleton has ' + n + ' bones')
    const own = new Int32Array(n).fill(-1)
    for (let k = 0; k < bones.length; k++) {
      if (!(bones[k] >= 0 && bones[k] < n)) throw new Error('followOverrides: bone ' + bones[k] + ' out of range')
      own[bones[k]] = k
    }
    // near[b]: the entry bone b takes its matrix from (-1 = no bone above it is overridden, -2 = not known yet); parents may come in any order
    const near = new Int32Array(n).fill(-2)
    const chain = []
    for (let b = 0; b < n; b++) {
      chain.length = 0
      let cur = b
      while (cur >= 0 && near[cur] === -2 && own[cur] < 0) { chain.push(cur); cur = sk[cur].parentIndex }
      const found = cur < 0 ? -1 : own[cur] >= 0 ? own[cur] : near[cur]
      if (cur >= 0 && own[cur] >= 0) near[cur] = own[cur]
      for (const x of chain) near[x] = found
    }
    const S = Float64Array.from(world) // followers read S_a after bone a itself has been rewritten
    for (let b = 0; b < n; b++) {
      const k = near[b]
      if (k < 0) continue
      const o = k * 16, wb = b * 16
      if (own[b] >= 0) {
        for (let c = 0; c < 4; c++) { world[wb + c * 4] = matrices[o + c * 4]; world[wb + c * 4 + 1] = matrices[o + c * 4 + 1]; world[wb + c * 4 + 2] = matrices[o + c * 4 + 2]; world[wb + c * 4 + 3] = c === 3 ? 1 : 0 }
        continue
      }
      const a = bones[k] * 16
      // rel = S_a^-1 S_b: rows i of R_a^T are columns i of S_a
      const dx = S[wb + 12] - S[a + 12], dy = S[wb + 13] - S[a + 13], dz = S[wb + 14] - S[a + 14]
      const rel = this._follow
      for (let i = 0; i < 3; i++) {
        const ax = S[a + i * 4], ay = S[a + i * 4 + 1], az = S[a + i * 4 + 2]
        for (let j = 0; j < 3; j++) rel[i * 4 + j] = ax * S[wb + j * 4] + ay * S[wb + j * 4 + 1] + az * S[wb + j * 4 + 2]
        rel[i * 4 + 3] = ax * dx + ay * dy + az * dz
      }
      // W_b = O_a rel, upper three rows
      for (let i = 0; i < 3; i++) {
        const o0 = matrices[o + i], o1 = matrices[o + 4 + i], o2 = matrices[o + 8 + i]
        for (let j = 0; j < 4; j++) world[wb + j * 4 + i] = o0 * rel[j] + o1 * rel[4 + j] + o2 * rel[8 + j] + (j === 3 ? matrices[o + 12 + i] : 0)
      }
      world[wb + 3] = 0; world[wb + 7] = 0; world[wb + 11] = 0; world[wb + 15] = 1
    }
  }

  /**
   * The PMX after-physics bones (flag 0x1000, "deform after physics") in evaluation order: ascending (transform level, index) — the list
   * rz_upload_after_physics takes and solveAfterPhysics() walks. Throws, naming the bone, when a listed bone's parent, append parent or
   * append parent's parent is listed LATER: the authoring error PMX editors warn about (MMD then shows a one-frame lag, which neither
   * twin reproduces).
   */
  afterPhysicsOrder(): number[] {
    const bones = this.skeleton.bones, n = bones.length
    const order = []
    for (let i = 0; i < n; i++) if (bones[i].afterPhysics) order.push(i)
    order.sort((a, b) => ((bones[a].transformLevel || 0) - (bones[b].transformLevel || 0)) || (a - b))
    const pos = new Int32Array(n).fill(-1)
    order.forEach((b, k) => { pos[b] = k })
    for (let k = 0; k < order.length; k++) {
      const b = order[k], ap = this._appendInEffect(b)
      const reads = [bones[b].parentIndex, ap, ap >= 0 ? bones[ap].parentIndex : -1]
      const what = ['parent', 'append parent', "append parent's parent"]
      for (let j = 0; j < 3; j++) {
        const r = reads[j]
        if (r >= 0 && r < n && r !== b && pos[r] > k) {
          throw new Error('afterPhysicsOrder: bone ' + b + ' (' + bones[b].name + ') is evaluated before its ' + what[j] + ', bone ' + r + ' (' + bones[r].name +
            '): an after-physics bone must come after the after-physics bones it reads (transform level, then index)')
        }
      }
    }
    return order
  }

  /** the append parent bone b's local matrix reads, or -1: none, or a ratio that leaves none in effect (computeWorldMatrices) */
  _appendInEffect(b: number): number {
    const bone = this.skeleton.bones[b], n = this.skeleton.bones.length
    const ap = bone.appendParentIndex
    if (!bone.appendRotate || ap === undefined || ap === null || ap < 0 || ap >= n) return -1
    const ratio = bone.appendRatio === undefined || bone.appendRatio === null ? 1 : Math.max(-1, Math.min(1, Math.fround(bone.appendRatio)))
    return Math.abs(ratio) > 1e-6 ? ap : -1
  }

  /**
   * The after-physics bones solved again on the final pose: the host twin of the device stage rz_upload_after_physics
   * (csrc/kernels/after.hip), the definition of tests/after_ref.py in doubles with f32 stores. `world` holds the world matrices as the
   * frame leaves them (n x 16, column-major: computeWorldMatrices(), then the physics hook's overrides, then followOverrides() if used)
   * and is rewritten in place; `overriddenBones` is the override set O. For b in afterPhysicsOrder(), unless b is in O:
   * P = world[parent(b)]; with an append parent a in effect, a's local transform as finally posed is read from `world`
   * (R_a = rot(W[parent(a)])^T rot(W[a]), t_a = rot(W[parent(a)])^T (pos(W[a]) - pos(W[parent(a)])) - bind_a; a root a: W[a] itself),
   * q_a = quat(R_a) by the branch on the largest of trace, m00, m11, m22, normalised, and the local matrix is formed as
   * computeWorldMatrices() forms it with q_a and t_a in the place of a's pose; world[b] = P L, and later entries read it. Non-listed bones
   * below a listed bone keep their matrices; IK is not solved again. For host-FK users of the { physics } hook: call it at the hook's end.
   */
  solveAfterPhysics(world: Float32Array, overriddenBones: ArrayLike<number>): void {
    const bones = this.skeleton.bones, n = bones.length
    if (world.length !== n * 16) throw new Error('solveAfterPhysics: world holds ' + world.length + ' floats, the skeleton has ' + n + ' bones')
    const skip = new Uint8Array(n)
    for (let k = 0; k < overriddenBones.length; k++) {
      if (!(overriddenBones[k] >= 0 && overriddenBones[k] < n)) throw new Error('solveAfterPhysics: bone ' + overriddenBones[k] + ' out of range')
      skip[overriddenBones[k]] = 1
    }
    const order = this.afterPhysicsOrder()
    const { rot, tra, moved } = this.posedLocals()
    const useT = this.applyLocalTranslations || moved
    // row-major 3 x 3 of a quaternion (math.ts: fromQuat)
    const qmat = (x, y, z, w) => {
      const x2 = x + x, y2 = y + y, z2 = z + z
      const xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2, wx = w * x2, wy = w * y2, wz = w * z2
      return [1 - (yy + zz), xy - wz, xz + wy, xy + wz, 1 - (xx + zz), yz - wx, xz - wy, yz + wx, 1 - (xx + yy)]
    }
    const mul3 = (a, b) => {
      const o = new Array(9)
      for (let i = 0; i < 3; i++) for (let j = 0; j < 3; j++) o[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j]
      return o
    }
    // rows (R row-major, p) of a column-major 4 x 4 in `world`
    const rows = (b) => {
      const o = b * 16
      return { R: [world[o], world[o + 4], world[o + 8], world[o + 1], world[o + 5], world[o + 9], world[o + 2], world[o + 6], world[o + 10]], p: [world[o + 12], world[o + 13], world[o + 14]] }
    }
    for (const b of order) {
      if (skip[b]) continue
      const bone = bones[b]
      let R = qmat(rot[b * 4], rot[b * 4 + 1], rot[b * 4 + 2], rot[b * 4 + 3])
      let ax = 0, ay = 0, az = 0
      const a = this._appendInEffect(b)
      if (a >= 0) {
        const A = rows(a)
        let Ra = A.R, pa = A.p
        const g = bones[a].parentIndex
        if (g >= 0) {
          const G = rows(g)
          const Gt = [G.R[0], G.R[3], G.R[6], G.R[1], G.R[4], G.R[7], G.R[2], G.R[5], G.R[8]]
          const d = [pa[0] - G.p[0], pa[1] - G.p[1], pa[2] - G.p[2]]
          Ra = mul3(Gt, Ra)
          pa = [Gt[0] * d[0] + Gt[1] * d[1] + Gt[2] * d[2], Gt[3] * d[0] + Gt[4] * d[1] + Gt[5] * d[2], Gt[6] * d[0] + Gt[7] * d[1] + Gt[8] * d[2]]
        }
        const ba = bones[a].bindTranslation
        const ta = [pa[0] - ba[0], pa[1] - ba[1], pa[2] - ba[2]]
        // q_a = quat(R_a): the branch on the largest of trace, m00, m11, m22, then normalised
        const m = Ra, tr = m[0] + m[4] + m[8]
        let qx, qy, qz, qw
        if (tr >= m[0] && tr >= m[4] && tr >= m[8]) {
          const s = Math.sqrt(tr + 1) * 2
          qw = 0.25 * s; qx = (m[7] - m[5]) / s; qy = (m[2] - m[6]) / s; qz = (m[3] - m[1]) / s
        } else if (m[0] >= m[4] && m[0] >= m[8]) {
          const s = Math.sqrt(1 + m[0] - m[4] - m[8]) * 2
          qw = (m[7] - m[5]) / s; qx = 0.25 * s; qy = (m[1] + m[3]) / s; qz = (m[2] + m[6]) / s
        } else if (m[4] >= m[8]) {
          const s = Math.sqrt(1 + m[4] - m[0] - m[8]) * 2
          qw = (m[2] - m[6]) / s; qx = (m[1] + m[3]) / s; qy = 0.25 * s; qz = (m[5] + m[7]) / s
        } else {
          const s = Math.sqrt(1 + m[8] - m[0] - m[4]) * 2
          qw = (m[3] - m[1]) / s; qx = (m[2] + m[6]) / s; qy = (m[5] + m[7]) / s; qz = 0.25 * s
        }
        const il = 1 / Math.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
        qx *= il; qy *= il; qz *= il; qw *= il
        const raw = bone.appendRatio === undefined || bone.appendRatio === null ? 1 : Math.fround(bone.appendRatio)
        const ratio = Math.max(-1, Math.min(1, raw))
        if (bone.appendMove) { ax = ta[0] * raw; ay = ta[1] * raw; az = ta[2] * raw }
        if (ratio < 0) { qx = -qx; qy = -qy; qz = -qz }
        // Quat.slerp(identity, q_a, |ratio|): the shorter arc
        const t = Math.abs(ratio)
        let c = qw
        if (c < 0) { c = -c; qx = -qx; qy = -qy; qz = -qz; qw = -qw }
        let sx, sy, sz, sw
        if (c > 0.9995) {
          sx = t * qx; sy = t * qy; sz = t * qz; sw = 1 + t * (qw - 1)
          const l = 1 / Math.sqrt(sx * sx + sy * sy + sz * sz + sw * sw)
          sx *= l; sy *= l; sz *= l; sw *= l
        } else {
          const th0 = Math.acos(c), sn = Math.sin(th0), th = th0 * t
          const s0 = Math.sin(th0 - th) / sn, s1 = Math.sin(th) / sn
          sx = s1 * qx; sy = s1 * qy; sz = s1 * qz; sw = s0 + s1 * qw
        }
        R = mul3(qmat(sx, sy, sz, sw), R)
      }
      const bt = bone.bindTranslation
      let tx = bt[0], ty = bt[1], tz = bt[2]
      if (useT) { tx += tra[b * 3]; ty += tra[b * 3 + 1]; tz += tra[b * 3 + 2] }
      tx += R[0] * ax + R[1] * ay + R[2] * az; ty += R[3] * ax + R[4] * ay + R[5] * az; tz += R[6] * ax + R[7] * ay + R[8] * az
      let W = R, px = tx, py = ty, pz = tz
      if (bone.parentIndex >= 0) {
        const P = rows(bone.parentIndex)
        W = mul3(P.R, R)
        px = P.R[0] * tx + P.R[1] * ty + P.R[2] * tz + P.p[0]; py = P.R[3] * tx + P.R[4] * ty + P.R[5] * tz + P.p[1]; pz = P.R[6] * tx + P.R[7] * ty + P.R[8] * tz + P.p[2]
      }
      const o = b * 16
      world[o] = W[0]; world[o + 1] = W[3]; world[o + 2] = W[6]; world[o + 3] = 0
      world[o + 4] = W[1]; world[o + 5] = W[4]; world[o + 6] = W[7]; world[o + 7] = 0
      world[o + 8] = W[2]; world[o + 9] = W[5]; world[o + 10] = W[8]; world[o + 11] = 0
      world[o + 12] = px; world[o + 13] = py; world[o + 14] = pz; world[o + 15] = 1
    }
  }

  /**
   * PMX inverse kinematics on the host: CCD in the clamp form, the arithmetic of tests/ik_ref.py (the definition; GPU twin:
   * csrc/kernels/ik.hip.h) in doubles, the solved rotations stored to a Float32Array pose copy like posedLocals() does for bone
   * morphs - the runtime's tween and animation state is never overwritten. Chains in ascending order of the IK bone; per iteration and
   * link L (file order: effector outwards): a, b = effector and goal in L's frame, q[L] = normalize(clamp(q[L] * quat(a x b,
   * min(atan2(|a x b|, a . b), limitAngle)))), Euler limits in three.js 'XYZ' order; the bones that depend on q[L] are re-solved after
   * every link. Returns the local pose computeWorldMatrices() then solves; called from there only when IK is on.
   */
  solveIK(): PosedLocals {
    const src = this.posedLocals()
    const bones = this.skeleton.bones, n = bones.length
    const useT = this.applyLocalTranslations || src.moved
    if (this.ikRotations.length !== n * 4) {
      this.ikRotations = new Float32Array(n * 4); this.ikTranslations = new Float32Array(n * 3)
      this._ikR = new Float64Array(n * 9); this._ikP = new Float64Array(n * 3)
    }
    const rot = this.ikRotations, tra = this.ikTranslations, R = this._ikR, P = this._ikP
    rot.set(src.rot)
    if (useT) tra.set(src.tra); else tra.fill(0)
    const sq = this._q
    const M = new Float64Array(9), A = new Float64Array(9), X = new Float64Array(9)
    const qmat = (o, x, y, z, w) => {
      const x2 = x + x, y2 = y + y, z2 = z + z
      const xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2, wx = w * x2, wy = w * y2, wz = w * z2
      o[0] = 1 - (yy + zz); o[1] = xy - wz; o[2] = xz + wy
      o[3] = xy + wz; o[4] = 1 - (xx + zz); o[5] = yz - wx
      o[6] = xz - wy; o[7] = yz + wx; o[8] = 1 - (xx + yy)
    }
    const solveBone = (i) => {
      const b = bones[i]
      qmat(M, rot[i * 4], rot[i * 4 + 1], rot[i * 4 + 2], rot[i * 4 + 3])
      let ax = 0, ay = 0, az = 0
      const ap = b.appendParentIndex
      if (b.appendRotate && ap !== undefined && ap !== null && ap >= 0 && ap < n) {
        const ratio = b.appendRatio === undefined || b.appendRatio === null ? 1 : Math.max(-1, Math.min(1, b.appendRatio))
        if (Math.abs(ratio) > 1e-6) {
          let qx = rot[ap * 4], qy = rot[ap * 4 + 1], qz = rot[ap * 4 + 2]
          if (ratio < 0) { qx = -qx; qy = -qy; qz = -qz }
          slerpInto(sq, 0, 0, 0, 1, qx, qy, qz, rot[ap * 4 + 3], Math.abs(ratio))
          qmat(A, sq[0], sq[1], sq[2], sq[3])
          for (let r = 0; r < 3; r++) for (let c = 0; c < 3; c++) X[r * 3 + c] = A[r * 3] * M[c] + A[r * 3 + 1] * M[3 + c] + A[r * 3 + 2] * M[6 + c]
          M.set(X)
          if (b.appendMove) {
            const rr = b.appendRatio === undefined || b.appendRatio === null ? 1 : b.appendRatio
            ax = tra[ap * 3] * rr; ay = tra[ap * 3 + 1] * rr; az = tra[ap * 3 + 2] * rr
          }
        }
      }
      const tx = b.bindTranslation[0] + tra[i * 3] + (M[0] * ax + M[1] * ay + M[2] * az)
      const ty = b.bindTranslation[1] + tra[i * 3 + 1] + (M[3] * ax + M[4] * ay + M[5] * az)
      const tz = b.bindTranslation[2] + tra[i * 3 + 2] + (M[6] * ax + M[7] * ay + M[8] * az)
      const p = b.parentIndex, o = i * 9
      if (p >= 0 && p < n) {
        const q = p * 9
        for (let r = 0; r < 3; r++) {
          for (let c = 0; c < 3; c++) X[r * 3 + c] = R[q + r * 3] * M[c] + R[q + r * 3 + 1] * M[3 + c] + R[q + r * 3 + 2] * M[6 + c]
          P[i * 3 + r] = R[q + r * 3] * tx + R[q + r * 3 + 1] * ty + R[q + r * 3 + 2] * tz + P[p * 3 + r]
        }
        for (let k = 0; k < 9; k++) R[o + k] = X[k]
      } else {
        for (let k = 0; k < 9; k++) R[o + k] = M[k]
        P[i * 3] = tx; P[i * 3 + 1] = ty; P[i * 3 + 2] = tz
      }
    }
    const dependents = (L) => {
      let d = this._ikDeps[L]
      if (d) return d
      const hit = new Uint8Array(n)
      d = []
      for (let k = 0; k < n; k++) {      // parent-first order: a bone depends on q[L] if it is L, appends from L, or its parent does
        const i = this.solveOrder[k], b = bones[i]
        const p = b.parentIndex
        if (i === L || (b.appendRotate && b.appendParentIndex === L) || (p >= 0 && p < n && hit[p])) { hit[i] = 1; d.push(i) }
      }
      this._ikDeps[L] = d
      return d
    }
    for (let k = 0; k < n; k++) solveBone(this.solveOrder[k])
    const v = [0, 0, 0, 0, 0, 0]
    const chains = this.getIKChains()
    for (let ci = 0; ci < chains.length; ci++) {
      if (this.ikChainOn && !this.ikChainOn[ci]) continue      // switched off: its links keep the posed rotations
      const ch = chains[ci]
      const G = ch.goal, E = ch.effector
      for (let it = 0; it < ch.loops; it++) {
        let rotated = false
        for (const link of ch.links) {
          const L = link.bone, o = L * 9
          for (let s = 0; s < 2; s++) {          // v[0..2] = Rw^T (E - L), v[3..5] = Rw^T (G - L)
            const T = s === 0 ? E : G
            const dx = P[T * 3] - P[L * 3], dy = P[T * 3 + 1] - P[L * 3 + 1], dz = P[T * 3 + 2] - P[L * 3 + 2]
            for (let c = 0; c < 3; c++) v[s * 3 + c] = R[o + c] * dx + R[o + 3 + c] * dy + R[o + 6 + c] * dz
          }
          const la = Math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), lb = Math.sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5])
          if (la < 1e-6 || lb < 1e-6) continue
          const ax = v[0] / la, ay = v[1] / la, az = v[2] / la, bx = v[3] / lb, by = v[4] / lb, bz = v[5] / lb
          const cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx
          const nn = Math.sqrt(cx * cx + cy * cy + cz * cz)
          if (nn < 1e-7) continue
          const ang = Math.min(Math.atan2(nn, ax * bx + ay * by + az * bz), ch.limitAngle)
          const sn = Math.sin(ang * 0.5) / nn, rx = cx * sn, ry = cy * sn, rz = cz * sn, rw = Math.cos(ang * 0.5)
          const x = rot[L * 4], y = rot[L * 4 + 1], z = rot[L * 4 + 2], w = rot[L * 4 + 3]      // Hamilton product q[L] * dq
          let qx = w * rx + x * rw + y * rz - z * ry, qy = w * ry - x * rz + y * rw + z * rx
          let qz = w * rz + x * ry - y * rx + z * rw, qw = w * rw - x * rx - y * ry - z * rz
          if (link.min && link.max) {
            qmat(M, qx, qy, qz, qw)
            let e1 = Math.asin(Math.max(-1, Math.min(1, M[2]))), e0, e2
            if (Math.abs(M[2]) < 0.9999999) { e0 = Math.atan2(-M[5], M[8]); e2 = Math.atan2(-M[1], M[0]) } else { e0 = Math.atan2(M[7], M[4]); e2 = 0 }
            const cl = (e, a) => Math.min(Math.max(e, Math.min(link.min[a], link.max[a])), Math.max(link.min[a], link.max[a]))
            e0 = cl(e0, 0); e1 = cl(e1, 1); e2 = cl(e2, 2)
            const c1 = Math.cos(e0 / 2), c2 = Math.cos(e1 / 2), c3 = Math.cos(e2 / 2), s1 = Math.sin(e0 / 2), s2 = Math.sin(e1 / 2), s3 = Math.sin(e2 / 2)
            qx = s1 * c2 * c3 + c1 * s2 * s3; qy = c1 * s2 * c3 - s1 * c2 * s3; qz = c1 * c2 * s3 + s1 * s2 * c3; qw = c1 * c2 * c3 - s1 * s2 * s3
          }
          const il = 1 / Math.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
          rot[L * 4] = qx * il; rot[L * 4 + 1] = qy * il; rot[L * 4 + 2] = qz * il; rot[L * 4 + 3] = qw * il
          rotated = true
          const dep = dependents(L)
          for (let k = 0; k < dep.length; k++) solveBone(dep[k])
        }
        const dx = P[G * 3] - P[E * 3], dy = P[G * 3 + 1] - P[E * 3 + 1], dz = P[G * 3 + 2] - P[E * 3 + 2]
        if (Math.sqrt(dx * dx + dy * dy + dz * dz) < 1e-4 || !rotated) break
      }
    }
    return { rot, tra, moved: true }
  }

  /** Pose every bone the sampler keys at `frame` (rotation + translation), and every morph it keys. Un-keyed bones keep their state. */
  applySampledFrame(sampler: VMDSampler, frame: number): void {
    if (this.ikKeys) this.applyIKState(sampler, frame)
    const rot = this.runtimeSkeleton.localRotations, tra = this.runtimeSkeleton.localTranslations
    this.applyLocalTranslations = true
    for (const name of sampler.boneNames()) {
      const idx = this.runtimeSkeleton.nameIndex[name]
      if (idx === undefined) continue
      const s = sampler.sampleBone(name, frame)
      rot[idx * 4] = s.rotation[0]; rot[idx * 4 + 1] = s.rotation[1]; rot[idx * 4 + 2] = s.rotation[2]; rot[idx * 4 + 3] = s.rotation[3]
      tra[idx * 3] = s.position[0]; tra[idx * 3 + 1] = s.position[1]; tra[idx * 3 + 2] = s.position[2]
      this.rotTweenState.active[idx] = 0
    }
    for (const name of sampler.morphNames()) {
      const w = sampler.sampleMorph(name, frame)
      if (w !== null) this.setMorphWeights([name], [w])
    }
  }

  /**
   * The host twin of rz_set_pose_blended (include/reze_deform.h; tests/motion_ref.py is the definition): A = samplerA at frameA and
   * B = samplerB at frameB, cross-faded by `blend` — rotations by Quat.slerp (kernels.slerpInto), translations and morph weights linearly.
   * A clip that does not key a bone or morph the other one keys counts as rest there (identity, zero translation, weight 0); a bone or
   * morph keyed by neither clip is left alone, as applySampledFrame leaves it. No samplerB or blend 0: exactly A (B is not sampled);
   * blend 1: exactly B. Group morphs are blended as raw weights: getEffectiveMorphWeights() is linear in them.
   */
  applyBlendedFrame(samplerA: VMDSampler, frameA: number, samplerB?: VMDSampler | null, frameB?: number, blend?: number): void {
    const t = samplerB && blend !== undefined && blend !== null ? blend : 0
    if (!(t >= 0 && t <= 1)) throw new Error('applyBlendedFrame: blend must be in [0, 1], got ' + blend)
    // IK switches do not cross-fade: clip A's at frameA below blend 0.5 (as float32, what the device is handed), clip B's at frameB from there on
    if (this.ikKeys) { if (samplerB && !(Math.fround(t) < 0.5)) this.applyIKState(samplerB, frameB === undefined || frameB === null ? 0 : frameB); else this.applyIKState(samplerA, frameA) }
    const rot = this.runtimeSkeleton.localRotations, tra = this.runtimeSkeleton.localTranslations
    this.applyLocalTranslations = true
    const fb = frameB === undefined || frameB === null ? 0 : frameB
    const bones = new Set(samplerA.boneNames())
    if (samplerB) for (const name of samplerB.boneNames()) bones.add(name)
    const rest = { rotation: [0, 0, 0, 1], position: [0, 0, 0] }
    const q = [0, 0, 0, 1]
    for (const name of bones) {
      const idx = this.runtimeSkeleton.nameIndex[name]
      if (idx === undefined) continue
      const a = t < 1 ? samplerA.sampleBone(name, frameA) || rest : rest
      const b = t > 0 ? samplerB.sampleBone(name, fb) || rest : rest
      let r = a.rotation, p = a.position
      if (t === 1) { r = b.rotation; p = b.position }
      else if (t > 0) {
        r = slerpInto(q, a.rotation[0], a.rotation[1], a.rotation[2], a.rotation[3], b.rotation[0], b.rotation[1], b.rotation[2], b.rotation[3], t)
        p = [a.position[0] + (b.position[0] - a.position[0]) * t, a.position[1] + (b.position[1] - a.position[1]) * t, a.position[2] + (b.position[2] - a.position[2]) * t]
      }
      rot[idx * 4] = r[0]; rot[idx * 4 + 1] = r[1]; rot[idx * 4 + 2] = r[2]; rot[idx * 4 + 3] = r[3]
      tra[idx * 3] = p[0]; tra[idx * 3 + 1] = p[1]; tra[idx * 3 + 2] = p[2]
      this.rotTweenState.active[idx] = 0
    }
    const morphs = new Set(samplerA.morphNames())
    if (samplerB) for (const name of samplerB.morphNames()) morphs.add(name)
    for (const name of morphs) {
      const wa = t < 1 ? samplerA.sampleMorph(name, frameA) || 0 : 0
      const wb = t > 0 ? samplerB.sampleMorph(name, fb) || 0 : 0
      this.setMorphWeights([name], [t === 0 ? wa : t === 1 ? wb : wa + (wb - wa) * t])
    }
  }

  /** effective weights (own track, then the group tracks that list the morph) of one sampler at `frame` into w, driven[i] = 1 where a feed of morph i holds a key: what VMDSampler.flatten() lays out for the device */
  _sampleEffective(sampler: VMDSampler, frame: number, w: Float64Array, driven: Uint8Array): void {
    w.fill(0); driven.fill(0)
    if (!this.morphs) return
    const { names, types, groups } = this.morphs
    for (let i = 0; i < names.length; i++) {
      if (types[i] !== 1 && types[i] !== 2) continue
      const own = sampler.sampleMorph(names[i], frame)
      if (own !== null) { w[i] += own; driven[i] = 1 }
    }
    for (let g = 0; g < names.length; g++) {
      if (types[g] !== 0 || !groups[g]) continue
      const wg = sampler.sampleMorph(names[g], frame)
      if (wg === null) continue
      for (const [child, ratio] of groups[g]) if (types[child] === 1 || types[child] === 2) { w[child] += wg * ratio; driven[child] = 1 }
    }
  }

  /**
   * The host twin of rz_set_pose_layered (include/reze_deform.h; tests/layer_ref.py is the definition). `base` is applyBlendedFrame's state
   * { a, frameA, b?, frameB?, blend? } with samplers for a and b; `layers` are { sampler, frame, weight = 1, mask = null, additive = false }
   * applied in order, `mask` a key of `masks` (name -> { bones: Uint8Array[B], morphs: Uint8Array[M] | null }). A layer without a sampler or
   * with weight 0 is skipped. A layer acts on a bone only where its clip keys the bone and the mask includes it — override: slerp / lerp
   * towards the layer's sample (the sample itself at weight 1); additive: q * slerp(identity, qL, weight), t + tL * weight — and on a
   * vertex or bone morph only where the clip keys the morph or a group morph that lists it and the mask includes it, on the EFFECTIVE
   * weights. A clip that does not key a bone or morph another one keys counts as rest there; a bone or morph that no clip keys is left
   * alone, as applyBlendedFrame leaves it. Morphs are written back as own weights: a group morph some clip keys is set to 0 and what it
   * fed is carried by the morphs it lists, so that getEffectiveMorphWeights() gives the layered weights.
   */
  applyLayeredFrame(base: LayeredBase, layers: HostLayer[], masks?: Record<string, HostMask> | null): void {
    const t = base.b && base.blend !== undefined && base.blend !== null ? base.blend : 0
    if (!(t >= 0 && t <= 1)) throw new Error('applyLayeredFrame: blend must be in [0, 1], got ' + base.blend)
    if (layers.length > 4) throw new Error('applyLayeredFrame: ' + layers.length + ' layers, at most 4')
    // (layers never switch IK: the base state chooses, as in applyBlendedFrame)
    if (this.ikKeys) { if (base.b && !(Math.fround(t) < 0.5)) this.applyIKState(base.b, base.frameB === undefined || base.frameB === null ? 0 : base.frameB); else this.applyIKState(base.a, base.frameA) }
    const live = []
    layers.forEach((l, k) => {
      if (!l.sampler || l.weight === 0) return
      const w = l.weight === undefined || l.weight === null ? 1 : l.weight
      if (!(w >= 0 && w <= 1)) throw new Error('applyLayeredFrame: layer ' + k + ': weight must be in [0, 1], got ' + l.weight)
      if (!Number.isFinite(l.frame)) throw new Error('applyLayeredFrame: layer ' + k + ': the frame is not finite')
      let mask = null
      if (l.mask !== undefined && l.mask !== null) {
        mask = masks ? masks[l.mask] : undefined
        if (!mask) throw new Error('applyLayeredFrame: layer ' + k + ': unknown mask "' + l.mask + '"')
      }
      live.push({ sampler: l.sampler, frame: l.frame, weight: w, mask, additive: !!l.additive })
    })
    const rot = this.runtimeSkeleton.localRotations, tra = this.runtimeSkeleton.localTranslations
    this.applyLocalTranslations = true
    const fb = base.frameB === undefined || base.frameB === null ? 0 : base.frameB
    const useA = t < 1, useB = t > 0
    const bones = new Set(base.a.boneNames())
    if (base.b) for (const name of base.b.boneNames()) bones.add(name)
    for (const l of live) for (const name of l.sampler.boneNames()) bones.add(name)
    const rest = { rotation: [0, 0, 0, 1], position: [0, 0, 0] }
    const q = [0, 0, 0, 1], s = [0, 0, 0, 1]
    for (const name of bones) {
      const idx = this.runtimeSkeleton.nameIndex[name]
      if (idx === undefined) continue
      const a = useA ? base.a.sampleBone(name, base.frameA) || rest : rest
      const b = useB ? base.b.sampleBone(name, fb) || rest : rest
      let r = a.rotation.slice(), p = a.position.slice()
      if (t === 1) { r = b.rotation.slice(); p = b.position.slice() }
      else if (t > 0) {
        r = Array.from(slerpInto(q, a.rotation[0], a.rotation[1], a.rotation[2], a.rotation[3], b.rotation[0], b.rotation[1], b.rotation[2], b.rotation[3], t))
        p = [a.position[0] + (b.position[0] - a.position[0]) * t, a.position[1] + (b.position[1] - a.position[1]) * t, a.position[2] + (b.position[2] - a.position[2]) * t]
      }
      for (const l of live) {
        if (l.mask && !l.mask.bones[idx]) continue
        const o = l.sampler.sampleBone(name, l.frame)
        if (!o) continue
        const w = l.weight, lr = o.rotation, lp = o.position
        if (l.additive) {
          slerpInto(s, 0, 0, 0, 1, lr[0], lr[1], lr[2], lr[3], w)
          const x = r[0], y = r[1], z = r[2], ww = r[3]      // Hamilton product r * s (Quat.multiply)
          r = [ww * s[0] + x * s[3] + y * s[2] - z * s[1], ww * s[1] - x * s[2] + y * s[3] + z * s[0], ww * s[2] + x * s[1] - y * s[0] + z * s[3], ww * s[3] - x * s[0] - y * s[1] - z * s[2]]
          p = [p[0] + lp[0] * w, p[1] + lp[1] * w, p[2] + lp[2] * w]
        } else if (w === 1) {
          r = lr.slice(); p = lp.slice()
        } else {
          r = Array.from(slerpInto(q, r[0], r[1], r[2], r[3], lr[0], lr[1], lr[2], lr[3], w))
          p = [p[0] + (lp[0] - p[0]) * w, p[1] + (lp[1] - p[1]) * w, p[2] + (lp[2] - p[2]) * w]
        }
      }
      rot[idx * 4] = r[0]; rot[idx * 4 + 1] = r[1]; rot[idx * 4 + 2] = r[2]; rot[idx * 4 + 3] = r[3]
      tra[idx * 3] = p[0]; tra[idx * 3 + 1] = p[1]; tra[idx * 3 + 2] = p[2]
      this.rotTweenState.active[idx] = 0
    }
    if (!this.morphs) return
    const M = this.morphs.names.length, types = this.morphs.types
    const w = new Float64Array(M), wl = new Float64Array(M), any = new Uint8Array(M), dl = new Uint8Array(M)
    if (useA) { this._sampleEffective(base.a, base.frameA, wl, dl); for (let i = 0; i < M; i++) { w[i] = wl[i]; any[i] |= dl[i] } }
    if (useB) {
      this._sampleEffective(base.b, fb, wl, dl)
      for (let i = 0; i < M; i++) { w[i] = t === 1 ? wl[i] : w[i] + (wl[i] - w[i]) * t; any[i] |= dl[i] }
    }
    // (a base clip that is not sampled still keys its morphs: they are at rest, not left alone — as in applyBlendedFrame)
    const keyedBy = (smp) => {
      const names = new Set(smp.morphNames())
      for (let i = 0; i < M; i++) {
        if (!names.has(this.morphs.names[i])) continue
        if (types[i] === 1 || types[i] === 2) any[i] = 1
        else if (types[i] === 0 && this.morphs.groups[i]) for (const [child] of this.morphs.groups[i]) if (types[child] === 1 || types[child] === 2) any[child] = 1
      }
      return names
    }
    const groupsKeyed = new Set()
    const samplers = [base.a].concat(base.b ? [base.b] : [], live.map((l) => l.sampler))
    for (const smp of samplers) for (const name of keyedBy(smp)) { const g = this.morphNameIndex[name]; if (g !== undefined && types[g] === 0) groupsKeyed.add(g) }
    for (const l of live) {
      this._sampleEffective(l.sampler, l.frame, wl, dl)
      for (let i = 0; i < M; i++) {
        if (!dl[i] || (l.mask && l.mask.morphs && !l.mask.morphs[i])) continue
        if (l.additive) w[i] = w[i] + wl[i] * l.weight
        else w[i] = l.weight === 1 ? wl[i] : w[i] + (wl[i] - w[i]) * l.weight
      }
    }
    for (const g of groupsKeyed) this.morphWeights[g] = 0
    const now = Float64Array.from(this.getEffectiveMorphWeights())      // what the group morphs no clip keys still feed
    for (let i = 0; i < M; i++) if (any[i]) this.morphWeights[i] += w[i] - now[i]
  }

  // ---- morphs (no reference counterpart; PMX layout per pmx-loader.ts:471-488) ----
  getMorphNames(): string[] { return this.morphs ? this.morphs.names.slice() : [] }
  getMorphCount(): number { return this.morphs ? this.morphs.names.length : 0 }
  getMorphs(): MorphSet | null { return this.morphs }

  /** names or indices + weights; unknown names are ignored like unknown bones in rotateBones. */
  setMorphWeights(namesOrIndices: Array<string | number>, weights: ArrayLike<number>): void {
    if (!this.morphs) return
    for (let i = 0; i < namesOrIndices.length; i++) {
      const key = namesOrIndices[i]
      const idx = typeof key === 'number' ? key : this.morphNameIndex[key]
      if (idx === undefined || idx < 0 || idx >= this.morphWeights.length) continue
      this.morphWeights[idx] = weights[i]
    }
  }

  getMorphWeights(): Float32Array { return this.morphWeights }

  /**
   * Weights the deformation consumes: vertex morphs (type 1) and bone morphs (type 2) keep their own weight plus, for
   * every group morph (type 0) that lists them, w_group * ratio (pmx-loader.ts:479-482). Other morph types
   * (UV / material / flip / impulse) touch neither positions nor bones and contribute nothing.
   */
  getEffectiveMorphWeights(): Float32Array { return this._flattenGroups(this.effectiveMorphWeights, 1, 2) }

  // own weight of the morphs whose type lies in [lo, hi], plus what group morphs feed them
  _flattenGroups(out: Float32Array, lo: number, hi: number): Float32Array {
    if (!this.morphs) return out
    const { types, groups } = this.morphs
    const w = this.morphWeights
    for (let i = 0; i < out.length; i++) out[i] = types[i] >= lo && types[i] <= hi ? w[i] : 0
    for (let g = 0; g < out.length; g++) {
      if (types[g] !== 0 || w[g] === 0 || !groups[g]) continue
      for (const [child, ratio] of groups[g]) {
        if (child >= 0 && child < out.length && types[child] >= lo && types[child] <= hi) out[child] += w[g] * ratio
      }
    }
    return out
  }

  /**
   * Texture coordinates with the UV morphs (PMX type 3) applied: uv + sum over entries of w_morph * (du, dv), ascending
   * morph order, f32. UVs never pass through the deformation kernel — vs() forwards them untouched (engine.ts:273) and a
   * renderer binds them from the static vertex buffer — so this is a sparse host-side update of a V x 2 array, not GPU
   * work. The reference has no counterpart (its loader skips the section, pmx-loader.ts:498-507).
   */
  getMorphedUVs(): Float32Array {
    const V = this.vertexCount
    if (!this._uv) this._uv = new Float32Array(V * 2)
    const uv = this._uv, vd = this.vertexData
    for (let v = 0; v < V; v++) { uv[v * 2] = vd[v * VERTEX_STRIDE + 6]; uv[v * 2 + 1] = vd[v * VERTEX_STRIDE + 7] }
    const ue = this.morphs && this.morphs.uvEntries
    if (!ue || ue.morph.length === 0) return uv
    if (!this._uvWeights) this._uvWeights = new Float32Array(this.morphWeights.length)
    const w = this._flattenGroups(this._uvWeights, 3, 3)
    for (let k = 0; k < ue.morph.length; k++) {
      const wk = w[ue.morph[k]]
      if (wk === 0) continue
      const v = ue.vertex[k]
      uv[v * 2] += wk * ue.delta[k * 2]; uv[v * 2 + 1] += wk * ue.delta[k * 2 + 1]
    }
    return uv
  }
}

export { Model, VERTEX_STRIDE }
