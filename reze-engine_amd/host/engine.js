'use strict'
/*
 * Source: host/src/engine.ts (TypeScript). host/engine.js is that file with its types erased (tools/ts_erase.py; no tsc in the image) - edit the .ts.
 * engine.js — the Engine class with the reference's public surface (engine/src/engine.ts:35-185,
 * 1419-1725): new Engine(canvas|null, options?), init(), loadModel(), loadAnimation(),
 * playAnimation(), stopAnimation(), rotateBones(), render(), runRenderLoop(), stopRenderLoop(),
 * getStats(), dispose(). What changes is what sits behind it: the WebGPU buffer uploads of
 * setupModelBuffers() (:1728-1832) and the per-frame writeBuffer + palette dispatch of
 * updateModelPose() (:2375-2402), and the skinning that the reference re-runs inside every vertex
 * shader invocation (:253-272), become calls into the HIP addon: upload once, then per frame
 * evaluatePose() on the CPU -> setPose(world matrices, morph weights) -> deform() on the MI355X.
 * Rendering (pipelines, bloom, camera, textures) and physics are out of scope and absent.
 *
 * Additions (SURVEY §8b): setMorphWeights(), getDeformed(), step(timeMs) — a deterministic clock
 * replacing performance.now()/window.setTimeout so a VMD can be stepped reproducibly — and
 * options { device, morphLayout: 'sparse'|'dense', realtime }.
 */
const { Quat, Vec3 } = require('./math')
const { PmxLoader } = require('./pmx-loader')
const { VMDLoader } = require('./vmd-loader')
const { VMDSampler } = require('./vmd-sampler')
const { requireAddon } = require('./addon')

let wallClock
try {
  const { performance } = require('perf_hooks')
  wallClock = () => performance.now()
} catch (e) {
  wallClock = () => Date.now()
}
// the reference's fixedTimeStep and maxSubSteps (physics.ts:534-569); h = 0 in the upload selects the same 1/75 s on the device
const PHYSICS_H = 1 / 75, PHYSICS_MAX_SUBSTEPS = 10

class Engine {
  constructor(canvas, options) {
    this.canvas = canvas || null // accepted for signature compatibility; nothing is drawn
    const o = options || {}
    // render-only options are accepted and kept so existing call sites keep working (engine.ts:145-154)
    this.ambient = o.ambient === undefined ? 1.0 : o.ambient
    this.bloomIntensity = o.bloomIntensity === undefined ? 0.12 : o.bloomIntensity
    this.rimLightIntensity = o.rimLightIntensity === undefined ? 0.45 : o.rimLightIntensity
    this.cameraDistance = o.cameraDistance === undefined ? 26.6 : o.cameraDistance
    this.cameraTarget = o.cameraTarget === undefined ? new Vec3(0, 12.5, 0) : o.cameraTarget
    this.device = o.device === undefined ? 0 : o.device
    // devices: [0,1,...]  one context per GPU in this process; the mesh is vertex-sharded across them (SURVEY §8e)
    this.devices = Array.isArray(o.devices) && o.devices.length > 0 ? o.devices.slice() : [this.device]
    this.deviceFK = o.deviceFK === true // forward kinematics on the GPU: upload local rotations instead of world matrices
    this.outline = o.outline === true // also produce the outline pass's inverted hull (engine.ts:458-461) every frame
    this.bounds = o.bounds === true // also reduce the deformed mesh's bounding box every frame
    // SDEF vertices (PMX weight type 3) skinned as MMD does; off (the default), they are skinned as BDEF2 like the reference does
    this.sdef = o.sdef === true
    // QDEF vertices (PMX 2.1 weight type 4) blended as dual quaternions; off (the default), they are skinned as BDEF4 like the reference does
    this.qdef = o.qdef === true
    this.ik = o.ik === true // PMX inverse kinematics: off unless asked for (device solve with deviceFK, else Model.solveIK on the host)
    // gather: true = RCCL all-gather of the deformed mesh after every frame (needs distinct GPUs);
    // 'direct' = every shard's kernel stores straight into GPU devices[0]'s buffer over xGMI (no collective)
    this.gather = o.gather === 'direct' ? 'direct' : o.gather === true
    this.morphLayout = o.morphLayout || 'sparse'
    this.realtime = o.realtime !== false // false: time only advances through step()
    // physics hand-off (engine.ts:2379-2381): an object with the reference Physics' step(dt, worldMats, inverseBind),
    // called between evaluatePose() and the world-matrix upload; it may overwrite world matrices in place. Physics
    // itself (Bullet via @fred3d/ammo) is out of scope — this is only the seam it plugs into.
    this.physics = o.physics || null
    this.lastPhysicsTime = null
    // devicePhysics: the model's PMX rigid bodies and joints simulated on the GPU (rz_upload_physics / rz_physics_step), which writes the
    // override table there. It acts on device-solved poses only, and a host { physics } would fight it over the same bones.
    this.devicePhysics = o.devicePhysics === true
    if (this.devicePhysics && !this.deviceFK) throw new Error('devicePhysics needs new Engine(canvas, { deviceFK: true }); with host FK pass { physics }')
    if (this.devicePhysics && this.physics) throw new Error('devicePhysics and { physics } are exclusive: both would write the physics-driven bones')
    // physicsContacts: contacts between the table's spheres and capsules (rz_physics_contacts), enabled on every shard behind the upload;
    // 'boxes': its boxes take part as well; 'all': and its boxes meet each other
    this.physicsContacts = o.physicsContacts === 'boxes' || o.physicsContacts === 'all' ? o.physicsContacts : o.physicsContacts === true
    if (this.physicsContacts && !this.devicePhysics) throw new Error('physicsContacts needs new Engine(canvas, { deviceFK: true, devicePhysics: true })')
    // physicsSprings: the linear springs of the table's joints (PMX spring_position; rz_physics_springs), enabled on every shard behind the
    // upload and ahead of the contacts
    this.physicsSprings = o.physicsSprings === true
    if (this.physicsSprings && !this.devicePhysics) throw new Error('physicsSprings needs new Engine(canvas, { deviceFK: true, devicePhysics: true })')
    // physicsAligned: the table's PMX type-2 bodies are simulated and their bones keep their animated positions (rz_physics_aligned), enabled
    // on every shard right behind the table's upload, ahead of the springs and the contacts (it rebuilds what the upload derived)
    this.physicsAligned = o.physicsAligned === true
    if (this.physicsAligned && !this.devicePhysics) throw new Error('physicsAligned needs new Engine(canvas, { deviceFK: true, devicePhysics: true })')
    // followOverrides: bones below an overridden bone follow it (rz_override_follow; the definition is tests/follow_ref.py), for the
    // overrides devicePhysics writes and for those fed through setBoneWorldOverrides; set on every shard behind the topology upload, and
    // on every fork. The stage is the device hierarchy solve's: host FK users call Model.followOverrides from their { physics } hook.
    this.followOverrides = o.followOverrides === true
    if (this.followOverrides && !this.deviceFK) throw new Error('followOverrides needs new Engine(canvas, { deviceFK: true }); with host FK call Model.followOverrides from the { physics } hook')
    // afterPhysics: the model's PMX after-physics bones (flag 0x1000) are solved again behind the overrides, from the final pose of the bones
    // they read (rz_upload_after_physics; the definition is tests/after_ref.py): Model.afterPhysicsOrder() goes up on every shard behind
    // the topology upload — behind the IK table when both are on — and forks borrow it with the rest of the static data. The stage is the
    // device frame's: host FK users call Model.solveAfterPhysics at the end of their { physics } hook.
    this.afterPhysics = o.afterPhysics === true
    if (this.afterPhysics && !this.deviceFK) throw new Error('afterPhysics needs new Engine(canvas, { deviceFK: true }); with host FK call Model.solveAfterPhysics(world, overriddenBones) from the { physics } hook')
    // ikKeys: honour the motion's VMD show / IK keys, which switch single IK chains off and on over time (tests/ik_switch_ref.py is the
    // definition). Host path: seekFrame / playAnimation / seekMotions set the model's chain switches before the pose solve. Device path:
    // the keys are uploaded behind the motion (rz_upload_ik_keys) and the sampling pose calls evaluate them; host-sampled frames of
    // { deviceFK } send the model's switches with the pose (rz_set_ik_enabled). Off by default: a motion with such keys plays as before.
    this.ikKeys = o.ikKeys === true
    if (this.ikKeys && !this.ik) throw new Error('ikKeys needs new Engine(canvas, { ik: true }): the keys switch chains of the IK solve')
    // crowdMorphs: a crowd (setInstanceCount) of a model with vertex morphs takes the crowd skin kernels, which walk each vertex's morph
    // row once per pose of a group (tuning key inst_morphs = 1), instead of the single-mesh kernel run once per instance; set on every
    // shard behind setInstanceCount and on every fork. The frames are the same bits either way. Off by default.
    this.crowdMorphs = o.crowdMorphs === true
    this.ikManual = null // setIKEnabled(): [instances][chains], 1 / 0 = held on / off by hand, -1 = left to the motion
    this.ikManualSent = new WeakSet() // the contexts whose mask carries switches set by hand
    this.physicsAccumulator = 0 // seconds of clock advance not yet turned into substeps
    this.physicsResident = false
    this.native = null
    // deviceSampling (needs deviceFK): seekFrame() sends one float — the frame — and the motion is sampled on the GPU
    this.deviceSampling = o.deviceSampling === true && o.deviceFK === true
    this.instances = 1
    this.animationOnDevice = null
    // the motion library (loadMotion / seekMotions): name -> sampler; a clip's index on the device is its position in this map
    this.motions = new Map()
    this.motionsVersion = 0
    this.motionsOnDevice = -1
    this.motionsFor = null
    // the masks of layered motion states (setMotionMask): name -> spec; a mask's index on the device is its position in this map
    this.motionMasks = new Map()
    this.masksVersion = 0
    this.masksOnDevice = -1
    this.masksFor = null
    // framesInFlight: 2 = consecutive frames alternate between the context and a fork of it (rz_fork: the fork borrows the
    // static buffers, owns its stream, pose slots and outputs), so the tail of frame f overlaps the launch ramp of frame
    // f + 1 — what a WebGPU queue does with consecutive command buffers (engine.ts:2124-2136 submits one per frame).
    // getDeformed() / getOutlineHull() / getBounds() read the frame rendered last. Single GPU, no gather.
    this.framesInFlight = o.framesInFlight === 2 ? 2 : 1
    this.overrides = null
    this.autotune = o.autotune === true // search launch shapes once, on the first rendered frame (rz_autotune)
    this.tuned = false
    this.ctx = null // context of shard 0 (the only one on a single GPU)
    this.shards = [] // [{ ctx, begin, count }]
    this.currentModel = null
    this.animationFrames = []
    this.hasAnimation = false
    this.playingAnimation = false
    this.timers = [] // { due, fn, id, handle }
    this.nextTimerId = 1
    this.animationTimers = []
    this.breathingTimer = null
    this.breathingBaseRotations = new Map()
    this.nowMs = 0 // manual clock value
    this.loopHandle = null
    this.renderLoopCallback = null
    this.stats = { fps: 0, frameTime: 0, gpuMemory: 0, deformMs: 0, vertsPerSec: 0, hbmGBps: 0 }
    this.frameTimeSamples = []
    this.frameTimeSum = 0
    this.framesSinceLastUpdate = 0
    this.lastFpsUpdate = 0
    this.outPos = null
    this.outNrm = null
  }

  now() { return this.realtime ? wallClock() : this.nowMs }

  // ---- lifecycle ----
  /** engine.ts:157-185: acquire the device. Throws when the addon or an MI355X is not available. */
  async init() {
    if (this.framesInFlight === 2 && (this.devices.length > 1 || this.gather)) throw new Error('framesInFlight: 2 needs a single GPU and no gather')
    if (this.framesInFlight === 2 && this.devicePhysics) throw new Error('devicePhysics steps one context: it cannot run with framesInFlight: 2 (rz_physics_step is refused while forks exist)')
    this.native = requireAddon()
    this.shards = this.devices.map((d) => ({ ctx: this.native.create(d), begin: 0, count: 0, fork: null, last: null, flip: 0 }))
    this.ctx = this.shards[0].ctx
    this.lastFpsUpdate = this.now()
  }

  dispose() {
    this.stopRenderLoop()
    this.stopAnimation()
    this.stopBreathing()
    this.dropForks()
    for (const s of this.shards) this.native.destroy(s.ctx)
    this.shards = []
    this.ctx = null
  }

  // ---- frames in flight ----
  /** Forks borrow the lender's static buffers: they go before anything static is replaced, and before the lender. */
  dropForks() {
    for (const s of this.shards) {
      if (s.fork) { this.native.destroy(s.fork); s.fork = null }
      s.last = null
      s.flip = 0
    }
  }

  /** The context the NEXT frame of shard `s` runs on. */
  frameContext(s) {
    if (this.framesInFlight !== 2 || (this.autotune && !this.tuned)) { s.last = s.ctx; return s.ctx }
    if (!s.fork) { // made after the launch-shape search, so that it inherits the tuned plan
      s.fork = this.native.fork(s.ctx)
      if (this.followOverrides) this.native.overrideFollow(s.fork, 1) // (rz_fork hands the flag down already: said again, so a fork never depends on when its lender was set)
      if (this.crowdMorphs) this.native.setTuning(s.fork, 'inst_morphs', 1) // (a fork inherits its lender's tuning: said again for the same reason)
      if (this.overrides) this.native.overrideWorld(s.fork, this.overrides[0], this.overrides[1], this.overrides[2])
    }
    s.flip ^= 1
    s.last = s.flip ? s.fork : s.ctx
    return s.last
  }

  // ---- timers (window.setTimeout replacement that also works on a manual clock) ----
  setTimer(fn, delayMs) {
    const t = { due: this.now() + delayMs, fn, id: this.nextTimerId++, handle: null }
    if (this.realtime) t.handle = setTimeout(() => { this.dropTimer(t.id); fn() }, delayMs)
    this.timers.push(t)
    return t.id
  }

  dropTimer(id) {
    const i = this.timers.findIndex((t) => t.id === id)
    if (i >= 0) { if (this.timers[i].handle) clearTimeout(this.timers[i].handle); this.timers.splice(i, 1) }
  }

  fireDueTimers() {
    for (;;) { // earliest first; a callback may schedule more
      let best = -1
      for (let i = 0; i < this.timers.length; i++) {
        if (this.timers[i].due <= this.nowMs && (best < 0 || this.timers[i].due < this.timers[best].due)) best = i
      }
      if (best < 0) return
      const t = this.timers.splice(best, 1)[0]
      t.fn()
    }
  }

  // ---- model ----
  /** engine.ts:1704-1721 */
  async loadModel(path) {
    const parts = path.split('/')
    parts.pop()
    this.modelDir = parts.join('/') + '/'
    const model = await PmxLoader.load(path)
    await this.setupModelBuffers(model)
  }

  /** engine.ts:1728-1832: one-off static upload (vertex / joints / weights / inverse bind [+ morph targets]). */
  async setupModelBuffers(model) {
    if (!this.ctx) throw new Error('Engine.init() has not been called')
    this.dropForks()
    this.overrides = null // they name bones of the previous model; the library drops its copy with the skeleton (rz_upload_skeleton)
    this.currentModel = model
    model.setClock(() => this.now())
    model.setIKKeys(this.ikKeys)
    this.ikManual = null
    model.setIK(this.ik && !this.deviceFK) // host solve: only without the device hierarchy (a model without IK bones: a no-op)
    const n = this.native, skinning = model.getSkinning(), skeleton = model.getSkeleton()
    const morphs = model.getMorphs()
    const V = model.getVertexCount()
    const G = this.shards.length
    const tables = this.devicePhysics ? model.physicsTables() : null
    this.physicsResident = false
    for (let r = 0; r < G; r++) {
      const s = this.shards[r]
      const range = n.shardRange(V, G, r)
      s.begin = range[0]; s.count = range[1]
      if (s.count === 0) continue
      const b = s.begin, e = s.begin + s.count
      // static data is cut once; subarray() views are zero-copy into the addon
      n.uploadMesh(s.ctx, model.getVertices().subarray(b * 8, e * 8), skinning.joints.subarray(b * 4, e * 4), skinning.weights.subarray(b * 4, e * 4))
      n.uploadSkeleton(s.ctx, skeleton.inverseBindMatrices)
      if (this.deviceFK) {
        const B = skeleton.bones.length
        const parents = new Int32Array(B), bind = new Float32Array(B * 3), ap = new Int32Array(B).fill(-1), ar = new Float32Array(B).fill(1)
        const am = new Uint8Array(B)
        skeleton.bones.forEach((bn, i) => {
          parents[i] = bn.parentIndex
          bind.set(bn.bindTranslation, i * 3)
          if (bn.appendRotate && bn.appendParentIndex !== undefined && bn.appendParentIndex !== null) {
            ap[i] = bn.appendParentIndex
            ar[i] = bn.appendRatio === undefined || bn.appendRatio === null ? 1 : bn.appendRatio
            am[i] = bn.appendMove ? 1 : 0
          }
        })
        n.uploadSkeletonTopology(s.ctx, parents, bind, ap, ar, am)
        if (this.followOverrides) n.overrideFollow(s.ctx, 1) // a new topology cleared it
        // IK is per skeleton, not per vertex: every shard gets the same table, after the topology its chains are checked against
        const chains = this.ik ? model.getIKChains() : []
        if (chains.length > 0) {
          let nl = 0
          for (const ch of chains) nl += ch.links.length
          const goal = new Uint32Array(chains.length), eff = new Uint32Array(chains.length), loops = new Uint32Array(chains.length)
          const theta = new Float32Array(chains.length), off = new Uint32Array(chains.length + 1)
          const lb = new Uint32Array(nl), ll = new Uint8Array(nl), lmin = new Float32Array(nl * 3), lmax = new Float32Array(nl * 3)
          let e = 0
          chains.forEach((ch, k) => {
            goal[k] = ch.goal; eff[k] = ch.effector; loops[k] = ch.loops; theta[k] = ch.limitAngle
            for (const l of ch.links) {
              lb[e] = l.bone
              if (l.min && l.max) { ll[e] = 1; lmin.set(l.min, e * 3); lmax.set(l.max, e * 3) }
              e++
            }
            off[k + 1] = e
          })
          n.uploadIK(s.ctx, goal, eff, loops, theta, off, lb, ll, lmin, lmax)
        }
        // the after-physics bones in evaluation order: checked against the topology and the IK table just uploaded (a new topology cleared the list)
        if (this.afterPhysics) {
          const order = model.afterPhysicsOrder()
          if (order.length > 0) n.uploadAfterPhysics(s.ctx, Uint32Array.from(order))
        }
        // so is physics: every shard simulates the same bodies (the solve is deterministic), so no shard waits for another's overrides
        if (tables && tables.nBodies > 0) {
          n.uploadPhysics(s.ctx, tables)
          if (this.physicsAligned) n.physicsAligned(s.ctx, 1)
          if (this.physicsSprings) n.physicsSprings(s.ctx, 1)
          if (this.physicsContacts) n.physicsContacts(s.ctx, this.physicsContacts === 'all' ? 3 : this.physicsContacts === 'boxes' ? 2 : 1)
          this.physicsResident = true
        }
      }
      if (morphs && morphs.names.length > 0) {
        const M = morphs.names.length
        if (this.morphLayout === 'dense') {
          const dense = new Float32Array(M * s.count * 3)
          for (let m = 0; m < M; m++) {
            for (let k = morphs.offsets[m]; k < morphs.offsets[m + 1]; k++) {
              const v = morphs.vertexIndex[k]
              if (v < b || v >= e) continue
              const d = (m * s.count + (v - b)) * 3
              dense[d] += morphs.deltas[k * 3]; dense[d + 1] += morphs.deltas[k * 3 + 1]; dense[d + 2] += morphs.deltas[k * 3 + 2]
            }
          }
          n.uploadMorphsDense(s.ctx, M, dense)
        } else if (G === 1) {
          n.uploadMorphsSparse(s.ctx, morphs.offsets, morphs.vertexIndex, morphs.deltas)
        } else { // re-base the sparse entries that fall inside this shard
          const off = new Uint32Array(M + 1), vi = [], dl = []
          for (let m = 0; m < M; m++) {
            for (let k = morphs.offsets[m]; k < morphs.offsets[m + 1]; k++) {
              const v = morphs.vertexIndex[k]
              if (v >= b && v < e) { vi.push(v - b); dl.push(morphs.deltas[k * 3], morphs.deltas[k * 3 + 1], morphs.deltas[k * 3 + 2]) }
            }
            off[m + 1] = vi.length
          }
          n.uploadMorphsSparse(s.ctx, off, Uint32Array.from(vi), Float32Array.from(dl))
        }
        // PMX bone morphs: with the hierarchy solved on the GPU they are folded there (host FK: Model.posedLocals())
        const be = morphs.boneEntries
        if (this.deviceFK && be && be.morph.length > 0) n.uploadBoneMorphs(s.ctx, be.morph, be.bone, be.translation, be.rotation)
      }
      if (this.sdef) { // this shard's SDEF vertices, indices re-based to the shard (the table is sorted by vertex)
        const t = model.getSdef()
        let k0 = 0
        while (k0 < t.index.length && t.index[k0] < b) k0++
        let k1 = k0
        while (k1 < t.index.length && t.index[k1] < e) k1++
        const idx = new Uint32Array(k1 - k0)
        for (let k = k0; k < k1; k++) idx[k - k0] = t.index[k] - b
        n.uploadSdef(s.ctx, idx, t.c.slice(k0 * 3, k1 * 3), t.r0.slice(k0 * 3, k1 * 3), t.r1.slice(k0 * 3, k1 * 3))
      }
      if (this.qdef) { // this shard's QDEF vertices, re-based to the shard (the list is ascending)
        const q = model.getQdef()
        let k0 = 0
        while (k0 < q.length && q[k0] < b) k0++
        let k1 = k0
        while (k1 < q.length && q[k1] < e) k1++
        const idx = new Uint32Array(k1 - k0)
        for (let k = k0; k < k1; k++) idx[k - k0] = q[k] - b
        n.uploadQdef(s.ctx, idx)
      }
    }
    if (this.outline) {
      // per-vertex edge size = edgeSize of the material whose index range draws the vertex (edge flag 0x10), else 0
      const edge = new Float32Array(V)
      const indices = model.getIndices()
      let first = 0
      for (const mat of model.getMaterials()) {
        const size = (mat.edgeFlag & 0x10) !== 0 ? mat.edgeSize : 0
        for (let k = first; k < first + mat.vertexCount && k < indices.length; k++) edge[indices[k]] = size
        first += mat.vertexCount
      }
      this.edgeScale = edge
      for (const s of this.shards) if (s.count > 0) n.uploadEdgeScale(s.ctx, edge.subarray(s.begin, s.begin + s.count))
      this.outHull = new Float32Array(V * 3)
    }
    if (this.bounds) for (const s of this.shards) if (s.count > 0) n.enableAabb(s.ctx, true)
    if (this.gather === 'direct' && G > 1) n.gatherDirect(this.shards.map((s) => s.ctx), V, 0)
    else if (this.gather && G > 1) n.commInitAll(this.shards.map((s) => s.ctx), V)
    this.tuned = false
    this.physicsAccumulator = 0
    this.lastPhysicsTime = this.physicsResident ? this.now() : null
    this.outPos = new Float32Array(V * 3)
    this.outNrm = new Float32Array(V * 3)
    this.stats.gpuMemory = Math.round(((V * 60 + skeleton.bones.length * 176 +
      (morphs ? morphs.vertexIndex.length * 16 + V * 4 : 0)) / 1024 / 1024) * 100) / 100
  }

  rotateBones(bones, rotations, durationMs) {
    if (this.currentModel) this.currentModel.rotateBones(bones, rotations, durationMs)
  }

  /** uv with the UV morphs (PMX type 3) applied, V x 2 — host-side: UVs never pass through the deformation kernel (engine.ts:273) */
  getMorphedUVs() { return this.currentModel ? this.currentModel.getMorphedUVs() : new Float32Array(0) }

  setMorphWeights(namesOrIndices, weights) {
    if (this.currentModel) this.currentModel.setMorphWeights(namesOrIndices, weights)
  }

  // ---- animation ("VMD step", engine.ts:1419-1662) ----
  async loadAnimation(path) {
    this.animationFrames = await VMDLoader.load(path)
    this.hasAnimation = true
  }

  playAnimation(options) {
    if (this.animationFrames.length === 0) return
    this.stopAnimation()
    this.stopBreathing()
    this.playingAnimation = true
    const opt = options || {}
    let breathBones = []
    let breathRanges
    const enableBreath = opt.breathBones !== undefined && opt.breathBones !== null
    if (enableBreath) {
      if (Array.isArray(opt.breathBones)) breathBones = opt.breathBones
      else { breathBones = Object.keys(opt.breathBones); breathRanges = opt.breathBones }
    }
    const breathDuration = opt.breathDuration === undefined || opt.breathDuration === null ? 4000 : opt.breathDuration

    // per-bone key lists in time order
    const byBone = new Map()
    for (const kf of this.animationFrames) {
      for (const bf of kf.boneFrames) {
        if (!byBone.has(bf.boneName)) byBone.set(bf.boneName, [])
        byBone.get(bf.boneName).push({ boneName: bf.boneName, time: kf.time, rotation: bf.rotation })
      }
    }
    for (const keys of byBone.values()) keys.sort((a, b) => a.time - b.time)

    if (this.currentModel) {
      // time-0 keys apply instantly; every bone without one snaps to identity (:1474-1505)
      const names0 = [], rots0 = [], has0 = new Set()
      for (const [name, keys] of byBone.entries()) {
        if (keys.length > 0 && keys[0].time === 0) { names0.push(name); rots0.push(keys[0].rotation); has0.add(name) }
      }
      if (names0.length > 0) this.rotateBones(names0, rots0, 0)
      const reset = this.currentModel.getSkeleton().bones.map((b) => b.name).filter((n) => !has0.has(n))
      if (reset.length > 0) this.rotateBones(reset, reset.map(() => new Quat(0, 0, 0, 1)), 0)
    }

    // later keys: a tween from the previous key's time lasting until this key's time (:1527-1553)
    for (const keys of byBone.values()) {
      for (let i = 0; i < keys.length; i++) {
        const k = keys[i]
        if (k.time === 0) continue
        const prev = i > 0 ? keys[i - 1] : null
        const durationMs = (prev ? k.time - prev.time : k.time) * 1000
        const delayMs = (prev ? prev.time : 0) * 1000
        if (delayMs <= 0) this.rotateBones([k.boneName], [k.rotation], durationMs)
        else this.animationTimers.push(this.setTimer(() => this.rotateBones([k.boneName], [k.rotation], durationMs), delayMs))
      }
    }

    // morph keys (no reference counterpart: its VMD loader never reads the block): step to each key's weight
    const mf = this.animationFrames.morphFrames || []
    for (const f of mf) {
      const apply = () => this.setMorphWeights([f.morphName], [f.weight])
      if (f.time <= 0) apply(); else this.animationTimers.push(this.setTimer(apply, f.time * 1000))
    }

    // show / IK keys ({ ikKeys }): step every chain a key names at the key's time
    if (this.ikKeys && this.currentModel) {
      const model = this.currentModel, names = model.getIKChainNames()
      names.forEach((_, k) => model.setIKChainEnabled(k, true)) // a chain is on until a key of THIS motion names it: nothing of the playback before stays
      for (const f of this.animationFrames.ikFrames || []) {
        const apply = () => { for (const e of f.ik) if (names.indexOf(e.name) >= 0) model.setIKChainEnabled(e.name, e.enabled) }
        if (f.time <= 0) apply(); else this.animationTimers.push(this.setTimer(apply, f.time * 1000))
      }
    }

    if (enableBreath && this.currentModel) {
      let maxTime = 0
      for (const kf of this.animationFrames) if (kf.time > maxTime) maxTime = kf.time
      const last = new Map()
      for (const bone of breathBones) {
        const keys = byBone.get(bone)
        if (keys && keys.length > 0) last.set(bone, keys[keys.length - 1].rotation)
      }
      this.breathingTimer = this.setTimer(() => this.startBreathing(breathBones, last, breathRanges, breathDuration), maxTime * 1000 + 200)
    }
  }

  stopAnimation() {
    for (const id of this.animationTimers) this.dropTimer(id)
    this.animationTimers = []
    this.playingAnimation = false
  }

  stopBreathing() {
    if (this.breathingTimer !== null) { this.dropTimer(this.breathingTimer); this.breathingTimer = null }
    this.breathingBaseRotations.clear()
  }

  startBreathing(bones, baseRotations, rotationRanges, durationMs) {
    if (!this.currentModel) return
    for (const b of bones) if (baseRotations.has(b)) this.breathingBaseRotations.set(b, baseRotations.get(b))
    const half = (durationMs === undefined ? 4000 : durationMs) / 2
    const swing = (inhale) => {
      if (!this.currentModel) return
      const names = [], quats = []
      for (const b of bones) {
        const base = this.breathingBaseRotations.get(b)
        if (!base) continue
        const range = rotationRanges && rotationRanges[b] !== undefined && rotationRanges[b] !== null ? rotationRanges[b] : 0.02
        names.push(b)
        quats.push(base.multiply(Quat.fromEuler(inhale ? range : -range, 0, 0)))
      }
      if (names.length > 0) this.rotateBones(names, quats, half)
      this.breathingTimer = this.setTimer(() => swing(!inhale), half)
    }
    swing(false)
  }

  // ---- per frame ----
  /**
   * { devicePhysics }: the fixed substeps this frame owes (physics.ts:534-569 hands Bullet the frame's dt with fixedTimeStep 1/75 and
   * maxSubSteps 10): the time the clock advanced since the last frame joins the accumulator, min(10, floor(acc / h)) substeps leave it.
   * What the cap leaves over is dropped, as Bullet drops it, so a long stall does not come back as a burst. -1: no table resident.
   */
  physicsSubsteps() {
    if (!this.physicsResident) return -1
    const now = this.now()
    if (this.lastPhysicsTime !== null && now > this.lastPhysicsTime) this.physicsAccumulator += (now - this.lastPhysicsTime) / 1000
    this.lastPhysicsTime = now
    const owed = Math.floor(this.physicsAccumulator / PHYSICS_H)
    this.physicsAccumulator -= owed * PHYSICS_H
    return Math.min(PHYSICS_MAX_SUBSTEPS, owed)
  }

  /** Every body back onto its bone's solved pose with zero velocities (rz_physics_reset); the accumulated time is dropped. */
  resetPhysics() {
    if (!this.devicePhysics) throw new Error('resetPhysics needs new Engine(canvas, { deviceFK: true, devicePhysics: true })')
    if (!this.physicsResident) return
    for (const s of this.shards) if (s.count > 0) this.native.physicsReset(s.ctx)
    this.physicsAccumulator = 0
    this.lastPhysicsTime = this.now()
  }

  /** engine.ts:2124-2136 + 2375-2402 minus the draw calls: pose on the CPU, deformation on the GPU. */
  render() {
    if (!this.currentModel || !this.ctx) return
    const t0 = wallClock()
    const model = this.currentModel
    const gpuFK = this.deviceFK
    // VMD bone translations (seekFrame) travel with the rotations; the reference itself never writes localTranslations
    const tra = gpuFK && model.applyLocalTranslations ? model.runtimeSkeleton.localTranslations : null
    if (gpuFK) model.updateRotationTweens() // tweens stay on the host; the hierarchy solve moves to the GPU
    else model.evaluatePose()
    if (this.physics && !gpuFK) { // updateModelPose(): physics.step(deltaTime, worldMats, inverseBind) mutates in place
      const now = this.now()
      const dt = this.lastPhysicsTime === null ? 0 : (now - this.lastPhysicsTime) / 1000
      this.lastPhysicsTime = now
      this.physics.step(dt, model.getBoneWorldMatrices(), model.getBoneInverseBindMatrices())
    }
    const mw = model.getMorphCount() > 0 ? model.getEffectiveMorphWeights() : null
    const substeps = this.physicsSubsteps()
    // per-frame inputs are replicated to every shard (16-22 KB); launches are asynchronous, so the GPUs run concurrently
    for (const s of this.shards) {
      if (s.count === 0) continue
      const c = this.frameContext(s)
      if (gpuFK) this.native.setPoseLocal(c, model.runtimeSkeleton.localRotations, mw, tra)
      else this.native.setPose(c, model.getBoneWorldMatrices(), mw)
      if (gpuFK) this.sendIKSwitches(c, true)
      if (substeps >= 0) this.native.physicsStep(c, substeps) // 0 still re-places the following bodies on the new pose
      this.native.deform(c)
    }
    if (this.autotune && !this.tuned) { // the first frame supplied a pose: time the candidate launch shapes once per shard
      for (const s of this.shards) if (s.count > 0) this.native.autotune(s.ctx, 0)
      this.tuned = true
    }
    if (this.gather === 'direct' && this.shards.length > 1) this.native.gatherFence(this.ctx)
    else if (this.gather && this.shards.length > 1) this.native.allgatherAll(this.shards.map((s) => s.ctx), true)
    this.updateStats(wallClock() - t0)
  }

  /**
   * Frame-indexed playback (MMD semantics: Bezier-warped slerp / lerp between keys, bone translation, linear morph
   * keys) of the loaded animation: pose the model at `frame` (30 fps, fractional allowed) and deform one frame.
   * Independent of playAnimation()'s wall-clock tweens, which mirror the reference.
   */
  seekFrame(frame) {
    if (!this.currentModel) return
    if (!this.sampler || this.samplerFor !== this.animationFrames) {
      this.sampler = new VMDSampler(this.animationFrames)
      this.samplerFor = this.animationFrames
    }
    if (this.deviceSampling) return this.seekFrameOnDevice(frame)
    this.currentModel.applySampledFrame(this.sampler, frame)
    this.render()
  }

  /** seekFrame with { deviceFK, deviceSampling }: upload the flattened motion once, then one float per frame. */
  seekFrameOnDevice(frame) {
    const model = this.currentModel
    if (this.animationOnDevice !== this.animationFrames || this.animationFor !== model) {
      const flat = this.sampler.flatten(model.runtimeSkeleton.nameIndex, model.getMorphCount() > 0 ? model.getMorphs() : null, this.ikKeys ? model.getIKChainNames() : null)
      this.dropForks() // the motion is static data
      for (const s of this.shards) {
        if (s.count === 0) continue
        this.native.uploadAnimation(s.ctx, flat)
        this.uploadIKKeysOf(s.ctx, null, flat, model)
      }
      this.animationOnDevice = this.animationFrames
      this.animationFor = model
    }
    const t0 = wallClock()
    // a crowd (setInstanceCount) takes one frame per instance; a single number poses every instance at that frame
    const f = typeof frame === 'number' ? new Float32Array(this.instances).fill(frame) : Float32Array.from(frame)
    if (f.length !== this.instances) throw new Error('seekFrame: ' + f.length + ' frames for ' + this.instances + ' instances')
    const substeps = this.physicsSubsteps()
    for (const s of this.shards) {
      if (s.count === 0) continue
      const c = this.frameContext(s)
      this.native.setPoseSampled(c, f)
      this.sendIKSwitches(c, false)
      if (substeps >= 0) this.native.physicsStep(c, substeps)
      this.native.deform(c)
    }
    if (this.autotune && !this.tuned) { // as in render(): the first frame supplied a pose
      for (const s of this.shards) if (s.count > 0) this.native.autotune(s.ctx, 0)
      this.tuned = true
    }
    if (this.gather === 'direct' && this.shards.length > 1) this.native.gatherFence(this.ctx)
    else if (this.gather && this.shards.length > 1) this.native.allgatherAll(this.shards.map((s) => s.ctx), true)
    this.updateStats(wallClock() - t0)
  }

  /** Add or replace the motion `name` of the motion library. loadAnimation / seekFrame keep their single motion. */
  async loadMotion(name, path) {
    this.motions.set(name, new VMDSampler(await VMDLoader.load(path))) // (a replaced name keeps its place in the map: its clip index)
    this.motionsVersion++
  }

  /**
   * Pose from the motion library and deform one frame: per state, motion `a` at frameA cross-faded by `blend` into motion `b` at frameB
   * (no `b`, or blend 0: `a` alone). With { deviceFK, deviceSampling } the library is uploaded once per (library, model) and every call is
   * one rz_set_pose_blended — a crowd takes one state per instance, a single state poses every instance. Otherwise one character is
   * posed on the host (Model.applyBlendedFrame) and rendered. A state may carry up to four `layers` ({ motion, frame, weight?, mask?,
   * additive? }; masks from setMotionMask): on the device the call becomes one rz_set_pose_layered (the masks are uploaded once per
   * (mask set, model)), on the host Model.applyLayeredFrame. Without layers nothing changes.
   */
  seekMotions(state) {
    if (!this.currentModel) return
    const states = Array.isArray(state) ? state : new Array(this.deviceSampling ? this.instances : 1).fill(state)
    for (const st of states) {
      if (!this.motions.has(st.a)) throw new Error('seekMotions: unknown motion "' + st.a + '"')
      if (st.b !== undefined && st.b !== null && !this.motions.has(st.b)) throw new Error('seekMotions: unknown motion "' + st.b + '"')
      if (!st.layers) continue
      if (st.layers.length > 4) throw new Error('seekMotions: ' + st.layers.length + ' layers, at most 4')
      for (const l of st.layers) {
        if (!this.motions.has(l.motion)) throw new Error('seekMotions: unknown motion "' + l.motion + '"')
        if (l.mask !== undefined && l.mask !== null && !this.motionMasks.has(l.mask)) throw new Error('seekMotions: unknown mask "' + l.mask + '"')
      }
    }
    if (this.deviceSampling) return this.seekMotionsOnDevice(states)
    if (states.length !== 1) throw new Error('seekMotions: ' + states.length + ' states, but the host path poses one character (a crowd needs { deviceFK, deviceSampling })')
    const st = states[0]
    const hasB = st.b !== undefined && st.b !== null
    if (st.layers && st.layers.length) {
      const masks = this.resolveMotionMasks(this.currentModel)
      const resolved = {}
      Array.from(this.motionMasks.keys()).forEach((name, k) => { resolved[name] = masks[k] })
      this.currentModel.applyLayeredFrame({ a: this.motions.get(st.a), frameA: st.frameA, b: hasB ? this.motions.get(st.b) : null, frameB: st.frameB, blend: st.blend },
        st.layers.map((l) => ({ sampler: this.motions.get(l.motion), frame: l.frame, weight: l.weight, mask: l.mask, additive: l.additive })), resolved)
    } else this.currentModel.applyBlendedFrame(this.motions.get(st.a), st.frameA, hasB ? this.motions.get(st.b) : null, st.frameB, st.blend)
    this.render()
  }

  /**
   * Add or replace the mask `name` that the layers of a MotionState may name: the bones `spec.bones` (with `withDescendants`, every bone
   * below them in the skeleton's parent table as well) and the morphs `spec.morphs` (names, 'all' — the default — or 'none'). Names are
   * resolved against the model when the mask is first used; a bone the model lacks throws there.
   */
  setMotionMask(name, spec) {
    if (!spec || !Array.isArray(spec.bones)) throw new Error('setMotionMask(name, { bones: string[], withDescendants?, morphs? })')
    this.motionMasks.set(name, { bones: spec.bones.slice(), withDescendants: !!spec.withDescendants, morphs: Array.isArray(spec.morphs) ? spec.morphs.slice() : spec.morphs || 'all' }) // (a replaced name keeps its place in the map: its mask index)
    this.masksVersion++
  }

  /** every mask of setMotionMask resolved for `model`, in the map's order: one byte per bone and one per morph */
  resolveMotionMasks(model) {
    const bones = model.getSkeleton().bones, B = bones.length, M = model.getMorphCount()
    const out = []
    for (const [name, spec] of this.motionMasks) {
      const bm = new Uint8Array(B), mm = new Uint8Array(M)
      for (const bn of spec.bones) {
        const i = model.runtimeSkeleton.nameIndex[bn]
        if (i === undefined) throw new Error('setMotionMask "' + name + '": unknown bone "' + bn + '"')
        bm[i] = 1
      }
      if (spec.withDescendants) {
        for (let i = 0; i < B; i++) { // a bone is in when an ancestor is (parents may come after their children in a PMX: walk up)
          for (let p = bones[i].parentIndex, n = 0; p >= 0 && p < B && n < B; p = bones[p].parentIndex, n++) if (bm[p] === 1) { bm[i] = 2; break }
        }
        for (let i = 0; i < B; i++) if (bm[i]) bm[i] = 1
      }
      if (spec.morphs === 'all' || spec.morphs === undefined) mm.fill(1)
      else if (spec.morphs !== 'none') {
        const names = model.getMorphNames()
        for (const mn of spec.morphs) { const i = names.indexOf(mn); if (i >= 0) mm[i] = 1 }
      }
      out.push({ bones: bm, morphs: mm })
    }
    return out
  }

  /** seekMotions with { deviceFK, deviceSampling }: upload the flattened library once, then 20 bytes per instance and frame. */
  seekMotionsOnDevice(states) {
    const model = this.currentModel
    if (states.length !== this.instances) throw new Error('seekMotions: ' + states.length + ' states for ' + this.instances + ' instances')
    const names = Array.from(this.motions.keys())
    if (this.motionsOnDevice !== this.motionsVersion || this.motionsFor !== model) {
      const morphs = model.getMorphCount() > 0 ? model.getMorphs() : null
      const chainNames = this.ikKeys ? model.getIKChainNames() : null
      const flats = names.map((n) => this.motions.get(n).flatten(model.runtimeSkeleton.nameIndex, morphs, chainNames))
      this.dropForks() // the library is static data
      for (const s of this.shards) {
        if (s.count === 0) continue
        this.native.uploadMotions(s.ctx, flats)
        flats.forEach((f, k) => this.uploadIKKeysOf(s.ctx, k, f, model))
      }
      this.motionsOnDevice = this.motionsVersion
      this.motionsFor = model
    }
    const t0 = wallClock()
    const buf = new ArrayBuffer(states.length * 20), dv = new DataView(buf)
    states.forEach((st, i) => {
      const hasB = st.b !== undefined && st.b !== null
      dv.setUint32(i * 20, names.indexOf(st.a), true)
      dv.setFloat32(i * 20 + 4, st.frameA, true)
      dv.setUint32(i * 20 + 8, hasB ? names.indexOf(st.b) : 0xffffffff, true)
      dv.setFloat32(i * 20 + 12, hasB && st.frameB !== undefined ? st.frameB : 0, true)
      dv.setFloat32(i * 20 + 16, hasB && st.blend !== undefined ? st.blend : 0, true)
    })
    // layers: the longest list decides the count, shorter ones are padded with skipped layers; no layers at all is a blended pose, as ever
    const nLayers = states.reduce((n, st) => Math.max(n, st.layers ? st.layers.length : 0), 0)
    let lbuf = null
    if (nLayers > 0) {
      const maskNames = Array.from(this.motionMasks.keys())
      if (maskNames.length > 0 && (this.masksOnDevice !== this.masksVersion || this.masksFor !== model)) {
        const masks = this.resolveMotionMasks(model)
        const B = masks[0].bones.length, M = masks[0].morphs.length
        const bm = new Uint8Array(masks.length * B), mm = M > 0 ? new Uint8Array(masks.length * M) : null
        masks.forEach((m, k) => { bm.set(m.bones, k * B); if (mm) mm.set(m.morphs, k * M) })
        this.dropForks() // the masks are static data
        for (const s of this.shards) if (s.count > 0) this.native.uploadMotionMasks(s.ctx, masks.length, bm, mm)
        this.masksOnDevice = this.masksVersion
        this.masksFor = model
      }
      lbuf = new ArrayBuffer(states.length * nLayers * 20)
      const lv = new DataView(lbuf)
      states.forEach((st, i) => {
        for (let k = 0; k < nLayers; k++) {
          const l = st.layers && k < st.layers.length ? st.layers[k] : null, o = (i * nLayers + k) * 20
          lv.setUint32(o, l ? names.indexOf(l.motion) : 0xffffffff, true)
          lv.setFloat32(o + 4, l ? l.frame : 0, true)
          lv.setFloat32(o + 8, l ? (l.weight === undefined || l.weight === null ? 1 : l.weight) : 0, true)
          lv.setUint32(o + 12, l && l.mask !== undefined && l.mask !== null ? maskNames.indexOf(l.mask) : 0xffffffff, true)
          lv.setUint32(o + 16, l && l.additive ? 1 : 0, true)
        }
      })
    }
    const substeps = this.physicsSubsteps()
    for (const s of this.shards) {
      if (s.count === 0) continue
      const c = this.frameContext(s)
      if (lbuf) this.native.setPoseLayered(c, buf, nLayers, lbuf)
      else this.native.setPoseBlended(c, buf)
      this.sendIKSwitches(c, false)
      if (substeps >= 0) this.native.physicsStep(c, substeps)
      this.native.deform(c)
    }
    if (this.autotune && !this.tuned) { // as in render(): the first frame supplied a pose
      for (const s of this.shards) if (s.count > 0) this.native.autotune(s.ctx, 0)
      this.tuned = true
    }
    if (this.gather === 'direct' && this.shards.length > 1) this.native.gatherFence(this.ctx)
    else if (this.gather && this.shards.length > 1) this.native.allgatherAll(this.shards.map((s) => s.ctx), true)
    this.updateStats(wallClock() - t0)
  }

  /**
   * { ikKeys }: the IK on / off keys of a motion (clip null) or of clip `clip` of the library, right behind its upload, which dropped the
   * keys of the motion before it. A motion WITHOUT such keys uploads a set of no keys, which is resident and says "all on": the pose calls
   * then write an all-on mask, as the host path does, instead of leaving the switches of the motion before in place.
   */
  uploadIKKeysOf(ctx, clip, flat, model) {
    const chains = model.getIKChains().length
    if (!this.ikKeys || chains === 0) return
    if (flat.ikKeys) this.native.uploadIKKeys(ctx, clip, flat.ikKeys.frames, flat.ikKeys.enabled)
    else this.native.uploadIKKeys(ctx, clip, new Float32Array(0), new Uint8Array(0))
  }

  /**
   * What follows a pose call on the device path. With { ikKeys }, a host-sampled frame (`hostPose`: rz_set_pose_local) carries the model's
   * chain switches, which seekFrame / playAnimation / seekMotions set from the motion; device-sampled frames need nothing: their pose call
   * evaluates the uploaded keys. Switches held by hand (setIKEnabled) are laid over that state, switch by switch, and the result is sent;
   * once none is held any more, a context that carried some gets its own state back. Without either: no call.
   */
  sendIKSwitches(c, hostPose) {
    const on = this.currentModel.getIKChainEnabled(), n = on.length
    if (n === 0) return
    if (this.ikManual && this.ikManual.length !== this.instances * n) this.ikManual = null // (the crowd changed)
    const held = this.ikManual !== null && this.ikManual.some((v) => v >= 0)
    const fromKeys = this.ikKeys && !hostPose // the pose call has just written the mask
    if (!held && !(this.ikKeys && hostPose)) {
      if (this.ikManualSent.has(c)) { this.ikManualSent.delete(c); if (!fromKeys) this.native.setIKEnabled(c, null) }
      return
    }
    const mask = fromKeys ? Uint8Array.from(this.native.readIKEnabled(c)) : new Uint8Array(this.instances * n).fill(1)
    if (this.ikKeys && hostPose) for (let i = 0; i < this.instances; i++) on.forEach((v, k) => { mask[i * n + k] = v ? 1 : 0 })
    if (held) { this.ikManual.forEach((v, j) => { if (v >= 0) mask[j] = v }); this.ikManualSent.add(c) } else this.ikManualSent.delete(c)
    this.native.setIKEnabled(c, mask)
  }

  /**
   * Hold one IK chain off or on by hand ({ ik: true }): `nameOrIndex` is the name of the chain's IK bone or its index in
   * Model.getIKChains(); `instance` names one crowd member (default: all); `on` null hands the switch back to the motion. Host path: the
   * model's switch. Device path: from the next pose call on the held switches are laid over the state the motion's keys give (all on
   * without { ikKeys }) - only the named switch changes, as on the host path.
   */
  setIKEnabled(nameOrIndex, on, instance) {
    if (!this.ik) throw new Error('setIKEnabled needs new Engine(canvas, { ik: true })')
    const model = this.currentModel
    if (!model) return
    const names = model.getIKChainNames()
    const k = typeof nameOrIndex === 'number' ? nameOrIndex : names.indexOf(nameOrIndex)
    if (!(k >= 0 && k < names.length)) throw new Error('setIKEnabled: no IK chain ' + JSON.stringify(nameOrIndex))
    if (!this.deviceFK) { model.setIKChainEnabled(k, on === null || on === undefined ? true : on); return }
    if (instance !== undefined && !(instance >= 0 && instance < this.instances)) throw new Error('setIKEnabled: instance ' + instance + ' of ' + this.instances)
    if (!this.ikManual || this.ikManual.length !== this.instances * names.length) this.ikManual = new Int8Array(this.instances * names.length).fill(-1)
    for (let i = 0; i < this.instances; i++) if (instance === undefined || instance === i) this.ikManual[i * names.length + k] = on === null || on === undefined ? -1 : on ? 1 : 0
  }

  /**
   * Physics hand-off when the hierarchy is solved on the GPU ({ deviceFK }): the world matrices of physics-driven bones
   * (what physics.ts:715-751 writes with boneWorldMatrices.set(values, boneIndex * 16)) replace the solved ones after
   * the hierarchy solve in every following frame, until the next call; an empty list clears. Children keep the
   * matrices solved from the un-overridden parent, as in the reference. `instances` (optional) names the crowd member
   * of each entry. On the host-FK path use the { physics } option instead — there the host owns the world matrices.
   */
  setBoneWorldOverrides(boneIndices, worldMatrices, instances) {
    if (!this.ctx) throw new Error('Engine.init() has not been called')
    if (!this.deviceFK) throw new Error('setBoneWorldOverrides needs new Engine(canvas, { deviceFK: true }); with host FK pass { physics }')
    if (this.physicsResident) throw new Error('setBoneWorldOverrides: with { devicePhysics } the physics table owns the bone overrides')
    const b = boneIndices && boneIndices.length ? Uint32Array.from(boneIndices) : null
    const w = b ? (worldMatrices instanceof Float32Array ? worldMatrices : Float32Array.from(worldMatrices)) : null
    const i = b && instances ? Uint32Array.from(instances) : null
    this.overrides = b ? [b, w, i] : null
    for (const s of this.shards) {
      if (s.count === 0) continue
      this.native.overrideWorld(s.ctx, b, w, i)
      if (s.fork) this.native.overrideWorld(s.fork, b, w, i)
    }
  }

  /** Deterministic stepping: move the clock to timeMs, fire the timers that came due, render one frame. */
  step(timeMs) {
    if (this.realtime) throw new Error('step() needs new Engine(canvas, { realtime: false })')
    this.nowMs = timeMs
    this.fireDueTimers()
    this.render()
  }

  /**
   * A crowd of `n` independently posed copies of the loaded model (BASELINE config 4; the reference draws one model).
   * Needs { deviceFK, deviceSampling } — every instance is posed on the GPU at its own frame of the loaded motion,
   * seekFrame([f0, f1, ...]) — and a single GPU (instancing and vertex sharding are exclusive).
   */
  setInstanceCount(n) {
    if (!this.ctx || !this.currentModel) throw new Error('no model loaded')
    if (!this.deviceSampling) throw new Error('setInstanceCount needs new Engine(canvas, { deviceFK: true, deviceSampling: true })')
    if (this.shards.length > 1) throw new Error('instancing and vertex sharding are exclusive')
    if (this.outline || this.bounds) throw new Error('the outline hull and bounds are single-instance consumers')
    this.dropForks() // a fork takes its instance count from the lender when it is made
    if (n !== this.instances) this.overrides = null // (instance, bone) pairs of the old crowd: rz_set_instances dropped them on the lender too
    this.native.setInstances(this.ctx, n)
    if (this.crowdMorphs) for (const s of this.shards) this.native.setTuning(s.ctx, 'inst_morphs', 1)
    this.instances = n
    this.tuned = false
  }

  /** Blocking readback of the deformed mesh (the values the reference's vs() only ever feeds the rasteriser). */
  getDeformed(instance) {
    if (!this.ctx || !this.currentModel) throw new Error('no model loaded')
    if (instance !== undefined && instance !== 0) {
      if (!(instance > 0 && instance < this.instances)) throw new Error('instance ' + instance + ' out of range')
      const V = this.currentModel.getVertexCount()
      const pos = new Float32Array(V * 3), nrm = new Float32Array(V * 3)
      this.native.read(this.shards[0].last || this.ctx, instance, 0, V, pos, nrm)
      return { positions: pos, normals: nrm }
    }
    if (this.gather && this.shards.length > 1) { // shard 0's GPU holds the whole mesh (all-gather or peer-direct stores)
      this.native.readGathered(this.ctx, 0, this.currentModel.getVertexCount(), this.outPos, this.outNrm)
      return { positions: this.outPos, normals: this.outNrm }
    }
    for (const s of this.shards) {
      if (s.count === 0) continue
      this.native.read(s.last || s.ctx, 0, 0, s.count, this.outPos.subarray(s.begin * 3, (s.begin + s.count) * 3), this.outNrm.subarray(s.begin * 3, (s.begin + s.count) * 3))
    }
    return { positions: this.outPos, normals: this.outNrm }
  }

  /** Inverted-hull positions the outline pipeline draws: worldPos + worldNormal * edgeSize * 0.01 (needs { outline: true }). */
  getOutlineHull() {
    if (!this.outline) throw new Error('new Engine(canvas, { outline: true }) enables the outline hull')
    for (const s of this.shards) if (s.count > 0) this.native.readHull(s.last || s.ctx, 0, 0, s.count, this.outHull.subarray(s.begin * 3, (s.begin + s.count) * 3))
    return this.outHull
  }

  /** Axis-aligned bounds { min: [x,y,z], max: [x,y,z] } of the last deformed frame (needs { bounds: true }). */
  getBounds() {
    if (!this.bounds) throw new Error('new Engine(canvas, { bounds: true }) enables the bounding-box reduction')
    const b = new Float32Array(6)
    const min = [Infinity, Infinity, Infinity], max = [-Infinity, -Infinity, -Infinity]
    for (const s of this.shards) {
      if (s.count === 0) continue
      this.native.readAabb(s.last || s.ctx, 0, b)
      for (let k = 0; k < 3; k++) { min[k] = Math.min(min[k], b[k]); max[k] = Math.max(max[k], b[3 + k]) }
    }
    return { min, max }
  }

  runRenderLoop(callback) {
    this.renderLoopCallback = callback || null
    const tick = () => {
      this.render()
      if (this.renderLoopCallback) this.renderLoopCallback()
      this.loopHandle = setTimeout(tick, 0) // no requestAnimationFrame in Node: free-running
    }
    this.loopHandle = setTimeout(tick, 0)
  }

  stopRenderLoop() {
    if (this.loopHandle !== null) { clearTimeout(this.loopHandle); this.loopHandle = null }
    this.renderLoopCallback = null
  }

  /** engine.ts:2423-2445 (60-sample moving average, 1 Hz fps) + deformation figures. */
  updateStats(frameTime) {
    this.frameTimeSamples.push(frameTime)
    this.frameTimeSum += frameTime
    if (this.frameTimeSamples.length > 60) this.frameTimeSum -= this.frameTimeSamples.shift()
    this.stats.frameTime = Math.round((this.frameTimeSum / this.frameTimeSamples.length) * 100) / 100
    const now = wallClock()
    this.framesSinceLastUpdate++
    const elapsed = now - this.lastFpsUpdate
    if (elapsed >= 1000) {
      this.stats.fps = Math.round((this.framesSinceLastUpdate / elapsed) * 1000)
      this.framesSinceLastUpdate = 0
      this.lastFpsUpdate = now
    }
  }

  /** Time `frames` back-to-back frames of the current pose on the GPU (HIP events) and fold them into getStats(). */
  measure(frames) {
    const t = this.native.timeFrames(this.ctx, frames || 100)
    this.stats.deformMs = t.frameMs
    this.stats.vertsPerSec = t.vertsPerFrame / (t.frameMs * 1e-3)
    this.stats.hbmGBps = t.algorithmicBytesPerFrame / (t.deformKernelMs * 1e-3) / 1e9
    return t
  }

  getStats() { return Object.assign({}, this.stats) }
}

module.exports = { Engine }
