'use strict'
/* The host twins of the IK chain switches. usage: node ik_switch_host.js <in.json> <out.json>
 * in.mode = 'parse': { vmds: [path] } -> per file { bone, morph, ik } or { error }.
 * in.mode = 'solve': { parents, bind, chains (in the order wanted), masks: [[0|1]], poses: [{q, t}] } -> per (mask, pose) the world matrices
 *   of Model.solveIK() under the mask set by setIKChainEnabled, plus getIKChainEnabled().
 * in.mode = 'state': { vmd, frames, names, states: [[frameA, vmdB|null, frameB, blend]] } -> VMDSampler.ikStateAt per frame (as
 *   [name, on] pairs), flatten().ikKeys for `names`, and the switches a model with chains `names` has after applyBlendedFrame per state. */
const fs = require('fs'), path = require('path')
const { Model, VMDLoader, VMDSampler } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const inp = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'))
const mkModel = (parents, bind, chains, names) => {
  const bones = parents.map((p, i) => ({ name: names ? names[i] : 'b' + i, parentIndex: p, bindTranslation: bind[i], children: [] }))
  for (const ch of chains) bones[ch.goal].ik = { effector: ch.effector, loops: ch.loops, limitAngle: ch.limitAngle, links: ch.links.map((l) => (l.min ? { bone: l.bone, min: l.min, max: l.max } : { bone: l.bone })) }
  return new Model(new Float32Array(8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(parents.length * 16) },
    { joints: new Uint16Array(4), weights: new Uint8Array(4).fill(255) }, [], [], null)
}
let out
if (inp.mode === 'parse') {
  out = inp.vmds.map((p) => {
    try {
      const r = VMDLoader.loadFromBuffer(fs.readFileSync(p))
      return {
        bone: r.map((g) => ({ time: g.time, frames: g.boneFrames.map((b) => [b.boneName, b.frame, [b.rotation.x, b.rotation.y, b.rotation.z, b.rotation.w], [b.position.x, b.position.y, b.position.z], Array.from(b.interpolation)]) })),
        morph: r.morphFrames, ik: r.ikFrames,
      }
    } catch (e) { return { error: String(e) } }
  })
} else if (inp.mode === 'solve') {
  const m = mkModel(inp.parents, inp.bind, inp.chains)
  const order = m.getIKChains().map((ch) => inp.chains.findIndex((c) => c.goal === ch.goal)) // model order (ascending goal) -> the test's order
  out = inp.masks.map((mask) => {
    order.forEach((k, ci) => m.setIKChainEnabled(ci % 2 ? 'b' + inp.chains[k].goal : ci, !!mask[k])) // by index and by name
    return { enabled: m.getIKChainEnabled(), worlds: inp.poses.map((pose) => {
      m.runtimeSkeleton.localRotations.set(pose.q); m.runtimeSkeleton.localTranslations.set(pose.t)
      m.applyLocalTranslations = true
      m.setIK(true)
      m.computeWorldMatrices()
      return Array.from(m.getBoneWorldMatrices())
    }) }
  })
} else {
  const load = (p) => new VMDSampler(VMDLoader.loadFromBuffer(fs.readFileSync(p)))
  const s = load(inp.vmd)
  const n = inp.names.length
  const parents = [-1].concat(inp.names.map(() => 0), inp.names.map(() => 0)), bind = parents.map(() => [0, 1, 0])
  const names = ['root'].concat(inp.names.map((x) => 'eff_' + x), inp.names)
  const m = mkModel(parents, bind, inp.names.map((_, k) => ({ goal: 1 + n + k, effector: 1 + k, loops: 1, limitAngle: 1, links: [] })), names)
  const before = inp.states.map((st) => { m.applyBlendedFrame(s, st[0], st[1] ? load(st[1]) : null, st[2], st[3]); return m.getIKChainEnabled() })
  m.setIKKeys(true)
  out = {
    states: inp.frames.map((f) => Array.from(s.ikStateAt(f))), keys: (() => { const k = s.flatten({}, null, inp.names).ikKeys; return k ? { frames: Array.from(k.frames), enabled: Array.from(k.enabled) } : null })(),
    noNames: s.flatten({}, null).ikKeys === undefined, before,
    chosen: inp.states.map((st) => { m.applyBlendedFrame(s, st[0], st[1] ? load(st[1]) : null, st[2], st[3]); return m.getIKChainEnabled() }),
    layered: inp.states.map((st) => { m.applyLayeredFrame({ a: s, frameA: st[0], b: st[1] ? load(st[1]) : null, frameB: st[2], blend: st[3] }, []); return m.getIKChainEnabled() }),
  }
}
fs.writeFileSync(process.argv[3], JSON.stringify(out))
