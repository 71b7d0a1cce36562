'use strict'
/* Model.applyLayeredFrame (the host twin of rz_set_pose_layered) on a synthetic PMX with three synthetic VMDs (walk, run, a morph-only face
 * file), no GPU: for every state the local rotations, local translations and effective morph weights it leaves, next to the three flattened
 * motions and the masks Engine.setMotionMask resolves, so that pytest can hold them to tests/layer_ref.py. The model is put back at rest
 * before every state (a bone or morph that no clip keys is left alone).
 * usage: node motion_layers.js <model.pmx> <walk.vmd> <run.vmd> <face.vmd> <states.json>   -> one JSON line */
const path = require('path'), fs = require('fs')
const { Engine, PmxLoader, VMDLoader, VMDSampler } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmdA, vmdB, vmdC, statesFile] = process.argv.slice(2)
const model = PmxLoader.loadFromBuffer(fs.readFileSync(pmx))
const samplers = {}
;[['walk', vmdA], ['run', vmdB], ['face', vmdC]].forEach(([n, f]) => { samplers[n] = new VMDSampler(VMDLoader.loadFromBuffer(fs.readFileSync(f))) })
const { masks: maskSpecs, states } = JSON.parse(fs.readFileSync(statesFile, 'utf8'))
const plain = (o) => { const r = {}; for (const k of Object.keys(o)) r[k] = Array.from(o[k]); return r }
const out = { bones: model.runtimeSkeleton.localRotations.length / 4, morphs: model.getMorphCount(), results: [], masks: {} }
out.flats = ['walk', 'run', 'face'].map((n) => plain(samplers[n].flatten(model.runtimeSkeleton.nameIndex, model.getMorphs())))
const engine = new Engine(null, { realtime: false })
for (const name of Object.keys(maskSpecs)) engine.setMotionMask(name, maskSpecs[name])
const resolved = engine.resolveMotionMasks(model), masks = {}
Object.keys(maskSpecs).forEach((name, k) => { masks[name] = resolved[k]; out.masks[name] = { bones: Array.from(resolved[k].bones), morphs: Array.from(resolved[k].morphs) } })
engine.setMotionMask('direct', { bones: maskSpecs.upper.bones })
out.descendantsAdded = out.masks.upper.bones.reduce((a, b) => a + b, 0) - engine.resolveMotionMasks(model)[2].bones.reduce((a, b) => a + b, 0)
const rot = model.runtimeSkeleton.localRotations, tra = model.runtimeSkeleton.localTranslations
const toHost = (st) => [{ a: samplers[st.a], frameA: st.frameA, b: st.b ? samplers[st.b] : null, frameB: st.frameB, blend: st.blend },
  (st.layers || []).map((l) => ({ sampler: samplers[l.motion], frame: l.frame, weight: l.weight, mask: l.mask, additive: l.additive }))]
for (const st of states) {
  for (let b = 0; b < out.bones; b++) { rot.set([0, 0, 0, 1], b * 4); tra.set([0, 0, 0], b * 3) }
  model.getMorphWeights().fill(0)
  const [base, layers] = toHost(st)
  model.applyLayeredFrame(base, layers, masks)
  out.results.push({ rot: Array.from(rot), tra: Array.from(tra), mw: Array.from(model.getEffectiveMorphWeights()) })
}
let threw = 0
const base = { a: samplers.walk, frameA: 1 }
for (const bad of [[{ sampler: samplers.run, frame: 1, weight: 1.5 }], [{ sampler: samplers.run, frame: NaN }], [{ sampler: samplers.run, frame: 1, mask: 'nope' }],
  new Array(5).fill({ sampler: samplers.run, frame: 1 })]) { try { model.applyLayeredFrame(base, bad, masks) } catch (e) { threw++ } }
out.badLayerThrows = threw
console.log(JSON.stringify(out))
