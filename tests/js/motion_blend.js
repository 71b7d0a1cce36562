'use strict'
/* Model.applyBlendedFrame (the host twin of rz_set_pose_blended) on a synthetic PMX with two synthetic VMDs, no GPU: for every state the
 * local rotations, local translations and effective morph weights it leaves, next to the two flattened motions, so that pytest can hold
 * them to tests/motion_ref.py. The model is put back at rest before every state (a bone keyed by neither clip is left alone).
 * usage: node motion_blend.js <model.pmx> <a.vmd> <b.vmd> <states.json>   -> one JSON line */
const path = require('path'), fs = require('fs')
const { PmxLoader, VMDLoader, VMDSampler } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmdA, vmdB, statesFile] = process.argv.slice(2)
const model = PmxLoader.loadFromBuffer(fs.readFileSync(pmx))
const samplers = [vmdA, vmdB].map((f) => new VMDSampler(VMDLoader.loadFromBuffer(fs.readFileSync(f))))
const states = JSON.parse(fs.readFileSync(statesFile, 'utf8'))
const plain = (o) => { const r = {}; for (const k of Object.keys(o)) r[k] = Array.from(o[k]); return r }
const out = { bones: model.runtimeSkeleton.localRotations.length / 4, morphs: model.getMorphCount(), results: [] }
out.flats = samplers.map((s) => plain(s.flatten(model.runtimeSkeleton.nameIndex, model.getMorphs())))
const rot = model.runtimeSkeleton.localRotations, tra = model.runtimeSkeleton.localTranslations
for (const st of states) {
  for (let b = 0; b < out.bones; b++) { rot.set([0, 0, 0, 1], b * 4); tra.set([0, 0, 0], b * 3) }
  model.getMorphWeights().fill(0)
  model.applyBlendedFrame(samplers[st[0]], st[1], st[2] === null ? null : samplers[st[2]], st[3], st[4])
  out.results.push({ rot: Array.from(rot), tra: Array.from(tra), mw: Array.from(model.getEffectiveMorphWeights()) })
}
let threw = 0
for (const bad of [-0.1, 1.5, NaN]) { try { model.applyBlendedFrame(samplers[0], 1, samplers[1], 1, bad) } catch (e) { threw++ } }
out.badBlendThrows = threw
console.log(JSON.stringify(out))
