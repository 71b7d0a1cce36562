'use strict'
// node sampler_long.js <motion.vmd> <frames.json>: every bone track and every morph track of the motion sampled by host/vmd-sampler.js at
// the listed frames -> one JSON line { keys, bones, morphs, samples: [{ <bone>: { rotation, position }, <morph>: weight }] }
const path = require('path'), fs = require('fs')
const { VMDLoader, VMDSampler } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const s = new VMDSampler(VMDLoader.loadFromBuffer(fs.readFileSync(process.argv[2])))
const frames = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'))
const bones = s.boneNames(), morphs = s.morphNames()
let keys = 0
for (const b of bones) keys += s.bones.get(b).length
const samples = frames.map((f) => {
  const o = {}
  for (const b of bones) { const r = s.sampleBone(b, f); o[b] = { rotation: Array.from(r.rotation), position: Array.from(r.position) } }
  for (const m of morphs) o[m] = s.sampleMorph(m, f)
  return o
})
console.log(JSON.stringify({ keys, bones, morphs, samples }))
