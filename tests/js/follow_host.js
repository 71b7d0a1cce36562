'use strict'
/* Model.followOverrides (host/model.js), the host twin of rz_override_follow, on the cases of a JSON file:
 *   [{ parents: [B], world: [B*16] (the solved matrices S), bones: [n], mats: [n*16] }, ...]
 * usage: node follow_host.js <cases.json>      prints [[B*16 floats], ...]: every case's world matrices after the call */
const fs = require('fs'), path = require('path')
const { Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'))
const out = cases.map((c) => {
  const bones = c.parents.map((p, i) => ({ name: 'b' + i, parentIndex: p, bindTranslation: [0, 0, 0], children: [] }))
  const model = new Model(new Float32Array(8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(bones.length * 16) },
    { joints: new Uint16Array(4), weights: new Uint8Array(4) })
  const world = Float32Array.from(c.world)
  model.followOverrides(world, Uint32Array.from(c.bones), Float32Array.from(c.mats))
  return Array.from(world)
})
console.log(JSON.stringify(out))
