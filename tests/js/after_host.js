'use strict'
/* Model.afterPhysicsOrder / Model.solveAfterPhysics (host/model.js), the host twin of rz_upload_after_physics, on the cases of a JSON file:
 *   [{ parents, bind: [B*3], ap, ratio, move, flagged: [bones], levels: {bone: level}, q: [B*4], t: [B*3], world: [B*16] (the frame
 *      without the stage), overridden: [bones] }, ...]
 * usage: node after_host.js <cases.json>      prints [{ order: [...], world: [B*16 floats] } | { error: message }, ...] */
const fs = require('fs'), path = require('path')
const { Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'))
const out = cases.map((c) => {
  const B = c.parents.length
  const bones = c.parents.map((p, i) => {
    const b = { name: 'b' + i, parentIndex: p, bindTranslation: [c.bind[i * 3], c.bind[i * 3 + 1], c.bind[i * 3 + 2]], children: [] }
    if (c.ap[i] >= 0) { b.appendParentIndex = c.ap[i]; b.appendRatio = c.ratio[i]; b.appendRotate = true; b.appendMove = !!c.move[i] }
    if (c.flagged.includes(i)) b.afterPhysics = true
    if (c.levels[i]) b.transformLevel = c.levels[i]
    return b
  })
  const model = new Model(new Float32Array(8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(B * 16) },
    { joints: new Uint16Array(4), weights: new Uint8Array(4) })
  try {
    const order = model.afterPhysicsOrder()
    if (!c.world) return { order }
    model.runtimeSkeleton.localRotations.set(Float32Array.from(c.q))
    model.runtimeSkeleton.localTranslations.set(Float32Array.from(c.t))
    model.applyLocalTranslations = true
    const world = Float32Array.from(c.world)
    model.solveAfterPhysics(world, c.overridden)
    return { order, world: Array.from(world) }
  } catch (err) { return { error: err.message } }
})
console.log(JSON.stringify(out))
