'use strict'
/* End-to-end after-physics bones through the N-API boundary on a PMX with flag 0x1000 bones and rigid-body and joint sections, under one
 * fixed local pose:
 *   on:   new Engine(null, { deviceFK: true, devicePhysics: true, afterPhysics: true })
 *   off:  new Engine(null, { deviceFK: true, devicePhysics: true })
 * usage: node after_e2e.js <model.pmx> <localRotations.f32> <outdir> <time ms>...
 * Dumps per engine the world matrices (world_<tag>.f32) and deformed positions (pos_<tag>.f32) of every frame; prints the tuning keys. */
const fs = require('fs'), path = require('path')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, rot, out, ...ts] = process.argv.slice(2)
const cat = (parts) => {
  const all = new Float32Array(parts.reduce((n, p) => n + p.length, 0))
  let o = 0
  for (const p of parts) { all.set(p, o); o += p.length }
  return Buffer.from(all.buffer)
}
;(async () => {
  console.warn = () => {}
  const times = ts.map(Number)
  const raw = fs.readFileSync(rot)
  const q = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength))
  const res = {}
  for (const [tag, opts] of [['on', { deviceFK: true, devicePhysics: true, afterPhysics: true }], ['off', { deviceFK: true, devicePhysics: true }]]) {
    const e = new Engine(null, Object.assign({ realtime: false }, opts))
    await e.init(); await e.loadModel(pmx)
    e.currentModel.runtimeSkeleton.localRotations.set(q)
    const B = e.currentModel.getSkeleton().bones.length
    const pos = [], world = []
    for (const t of times) {
      e.step(t)
      pos.push(Float32Array.from(e.getDeformed().positions))
      const w = new Float32Array(B * 16)
      e.native.readWorld(e.ctx, 0, w)
      world.push(w)
    }
    fs.writeFileSync(path.join(out, 'pos_' + tag + '.f32'), cat(pos))
    fs.writeFileSync(path.join(out, 'world_' + tag + '.f32'), cat(world))
    res[tag] = [e.native.getTuning(e.ctx, 'after_physics'), e.native.getTuning(e.ctx, 'after_physics_levels')]
    if (tag === 'on') res.order = e.currentModel.afterPhysicsOrder()
    e.dispose()
  }
  console.log(JSON.stringify(res))
})().catch((e) => { console.error(e); process.exit(1) })
