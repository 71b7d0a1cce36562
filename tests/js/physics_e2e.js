'use strict'
/* End-to-end device physics through the N-API boundary on a PMX with rigid-body and joint sections, under one fixed local pose:
 *   on:   new Engine(null, { deviceFK: true, devicePhysics: true })   rz_upload_physics at loadModel, rz_physics_step before every frame
 *   off:  new Engine(null, { deviceFK: true })                        the strands stay frozen to their parents
 * usage: node physics_e2e.js <model.pmx> <localRotations.f32> <outdir> <time ms>...
 * Dumps per engine the deformed positions of every frame (pos_<tag>.f32) and, for `on`, the world matrices (world_on.f32), the body
 * state (state_on.f32), and the frame after resetPhysics() at the last time (reset_on.f32). Prints the substeps every frame asked for. */
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
  const res = { times }
  for (const [tag, opts] of [['on', { deviceFK: true, devicePhysics: true }], ['off', { deviceFK: true }]]) {
    const e = new Engine(null, Object.assign({ realtime: false }, opts))
    await e.init(); await e.loadModel(pmx)
    const substeps = [], step = e.native.physicsStep
    e.native = Object.assign({}, e.native, { physicsStep: (c, n) => { substeps.push(n); step(c, n) } })
    e.currentModel.runtimeSkeleton.localRotations.set(q)
    const B = e.currentModel.getSkeleton().bones.length, nb = e.currentModel.getRigidbodies().length
    const pos = [], world = [], state = []
    for (const t of times) {
      e.step(t)
      pos.push(Float32Array.from(e.getDeformed().positions))
      if (tag !== 'on') continue
      const w = new Float32Array(B * 16), s = new Float32Array(nb * 13)
      e.native.readWorld(e.ctx, 0, w); e.native.readPhysics(e.ctx, 0, s)
      world.push(w); state.push(s)
    }
    fs.writeFileSync(path.join(out, 'pos_' + tag + '.f32'), cat(pos))
    res[tag] = substeps.slice()
    if (tag === 'on') {
      fs.writeFileSync(path.join(out, 'world_on.f32'), cat(world))
      fs.writeFileSync(path.join(out, 'state_on.f32'), cat(state))
      e.resetPhysics()
      e.step(times[times.length - 1])
      fs.writeFileSync(path.join(out, 'reset_on.f32'), cat([Float32Array.from(e.getDeformed().positions)]))
      res.bodies = e.native.getTuning(e.ctx, 'physics_bodies')
    } else {
      let refused = false
      try { e.resetPhysics() } catch (err) { refused = /devicePhysics/.test(err.message) }
      res.offRefusesReset = refused
    }
    e.dispose()
  }
  console.log(JSON.stringify(res))
})().catch((e) => { console.error(e); process.exit(1) })
