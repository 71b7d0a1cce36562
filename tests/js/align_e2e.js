'use strict'
/* End-to-end PMX type-2 bodies through the N-API boundary on a PMX whose strands' first links are type 2, under one fixed local pose.
 * One engine per option of the comma-separated list, new Engine(null, { deviceFK: true, devicePhysics: true, ... }):
 *   aligned:  physicsAligned: true — rz_physics_aligned(ctx, 1) behind the table's upload
 *   off:      no physicsAligned at all: the same table, its type-2 bodies following their bones
 * usage: node align_e2e.js <options> <tuning keys> <model.pmx> <localRotations.f32> <outdir> <time ms>...
 * Dumps per option the deformed positions, world matrices and body state of every frame (pos_ / world_ / state_<option>.f32). Prints per
 * option the substeps every frame asked for and the comma-separated tuning keys asked for. */
const fs = require('fs'), path = require('path')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [options, keys, pmx, rot, out, ...ts] = process.argv.slice(2)
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
  for (const tag of options.split(',')) {
    const e = new Engine(null, Object.assign({ realtime: false, deviceFK: true, devicePhysics: true }, tag === 'off' ? {} : { physicsAligned: true }))
    await e.init(); await e.loadModel(pmx)
    const substeps = [], step = e.native.physicsStep
    e.native = Object.assign({}, e.native, { physicsStep: (c, n) => { substeps.push(n); step(c, n) } })
    e.currentModel.runtimeSkeleton.localRotations.set(q)
    const B = e.currentModel.getSkeleton().bones.length, nb = e.currentModel.getRigidbodies().length
    const pos = [], world = [], state = []
    for (const t of times) {
      e.step(t)
      pos.push(Float32Array.from(e.getDeformed().positions))
      const w = new Float32Array(B * 16), s = new Float32Array(nb * 13)
      e.native.readWorld(e.ctx, 0, w); e.native.readPhysics(e.ctx, 0, s)
      world.push(w); state.push(s)
    }
    fs.writeFileSync(path.join(out, 'pos_' + tag + '.f32'), cat(pos))
    fs.writeFileSync(path.join(out, 'world_' + tag + '.f32'), cat(world))
    fs.writeFileSync(path.join(out, 'state_' + tag + '.f32'), cat(state))
    res[tag] = { substeps: substeps.slice(), keys: keys.split(',').map((k) => e.native.getTuning(e.ctx, k)) }
    e.dispose()
  }
  console.log(JSON.stringify(res))
})().catch((e) => { console.error(e); process.exit(1) })
