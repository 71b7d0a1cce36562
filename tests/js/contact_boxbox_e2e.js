'use strict'
/* End-to-end contacts between boxes through the N-API boundary on a PMX with box colliders and box plates, under one fixed local pose:
 *   new Engine(null, { deviceFK: true, devicePhysics: true, physicsContacts: 'all' })   rz_physics_contacts(ctx, 3) behind the upload
 * usage: node contact_boxbox_e2e.js <model.pmx> <localRotations.f32> <outdir> <time ms>...
 * Dumps the deformed positions, world matrices and body state of every frame (pos / world / state.f32). Prints the substeps every frame
 * asked for and the contact tuning keys. */
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
  const e = new Engine(null, { realtime: false, deviceFK: true, devicePhysics: true, physicsContacts: 'all' })
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
  fs.writeFileSync(path.join(out, 'pos.f32'), cat(pos))
  fs.writeFileSync(path.join(out, 'world.f32'), cat(world))
  fs.writeFileSync(path.join(out, 'state.f32'), cat(state))
  const keys = ['physics_contacts', 'physics_contact_follow', 'physics_contact_pairs', 'physics_contact_colours', 'physics_contact_boxes', 'physics_contact_box_pairs', 'physics_contact_box_box'].map((k) => e.native.getTuning(e.ctx, k))
  e.dispose()
  console.log(JSON.stringify({ times, substeps, keys }))
})().catch((e) => { console.error(e); process.exit(1) })
