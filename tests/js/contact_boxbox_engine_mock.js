'use strict'
/* CPU test of Engine { physicsContacts: 'all' } with a recording stand-in for the native addon, on a PMX whose colliders are boxes:
 * physicsContacts(ctx, 3) follows uploadPhysics on every shard at loadModel, 'boxes' still passes 2 and `true` 1, and 'all' without
 * devicePhysics throws as they do.
 * usage: node contact_boxbox_engine_mock.js <model.pmx> */
const fs = require('fs'), path = require('path')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx] = process.argv.slice(2)
const mkNative = (calls) => ({
  create: () => ({}), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, shardRange: (v, g, r) => [r * (v >> 1), r ? v - (v >> 1) : (g > 1 ? v >> 1 : v)],
  uploadSkeletonTopology: (c) => calls[c.id].push('topology'),
  uploadPhysics: (c) => calls[c.id].push('uploadPhysics'),
  physicsStep: (c, n) => calls[c.id].push('physicsStep:' + n), physicsReset: (c) => calls[c.id].push('physicsReset'),
  physicsContacts: (c, on) => calls[c.id].push('physicsContacts:' + on),
  setPoseLocal: (c) => calls[c.id].push('setPoseLocal'), deform: (c) => calls[c.id].push('deform'), overrideWorld: () => {}, read: () => {},
})
const threw = (fn, re) => { try { fn() } catch (err) { return re.test(err.message) } return false }
;(async () => {
  const buf = fs.readFileSync(pmx)
  const out = { shards: 3 }
  out.needsDevicePhysics = threw(() => new Engine(null, { deviceFK: true, physicsContacts: 'all' }), /devicePhysics/)
  for (const [tag, opt] of [['all', 'all'], ['boxes', 'boxes'], ['plain', true], ['other', 'everything']]) {
    const calls = Array.from({ length: out.shards }, () => [])
    const e = new Engine(null, { realtime: false, deviceFK: true, devicePhysics: true, physicsContacts: opt })
    e.native = mkNative(calls); e.ctx = { id: 0 }
    e.shards = calls.map((_, id) => ({ ctx: id ? { id } : e.ctx, begin: 0, count: 0 }))
    await e.setupModelBuffers(PmxLoader.loadFromBuffer(buf))
    e.step(0); e.step(50)
    out[tag] = calls
  }
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
