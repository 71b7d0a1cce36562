'use strict'
/* CPU test of Engine { physicsContacts } with a recording stand-in for the native addon, on a PMX with rigid-body and joint sections:
 * physicsContacts(ctx, 1) follows uploadPhysics on every shard at loadModel, the engine makes no such call without the option (the
 * stand-in for that engine has no physicsContacts at all), and the invalid combinations throw.
 * usage: node contacts_engine_mock.js <model.pmx> */
const fs = require('fs'), path = require('path')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx] = process.argv.slice(2)
const mkNative = (calls, withContacts) => Object.assign({
  create: () => ({}), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, shardRange: (v, g, r) => [r * (v >> 1), r ? v - (v >> 1) : (g > 1 ? v >> 1 : v)],
  uploadSkeletonTopology: (c) => calls[c.id].push('topology'),
  uploadPhysics: (c) => calls[c.id].push('uploadPhysics'),
  physicsStep: (c, n) => calls[c.id].push('physicsStep:' + n), physicsReset: (c) => calls[c.id].push('physicsReset'),
  setPoseLocal: (c) => calls[c.id].push('setPoseLocal'), deform: (c) => calls[c.id].push('deform'), overrideWorld: () => {}, read: () => {},
}, withContacts ? { physicsContacts: (c, on) => calls[c.id].push('physicsContacts:' + on) } : {})
const threw = (fn, re) => { try { fn() } catch (err) { return re.test(err.message) } return false }
;(async () => {
  const buf = fs.readFileSync(pmx)
  const out = { shards: 3 }
  out.needsDevicePhysics = threw(() => new Engine(null, { deviceFK: true, physicsContacts: true }), /devicePhysics/)
  out.needsDeviceFK = threw(() => new Engine(null, { devicePhysics: true, physicsContacts: true }), /deviceFK/)
  for (const on of [true, false]) {
    const calls = Array.from({ length: out.shards }, () => [])
    const e = new Engine(null, Object.assign({ realtime: false, deviceFK: true, devicePhysics: true }, on ? { physicsContacts: true } : {}))
    e.native = mkNative(calls, on); e.ctx = { id: 0 }
    e.shards = calls.map((_, id) => ({ ctx: id ? { id } : e.ctx, begin: 0, count: 0 }))
    await e.setupModelBuffers(PmxLoader.loadFromBuffer(buf))
    e.step(0); e.step(50)
    out[on ? 'on' : 'off'] = calls
  }
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
