'use strict'
/* CPU test of Engine { physicsAligned } with a recording stand-in for the native addon, on a PMX with rigid-body and joint sections:
 * physicsAligned(ctx, 1) follows uploadPhysics on every shard at loadModel, ahead of physicsSprings and physicsContacts when those are
 * asked for too ('all'); the engine makes no such call without the option ('off': the stand-in for that engine has no physicsAligned at
 * all), and the option without devicePhysics throws.
 * usage: node align_engine_mock.js <model.pmx> <option: aligned | all | off>...
 * Prints the calls per option and shard; needsDevicePhysics / needsDeviceFK: { physicsAligned: true } without the other one throws. */
const fs = require('fs'), path = require('path')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, ...options] = process.argv.slice(2)
const mkNative = (calls, withAligned) => Object.assign({
  create: () => ({}), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, shardRange: (v, g, r) => [r * (v >> 1), r ? v - (v >> 1) : (g > 1 ? v >> 1 : v)],
  uploadSkeletonTopology: (c) => calls[c.id].push('topology'),
  uploadPhysics: (c) => calls[c.id].push('uploadPhysics'),
  physicsContacts: (c, on) => calls[c.id].push('physicsContacts:' + on),
  physicsStep: (c, n) => calls[c.id].push('physicsStep:' + n), physicsReset: (c) => calls[c.id].push('physicsReset'),
  setPoseLocal: (c) => calls[c.id].push('setPoseLocal'), deform: (c) => calls[c.id].push('deform'), overrideWorld: () => {}, read: () => {},
  physicsSprings: (c, on) => calls[c.id].push('physicsSprings:' + on),
}, withAligned ? { physicsAligned: (c, on) => calls[c.id].push('physicsAligned:' + on) } : {})
const threw = (fn, re) => { try { fn() } catch (err) { return re.test(err.message) } return false }
const optsOf = (tag) => (tag === 'off' ? {} : tag === 'all' ? { physicsAligned: true, physicsSprings: true, physicsContacts: true } : { physicsAligned: true })
;(async () => {
  const buf = fs.readFileSync(pmx)
  const out = { shards: 3 }
  out.needsDevicePhysics = threw(() => new Engine(null, { deviceFK: true, physicsAligned: true }), /physicsAligned needs/)
  out.needsDeviceFK = threw(() => new Engine(null, { devicePhysics: true, physicsAligned: true }), /deviceFK/)
  for (const tag of options) {
    const calls = Array.from({ length: out.shards }, () => [])
    const e = new Engine(null, Object.assign({ realtime: false, deviceFK: true, devicePhysics: true }, optsOf(tag)))
    e.native = mkNative(calls, tag !== 'off'); e.ctx = { id: 0 }
    e.shards = calls.map((_, id) => ({ ctx: id ? { id } : e.ctx, begin: 0, count: 0 }))
    await e.setupModelBuffers(PmxLoader.loadFromBuffer(buf))
    e.step(0); e.step(50)
    out[tag] = calls
  }
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
