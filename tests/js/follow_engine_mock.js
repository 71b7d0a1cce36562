'use strict'
/* CPU test of Engine { followOverrides } with a recording stand-in for the native addon, on a PMX with rigid-body and joint sections:
 * overrideFollow(ctx, 1) follows uploadSkeletonTopology on every shard at loadModel, with devicePhysics and without it; a fork made for
 * framesInFlight: 2 gets the call too; the engine makes no such call without the option ('off': the stand-in for that engine has no
 * overrideFollow at all); the option without deviceFK throws.
 * usage: node follow_engine_mock.js <model.pmx> <option: follow | physics | fork | off>...
 * Prints the calls per option and shard. */
const fs = require('fs'), path = require('path')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, ...options] = process.argv.slice(2)
const mkNative = (calls, withFollow) => Object.assign({
  create: () => ({}), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, shardRange: (v, g, r) => [r * (v >> 1), r ? v - (v >> 1) : (g > 1 ? v >> 1 : v)],
  uploadSkeletonTopology: (c) => calls[c.id].push('topology'),
  uploadPhysics: (c) => calls[c.id].push('uploadPhysics'),
  physicsStep: (c, n) => calls[c.id].push('physicsStep:' + n), physicsReset: (c) => calls[c.id].push('physicsReset'),
  fork: (c) => { calls[c.id].push('fork'); return { id: c.id, fork: true } },
  setPoseLocal: (c) => calls[c.id].push('setPoseLocal' + (c.fork ? ':fork' : '')), deform: (c) => calls[c.id].push('deform'),
  overrideWorld: (c) => calls[c.id].push('overrideWorld' + (c.fork ? ':fork' : '')), read: () => {},
}, withFollow ? { overrideFollow: (c, on) => calls[c.id].push('overrideFollow:' + on + (c.fork ? ':fork' : '')) } : {})
const threw = (fn, re) => { try { fn() } catch (err) { return re.test(err.message) } return false }
const optsOf = (tag) => (tag === 'off' ? { devicePhysics: true } : tag === 'physics' ? { followOverrides: true, devicePhysics: true }
  : tag === 'fork' ? { followOverrides: true, framesInFlight: 2 } : { followOverrides: true })
;(async () => {
  const buf = fs.readFileSync(pmx)
  const out = { shards: 3 }
  out.needsDeviceFK = threw(() => new Engine(null, { followOverrides: true }), /followOverrides needs/)
  out.needsDeviceFKWithPhysicsHook = threw(() => new Engine(null, { followOverrides: true, physics: { step() {} } }), /followOverrides needs/)
  for (const tag of options) {
    const calls = Array.from({ length: out.shards }, () => [])
    const e = new Engine(null, Object.assign({ realtime: false, deviceFK: true }, optsOf(tag)))
    e.native = mkNative(calls, tag !== 'off'); e.ctx = { id: 0 }
    e.shards = calls.map((_, id) => ({ ctx: id ? { id } : e.ctx, begin: 0, count: 0 }))
    await e.setupModelBuffers(PmxLoader.loadFromBuffer(buf))
    if (tag === 'fork') {
      e.shards.forEach((s) => { s.count = 1 })
      e.setBoneWorldOverrides([1], Float32Array.from({ length: 16 }, (_, k) => (k % 5 === 0 ? 1 : 0)))
    }
    e.step(0); e.step(50)
    out[tag] = calls
  }
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
