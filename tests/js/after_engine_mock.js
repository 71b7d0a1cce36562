'use strict'
/* CPU test of the loader's after-physics fields and of Engine { afterPhysics } with a recording stand-in for the native addon, on a
 * synthetic PMX with flag 0x1000 bones, transform levels and an IK block: uploadAfterPhysics(ctx, order) follows uploadSkeletonTopology on
 * every shard at loadModel — and uploadIK when { ik } is on too; a fork made for framesInFlight: 2 gets no call of its own (it borrows
 * the list); the engine makes no such call without the option ('off': the stand-in for that engine has no uploadAfterPhysics at all);
 * the option without deviceFK throws.
 * usage: node after_engine_mock.js <model.pmx> <option: after | ik | fork | off>...
 * Prints the loader's fields, Model.afterPhysicsOrder() and the calls per option and shard. */
const fs = require('fs'), path = require('path')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, ...options] = process.argv.slice(2)
const mkNative = (calls, withAfter) => Object.assign({
  create: () => ({}), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, shardRange: (v, g, r) => [r * (v >> 1), r ? v - (v >> 1) : (g > 1 ? v >> 1 : v)],
  uploadSkeletonTopology: (c) => calls[c.id].push('topology'),
  uploadIK: (c) => calls[c.id].push('uploadIK'),
  fork: (c) => { calls[c.id].push('fork'); return { id: c.id, fork: true } },
  setPoseLocal: (c) => calls[c.id].push('setPoseLocal' + (c.fork ? ':fork' : '')), deform: (c) => calls[c.id].push('deform'),
  overrideWorld: (c) => calls[c.id].push('overrideWorld' + (c.fork ? ':fork' : '')), read: () => {},
}, withAfter ? { uploadAfterPhysics: (c, bones) => calls[c.id].push('uploadAfterPhysics:' + Array.from(bones).join(',') + (c.fork ? ':fork' : '') + (bones instanceof Uint32Array ? '' : ':not-u32')) } : {})
const threw = (fn, re) => { try { fn() } catch (err) { return re.test(err.message) } return false }
const optsOf = (tag) => (tag === 'off' ? {} : tag === 'ik' ? { afterPhysics: true, ik: true } : tag === 'fork' ? { afterPhysics: true, framesInFlight: 2 } : { afterPhysics: true })
;(async () => {
  const buf = fs.readFileSync(pmx)
  const out = { shards: 3 }
  const model = PmxLoader.loadFromBuffer(buf)
  const bones = model.getSkeleton().bones
  out.fields = bones.map((b) => ({ after: 'afterPhysics' in b ? b.afterPhysics : null, level: 'transformLevel' in b ? b.transformLevel : null }))
  out.order = model.afterPhysicsOrder()
  out.needsDeviceFK = threw(() => new Engine(null, { afterPhysics: true }), /afterPhysics needs.*solveAfterPhysics/)
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
