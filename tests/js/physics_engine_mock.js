'use strict'
/* CPU test of Engine { devicePhysics } with a recording stand-in for the native addon, on a PMX with rigid-body and joint sections:
 * the table is uploaded once per shard after the topology, every frame asks for min(10, floor(accumulated / h)) substeps between the
 * pose and the frame, resetPhysics() reaches every shard and drops the accumulated time, and the option's preconditions throw.
 * usage: node physics_engine_mock.js <model.pmx> <time ms>... */
const fs = require('fs'), path = require('path')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, ...ts] = process.argv.slice(2)
const mkNative = (calls) => ({
  create: () => ({}), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, shardRange: (v, g, r) => [r * (v >> 1), r ? v - (v >> 1) : (g > 1 ? v >> 1 : v)],
  uploadSkeletonTopology: (c) => calls.push(['topology', c.id]),
  uploadPhysics: (c, t, o) => calls.push(['uploadPhysics', c.id, t.nBodies, t.nJoints, t.bone.length, t.offsetRot.length, o === undefined]),
  physicsStep: (c, n) => calls.push(['physicsStep', c.id, n]), physicsReset: (c) => calls.push(['physicsReset', c.id]),
  setPoseLocal: (c) => calls.push(['setPoseLocal', c.id]), deform: (c) => calls.push(['deform', c.id]), overrideWorld: () => calls.push(['overrideWorld']), read: () => {},
})
const threw = (fn, re) => { try { fn() } catch (err) { return re.test(err.message) } return false }
;(async () => {
  const buf = fs.readFileSync(pmx)
  const out = {}
  out.needsDeviceFK = threw(() => new Engine(null, { devicePhysics: true }), /deviceFK/)
  out.exclusiveWithHook = threw(() => new Engine(null, { deviceFK: true, devicePhysics: true, physics: { step() {} } }), /exclusive/)
  let msg = ''
  await new Engine(null, { deviceFK: true, devicePhysics: true, framesInFlight: 2 }).init().catch((err) => { msg = err.message })
  out.noFramesInFlight = /framesInFlight/.test(msg)
  const calls = []
  const e = new Engine(null, { realtime: false, deviceFK: true, devicePhysics: true })
  e.native = mkNative(calls); e.ctx = { id: 0 }; e.shards = [{ ctx: e.ctx, begin: 0, count: 0 }, { ctx: { id: 1 }, begin: 0, count: 0 }]
  await e.setupModelBuffers(PmxLoader.loadFromBuffer(buf))
  out.upload = calls.slice()
  calls.length = 0
  for (const t of ts.map(Number)) e.step(t)
  out.frames = calls.slice()
  out.overridesRefused = threw(() => e.setBoneWorldOverrides([1], new Float32Array(16)), /devicePhysics/)
  calls.length = 0
  const last = Number(ts[ts.length - 1])
  e.step(last + 10)            // 10 ms: under one substep, it stays in the accumulator ...
  e.resetPhysics()             // ... until the reset drops it
  e.step(last + 20)
  out.reset = calls.filter((c) => c[0] === 'physicsStep' || c[0] === 'physicsReset')
  // without the option nothing of it is called; resetPhysics says what it needs
  calls.length = 0
  const p = new Engine(null, { realtime: false, deviceFK: true })
  p.native = mkNative(calls); p.ctx = { id: 0 }; p.shards = [{ ctx: p.ctx, begin: 0, count: 0 }]
  await p.setupModelBuffers(PmxLoader.loadFromBuffer(buf))
  p.step(0); p.step(100)
  out.plain = calls.map((c) => c[0])
  out.plainRefusesReset = threw(() => p.resetPhysics(), /devicePhysics/)
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
