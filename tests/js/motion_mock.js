'use strict'
/* CPU test of Engine.loadMotion / seekMotions with a recording stand-in for the native addon: the library is uploaded once per (library,
 * model) and again after loadMotion replaces a clip; one 20-byte state goes out per instance; forks are dropped before the upload; an
 * unknown name and a wrong state count throw; without { deviceSampling } one character is posed on the host. Prints one JSON line.
 * usage: node motion_mock.js <a.vmd> <b.vmd> */
const path = require('path')
const { Engine, Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [vmdA, vmdB] = process.argv.slice(2)
const mk = () => {
  const bones = ['bone0', 'bone1', 'bone3'].map((name, i) => ({ name, parentIndex: i - 1, bindTranslation: [0, 1, 0], children: [] }))
  return new Model(new Float32Array(8 * 8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(48) },
    { joints: new Uint16Array(8 * 4), weights: new Uint8Array(8 * 4).fill(255) }, [], [], null)
}
const decode = (buf) => {
  const dv = new DataView(buf), out = []
  for (let i = 0; i < buf.byteLength / 20; i++) out.push([dv.getUint32(i * 20, true), dv.getFloat32(i * 20 + 4, true), dv.getUint32(i * 20 + 8, true), dv.getFloat32(i * 20 + 12, true), dv.getFloat32(i * 20 + 16, true)])
  return out
}
const errorOf = (fn) => { try { fn(); return null } catch (e) { return String(e.message) } }
;(async () => {
  const calls = []
  let id = 0
  const native = {
    create: () => ({ id: 'ctx' + id++ }), destroy: (c) => calls.push({ destroy: c.id }), uploadMesh: () => {}, uploadSkeleton: () => {}, uploadSkeletonTopology: () => {},
    uploadBoneMorphs: () => {}, setInstances: (c, n) => calls.push({ setInstances: n }), shardRange: (v) => [0, v], fork: (c) => { const f = { id: 'fork' + id++ }; calls.push({ fork: f.id }); return f },
    uploadMotions: (c, flats) => calls.push({ uploadMotions: c.id, clips: flats.length, tracks: flats.map((f) => f.trackBone.length) }),
    setPoseBlended: (c, buf) => calls.push({ setPoseBlended: c.id, states: decode(buf) }), deform: (c) => calls.push({ deform: c.id }),
    setPoseLocal: (c, q, mw, t) => calls.push({ setPoseLocal: c.id }), setPose: (c, w) => calls.push({ setPose: c.id, w0: Array.from(w.slice(16, 32)) }),
  }
  const out = {}
  const e = new Engine(null, { realtime: false, deviceFK: true, deviceSampling: true, framesInFlight: 2 })
  e.native = native
  e.shards = [{ ctx: native.create(), begin: 0, count: 0, fork: null, last: null, flip: 0 }]
  e.ctx = e.shards[0].ctx
  await e.setupModelBuffers(mk())
  await e.loadMotion('walk', vmdA)
  await e.loadMotion('run', vmdB)
  e.seekMotions({ a: 'walk', frameA: 3.5 })
  e.seekMotions({ a: 'walk', frameA: 4.5, b: 'run', frameB: 2, blend: 0.25 })         // the second frame runs on the fork
  out.forkMade = calls.some((c) => c.fork)
  await e.loadMotion('run', vmdA)                                                    // replaces a clip: uploaded again, the fork goes first
  e.seekMotions({ a: 'run', frameA: 1 })
  e.setInstanceCount(3)
  e.seekMotions([{ a: 'walk', frameA: 1 }, { a: 'run', frameA: 2, b: 'walk', frameB: 3, blend: 1 }, { a: 'walk', frameA: 5, b: 'walk', frameB: 6, blend: 0.5 }])
  e.seekMotions({ a: 'run', frameA: 9 })                                             // one state poses every instance
  out.calls = calls.slice()
  out.unknown = errorOf(() => e.seekMotions({ a: 'jump', frameA: 0 }))
  out.unknownB = errorOf(() => e.seekMotions({ a: 'walk', frameA: 0, b: 'jump', frameB: 0, blend: 0.5 }))
  out.wrongCount = errorOf(() => e.seekMotions([{ a: 'walk', frameA: 0 }, { a: 'walk', frameA: 1 }]))
  // host path: one character through Model.applyBlendedFrame + render()
  calls.length = 0
  const h = new Engine(null, { realtime: false })
  h.native = native
  h.shards = [{ ctx: native.create(), begin: 0, count: 0, fork: null, last: null, flip: 0 }]
  h.ctx = h.shards[0].ctx
  await h.setupModelBuffers(mk())
  await h.loadMotion('walk', vmdA)
  await h.loadMotion('run', vmdB)
  h.seekMotions({ a: 'walk', frameA: 4.5, b: 'run', frameB: 2, blend: 0.25 })
  out.hostCalls = calls.slice()
  out.hostRot1 = Array.from(h.currentModel.runtimeSkeleton.localRotations.slice(4, 8))
  out.hostCrowd = errorOf(() => h.seekMotions([{ a: 'walk', frameA: 0 }, { a: 'walk', frameA: 1 }]))
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
