'use strict'
/* CPU test of Engine.setMotionMask / seekMotions with layers against a recording stand-in for the native addon: a state without layers sends
 * what it sent before; the masks are uploaded once per (mask set, model) and again after setMotionMask; a state with layers is one
 * setPoseLayered in front of the same deform; shorter layer lists are padded with skipped layers; an unknown mask, motion or bone and more
 * than four layers throw; without { deviceSampling } one character is posed on the host. Prints one JSON line.
 * usage: node motion_layers_mock.js <model.pmx> <walk.vmd> <run.vmd> <face.vmd> */
const path = require('path'), fs = require('fs')
const { Engine, PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmdA, vmdB, vmdC] = process.argv.slice(2)
const mk = () => PmxLoader.loadFromBuffer(fs.readFileSync(pmx))
const f5 = (x) => Math.round(x * 1e5) / 1e5
const decode = (buf, kinds) => {
  const dv = new DataView(buf), out = []
  for (let i = 0; i < buf.byteLength / 20; i++) out.push(kinds.map((k, j) => (k === 'u' ? dv.getUint32(i * 20 + j * 4, true) : f5(dv.getFloat32(i * 20 + j * 4, true)))))
  return out
}
const errorOf = (fn) => { try { fn(); return null } catch (e) { return String(e.message) } }
;(async () => {
  const calls = []
  let id = 0
  const recorded = {
    create: () => ({ id: 'ctx' + id++ }), destroy: (c) => calls.push({ destroy: c.id }), shardRange: (v) => [0, v], fork: (c) => { const f = { id: 'fork' + id++ }; calls.push({ fork: f.id }); return f },
    uploadMotions: (c, flats) => calls.push({ uploadMotions: c.id, clips: flats.length }),
    uploadMotionMasks: (c, n, bones, morphs) => calls.push({ uploadMotionMasks: c.id, n, bones: bones.length, morphs: morphs !== null && morphs.length === n * 9 }),
    setPoseBlended: (c, buf) => calls.push({ setPoseBlended: c.id, states: decode(buf, ['u', 'f', 'u', 'f', 'f']) }),
    setPoseLayered: (c, buf, n, lbuf) => calls.push({ setPoseLayered: c.id, nLayers: n, states: decode(buf, ['u', 'f', 'u', 'f', 'f']), layers: decode(lbuf, ['u', 'f', 'f', 'u', 'u']) }),
    deform: (c) => calls.push({ deform: c.id }), setPose: (c) => calls.push({ setPose: c.id }),
  }
  const native = new Proxy(recorded, { get: (t, k) => (k in t ? t[k] : () => {}) })       // every other upload of loadModel is a no-op here
  const setup = async (opts) => {
    const e = new Engine(null, opts)
    e.native = native
    e.shards = [{ ctx: native.create(), begin: 0, count: 0, fork: null, last: null, flip: 0 }]
    e.ctx = e.shards[0].ctx
    await e.setupModelBuffers(mk())
    await e.loadMotion('walk', vmdA); await e.loadMotion('run', vmdB); await e.loadMotion('face', vmdC)
    return e
  }
  const out = {}
  const e = await setup({ realtime: false, deviceFK: true, deviceSampling: true })
  e.setMotionMask('upper', { bones: ['bone3'], withDescendants: true })
  e.seekMotions({ a: 'walk', frameA: 3.5 })
  out.plain = calls.filter((c) => c.setPoseBlended || c.setPoseLayered || c.deform || c.uploadMotionMasks).map((c) => Object.keys(c)[0])
  e.seekMotions({ a: 'walk', frameA: 3.5, layers: [{ motion: 'face', frame: 3.5 }] })
  e.seekMotions({ a: 'walk', frameA: 3.5, layers: [{ motion: 'face', frame: 3.5 }] })
  e.setMotionMask('face', { bones: [], morphs: ['v0', 'blink'] })
  e.seekMotions({ a: 'walk', frameA: 1, layers: [{ motion: 'run', frame: 2, weight: 0.5, mask: 'upper' }, { motion: 'face', frame: 7, weight: 0.25, mask: 'face', additive: true }] })
  e.setInstanceCount(3)
  e.seekMotions([{ a: 'walk', frameA: 1, layers: [{ motion: 'face', frame: 1 }] }, { a: 'run', frameA: 2, layers: [{ motion: 'run', frame: 4, weight: 0.5, mask: 'upper' }, { motion: 'face', frame: 4, mask: 'face', additive: true }] },
    { a: 'walk', frameA: 5 }])
  out.calls = calls.slice()
  out.unknownMask = errorOf(() => e.seekMotions({ a: 'walk', frameA: 0, layers: [{ motion: 'run', frame: 0, mask: 'legs' }] }))
  out.unknownMotion = errorOf(() => e.seekMotions({ a: 'walk', frameA: 0, layers: [{ motion: 'jump', frame: 0 }] }))
  out.tooMany = errorOf(() => e.seekMotions({ a: 'walk', frameA: 0, layers: new Array(5).fill({ motion: 'run', frame: 0 }) }))
  e.setMotionMask('bad', { bones: ['no such bone'] })
  out.unknownBone = errorOf(() => e.seekMotions({ a: 'walk', frameA: 0, layers: [{ motion: 'run', frame: 0, mask: 'upper' }] }))
  // host path: one character through Model.applyLayeredFrame + render()
  const h = await setup({ realtime: false })
  h.setMotionMask('upper', { bones: ['bone3'], withDescendants: true })
  calls.length = 0
  h.seekMotions({ a: 'walk', frameA: 4.5, layers: [{ motion: 'run', frame: 2, weight: 0.5, mask: 'upper' }] })
  out.hostCalls = calls.slice()
  out.hostCrowd = errorOf(() => h.seekMotions([{ a: 'walk', frameA: 0, layers: [] }, { a: 'walk', frameA: 1 }]))
  console.log(JSON.stringify(out))
})().catch((err) => { console.error(err); process.exit(1) })
