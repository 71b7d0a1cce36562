'use strict'
/* CPU test of { qdef: true } with a recording stand-in for the native addon: loadModel uploads, on every shard context, the model's QDEF
 * vertices that fall in the shard with indices re-based to it; { qdef: false } (the default) never calls uploadQdef. Prints one JSON line. */
const path = require('path')
const { Engine, Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const V = 600
const qdefIdx = [0, 17, 250, 255, 256, 257, 400, 599]
const mk = () => {
  const bones = ['root', 'a', 'b'].map((name, i) => ({ name, parentIndex: i - 1, bindTranslation: [0, 1, 0], children: [] }))
  const m = new Model(new Float32Array(V * 8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(48) },
    { joints: new Uint16Array(V * 4), weights: new Uint8Array(V * 4).fill(255) }, [], [], null)
  m.qdef = Uint32Array.from(qdefIdx)
  return m
}
const run = async (opts) => {
  const calls = []
  let id = 0
  const native = {
    create: () => ({ id: 'ctx' + id++ }), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {},
    uploadSdef: () => calls.push({ sdef: true }),
    uploadQdef: (c, idx) => calls.push({ ctx: c.id, idx: Array.from(idx) }),
    shardRange: (v, n, r) => { const chunk = 256; const b = Math.min(v, r * chunk); return [b, r === n - 1 ? v - b : Math.min(chunk, v - b)] },
  }
  const e = new Engine(null, Object.assign({ realtime: false }, opts))
  e.native = native
  e.shards = [0, 1].map(() => ({ ctx: native.create(), begin: 0, count: 0, fork: null, last: null, flip: 0 }))
  e.ctx = e.shards[0].ctx
  await e.setupModelBuffers(mk())
  return { calls, shards: e.shards.map((s) => [s.begin, s.count]) }
}
;(async () => {
  console.log(JSON.stringify({ on: await run({ qdef: true }), off: await run({}), qdefIdx }))
})().catch((err) => { console.error(err); process.exit(1) })
