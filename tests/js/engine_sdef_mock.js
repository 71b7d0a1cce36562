'use strict'
/* CPU test of { sdef: true } with a recording stand-in for the native addon: loadModel uploads, on every shard context, the model's SDEF
 * vertices that fall in the shard with indices re-based to it; { sdef: false } (the default) never calls uploadSdef. Prints one JSON line. */
const path = require('path')
const { Engine, Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const V = 600
const sdefIdx = [3, 17, 250, 255, 256, 257, 400, 599]
const mk = () => {
  const bones = ['root', 'a', 'b'].map((name, i) => ({ name, parentIndex: i - 1, bindTranslation: [0, 1, 0], children: [] }))
  const m = new Model(new Float32Array(V * 8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(48) },
    { joints: new Uint16Array(V * 4), weights: new Uint8Array(V * 4).fill(255) }, [], [], null)
  const n = sdefIdx.length
  m.sdef = { index: Uint32Array.from(sdefIdx), c: Float32Array.from({ length: n * 3 }, (_, i) => i), r0: Float32Array.from({ length: n * 3 }, (_, i) => 100 + i),
    r1: Float32Array.from({ length: n * 3 }, (_, i) => 200 + i) }
  return m
}
const run = async (opts) => {
  const calls = []
  let id = 0
  const native = {
    create: () => ({ id: 'ctx' + id++ }), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {},
    uploadSdef: (c, idx, cc, r0, r1) => calls.push({ ctx: c.id, idx: Array.from(idx), c: Array.from(cc), r0: Array.from(r0), r1: Array.from(r1) }),
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
  console.log(JSON.stringify({ on: await run({ sdef: true }), off: await run({}), sdefIdx }))
})().catch((err) => { console.error(err); process.exit(1) })
