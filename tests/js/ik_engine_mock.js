'use strict'
/* CPU test of { ik: true } with a recording stand-in for the native addon: with deviceFK, loadModel uploads the model's IK chains once
 * per shard context, after that context's topology; without deviceFK it switches the host solver on and uploads nothing; { ik: false }
 * (the default) does neither. Prints one JSON line. */
const path = require('path')
const { Engine, Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const V = 600
const mk = (withIk) => {
  const names = ['root', 'leg', 'knee', 'ankle', 'legIK']
  const bones = names.map((name, i) => ({ name, parentIndex: i === 4 ? 0 : i - 1, bindTranslation: [0, 1, 0], children: [] }))
  if (withIk) bones[4].ik = { effector: 3, loops: 40, limitAngle: 2, links: [{ bone: 2, min: [-3.1415927, 0, 0], max: [-0.0087266, 0, 0] }, { bone: 1 }] }
  return new Model(new Float32Array(V * 8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(5 * 16) },
    { joints: new Uint16Array(V * 4), weights: new Uint8Array(V * 4).fill(255) }, [], [], null)
}
const run = async (opts, withIk) => {
  const calls = []
  let id = 0
  const native = {
    create: () => ({ id: 'ctx' + id++ }), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {},
    uploadSkeletonTopology: (c) => calls.push({ fn: 'topology', ctx: c.id }),
    uploadIK: (c, goal, eff, loops, theta, off, lb, ll, lmin, lmax) => calls.push({ fn: 'ik', ctx: c.id, goal: Array.from(goal), effector: Array.from(eff),
      loops: Array.from(loops), theta: Array.from(theta), off: Array.from(off), bone: Array.from(lb), limited: Array.from(ll), min: Array.from(lmin), max: Array.from(lmax) }),
    shardRange: (v, n, r) => { const chunk = 256; const b = Math.min(v, r * chunk); return [b, r === n - 1 ? v - b : Math.min(chunk, v - b)] },
  }
  const e = new Engine(null, Object.assign({ realtime: false }, opts))
  e.native = native
  e.shards = [0, 1].map(() => ({ ctx: native.create(), begin: 0, count: 0, fork: null, last: null, flip: 0 }))
  e.ctx = e.shards[0].ctx
  const model = mk(withIk)
  await e.setupModelBuffers(model)
  return { calls, hostIK: model.ikEnabled }
}
;(async () => {
  console.log(JSON.stringify({
    device: await run({ deviceFK: true, ik: true }, true), host: await run({ ik: true }, true), off: await run({ deviceFK: true }, true),
    none: await run({ deviceFK: true, ik: true }, false), hostNone: await run({ ik: true }, false),
  }))
})().catch((err) => { console.error(err); process.exit(1) })
