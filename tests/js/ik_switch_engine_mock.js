'use strict'
/* CPU test of { ikKeys: true } with a recording stand-in for the native addon: with { ik, ikKeys, deviceFK, deviceSampling } uploadIKKeys
 * follows uploadAnimation / uploadMotions on every shard with instances; host-sampled deviceFK frames send setIKEnabled behind
 * setPoseLocal; a motion or library WITHOUT keys that follows one with keys uploads a set of no keys ("all on") instead of leaving the old
 * switches in place; switches held by hand are laid over the motion's, one by one, and handed back; without ikKeys the engine makes none
 * of the new calls; ikKeys without ik throws. Prints one JSON line. */
const path = require('path')
const { Engine, Model, Quat, Vec3 } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const V = 600
const mk = () => {
  const names = ['root', 'leg', 'knee', 'ankle', 'legIK', 'toe', 'toeIK']
  const parent = [-1, 0, 1, 2, 0, 3, 4]
  const bones = names.map((name, i) => ({ name, parentIndex: parent[i], bindTranslation: [0, 1, 0], children: [] }))
  bones[4].ik = { effector: 3, loops: 40, limitAngle: 2, links: [{ bone: 2, min: [-3.1415927, 0, 0], max: [-0.0087266, 0, 0] }, { bone: 1 }] }
  bones[6].ik = { effector: 5, loops: 3, limitAngle: 4, links: [{ bone: 3 }] }
  return new Model(new Float32Array(V * 8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(7 * 16) },
    { joints: new Uint16Array(V * 4), weights: new Uint8Array(V * 4).fill(255) }, [], [], null)
}
const motion = (ik) => {
  const q = new Quat(0, 0, 0, 1), p = new Vec3(0, 0, 0)
  const kf = [{ time: 0, boneFrames: [{ boneName: 'legIK', frame: 0, rotation: q, position: p }] }, { time: 1, boneFrames: [{ boneName: 'legIK', frame: 30, rotation: q, position: p }] }]
  kf.morphFrames = []
  kf.ikFrames = ik ? [{ frame: 0, time: 0, show: true, ik: [{ name: 'legIK', enabled: false }, { name: 'armIK', enabled: false }] }, { frame: 20, time: 20 / 30, show: true, ik: [{ name: 'legIK', enabled: true }, { name: 'toeIK', enabled: false }] }] : []
  return kf
}
const run = async (opts, scenario) => {
  const calls = []
  let id = 0
  const rec = (fn, extra) => (c, ...a) => { calls.push(Object.assign({ fn, ctx: c.id }, extra ? extra(...a) : {})) }
  const native = {
    create: () => ({ id: 'ctx' + id++ }), destroy: () => {}, uploadMesh: () => {}, uploadSkeleton: () => {}, uploadSkeletonTopology: () => {}, uploadIK: rec('ik'),
    uploadAnimation: rec('animation'), uploadMotions: rec('motions', (f) => ({ n: f.length })),
    uploadIKKeys: rec('ikKeys', (clip, frames, enabled) => ({ clip, frames: Array.from(frames), enabled: Array.from(enabled) })),
    setIKEnabled: rec('setIK', (m) => ({ mask: m ? Array.from(m) : null })),
    readIKEnabled: (c) => { calls.push({ fn: 'readIK', ctx: c.id }); return Uint8Array.from([0, 1]) }, // what the keys give at frame 10: legIK off
    setPoseSampled: rec('sampled'), setPoseBlended: rec('blended'), setPoseLocal: rec('local'), setPose: rec('world'), deform: () => {}, timing: () => ({}),
    shardRange: (v, n, r) => { const chunk = 256; const b = Math.min(v, r * chunk); return [b, r === n - 1 ? v - b : Math.min(chunk, v - b)] },
  }
  const e = new Engine(null, Object.assign({ realtime: false }, opts))
  e.native = native
  e.shards = [0, 1, 2].map(() => ({ ctx: native.create(), begin: 0, count: 0, fork: null, last: null, flip: 0 }))
  e.ctx = e.shards[0].ctx
  const model = mk()
  await e.setupModelBuffers(model)
  e.shards[2].count = 0 // a shard without instances / vertices takes no call
  e.updateStats = () => {}
  const { VMDSampler } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
  if (scenario === 'seek') {
    e.animationFrames = motion(true); e.hasAnimation = true
    e.seekFrame(10); e.seekFrame(25)
  } else if (scenario === 'motions') {
    e.motions.set('walk', new VMDSampler(motion(true))); e.motions.set('idle', new VMDSampler(motion(false))); e.motionsVersion++
    e.seekMotions({ a: 'walk', frameA: 3 })
  } else if (scenario === 'manual') {
    e.animationFrames = motion(true); e.hasAnimation = true
    e.setIKEnabled('toeIK', false)
    e.seekFrame(10)
    e.setIKEnabled('toeIK', null) // handed back
    e.seekFrame(10); e.seekFrame(10)
  } else if (scenario === 'seekThenPlain') {
    e.animationFrames = motion(true); e.hasAnimation = true
    e.seekFrame(10)
    e.animationFrames = motion(false)
    e.seekFrame(10)
  } else if (scenario === 'play') {
    model.setIKChainEnabled('toeIK', false) // left by an earlier playback or by hand
    e.animationFrames = motion(true); e.hasAnimation = true
    e.playAnimation()
  } else if (scenario === 'motionsPlain') {
    e.motions.set('idle', new VMDSampler(motion(false))); e.motionsVersion++
    e.seekMotions({ a: 'idle', frameA: 3 })
  }
  return { calls: calls.filter((c) => c.fn !== 'ik'), enabled: model.getIKChainEnabled() }
}
;(async () => {
  const dev = { ik: true, deviceFK: true, deviceSampling: true }
  let threw = null
  try { new Engine(null, { ikKeys: true, realtime: false }) } catch (err) { threw = String(err.message) }
  console.log(JSON.stringify({
    seek: await run(Object.assign({ ikKeys: true }, dev), 'seek'), motions: await run(Object.assign({ ikKeys: true }, dev), 'motions'),
    seekOff: await run(dev, 'seek'), motionsOff: await run(dev, 'motions'),
    hostSampled: await run({ ik: true, ikKeys: true, deviceFK: true }, 'seek'), hostSampledOff: await run({ ik: true, deviceFK: true }, 'seek'),
    host: await run({ ik: true, ikKeys: true }, 'seek'), hostOff: await run({ ik: true }, 'seek'),
    manual: await run(dev, 'manual'), manualKeys: await run(Object.assign({ ikKeys: true }, dev), 'manual'),
    seekThenPlain: await run(Object.assign({ ikKeys: true }, dev), 'seekThenPlain'), motionsPlain: await run(Object.assign({ ikKeys: true }, dev), 'motionsPlain'),
    play: await run({ ik: true, ikKeys: true }, 'play'), threw,
  }))
})().catch((err) => { console.error(err); process.exit(1) })
