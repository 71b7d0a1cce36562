'use strict'
/* End-to-end VMD IK on / off keys through the N-API boundary on a PMX leg rig + a VMD whose show / IK keys switch the right leg off at frame 30:
 *   device:  new Engine(null, { deviceFK: true, deviceSampling: true, ik: true, ikKeys: true })   rz_upload_ik_keys, evaluated by rz_set_pose_sampled
 *   local:   new Engine(null, { deviceFK: true, ik: true, ikKeys: true })                         host-sampled pose + rz_set_ik_enabled
 *   host:    new Engine(null, { ik: true, ikKeys: true })                                         Model.solveIK() with the model's switches
 *   nokeys:  new Engine(null, { ik: true })                                                       the keys are not honoured: as before
 * usage: node ik_switch_e2e.js <model.pmx> <motion.vmd> <outdir> <plain.vmd>. Dumps the deformed positions of frames 29 and 31 and, with
 * plain.vmd (a motion without a show / IK block) loaded behind it, of its frame 31, one file per engine: the old switches must not stay. */
const fs = require('fs'), path = require('path')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmd, out, plain] = process.argv.slice(2)
;(async () => {
  console.warn = () => {}
  const frames = [29, 31]
  const res = {}
  const dev = { deviceFK: true, deviceSampling: true, ik: true, ikKeys: true }
  for (const [tag, opts] of [['device', dev], ['local', { deviceFK: true, ik: true, ikKeys: true }], ['host', { ik: true, ikKeys: true }], ['nokeys', { ik: true }]]) {
    const e = new Engine(null, Object.assign({ realtime: false }, opts))
    await e.init(); await e.loadModel(pmx); await e.loadAnimation(vmd)
    const parts = [], masks = []
    const ikFrames = e.animationFrames.ikFrames.length
    const seek = (f) => {
      e.seekFrame(f); parts.push(Float32Array.from(e.getDeformed().positions))
      masks.push(opts.deviceFK ? Array.from(e.native.readIKEnabled(e.ctx)) : e.currentModel.getIKChainEnabled().map((x) => (x ? 1 : 0)))
    }
    for (const f of frames) seek(f)
    const switched = opts.deviceFK ? e.native.getTuning(e.ctx, 'ik_switched') : -1, keySets = opts.deviceFK ? e.native.getTuning(e.ctx, 'ik_key_sets') : -1
    await e.loadAnimation(plain)
    seek(31)
    const all = new Float32Array(parts.reduce((n, p) => n + p.length, 0))
    let o = 0
    for (const p of parts) { all.set(p, o); o += p.length }
    fs.writeFileSync(path.join(out, 'pos_' + tag + '.f32'), Buffer.from(all.buffer))
    res[tag] = { masks, ikFrames, switched, keySets }
    e.dispose()
  }
  console.log(JSON.stringify(Object.assign({ frames }, res)))
})().catch((e) => { console.error(e); process.exit(1) })
