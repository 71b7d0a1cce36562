'use strict'
/* End-to-end IK through the N-API boundary on a PMX + VMD that keys only the centre and the IK goals:
 *   device: new Engine(null, { deviceFK: true, deviceSampling: true, ik: true })   rz_upload_ik, solved by rz_fk_kernel<RzIkParams>
 *   host:   new Engine(null, { ik: true })                                         Model.solveIK()
 *   off:    new Engine(null, {})                                                   no IK: the legs do not follow
 * usage: node ik_e2e.js <model.pmx> <motion.vmd> <outdir>. Dumps the deformed positions of every frame, one file per engine. */
const fs = require('fs'), path = require('path')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmd, out] = process.argv.slice(2)
;(async () => {
  console.warn = () => {}
  const frames = [0, 7.5, 16, 23.25, 30]
  const res = {}
  for (const [tag, opts] of [['device', { deviceFK: true, deviceSampling: true, ik: true }], ['host', { ik: true }], ['off', {}]]) {
    const e = new Engine(null, Object.assign({ realtime: false }, opts))
    await e.init(); await e.loadModel(pmx); await e.loadAnimation(vmd)
    const parts = []
    for (const f of frames) { e.seekFrame(f); parts.push(Float32Array.from(e.getDeformed().positions)) }
    const all = new Float32Array(parts.reduce((n, p) => n + p.length, 0))
    let o = 0
    for (const p of parts) { all.set(p, o); o += p.length }
    fs.writeFileSync(path.join(out, 'pos_' + tag + '.f32'), Buffer.from(all.buffer))
    res[tag] = { chains: e.currentModel.getIKChains().length, hostIK: e.currentModel.ikEnabled }
    e.dispose()
  }
  console.log(JSON.stringify(Object.assign({ frames }, res)))
})().catch((e) => { console.error(e); process.exit(1) })
