'use strict'
/* End-to-end QDEF through the N-API boundary: Engine({ qdef: true | false }) -> reze_deform.node -> libreze_deform.so -> MI355X.
 * usage: node qdef_e2e.js <model.pmx> <outdir>
 * Loads the model twice (with and without QDEF), twists bones with rotateBones, and dumps the parse, the world matrices the frame used
 * and the deformed output; pytest recomputes both frames with tests/qdef_ref.py. */
const fs = require('fs'), path = require('path')
const { Engine, Quat } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const twistOf = require('./qdef_twist')
const [pmx, out] = process.argv.slice(2)
const dump = (name, ta) => fs.writeFileSync(path.join(out, name), Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength))
;(async () => {
  console.warn = () => {}
  for (const on of [true, false]) {
    const engine = new Engine(null, { realtime: false, qdef: on })
    await engine.init()
    await engine.loadModel(pmx)
    const model = engine.currentModel
    const names = model.getBoneNames()
    engine.step(0)
    const [twist, quats] = twistOf(names, Quat)
    engine.rotateBones(twist, quats, 100)
    engine.step(1000)
    const d = engine.getDeformed()
    const tag = on ? 'on' : 'off'
    dump('pos_' + tag + '.f32', d.positions); dump('nrm_' + tag + '.f32', d.normals)
    if (on) {
      dump('vertices.f32', model.getVertices()); dump('joints.u16', model.getSkinning().joints)
      dump('weights.u8', model.getSkinning().weights); dump('invbind.f32', model.getSkeleton().inverseBindMatrices)
      dump('world.f32', model.getBoneWorldMatrices())
      console.log(JSON.stringify({ index: Array.from(model.getQdef()) }))
    }
    engine.dispose()
  }
})().catch((e) => { console.error(e); process.exit(1) })
