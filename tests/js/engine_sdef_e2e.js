'use strict'
/* End-to-end SDEF through the N-API boundary: Engine({ sdef: true | false }) -> reze_deform.node -> libreze_deform.so -> MI355X.
 * usage: node engine_sdef_e2e.js <model.pmx> <outdir>
 * Loads the model twice (with and without SDEF), twists bones with rotateBones, and dumps the parse, the world matrices the frame used
 * and the deformed output; pytest recomputes both frames with tests/sdef_ref.py. */
const fs = require('fs'), path = require('path')
const { Engine, Quat } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, out] = process.argv.slice(2)
const dump = (name, ta) => fs.writeFileSync(path.join(out, name), Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength))
;(async () => {
  console.warn = () => {}
  for (const on of [true, false]) {
    const engine = new Engine(null, { realtime: false, sdef: on })
    await engine.init()
    await engine.loadModel(pmx)
    const model = engine.currentModel
    const names = model.getBoneNames()
    engine.step(0)
    const twist = []
    for (let b = 2; b < names.length; b += 3) twist.push(names[b])
    engine.rotateBones(twist, twist.map((_, k) => new Quat(0.5 + 0.01 * k, 0.3, -0.2, 0.7).normalize()), 100)
    engine.step(1000)
    const d = engine.getDeformed()
    const tag = on ? 'on' : 'off'
    dump('pos_' + tag + '.f32', d.positions); dump('nrm_' + tag + '.f32', d.normals)
    if (on) {
      dump('vertices.f32', model.getVertices()); dump('joints.u16', model.getSkinning().joints)
      dump('weights.u8', model.getSkinning().weights); dump('invbind.f32', model.getSkeleton().inverseBindMatrices)
      dump('world.f32', model.getBoneWorldMatrices())
      const s = model.getSdef()
      console.log(JSON.stringify({ index: Array.from(s.index), c: Array.from(s.c), r0: Array.from(s.r0), r1: Array.from(s.r1) }))
    }
    engine.dispose()
  }
})().catch((e) => { console.error(e); process.exit(1) })
