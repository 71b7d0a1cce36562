'use strict'
/* Layered motion states through the N-API boundary: the same synthetic PMX and three VMDs (walk, run, a morph-only face file) posed at the
 * same states, with the same masks (Engine.setMotionMask, one of them withDescendants), by
 *   A: new Engine(null, { realtime: false })                                         seekMotions -> Model.applyLayeredFrame + host FK
 *   B: new Engine(null, { realtime: false, deviceFK: true, deviceSampling: true })   rz_upload_motion_masks + rz_set_pose_layered
 * then a crowd of three on B, each instance against the single-character frame of its state, bit for bit. The host model is put back at
 * rest before every state: the host leaves a bone or morph that no clip of the state keys alone, the device poses it at rest.
 * usage: node motion_layers_e2e.js <model.pmx> <walk.vmd> <run.vmd> <face.vmd> <states.json>   -> one JSON line */
const path = require('path'), fs = require('fs')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmdA, vmdB, vmdC, statesFile] = process.argv.slice(2)
const { masks, states } = JSON.parse(fs.readFileSync(statesFile, 'utf8'))
;(async () => {
  const quiet = console.warn; console.warn = () => {}
  const A = new Engine(null, { realtime: false })
  const B = new Engine(null, { realtime: false, deviceFK: true, deviceSampling: true })
  for (const e of [A, B]) {
    await e.init(); await e.loadModel(pmx); await e.loadMotion('walk', vmdA); await e.loadMotion('run', vmdB); await e.loadMotion('face', vmdC)
    for (const name of Object.keys(masks)) e.setMotionMask(name, masks[name])
  }
  let worst = 0, moved = 0
  const single = []
  const dist = (a, b) => { let m = 0; for (let k = 0; k < a.length; k++) m = Math.max(m, Math.abs(a[k] - b[k])); return m }
  states.forEach((st) => {
    const rs = A.currentModel.runtimeSkeleton
    for (let b = 0; b < rs.localRotations.length / 4; b++) { rs.localRotations.set([0, 0, 0, 1], b * 4); rs.localTranslations.set([0, 0, 0], b * 3) }
    A.currentModel.getMorphWeights().fill(0)
    A.seekMotions(st); B.seekMotions(st)
    const a = A.getDeformed(), b = B.getDeformed()
    for (let v = 0; v < a.positions.length / 3; v++) {
      let d2 = 0, r2 = 0, n2 = 0
      for (let k = 0; k < 3; k++) {
        const dp = b.positions[v * 3 + k] - a.positions[v * 3 + k], dn = b.normals[v * 3 + k] - a.normals[v * 3 + k]
        d2 += dp * dp; r2 += a.positions[v * 3 + k] * a.positions[v * 3 + k]; n2 += dn * dn
      }
      worst = Math.max(worst, Math.sqrt(d2) / Math.max(Math.sqrt(r2), 1), Math.sqrt(n2))
    }
    single.push({ p: Float32Array.from(b.positions), n: Float32Array.from(b.normals) })
    if (st.layers && st.layers.length) {      // what the layers moved: the same base without them
      B.seekMotions(Object.assign({}, st, { layers: [] }))
      moved = Math.max(moved, dist(B.getDeformed().positions, single[single.length - 1].p))
    }
  })
  const pick = [1, 2, 3]
  B.setInstanceCount(pick.length)
  B.seekMotions(pick.map((i) => states[i]))
  let equal = true
  pick.forEach((i, k) => {
    const d = B.getDeformed(k)
    const pa = new Uint32Array(d.positions.buffer, d.positions.byteOffset, d.positions.length), pb = new Uint32Array(single[i].p.buffer)
    const na = new Uint32Array(d.normals.buffer, d.normals.byteOffset, d.normals.length), nb = new Uint32Array(single[i].n.buffer)
    for (let j = 0; j < pa.length; j++) if (pa[j] !== pb[j] || na[j] !== nb[j]) { equal = false; break }
  })
  A.dispose(); B.dispose()
  console.warn = quiet
  console.log(JSON.stringify({ worst, moved, states: states.length, crowd: pick.length, crowd_bits_equal: equal }))
})().catch((e) => { console.error(e); process.exit(1) })
