'use strict'
/* The motion library through the N-API boundary: the same synthetic PMX and two VMDs posed at the same states by
 *   A: new Engine(null, { realtime: false })                                    seekMotions -> Model.applyBlendedFrame + host FK
 *   B: new Engine(null, { realtime: false, deviceFK: true, deviceSampling: true })   rz_upload_motions + rz_set_pose_blended
 * then a crowd of three on B, each instance against the single-character frame of its state, bit for bit.
 * usage: node motion_e2e.js <model.pmx> <walk.vmd> <run.vmd> <states.json>   -> one JSON line */
const path = require('path'), fs = require('fs')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const [pmx, vmdA, vmdB, statesFile] = process.argv.slice(2)
const states = JSON.parse(fs.readFileSync(statesFile, 'utf8'))
;(async () => {
  const quiet = console.warn; console.warn = () => {}
  const A = new Engine(null, { realtime: false })
  const B = new Engine(null, { realtime: false, deviceFK: true, deviceSampling: true })
  for (const e of [A, B]) { await e.init(); await e.loadModel(pmx); await e.loadMotion('walk', vmdA); await e.loadMotion('run', vmdB) }
  let worst = 0, moved = 0
  const single = [], first = []
  states.forEach((st, i) => {
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
    if (i === 0) first.push(Float32Array.from(a.positions))
    else for (let k = 0; k < a.positions.length; k++) moved = Math.max(moved, Math.abs(a.positions[k] - first[0][k]))
    single.push({ p: Float32Array.from(b.positions), n: Float32Array.from(b.normals) })
  })
  const pick = [1, 2, 4]
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
