'use strict'
/* Model.solveIK() on skeletons and poses a test supplies. usage: node ik_solve.js <in.json> <out.json>
 * in: { parents, bind [B][3], appendParent?, appendRatio?, chains: [{goal, effector, loops, limitAngle, links: [{bone, min, max}]}],
 *       poses: [{ q: [B*4], t: [B*3] }] }
 * out: per pose the world matrices with IK on, with IK off, and of a model whose bones carry no `ik` field at all ([B*16] each). */
const fs = require('fs'), path = require('path')
const { Model } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const inp = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'))
const B = inp.parents.length
const build = (withIk) => {
  const bones = inp.parents.map((p, i) => {
    const b = { name: 'b' + i, parentIndex: p, bindTranslation: inp.bind[i], children: [] }
    if (inp.appendParent && inp.appendParent[i] >= 0) { b.appendParentIndex = inp.appendParent[i]; b.appendRatio = inp.appendRatio[i]; b.appendRotate = true; b.appendMove = false }
    return b
  })
  if (withIk) for (const ch of inp.chains) bones[ch.goal].ik = { effector: ch.effector, loops: ch.loops, limitAngle: ch.limitAngle, links: ch.links.map((l) => (l.min ? { bone: l.bone, min: l.min, max: l.max } : { bone: l.bone })) }
  return new Model(new Float32Array(8), new Uint32Array(3), [], [], { bones, inverseBindMatrices: new Float32Array(B * 16) },
    { joints: new Uint16Array(4), weights: new Uint8Array(4).fill(255) }, [], [], null)
}
const m = build(true), plain = build(false)
const out = []
for (const pose of inp.poses) {
  const r = {}
  for (const [tag, model, on] of [['on', m, true], ['off', m, false], ['plain', plain, false]]) {
    model.runtimeSkeleton.localRotations.set(pose.q)
    model.runtimeSkeleton.localTranslations.set(pose.t)
    model.applyLocalTranslations = true
    model.setIK(on)
    model.computeWorldMatrices()
    r[tag] = Array.from(model.getBoneWorldMatrices())
  }
  // the runtime's own pose is never overwritten by the solve
  r.kept = Array.from(m.runtimeSkeleton.localRotations).every((x, i) => x === Math.fround(pose.q[i]))
  out.push(r)
}
fs.writeFileSync(process.argv[3], JSON.stringify(out))
