'use strict'
/* Parses a PMX with the shipped loader and prints one JSON line: per bone its IK block (or null), and everything else the loader returns
 * (bones without the `ik` field, vertex / index / skinning bytes as hex digests) so that a test can compare it with the parse of the
 * same model written without IK blocks. usage: node ik_parse.js <model.pmx> */
const path = require('path'), crypto = require('crypto')
const { PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const sha = (ta) => crypto.createHash('sha1').update(Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)).digest('hex')
;(async () => {
  const m = await PmxLoader.load(process.argv[2])
  const bones = m.getSkeleton().bones
  const ik = bones.map((b) => (b.ik ? b.ik : null))
  const rest = bones.map((b) => { const o = Object.assign({}, b); delete o.ik; return o })
  const keys = bones.map((b) => Object.keys(b).join(','))
  console.log(JSON.stringify({
    ik, rest, keys, chains: m.getIKChains(), vertices: sha(m.getVertices()), indices: sha(m.getIndices()), joints: sha(m.getSkinning().joints),
    weights: sha(m.getSkinning().weights), invBind: sha(m.getSkeleton().inverseBindMatrices), morphs: m.getMorphNames(), materials: m.getMaterials().length,
  }))
})().catch((e) => { console.error(e); process.exit(1) })
