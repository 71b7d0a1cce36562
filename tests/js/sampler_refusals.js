'use strict'
// The refusals of non-finite frames and keys through the N-API addon: the C ABI's messages reach JavaScript unchanged, and the motion that
// was resident before a refused call still poses the mesh with the same bits. -> one JSON line { messages: [...], sameBits }
const path = require('path')
const a = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host', 'addon.js')).requireAddon()
const ctx = a.create(0)
const V = 300, B = 5
const mesh = new Float32Array(V * 8).map((_, i) => Math.sin(i)), joints = new Uint16Array(V * 4).map((_, i) => (i % 4 === 0 ? (i >> 2) % B : 0)), weights = new Uint8Array(V * 4)
for (let v = 0; v < V; v++) weights[v * 4] = 255
const ib = new Float32Array(B * 16); for (let b = 0; b < B; b++) for (let k = 0; k < 4; k++) ib[b * 16 + k * 5] = 1
a.uploadMesh(ctx, mesh, joints, weights); a.uploadSkeleton(ctx, ib)
a.uploadSkeletonTopology(ctx, new Int32Array([-1, 0, 1, 0, 3]), new Float32Array(B * 3).fill(0.25), new Int32Array(B).fill(-1), new Float32Array(B).fill(1), new Uint8Array(B))
const s = Math.sin(0.3), c = Math.cos(0.3)
const good = () => ({ trackBone: new Int32Array([1, 3]), keyOff: new Uint32Array([0, 2, 4]), keyFrame: new Float32Array([0, 10, 0, 20]),
  keyRot: new Float32Array([0, 0, 0, 1, s, 0, 0, c, 0, 0, 0, 1, 0, s, 0, c]), keyPos: new Float32Array(12).map((_, i) => 0.1 * i) })
a.uploadAnimation(ctx, good())
const frame = () => { a.setPoseSampled(ctx, new Float32Array([4.5])); a.deform(ctx); const p = new Float32Array(V * 3), n = new Float32Array(V * 3); a.read(ctx, 0, 0, V, p, n); return p }
const before = frame()
const messages = []
const refused = (f) => { try { f(); messages.push(null) } catch (e) { messages.push(e.message) } }
refused(() => a.setPoseSampled(ctx, new Float32Array([NaN])))
refused(() => a.setPoseSampled(ctx, new Float32Array([Infinity])))
refused(() => { const m = good(); m.keyRot[5] = NaN; a.uploadAnimation(ctx, m) })
refused(() => { const m = good(); m.keyPos[9] = -Infinity; a.uploadAnimation(ctx, m) })
refused(() => { const m = good(); m.keyFrame[0] = -Infinity; a.uploadAnimation(ctx, m) })
const after = frame()
let sameBits = true
for (let i = 0; i < before.length; i++) if (before[i] !== after[i]) sameBits = false
a.destroy(ctx)
console.log(JSON.stringify({ messages, sameBits }))
