'use strict'
/* CPU test of Engine { crowdMorphs } with a recording stand-in for the native addon: setInstanceCount(n) is followed by
 * setTuning(ctx, 'inst_morphs', 1) on every shard, a fork made for framesInFlight: 2 gets the call too, and the engine makes no such call
 * without the option.
 * usage: node crowd_morphs_engine_mock.js
 * Prints the calls per option. */
const path = require('path')
const { Engine } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const mkNative = (calls) => ({
  setInstances: (c, n) => calls.push('setInstances:' + n), destroy: () => {},
  setTuning: (c, k, v) => calls.push('setTuning:' + k + '=' + v + (c.fork ? ':fork' : '')),
  fork: (c) => { calls.push('fork'); return { fork: true } },
})
const out = {}
for (const [tag, opts] of [['on', { crowdMorphs: true }], ['fork', { crowdMorphs: true, framesInFlight: 2 }], ['off', { framesInFlight: 2 }]]) {
  const calls = []
  const e = new Engine(null, Object.assign({ realtime: false, deviceFK: true, deviceSampling: true }, opts))
  e.native = mkNative(calls); e.ctx = {}; e.currentModel = {}
  e.shards = [{ ctx: e.ctx, begin: 0, count: 1, fork: null, last: null, flip: 0 }]
  e.setInstanceCount(11)
  e.frameContext(e.shards[0]); e.frameContext(e.shards[0])
  out[tag] = calls
}
console.log(JSON.stringify(out))
