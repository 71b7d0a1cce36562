'use strict'
/* Test helper (tests/test_sdef_cpu.py): parses a PMX with THIS build's loader and prints, as one JSON line, the skinning arrays and the
 * SDEF table the loader collected (Geometry.sdef, reached through Model.getSdef()).  usage: node sdef_parse.js <pmx> */
const fs = require('fs'), path = require('path')
const { PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
console.warn = () => {}
const m = PmxLoader.loadFromBuffer(fs.readFileSync(process.argv[2]))
const s = m.getSdef(), k = m.getSkinning()
console.log(JSON.stringify({ joints: Array.from(k.joints), weights: Array.from(k.weights), index: Array.from(s.index), c: Array.from(s.c),
  r0: Array.from(s.r0), r1: Array.from(s.r1) }))
