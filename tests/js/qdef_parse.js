'use strict'
/* Test helper (tests/test_qdef_cpu.py): parses a PMX with THIS build's loader and prints, as one JSON line, the skinning arrays and the
 * QDEF list the loader collected (Geometry.qdef, reached through Model.getQdef()).  usage: node qdef_parse.js <pmx> */
const fs = require('fs'), path = require('path')
const { PmxLoader } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
console.warn = () => {}
const m = PmxLoader.loadFromBuffer(fs.readFileSync(process.argv[2]))
const k = m.getSkinning()
console.log(JSON.stringify({ joints: Array.from(k.joints), weights: Array.from(k.weights), index: Array.from(m.getQdef()), sdef: Array.from(m.getSdef().index) }))
