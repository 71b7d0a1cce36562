'use strict'
/* Test helper: Model.physicsTables() of a PMX file as JSON (tests/test_physics_cpu.py compares it with the Python tables).
 * usage: node physics_tables.js <pmx> */
const fs = require('fs'), path = require('path')
const host = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
console.warn = () => {}
const m = host.PmxLoader.loadFromBuffer(fs.readFileSync(process.argv[2]))
const t = m.physicsTables(), out = {}
for (const k of Object.keys(t)) out[k] = typeof t[k] === 'number' ? t[k] : Array.from(t[k])
console.log(JSON.stringify(out))
