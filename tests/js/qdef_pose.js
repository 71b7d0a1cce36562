'use strict'
/* Test helper (tests/test_qdef_cpu.py), no GPU: loads a PMX with THIS build's loader, sets the pose of qdef_e2e.js on the host model and
 * dumps what the float64 reference needs to judge that scene (joints, weights, inverse bind and world matrices); prints the QDEF list as
 * one JSON line.  usage: node qdef_pose.js <pmx> <outdir> */
const fs = require('fs'), path = require('path')
const { PmxLoader, Quat } = require(path.join(__dirname, '..', '..', 'reze-engine_amd', 'host'))
const twistOf = require('./qdef_twist')
const [pmx, out] = process.argv.slice(2)
const dump = (name, ta) => fs.writeFileSync(path.join(out, name), Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength))
console.warn = () => {}
const m = PmxLoader.loadFromBuffer(fs.readFileSync(pmx))
const [names, quats] = twistOf(m.getBoneNames(), Quat)
m.rotateBones(names, quats, 0)
m.evaluatePose()
dump('joints.u16', m.getSkinning().joints); dump('weights.u8', m.getSkinning().weights)
dump('invbind.f32', m.getSkeleton().inverseBindMatrices); dump('world.f32', m.getBoneWorldMatrices())
console.log(JSON.stringify({ index: Array.from(m.getQdef()) }))
