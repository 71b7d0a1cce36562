'use strict'
/* The pose of the QDEF Node tests (qdef_e2e.js on the GPU, qdef_pose.js on the CPU): every third bone twisted by 80-90 degrees against its
 * parent. Returns [names, quats] for rotateBones. */
module.exports = (names, Quat) => {
  const twist = []
  for (let b = 2; b < names.length; b += 3) twist.push(names[b])
  return [twist, twist.map((_, k) => new Quat(0.5 + 0.01 * k, 0.3, -0.2, 0.7).normalize())]
}
