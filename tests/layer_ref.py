"""The definition of a layered pose (include/reze_deform.h: rz_set_pose_layered; host/model.js: applyLayeredFrame), in float64.

(q, t, w) starts as motion_ref.blend_reference(base). Then the layers (clip, frame, weight, mask, mode) are applied in order; a layer with
clip None / NO_CLIP or weight 0 is skipped as a whole. L = sample(clip, frame) (helpers.sample_reference). A layer acts on bone b only when
the clip keys b (a track with at least one key) and the mask includes b (mask None / NO_MASK includes everything):
  override   q = Quat.slerp(q, qL, weight), t = t + (tL - t) * weight; at weight 1 q and t are qL and tL as sampled
  additive   q = Quat.multiply(q, Quat.slerp(identity, qL, weight)), t = t + tL * weight (the forms bone morphs use)
and on vertex morph m only when at least one of m's feeds in that clip holds a key and the mask includes m (morph masks None: every mask
includes every morph), with wL the effective weight: override w = w + (wL - w) * weight (wL at weight 1), additive w = w + wL * weight.
Test infrastructure."""
import numpy as np

import motion_ref
from helpers import sample_reference

NO_CLIP = motion_ref.NO_CLIP
NO_MASK = 0xffffffff
OVERRIDE, ADDITIVE = 0, 1
IDENT = np.array([0.0, 0.0, 0.0, 1.0])


def multiply(a, b):
    """Quat.multiply(a, b) (math.ts:77-85): the Hamilton product a * b, (x, y, z, w)"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def keyed_bones(clip, n_bones):
    """[B] bool: the clip has a track with at least one key for the bone"""
    k = np.zeros(n_bones, dtype=bool)
    for tr, b in enumerate(clip["track_bone"]):
        if 0 <= b < n_bones and int(clip["key_off"][tr + 1]) > int(clip["key_off"][tr]):
            k[b] = True
    return k


def keyed_morphs(clip, n_morphs):
    """[M] bool: at least one of the morph's feeds in the clip holds a key"""
    k = np.zeros(n_morphs, dtype=bool)
    if n_morphs and clip.get("mkey_off") is not None:
        for m in range(n_morphs):
            for f in range(int(clip["feed_off"][m]), int(clip["feed_off"][m + 1])):
                tr = int(clip["feed_track"][f])
                if int(clip["mkey_off"][tr + 1]) > int(clip["mkey_off"][tr]):
                    k[m] = True
    return k


def skipped(layer):
    clip, _frame, weight = layer[0], layer[1], layer[2]
    return clip is None or int(clip) == NO_CLIP or int(clip) < 0 or float(weight) == 0.0


def layered_reference(clips, base, layers, n_bones, n_morphs, bone_masks=None, morph_masks=None, dots=None):
    """(quats [B, 4], translations [B, 3], effective morph weights [M]) in float64 of `base` (a motion_ref state) with `layers`, a list of
    (clip, frame, weight, mask, mode). bone_masks [n_masks, B] / morph_masks [n_masks, M] or None. `dots`, a list, collects the |dot| of
    every slerp the layers perform and, as ('add', |qL.w|), of every additive sample."""
    q, t, w = motion_ref.blend_reference(clips, base, n_bones, n_morphs)
    q, t, w = q.copy(), t.copy(), w.copy()
    for layer in layers:
        if skipped(layer):
            continue
        clip, frame, weight, mask, mode = int(layer[0]), float(layer[1]), float(layer[2]), layer[3], int(layer[4])
        masked = not (mask is None or int(mask) == NO_MASK or int(mask) < 0)
        ql, tl, wl = sample_reference(clips[clip], frame, n_bones, n_morphs)
        acts = keyed_bones(clips[clip], n_bones)
        if masked:
            acts &= np.asarray(bone_masks)[int(mask)] != 0
        for b in np.flatnonzero(acts):
            if mode == ADDITIVE:
                if dots is not None:
                    dots.append(("add", abs(float(ql[b][3]))))
                q[b] = multiply(q[b], motion_ref.slerp(IDENT, ql[b], weight))
                t[b] = t[b] + tl[b] * weight
            elif weight == 1.0:
                q[b], t[b] = ql[b], tl[b]
            else:
                if dots is not None:
                    dots.append(("slerp", abs(float(q[b] @ ql[b]))))
                q[b] = motion_ref.slerp(q[b], ql[b], weight)
                t[b] = t[b] + (tl[b] - t[b]) * weight
        macts = keyed_morphs(clips[clip], n_morphs)
        if masked and morph_masks is not None:
            macts &= np.asarray(morph_masks)[int(mask)] != 0
        for m in np.flatnonzero(macts):
            if mode == ADDITIVE:
                w[m] = w[m] + wl[m] * weight
            elif weight == 1.0:
                w[m] = wl[m]
            else:
                w[m] = w[m] + (wl[m] - w[m]) * weight
    return q, t, w
