"""The definition of a blended pose (include/reze_deform.h: rz_set_pose_blended; host/model.js: applyBlendedFrame), in float64.

A state is (clip_a, frame_a, clip_b, frame_b, blend). A = sample(clip_a, frame_a) and B = sample(clip_b, frame_b) are what
host/vmd-sampler.js defines (helpers.sample_reference restates it: slerp warped by the R curve, per-axis lerp warped by X / Y / Z, linear
morph keys with own-track-then-group feeds; a bone or morph a clip does not key is at rest). clip_b None / NO_CLIP or blend == 0 gives
exactly A, blend == 1 exactly B; otherwise per bone q = Quat.slerp(qa, qb, blend) (math.ts:156-189), t = ta + (tb - ta) * blend, and per
vertex morph w = wa + (wb - wa) * blend on the effective weights. Test infrastructure."""
import numpy as np

from helpers import sample_reference

NO_CLIP = 0xffffffff


def slerp(a, b, t):
    """Quat.slerp (math.ts:156-189): b is negated when the dot product is negative; normalised lerp above 0.9995, sine form otherwise."""
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    c = float(a @ b)
    if c < 0:
        c, b = -c, -b
    if c > 0.9995:
        r = a + t * (b - a)
        return r / np.linalg.norm(r)
    th0 = np.arccos(c)
    return (np.sin(th0 - th0 * t) * a + np.sin(th0 * t) * b) / np.sin(th0)


def blend_reference(clips, state, n_bones, n_morphs):
    """(quats [B, 4], translations [B, 3], effective morph weights [M]) in float64 of one state over the library `clips` (a list of
    clip dicts with the rz_animation field names)."""
    ca, fa, cb, fb, blend = state
    has_b = cb is not None and int(cb) != NO_CLIP and int(cb) >= 0 and float(blend) != 0.0
    if not has_b:
        return sample_reference(clips[int(ca)], float(fa), n_bones, n_morphs)
    if float(blend) == 1.0:
        return sample_reference(clips[int(cb)], float(fb), n_bones, n_morphs)
    qa, ta, wa = sample_reference(clips[int(ca)], float(fa), n_bones, n_morphs)
    qb, tb, wb = sample_reference(clips[int(cb)], float(fb), n_bones, n_morphs)
    t = float(blend)
    q = np.array([slerp(qa[b], qb[b], t) for b in range(n_bones)]).reshape(n_bones, 4)
    return q, ta + (tb - ta) * t, wa + (wb - wa) * t


def min_abs_dot(clips, state, n_bones):
    """The smallest |qa . qb| over the bones of a state that blends two clips (1.0 for a state that does not): the sign choice of the
    blend's slerp is safe from rounding while this stays well above 0."""
    ca, fa, cb, fb, blend = state
    if cb is None or int(cb) == NO_CLIP or int(cb) < 0 or float(blend) in (0.0, 1.0):
        return 1.0
    qa = sample_reference(clips[int(ca)], float(fa), n_bones, 0)[0]
    qb = sample_reference(clips[int(cb)], float(fb), n_bones, 0)[0]
    return float(np.abs(np.sum(qa * qb, axis=1)).min())
