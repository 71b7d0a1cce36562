"""The scenes of the long-track sampler tests, shared by tests/test_gpu_sampler.py (which runs them on the device) and
tests/test_sampler_cpu.py (which holds their inputs to the conditions the GPU bars rest on). Deterministic, numpy only. Test infrastructure.

A real dance motion has tracks of thousands of keys, bunched where the motion is busy, with gaps of hundreds of frames elsewhere, runs of
duplicate frames and frame numbers in the tens of thousands. The device sampler guesses a key span by linear interpolation and repairs a
wrong guess by bisection (kernels/fk.hip.h: span_guess / span_bisect); on such tracks the guess lands thousands of keys away. Clip A has one
track of every shape that matters (KINDS below); consecutive keys of a track differ by far more than any bar, so a neighbouring span cannot
pass for the right one.

Every key of a bone lies within 45 degrees of a per-bone base rotation (synth.make_motion's rule; the base is identity for a bone that a
clip leaves at rest), some keys are stored negated. Key frames are integers except on the `frac` tracks, which the host-sampler test leaves
out (a VMD stores integer frames)."""
import numpy as np

V = 512
M_DENSE, M_SPARSE = 8, 260
DEFAULT_CURVE = np.array([20] * 8 + [107] * 8, dtype=np.uint8)
# (x1, y1, x2, y2) of the curves whose x(t) or y(t) is flat at an end
EXTREME = [(0, 127, 0, 127), (127, 0, 127, 0), (0, 127, 127, 0), (127, 0, 0, 127), (0, 0, 0, 0), (127, 127, 0, 0)]
T7_START = 40000            # the 70 000-key track begins where every other track of clip A has ended (the two-key track excepted)
_memo = {}


# ---- key frames of the eight track shapes ----
def _frames(kind, rng):
    """(frames float64 [n], gaps): gaps = indices i of the later key of every long gap (frames[i] - frames[i - 1] >= 200)"""
    if kind == "one":
        return np.array([100.0]), []
    if kind == "two":
        return np.array([50.0, 30050.0]), []
    if kind == "three":
        return np.array([10.0, 10.0, 40.0]), []
    if kind == "even":                                  # 64 keys, one every 16 frames: the linear guess is right
        return 7.0 + 16.0 * np.arange(64), []
    if kind == "bursts":                                # 1 000 keys: 20 bursts of 50 keys one frame apart, 200-900 frames between bursts
        f, gaps, at = [], [], 20.0
        for b in range(20):
            if b:
                at += float(rng.integers(200, 901))
                gaps.append(len(f))
            f.extend(at + np.arange(50))
            at += 49.0
        return np.array(f), gaps
    if kind == "runs":                                  # 4 096 keys in runs of 2-5 equal frames, the first and the last key included
        f, at = [], 2.0
        while len(f) < 4096:
            f.extend([at] * min(int(rng.integers(2, 6)), 4096 - len(f)))
            at += float(rng.integers(1, 5))
        if f[-1] != f[-2]:                              # (the last run was cut to one key: join it to the run before)
            f[-1] = f[-2]
        return np.array(f), []
    if kind == "long":                                  # 70 000 keys: steps of 1-3 frames, about 1 % of them gaps of 2 000 frames
        step = rng.integers(1, 4, size=69999).astype(np.float64)
        prob = np.full(69999, 0.004)                    # the gaps are bunched too: most of them lie in one quarter of the keys, so the
        prob[20000:37500] = 0.03                        # linear guess is thousands of keys off on either side of it
        gap = rng.random(69999) < prob
        gap[:200] = False
        step[gap] = 2000.0
        f = np.concatenate([[float(T7_START)], T7_START + np.cumsum(step)])
        return f, list(np.flatnonzero(gap) + 1)
    if kind == "frac":                                  # 300 keys at fractional frames (multiples of 1/64), the first one negative
        f = -600.5 + np.concatenate([[0.0], np.cumsum(np.round(rng.uniform(0.25, 8.0, size=299) * 64) / 64)])
        f[-1] = 900.75                                  # one float32 step below this key, frame - first rounds UP to last - first
        assert f[-2] < f[-1]
        return f, []
    raise ValueError(kind)


KINDS = ("one", "two", "three", "even", "bursts", "runs", "long", "frac")       # tracks 1 .. 8 of the issue's table
SMALL_STEPS = ("bursts", "long")        # rotation steps under 0.06 rad: the slerp's c > 0.9995 lerp branch; the others take the sine form


def _circle(rng, n, radius, lo, hi):
    """n points on a circle of `radius` in a random plane through the origin, consecutive points lo .. hi apart along the arc"""
    e1 = rng.normal(size=3)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(e1, rng.normal(size=3))
    e2 /= np.linalg.norm(e2)
    s = np.cumsum(rng.uniform(lo, hi, size=n)) / radius
    return radius * (np.cos(s)[:, None] * e1 + np.sin(s)[:, None] * e2)


def _quat_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def make_track(kind, seed, base):
    """One bone track: dict(kind, frame f32 [n], rot f32 [n,4], pos f32 [n,3], interp u8 [n,16], cat [n], gaps).
    Rotations: base * exp(v), v on a circle of radius 0.5 rad (inside the 45 degree ball), consecutive keys 0.035-0.055 rad apart
    (SMALL_STEPS) or 0.3-0.8 rad apart; a fifth of the keys negated. Positions: a circle of radius 0.3, steps 0.05-0.12.
    Curves per key (cat): 0 the default curve, 1 random bytes 0 .. 127, 2 extreme curves (EXTREME, one per axis and one for the rotation;
    only on the `bursts` and `long` tracks, and on the later key of each of their long gaps)."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    f, gaps = _frames(kind, rng)
    n = len(f)
    small = kind in SMALL_STEPS
    v = _circle(rng, n, 0.5, *((0.035, 0.055) if small else (0.3, 0.8)))
    ang = np.linalg.norm(v, axis=1, keepdims=True)
    dq = np.concatenate([v / ang * np.sin(ang / 2), np.cos(ang / 2)], axis=1)
    q = _quat_mul(np.asarray(base, dtype=np.float64)[None, :], dq)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[rng.random(n) < 0.2] *= -1.0
    pos = _circle(rng, n, 0.3, 0.05, 0.12)
    cat = rng.choice(3 if kind in ("bursts", "long") else 2, size=n, p=(0.3, 0.5, 0.2) if kind in ("bursts", "long") else (0.4, 0.6))
    interp = np.tile(DEFAULT_CURVE, (n, 1))
    rnd = rng.integers(0, 128, size=(n, 16)).astype(np.uint8)
    interp[cat == 1] = rnd[cat == 1]
    pick = rng.integers(0, 6, size=(n, 4))
    if kind == "frac":
        cat[-1] = 0                                     # (a frame one float32 step below the last key is sampled: its curves stay the default)
        interp[-1] = DEFAULT_CURVE
    for j, i in enumerate(gaps):                        # gap j: X Y Z R take EXTREME[j], [j + 1], [j + 2], [j + 3]
        cat[i] = 2
        pick[i] = (j + np.arange(4)) % 6
    ext = np.array(EXTREME, dtype=np.uint8)[pick]       # [n, 4 curves, (x1 y1 x2 y2)]
    ext = np.transpose(ext, (0, 2, 1)).reshape(n, 16)   # bytes [X_x1 Y_x1 Z_x1 R_x1 | .. y1 | .. x2 | .. y2]
    interp[cat == 2] = ext[cat == 2]
    return dict(kind=kind, frame=f.astype(np.float32), rot=q.astype(np.float32), pos=pos.astype(np.float32), interp=interp, cat=cat, gaps=gaps)


# ---- morph tracks ----
def make_morph_track(kind, seed):
    """(frames f32, weights f32): weights 0.5 +- a, a in 0.05 .. 0.45 with alternating sign, so consecutive keys differ by 0.1 at least"""
    rng = np.random.default_rng([seed, 77])
    if kind == "one":
        f = np.array([30.0])
    elif kind == "two":
        f = np.array([5.0, 20005.0])
    elif kind == "bursts":                              # 700 keys: 14 bursts of 50
        f, at = [], 12.0
        for b in range(14):
            at += float(rng.integers(200, 901)) if b else 0.0
            f.extend(at + np.arange(50))
            at += 49.0
        f = np.array(f)
    elif kind == "runs":                                # 5 000 keys in runs of 1-4 equal frames
        f, at = [], 3.0
        while len(f) < 5000:
            f.extend([at] * min(int(rng.integers(1, 5)), 5000 - len(f)))
            at += float(rng.integers(1, 4))
        f = np.array(f)
    elif kind == "uneven":                              # 300 keys, steps of 1-40 frames
        f = np.cumsum(rng.integers(1, 41, size=300)).astype(np.float64)
    elif kind == "none":
        f = np.zeros(0)
    else:
        raise ValueError(kind)
    w = 0.5 + np.where(np.arange(len(f)) % 2 == 0, 1.0, -1.0) * rng.uniform(0.05, 0.45, size=len(f))
    return f.astype(np.float32), w.astype(np.float32)


MORPH_TRACKS = ("one", "two", "bursts", "runs", "uneven", "none", "bursts")     # track 4 is the group morph's, track 5 holds no key


def _morph_part(n_morphs, seed):
    tracks = [make_morph_track(k, seed + i) for i, k in enumerate(MORPH_TRACKS)]
    # morph 0..3: own track; 1 also the group (x 0.5); 4 never keyed; 5 the group only (x -0.25); 6 a track without keys; 7 own track
    feeds = [[(0, 1.0)], [(1, 1.0), (4, 0.5)], [(2, 1.0)], [(3, 1.0)], [], [(4, -0.25)], [(5, 1.0)], [(6, 1.0)]]
    feeds += [[] for _ in range(n_morphs - 8)]
    for m in range(8, n_morphs):
        if m % 16 == 0:
            feeds[m] = [(m % 5, 0.3)]
    if n_morphs > 256:                                  # the second chunk of morphs samples the long tracks too
        feeds[256], feeds[257], feeds[258] = [(2, 1.0)], [(3, 0.7)], [(6, 1.0), (4, 0.5)]
    return dict(mkey_off=np.cumsum([0] + [len(f) for f, _ in tracks]).astype(np.uint32), mkey_frame=np.concatenate([f for f, _ in tracks]),
                mkey_weight=np.concatenate([w for _, w in tracks]), feed_off=np.cumsum([0] + [len(f) for f in feeds]).astype(np.uint32),
                feed_track=np.array([t for f in feeds for t, _ in f], dtype=np.int32), feed_ratio=np.array([r for f in feeds for _, r in f], dtype=np.float32))


# ---- skeletons and meshes ----
def _skeleton(n_bones, rng):
    """a root, two chains of depth 4 (bones 1-4 and 5-8), every other bone a child of the root"""
    parents = np.zeros(n_bones, dtype=np.int32)
    parents[0] = -1
    for b in (2, 3, 4, 6, 7, 8):
        parents[b] = b - 1
    bind = rng.uniform(-0.5, 0.5, size=(n_bones, 3)).astype(np.float32)
    return parents, bind


# bone -> kind of its track in clip A. B = 48: tracks 1-8 on bones 10-17, more of them down the two chains, a short one on an append bone.
ASSIGN_48 = {10: "one", 11: "two", 12: "three", 13: "even", 14: "bursts", 15: "runs", 16: "long", 17: "frac",
             1: "bursts", 2: "runs", 3: "frac", 4: "even", 5: "two", 6: "bursts", 7: "three", 8: "one", 40: "three"}
# B = 520: the 70 000-key track moves to bone 515 (the tail loop of skeletons beyond 512 bones); long tracks in both 256-bone chunks and in the tail
ASSIGN_520 = dict(ASSIGN_48)
ASSIGN_520.update({16: "bursts", 300: "bursts", 301: "runs", 302: "frac", 512: "bursts", 513: "runs", 515: "long", 517: "frac", 519: "even"})
APPEND_48 = {40: (16, 0.5, 0), 41: (14, -1.0, 1)}       # bone: (append parent, ratio, also appends movement)
APPEND_520 = {40: (515, 0.5, 0), 41: (14, -1.0, 1)}


def _mesh(n_bones, tracked, rng):
    pos = rng.uniform(-1.0, 1.0, size=(V, 3)).astype(np.float32)
    nrm = rng.normal(size=(V, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    tracked = np.asarray(sorted(tracked), dtype=np.int64)
    joints = np.zeros((V, 4), dtype=np.uint16)
    weights = np.zeros((V, 4), dtype=np.uint8)
    joints[:, 0] = tracked[np.arange(V) % len(tracked)]
    weights[:, 0] = 255
    two = np.arange(V) % 2 == 1                          # every second vertex BDEF2 over two tracked bones
    joints[two, 1] = tracked[(np.arange(V) * 7 + 3) % len(tracked)][two]
    w0 = rng.integers(1, 255, size=V)
    weights[two, 0] = w0[two]
    weights[two, 1] = 255 - w0[two]
    return pos, nrm, joints, weights


def scene(name="b48"):
    """name: 'b48' (B = 48, 8 dense morphs), 'b48_sparse' (the same bones, 260 sparse morphs), 'b520' (B = 520, 8 dense morphs).
    Returns dict(B, M, mesh (pos nrm joints weights parents bind inv_bind), ap / ratio / move (append arrays), dense or sparse, clip_a,
    clip_a_vmd (clip A without its fractional-frame tracks), clip_b, tracks {bone: track}, base, frames (f32), frames_b (f32))."""
    if name in _memo:
        return _memo[name]
    from reze_engine_amd import synth
    n_bones = 520 if name == "b520" else 48
    n_morphs = M_SPARSE if name == "b48_sparse" else M_DENSE
    assign = ASSIGN_520 if n_bones == 520 else ASSIGN_48
    append = APPEND_520 if n_bones == 520 else APPEND_48
    rng = np.random.default_rng(4800 + n_bones)
    parents, bind = _skeleton(n_bones, rng)
    rest_in_b = [20, 21]                                # bones only clip B keys: their base is identity
    base = synth.make_motion_base(n_bones, seed=11)
    keyed = np.zeros(n_bones, dtype=bool)
    keyed[list(assign)] = True
    base[~keyed] = (0.0, 0.0, 0.0, 1.0)
    tracks = {b: make_track(k, 100 + b, base[b]) for b, k in sorted(assign.items())}
    ap = np.full(n_bones, -1, dtype=np.int32)
    ratio = np.ones(n_bones, dtype=np.float32)
    move = np.zeros(n_bones, dtype=np.uint8)
    for b, (p, r, mv) in append.items():
        ap[b], ratio[b], move[b] = p, r, mv
    pos, nrm, joints, weights = _mesh(n_bones, list(assign) + list(append), rng)
    mesh = dict(pos=pos, nrm=nrm, joints=joints, weights=weights, parents=parents, bind=bind,
                inv_bind=synth.inverse_bind_translation_only(parents, bind))

    def clip(bones):
        order = list(bones)
        lost = make_track("three", 99, (0.0, 0.0, 0.0, 1.0))               # a track for a bone the model lacks, in the middle of the keys
        parts = [tracks[b] for b in order[:3]] + [lost] + [tracks[b] for b in order[3:]]
        tb = order[:3] + [n_bones + 5] + order[3:]
        c = dict(track_bone=np.array(tb, dtype=np.int32), key_off=np.cumsum([0] + [len(p["frame"]) for p in parts]).astype(np.uint32),
                 key_frame=np.concatenate([p["frame"] for p in parts]), key_rot=np.concatenate([p["rot"] for p in parts]),
                 key_pos=np.concatenate([p["pos"] for p in parts]), key_interp=np.concatenate([p["interp"] for p in parts]))
        c.update(_morph_part(n_morphs, 500))
        return c
    order = sorted(assign, key=lambda b: (KINDS.index(assign[b]) * 7 + b) % 11)      # the tracks in no particular order; the long one not last
    clip_a = clip(order)
    clip_a_vmd = clip([b for b in order if assign[b] != "frac"])
    kb = keyed.copy()
    kb[rest_in_b] = True
    clip_b = synth.make_motion(n_bones, n_morphs, seed=31, keyed=kb, base=base, flip=0.3, n_keys=7, group_feed=(2, 0.5))
    out = dict(name=name, B=n_bones, M=n_morphs, mesh=mesh, ap=ap, ratio=ratio, move=move, clip_a=clip_a, clip_a_vmd=clip_a_vmd, clip_b=clip_b,
               tracks=tracks, assign=assign, base=base)
    drng = np.random.default_rng(7)
    if name == "b48_sparse":
        off, vi, d3, _ = synth.make_morphs_sparse(V, M_SPARSE, density=0.02, seed=83)
        out["sparse"] = (off, vi, (d3 * np.float32(20.0)).astype(np.float32))               # deltas of about 1 unit
        out["dense"] = synth.sparse_to_dense(V, *out["sparse"])
    else:
        out["dense"] = drng.uniform(-1.0, 1.0, size=(M_DENSE, V, 3)).astype(np.float32)
    out["frames"], out["frame_notes"] = _sample_frames(tracks, assign)
    out["frames_b"] = np.array([-2.0, 3.25, 7.0, 11.5, 19.75, 26.0, 33.125, 400.0], dtype=np.float32)
    _memo[name] = out
    return out


def bone_of(sc, kind):
    """the first bone (ascending) that carries a track of `kind`; the table's tracks 1-8 sit on bones 10-17 of the B = 48 scene"""
    return min(b for b, k in sc["assign"].items() if k == kind and (b >= 10 or kind == "long"))


def _sample_frames(tracks, assign):
    """About 48 frames, each rounded to float32: see the notes returned beside them."""
    by = {}
    for b in sorted(assign):
        if b >= 10 or assign[b] == "long":
            by.setdefault(assign[b], tracks[b])
    t5, t6, t7, t8 = by["bursts"], by["runs"], by["long"], by["frac"]
    f5, f6, f7, f8 = (t["frame"].astype(np.float64) for t in (t5, t6, t7, t8))
    fr, notes = [], []

    def add(f, note):
        fr.append(np.float32(f)); notes.append(note)
    add(-700.0, "before every first key")
    add(f6[0], "on the first key of the runs track (a run of equal frames)")
    add(f6[-1], "on the last key of the runs track (a run of equal frames)")
    add(f7[0], "on the first key of the long track")
    add(f7[-1], "on the last key of the long track")
    add(f7[-1] + 1000.0, "past every last key")
    add(10.0, "on the two equal keys of the three-key track")
    add(25.0, "inside the three-key track")
    add(15050.0, "the middle of the two-key track")
    # runs of equal frames: one of each length 2 .. 5, well inside the track: on it, inside the span before it, just after it
    run_len = np.array([np.sum(f6 == x) for x in f6[1500:1600]])
    for n, off in ((5, 0.0), (2, 0.0), (3, -0.5), (4, 0.25), (5, 0.5), (2, -0.25)):
        i = 1500 + int(np.flatnonzero(run_len == n)[0])
        add(f6[i] + off, "a run of %d equal frames %+g" % (n, off))
    add(f5[50 * 7 + 17], "on a key inside a burst")
    add(f5[50 * 12 + 31] + 0.5, "between two keys of a burst")
    # long gaps, on the extreme curves: x = k / 1000 near both ends and the middle
    for t, f, which in ((t5, f5, (0, 1, 2, 3, 4, 5)), (t7, f7, (3, 4, 5, 6, 7, 8))):
        xs = (0.001, 0.5, 0.998, 0.003, 0.25, 0.999, 0.002, 0.75, 0.997)
        for n, j in enumerate(which):
            i = t["gaps"][j]
            a, b = f[i - 1], f[i]
            for x in xs[(n % 3) * 3:(n % 3) * 3 + 3] if n < 3 else xs[(n % 3) * 3:(n % 3) * 3 + 1]:
                add(a + (b - a) * x, "gap %d of the %s track at x = %g" % (j, t["kind"], x))
    # deep in the long track, between and on keys
    for i, off in ((100, 0.5), (35000, 0.5), (69998, 0.5), (50000, 0.0)):
        add(f7[i] + (off if f7[i + 1] > f7[i] + off else 0.0), "key %d of the long track %+g" % (i, off))
    # fractional frames beyond 100 000
    i = int(np.searchsorted(f7, 110000.0))
    add(f7[i] + 43.0 / 128.0, "a fractional frame beyond 100 000")
    i = int(np.searchsorted(f7, 1200000.0))
    add(f7[i] + 0.375, "a fractional frame beyond 1 000 000")
    add(f7[i + 3] + 0.125, "a fractional frame beyond 1 000 000")
    # one float32 step below and above a key, where the curves of both spans are the default one. Only on the long track, beyond every
    # other track's last key: there every other track is clamped, so no extreme curve is evaluated within 1e-4 of an end.
    c7 = t7["cat"]
    ok = np.flatnonzero((c7[1:-1] == 0) & (c7[2:] == 0) & (f7[1:-1] > f7[:-2]) & (f7[2:] > f7[1:-1]) & (f7[1:-1] > 31000.0)) + 1
    for i in (ok[0], ok[len(ok) // 2]):
        k = np.float32(f7[i])
        add(np.nextafter(k, np.float32(-np.inf)), "one float32 step below key %d of the long track (default curve)" % i)
        add(np.nextafter(k, np.float32(np.inf)), "one float32 step above key %d of the long track (default curve)" % i)
    # the fractional track: inside two spans, and one float32 step below its last key, where (frame - first) rounds to (last - first)
    # and the guessed key is the last one until the clamp pulls it back (its last key's curves are the default one)
    add(f8[40] + (f8[41] - f8[40]) * 0.3, "inside a span of the fractional track")
    add(f8[250] + (f8[251] - f8[250]) * 0.8, "inside a span of the fractional track")
    add(np.nextafter(np.float32(f8[-1]), np.float32(-np.inf)), "one float32 step below the last key of the fractional track")
    return np.array(fr, dtype=np.float32), notes


def crowd_frames(sc, n=48):
    """(indices, frames): n of the scene's frames spread over the whole list (the first and the last included), one per instance of the crowd"""
    idx = np.round(np.linspace(0, len(sc["frames"]) - 1, n)).astype(np.int64)
    return idx, sc["frames"][idx].copy()


def to_vmd_keys(sc):
    """(bone keys, morph keys) of clip_a_vmd for pmx_synth.write_vmd; bones are named b<index>, morph tracks m<track>"""
    c = sc["clip_a_vmd"]
    bone_keys = []
    for t, b in enumerate(c["track_bone"]):
        for k in range(int(c["key_off"][t]), int(c["key_off"][t + 1])):
            bone_keys.append(("b%d" % b, int(c["key_frame"][k]), tuple(float(x) for x in c["key_rot"][k]), tuple(float(x) for x in c["key_pos"][k]),
                              bytes(c["key_interp"][k]) + bytes(48)))
    morph_keys = []
    for t in range(len(c["mkey_off"]) - 1):
        for k in range(int(c["mkey_off"][t]), int(c["mkey_off"][t + 1])):
            morph_keys.append(("m%d" % t, int(c["mkey_frame"][k]), float(c["mkey_weight"][k])))
    return bone_keys, morph_keys
