"""Scenes for the per-chain switches of the IK stage (rz_set_ik_enabled / rz_upload_ik_keys; kernels/ik.hip.h: ik_stage<SW>), one per
edge of the stage, built from ik_scenes.py and synth.make_leg_rig, and the key tracks of VMD IK on / off keys at the edges of the step
function (ik_switch_ref.state_at). tests/test_ik_switch_cpu.py holds the scenes to "not vacuous" and "well conditioned" with the
definition alone; tests/test_gpu_ik_switch.py holds the device to the definition on them.

A scene is dict(mesh, sk, chains, I, masks [I][n_chains] in the order of `chains`, poses [8]): a crowd of I instances with a mask each;
the 8 poses are dealt to the instances batch by batch (instance i of batch j takes pose (j * I + i) mod 8)."""
import numpy as np

import ik_ref
import ik_scenes as iks

_memo = {}
N_POSES = 8


def _sk(mesh):
    return dict(parents=mesh["parents"], bind=mesh["bind"], ap=None, ratio=None,
                extent=ik_ref.extent(ik_ref.bind_positions(mesh["parents"], mesh["bind"])))


def _rig():
    if "rig" not in _memo:
        from reze_engine_amd import synth
        _memo["rig"] = (synth, synth.make_leg_rig(n_verts=1500))
    return _memo["rig"]


def _off(n, off):
    m = np.ones(n, dtype=np.uint8)
    m[list(off)] = 0
    return m


def _same(mask, I=8):
    return np.tile(np.asarray(mask, dtype=np.uint8)[None], (I, 1))


def _legs(n):
    if ("legs", n) not in _memo:
        _memo[("legs", n)] = iks.nine_legs(n, n_verts=300 if n == 9 else 400)
    return _memo[("legs", n)]


def _build(name):
    if name.startswith("nine legs"):
        m = _legs(9)
        if name == "nine legs, chains 0 4 8 off":              # all of wave 0's share of the stage is off while the other three waves solve
            return dict(mesh=m, chains=m["chains"], I=8, masks=_same(_off(9, (0, 4, 8))), poses=iks.poses(m, 10))
        # crowd of 5, a different mask each: all on, all off, one wave's share, every second, the last only
        masks = np.stack([_off(9, ()), _off(9, range(9)), _off(9, (1, 5)), _off(9, (0, 2, 4, 6, 8)), _off(9, range(8))])
        return dict(mesh=m, chains=m["chains"], I=5, masks=masks, poses=iks.poses(m, 10))
    if name.startswith("33 legs"):                              # 33 chains: two mask words; the bit either side of the word boundary
        m = _legs(33)
        return dict(mesh=m, chains=m["chains"], I=8, masks=_same(_off(33, (32,) if name.endswith("32 off") else (31,))), poses=iks.poses(m, 40))
    if name.startswith("three stages"):
        m = iks.three_stages()
        off = (1,) if name == "three stages, middle stage off" else (2,)        # a skipped ik_resolve between two live ones / a trailing one
        return dict(mesh=m, chains=m["chains"], I=8, masks=_same(_off(3, off)), poses=iks.poses(m, 30))
    if name.startswith("leg rig"):
        synth, m = _rig()
        ch = m["chains"]                                        # ascending goal: leg L, toe L, leg R, toe R
        poses = [synth.leg_rig_pose(m, 700 + k) for k in range(N_POSES)]
        if name == "leg rig, legs off, toes on":                # a later stage sees the un-solved legs
            return dict(mesh=m, chains=ch, I=8, masks=_same([0, 1, 0, 1]), poses=poses)
        if name == "leg rig, descending goals":                 # the host-order -> device-order permutation: toe R, leg R (off), toe L (off), leg L
            return dict(mesh=m, chains=list(reversed(ch)), I=8, masks=_same([1, 0, 0, 1]), poses=poses)
        return dict(mesh=m, chains=ch, I=3, masks=np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1]], dtype=np.uint8), poses=poses)
    if name == "long chain, off":                               # the widest path form; the odd instances solve it in the switched kernel
        m = iks.long_chain(64, (40, 20, 1))
        return dict(mesh=m, chains=m["chains"], I=8, masks=np.array([[k & 1] for k in range(8)], dtype=np.uint8), poses=iks.poses(m, 0))
    if name == "root link, off":
        m = iks.root_link()
        return dict(mesh=m, chains=m["chains"], I=8, masks=np.array([[k & 1] for k in range(8)], dtype=np.uint8), poses=iks.poses(m, 20))
    raise KeyError(name)


SCENES = ("nine legs, chains 0 4 8 off", "33 legs, chain 32 off", "33 legs, chain 31 off", "three stages, middle stage off",
          "three stages, last stage off", "leg rig, legs off, toes on", "leg rig, descending goals", "long chain, off", "root link, off",
          "leg rig, crowd of 3", "nine legs, crowd of 5")


def scene(name):
    if name not in _memo:
        s = _build(name)
        s["sk"] = _sk(s["mesh"])
        s["masks"] = np.asarray(s["masks"], dtype=np.uint8)
        assert s["masks"].shape == (s["I"], len(s["chains"])) and len(s["poses"]) == N_POSES
        _memo[name] = s
    return _memo[name]


def batches(s):
    """[[pose index per instance]] covering the 8 poses"""
    I = s["I"]
    return [[(j * I + i) % N_POSES for i in range(I)] for j in range((N_POSES + I - 1) // I)]


_refs = {}


def reference(name, pose, inst, dtype=np.float64):
    """the definition's world matrices [B,16] of pose `pose` under instance `inst`'s mask, computed once and not to be written to"""
    s = scene(name)
    key = (id(s["mesh"]), len(s["chains"]) and s["chains"][0]["goal"], pose, s["masks"][inst].tobytes(), np.dtype(dtype).name)      # (instances and scenes that share a mask share the solve)
    if key not in _refs:
        import ik_switch_ref
        q, t = s["poses"][pose]
        _refs[key] = ik_switch_ref.solve(s["sk"]["parents"], s["sk"]["bind"], q, t, s["chains"], s["masks"][inst], dtype=dtype)[0]
    return _refs[key]


# ---- key tracks on the leg rig: chain names are the goal bones' names ------------------------------------------------------------------

def rig_chain_names():
    _, m = _rig()
    return [m["names"][ch["goal"]] for ch in m["chains"]]          # leg_ik_L, toe_ik_L, leg_ik_R, toe_ik_R


def _nf(x, up):
    return float(np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf)))


def tracks():
    """{name: (keys in file order as (frame, [(chain name, enabled)]), frames to ask for)}. Chains flip between keys, so a wrong span is
    a wrong pose."""
    if "tracks" in _memo:
        return _memo["tracks"]
    L, TL, R, TR = rig_chain_names()
    main = [
        (10, [(L, True), (R, False)]),
        (5, [(L, False), ("arm_ik_model_lacks", False)]),             # out of order in the file: flatten sorts (stably)
        (20, [(TL, False)]), (20, [(TL, True), (TR, False)]), (20, [(TR, True), (R, True), (L, False)]),      # three keys on one frame: the last wins
        (30, [(R, False)]),                                                # names one chain only: the others keep their state
        (100001, [(L, False), (TL, False), (R, False), (TR, False)]),      # beyond 100 000: float32 frames are 1 / 128 apart there
        (100003, [(L, True), (TL, True), (R, True), (TR, True)]),
    ]
    ask = [-3.0, _nf(5, False), 5.0, _nf(5, True), 7.5, 10.0, 15.0, _nf(20, False), 20.0, _nf(20, True), 25.0, 30.0, 31.0, 50000.0,
           _nf(100001, False), 100001.0, _nf(100001, True), 100002.0, 100003.0, 100010.0, 1.0e6]
    one = [(12, [(R, False), (TL, False), (TR, False)])]
    rng = np.random.default_rng(77)
    names = [L, TL, R, TR]
    f300 = np.cumsum(rng.integers(0, 4, size=300))                           # runs of equal frames included
    many = [(int(f), [(names[int(rng.integers(0, 4))], bool(rng.integers(0, 2)))]) for f in f300]
    ask300 = [float(x) for x in rng.uniform(-2.0, float(f300[-1]) + 2.0, size=10)] + [float(f300[0]), float(f300[150]), _nf(f300[150], False), float(f300[-1])]
    _memo["tracks"] = {"eight keys": (main, ask), "one key": (one, [0.0, _nf(12, False), 12.0, _nf(12, True), 13.0, 1.0e5]), "300 keys": (many, ask300),
                       "no keys": ([], [0.0, 7.0])}
    return _memo["tracks"]


def rig_motion(seed=3, nk=8):
    """a motion of the centre and the four goals of the leg rig (tests/motion_scenes.py: leg_motion), keys on frames 2 .. 64"""
    import motion_scenes as ms
    return ms.leg_motion(np.random.default_rng(seed), nk=nk)


SAMPLED_FRAMES = [2.0, 5.0, 7.5, 10.0, 15.0, 20.0, 25.0, 31.0]         # under the "eight keys" track: a different row at nearly every frame
