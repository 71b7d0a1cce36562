"""Scenes for the linear joint springs (tests/test_spring_cpu.py, tests/test_gpu_springs.py): tables of physics_scenes and of the three contact
scenes modules with spring_position replaced and position_min / position_max widened on a copy. Every case the GPU tests run is listed in
CASES and checked for conditioning and for the springs' effect on the CPU."""
import numpy as np

import contact_box_scenes as bs
import contact_boxbox_scenes as bbs
import contact_scenes as cs
import physics_ref
import physics_scenes as ps
import spring_ref

KS = (0.0, 50.0, 200.0, 1000.0)
PLAY = 0.4
LDS_PER_JOINT = 24                  # the striding form's multipliers with the linear springs' three more
MOST_STRANDS = (ps.LDS_LIMIT - ps.LDS_PER_BODY) // (ps.LDS_PER_BODY + LDS_PER_JOINT)       # strands of one body under one shared base: 1364


def with_columns(sc, spring, pmin=None, pmax=None):
    t = dict(sc["table"])
    t["spring_position"] = np.asarray(spring, dtype=np.float32).reshape(t["n_joints"], 3)
    if pmin is not None:
        t["position_min"], t["position_max"] = np.asarray(pmin, dtype=np.float32), np.asarray(pmax, dtype=np.float32)
    return dict(sc, table=t)


def sprung(sc, seed):
    """mixed k from KS per axis and +-PLAY of play on two joints in three; every third joint stays locked, with a spring on it"""
    t = sc["table"]
    nj = t["n_joints"]
    rng = np.random.default_rng(900 + seed)
    k = rng.choice(KS, size=(nj, 3))
    locked = np.arange(nj) % 3 == 2
    k[locked, 0] = rng.choice(KS[1:], size=int(locked.sum()))
    pmin, pmax = np.array(t["position_min"], dtype=np.float32), np.array(t["position_max"], dtype=np.float32)
    pmin[~locked] -= np.float32(PLAY); pmax[~locked] += np.float32(PLAY)
    return with_columns(sc, k, pmin, pmax)


def one_axis(ax):
    """a small scene with a spring on one axis only and play on all three; joint frames (random `rotation`) and body frames (random
    `offset_rot`) all differ: a swapped axis, or B's frame for A's, moves the bodies elsewhere"""
    sc = ps.strands(2, 3, base=True, seed=31, sprung=True, n_verts=64)
    nj = sc["table"]["n_joints"]
    k = np.zeros((nj, 3)); k[:, ax] = 1000.0         # (y: at 200 a body still hangs at the end of its play, m g / k = 0.49 > 0.4)
    assert np.abs(sc["table"]["rotation"]).min() > 0 and (np.abs(sc["table"]["offset_rot"][:, :3]).max(axis=1) > 0).all()
    return with_columns(sc, k, np.full((nj, 3), -PLAY), np.full((nj, 3), PLAY))


def roles():
    """the "contents" scene (8 bodies, 6 joints): follower - dynamic (joints 0, 1, 4), dynamic - dynamic (2, 5), follower - follower (3:
    nothing may move), the zero-inertia body 6 (4, 5), position limits given max first (1), a spring on a locked axis (4: y; 5: all), k < 0 (2: y)"""
    sc = ps.scene("contents")
    t = sc["table"]
    k = [[200, 0, 50], [50, 50, 50], [1000, -50, 200], [200, 200, 200], [50, 200, 0], [0, 1000, 50]]
    pmin, pmax = np.array(t["position_min"], dtype=np.float32), np.array(t["position_max"], dtype=np.float32)
    pmin[0], pmax[0] = [-PLAY, 0, -PLAY], [PLAY, 0, PLAY]
    pmin[1], pmax[1] = [0.3, 0.3, 0.3], [-0.3, -0.3, -0.3]
    pmin[2] -= np.float32(PLAY); pmax[2] += np.float32(PLAY)
    pmin[3], pmax[3] = [-PLAY] * 3, [PLAY] * 3
    pmin[4], pmax[4] = [-PLAY, 0, 0], [PLAY, 0, 0]
    return with_columns(sc, k, pmin, pmax)


def strands_table(n):
    """n strands of one sprung body under one shared base, 1000 of them on bones, as physics_scenes' "most strands" has"""
    return sprung(ps.strands(n, 1, base=False, seed=28, n_verts=600, sprung=True, boned=1000), 28)


def _plain(make, calls=ps.CALLS):
    def build():
        sc = make()
        return sc, [ps.pose(sc, k) for k in range(len(calls))], calls
    return build


def _contact(module, name, seed):
    def build():
        sc, poses, calls = module.case(name)
        return sprung(sc, seed), poses, calls
    return build


# name: (builder of (scene, poses, calls), contact mode, (lanes per workgroup, joints in registers?) the launch must take)
CASES = {
    "own 64": (_plain(lambda: sprung(ps.scene("crowd"), 1)), 0, (64, 1)),
    "stride 64": (_plain(lambda: sprung(ps.scene("65 joints"), 2)), 0, (64, 0)),
    "own 256": (_plain(lambda: sprung(ps.scene("65 bodies 64 joints"), 3)), 0, (256, 1)),
    "stride 256": (_plain(lambda: sprung(ps.scene("257 joints"), 4)), 0, (256, 0)),
    "x only": (_plain(lambda: one_axis(0)), 0, (64, 1)),
    "y only": (_plain(lambda: one_axis(1)), 0, (64, 1)),
    "z only": (_plain(lambda: one_axis(2)), 0, (64, 1)),
    "roles": (_plain(roles), 0, (64, 1)),
    "h and iterations": (_plain(lambda: sprung(ps.strands(**ps.CROWD, h=1 / 120, iterations=1), 5)), 0, (64, 1)),
    "most strands": (_plain(lambda: strands_table(MOST_STRANDS), ps.EDGE_CALLS), 0, (256, 0)),
}
for _mode, _module in ((1, cs), (2, bs), (3, bbs)):
    for _form, _shape in cs.FORMS.items():
        CASES["contacts %d %s" % (_mode, _form)] = (_contact(_module, _form, 10 * _mode + len(CASES)), _mode, _shape)
ORDER = list(CASES)
CROWD = "own 64"
_memo = {}


def case(name):
    """(scene, poses, calls)"""
    if name not in _memo:
        _memo[name] = CASES[name][0]()
    return _memo[name]


def sim_of(name, dtype=np.float64, springs=True):
    sc = case(name)[0]
    return spring_ref.Sim(sc["table"], sc["parents"], sc["bind"], dtype=dtype, mode=CASES[name][1], springs=springs)


def reference(name, dtype=np.float64, springs=True):
    """the case's run under the definition (memoised, not to be written to): per call (world [B,16] with overrides, state [nb,13])"""
    key = (name, np.dtype(dtype).name, springs)
    if key not in _memo:
        sc, poses, calls = case(name)
        _memo[key] = ps.run_reference(sc, poses, calls, dtype=dtype, sim=sim_of(name, dtype, springs))
    return _memo[key]


def conditioning(name):
    """largest float32-probe deviation from the float64 run over the case's horizon, in units of extent"""
    a, b = reference(name), reference(name, dtype=np.float32)
    worst = max(max(float(np.abs(wa - wb).max()), float(np.abs(sa[:, :3] - sb[:, :3]).max())) for (wa, sa), (wb, sb) in zip(a, b))
    return worst / case(name)[0]["extent"]


def effect(name):
    """how far the springs move the bodies: the largest difference, over the calls, between the definition with and without the stage, in
    units of extent"""
    a, b = reference(name), reference(name, springs=False)
    return max(float(np.abs(sa[:, :3] - sb[:, :3]).max()) for (_, sa), (_, sb) in zip(a, b)) / case(name)[0]["extent"]


def axes_of(t):
    return int((np.asarray(t["spring_position"]) > 0).sum())


def node_case():
    """The Node end-to-end test's scene: the sprung "crowd" strands as a PMX file, run with the table its loader derives from the file,
    under one fixed local pose. Returns (scene, pmx bytes, q [B,4])."""
    if "node" not in _memo:
        sc = case(CROWD)[0]
        data, want = ps.write_pmx(sc)
        q, _ = ps.pose(sc, 70, amount=2.0)
        _memo["node"] = (dict(sc, table=want), data, q)
    return _memo["node"]
