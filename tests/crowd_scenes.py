"""The scenes of the crowd-front tests: small crowds whose skinning is laid out by hand, so that the closure of every vertex run — the
bones it names plus all their ancestors, what the front of rz_skin_instances_fk_kernel solves (kernels/crowd.hip, plan.cpp: ensure_subfk)
— is known before anything runs. Shared by tests/test_gpu_crowd_front.py, which runs them on the device, and
tests/test_crowd_scenes_cpu.py, which restates the plan arithmetic in numpy and holds every scene to the numbers it claims here.
Test infrastructure.

Every scene has two vertex runs ("grid_cap" = runs x pose groups pins that whatever the device's CU count). Run 0 names the bones the
scene is about; run 1 names only the few bones at the top of the first tree, so its closure is shorter and its records are padded up to
the stride. A rigid vertex carries its bone in all four joint slots (a zero-weight slot still names its bone: kernels/crowd.hip,
rz_run_subsets_kernel), so a run names exactly the bones laid out for it. Where V is no multiple of 4 the padding vertices of the last
quad name bone 0, and the scene pins bone 0 to the first tree's root, which run 1 names anyway. Bone indices are a random permutation
of the order the skeleton is built in, arranged so that every child comes before its parent; a few spare root bones nobody names keep the
longest run list shorter than the skeleton, which is what lets the plan take the bone-subset form at all.

`expect` holds what the scene CLAIMS: runs, named bones and closure per run, stride, doubling rounds, (pose, closure slot) items per
pose group, the pose-group size and block the tuning asks for, whether the front is planned (`fused`) and, if not, the one admission
test that refuses it (`refused`: "rounds", "items" or "lds")."""
import numpy as np

BBOX_LO = np.array([-8.0, 0.0, -3.0], dtype=np.float32)
BBOX_HI = np.array([8.0, 22.0, 4.0], dtype=np.float32)
SPARES = 4
TOP = 3                         # run 1 names the top min(TOP, L) bones of the first tree
_memo = {}


def rounds_of(longest_chain):
    """doubling rounds for a longest chain of that many bones: 0, 1, 2, 3 for 1, 2-4, 5-16, 17-64; None beyond (the front is refused)"""
    for r, top in enumerate((1, 4, 16, 64)):
        if longest_chain <= top:
            return r
    return None


def _skeleton(chains, rng, pin0):
    """parents-first skeleton of root chains of the given lengths + SPARES spare roots, then permuted. Returns (parents, bind, inv_bind,
    chain_bones: per chain the permuted indices root first, spare bones)"""
    from reze_engine_amd import synth
    nat_parents = []
    for n in chains:
        first = len(nat_parents)
        nat_parents += [-1] + list(range(first, first + n - 1))
    nat_parents += [-1] * SPARES
    nat_parents = np.array(nat_parents, dtype=np.int32)
    B = len(nat_parents)
    nat_bind = (rng.random((B, 3), dtype=np.float32) - 0.5).astype(np.float32)
    nat_ib = synth.inverse_bind_translation_only(nat_parents, nat_bind)
    perm = rng.permutation(B)                                     # new index of natural bone n
    if pin0:                                                      # bone 0 = the first tree's root
        perm = np.concatenate([[0], 1 + rng.permutation(B - 1)])
    first = 0
    for n in chains:                                              # along every chain the indices descend: each child comes before its parent
        lo = first + (1 if pin0 and first == 0 else 0)
        perm[lo:first + n] = np.sort(perm[lo:first + n])[::-1]
        first += n
    parents = np.full(B, -1, dtype=np.int32)
    bind = np.zeros((B, 3), dtype=np.float32)
    inv_bind = np.zeros((B, 16), dtype=np.float32)
    for n in range(B):
        parents[perm[n]] = -1 if nat_parents[n] < 0 else perm[nat_parents[n]]
        bind[perm[n]] = nat_bind[n]
        inv_bind[perm[n]] = nat_ib[n]
    chain_bones, first = [], 0
    for n in chains:
        chain_bones.append([int(perm[first + k]) for k in range(n)])
        first += n
    return parents, bind, inv_bind, chain_bones, [int(perm[first + k]) for k in range(SPARES)]


def _skin_run(n_verts, bones, rng, n_rigid):
    """joints / weights of one run: n_rigid rigid vertices dealt round-robin over `bones` (the bone in all four slots, weight 255 on the
    first), then four-bone blends of distinct bones of the run (as many distinct ones as it has), u8 weights summing to 255"""
    bones = np.asarray(bones, dtype=np.int64)
    j = np.zeros((n_verts, 4), dtype=np.uint16)
    w = np.zeros((n_verts, 4), dtype=np.uint8)
    n_rigid = min(n_rigid, n_verts)
    j[:n_rigid] = bones[np.arange(n_rigid) % len(bones)][:, None]
    w[:n_rigid, 0] = 255
    for v in range(n_rigid, n_verts):
        pick = rng.choice(bones, size=4, replace=len(bones) < 4)
        cut = np.sort(rng.integers(1, 255, size=3))
        j[v] = pick
        w[v] = np.diff(np.concatenate([[0], cut, [255]]))
    return j, w


def _scene(name, chains, named0, V, I, inst_loop, inst_block, seed, pin0=False, rigid0=None):
    """chains: bone counts of the root chains; named0: which bones run 0 names, as (chain, level) pairs — run 1 names the top min(TOP, L)
    bones of chain 0"""
    rng = np.random.default_rng(seed)
    parents, bind, inv_bind, cb, spares = _skeleton(chains, rng, pin0)
    B = len(parents)
    G = min(inst_loop, I)
    groups = (I + G - 1) // G
    per = ((V + 1) // 2 + 63) // 64 * 64                          # two runs: plan.cpp inst_runs with grid_cap = 2 x groups
    assert per < V <= 2 * per
    run0 = [cb[c][k] for c, k in named0]
    run1 = cb[0][:min(TOP, chains[0])]
    j0, w0 = _skin_run(per, run0, rng, max(4 * len(run0), 256) if rigid0 is None else rigid0)
    j1, w1 = _skin_run(V - per, run1, rng, (V - per) // 2)
    pos = (BBOX_LO + rng.random((V, 3), dtype=np.float32) * (BBOX_HI - BBOX_LO)).astype(np.float32)
    nrm = rng.standard_normal((V, 3), dtype=np.float32)
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    q = rng.normal(size=(I, B, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    lt = ((rng.random((I, B, 3), dtype=np.float32) - 0.5) * 0.3).astype(np.float32)
    # what the scene claims
    closure0 = len({(c, a) for c, k in named0 for a in range(k + 1)})
    longest = max(k + 1 for _, k in named0)
    stride = max(closure0, len(run1))
    rounds = rounds_of(longest)
    lds = G * (2 * stride + max(len(set(run0)), len(run1))) * 48
    budget = (80 if inst_block == 256 else 156) * 1024
    refused = "rounds" if rounds is None else "items" if G * stride > 2 * inst_block else "lds" if lds > budget else None
    expect = dict(runs=2, per=per, named=(len(set(run0)), len(run1)), closure=(closure0, len(run1)), stride=stride, rounds=rounds, longest=longest,
                  G=G, block=inst_block, groups=groups, items=tuple(min(G, I - g * G) * stride for g in range(groups)), lds=lds,
                  fused=refused is None, refused=refused)
    return dict(name=name, V=V, B=B, I=I, mesh=dict(pos=pos, nrm=nrm, joints=np.concatenate([j0, j1]), weights=np.concatenate([w0, w1])),
                parents=parents, bind=bind, inv_bind=inv_bind, ap=np.full(B, -1, dtype=np.int32), ratio=np.zeros(B, dtype=np.float32),
                mv=np.zeros(B, dtype=np.uint8), q=q, lt=lt, chains=cb, spares=spares, run_bones=(sorted(set(run0)), sorted(run1)),
                tuning=dict(inst_loop=inst_loop, inst_block=inst_block, grid_cap=2 * groups), expect=expect, clip=None, frames=None)


def _all(chain, n):
    return [(chain, k) for k in range(n)]


def _chain(L, block=512, tip=False):
    """one chain of L bones, I = 5 at 4 poses per workgroup: a full group and a tail of one pose. tip: run 0 names the last bone only"""
    name = "chain(%d)" % L + (" tip only" if tip else "") + (" at %d threads" % block if block != 512 else "")
    return _scene(name, [L], [(0, L - 1)] if tip else _all(0, L), V=1000, I=5, inst_loop=4, inst_block=block, seed=1000 + L + (500 if tip else 0) + block)


def _append(sc, rng, bones, outside):
    """give `bones` append parents dealt round-robin from `outside`, ratios in [-1.2, 1.2], every second one appends movement too"""
    for n, b in enumerate(bones):
        sc["ap"][b] = outside[n % len(outside)]
        sc["ratio"][b] = np.float32(rng.uniform(-1.2, 1.2))
        sc["mv"][b] = n & 1
    sc["append_bones"] = [int(b) for b in bones]


def _append_scene():
    """chain(17) where every second chain bone follows an append parent, all of them spare roots: outside every run's closure"""
    sc = _scene("chain(17) with append parents outside the closure", [17], _all(0, 17), V=1000, I=5, inst_loop=4, inst_block=512, seed=2017)
    _append(sc, np.random.default_rng(2018), sc["chains"][0][1::2], sc["spares"])
    return sc


SAMPLED_FRAMES = (-2.0, 3.4, 9.75, 17.5, 1000.0)       # one per instance: before every first key (they lie at 1 or later), inside, past every last key


def _sampled_scene():
    """the chain(17) skeleton under a motion of uneven keys with interpolation bytes (synth.make_motion, as tests/motion_scenes.py builds
    its clips): every chain bone but one is keyed; two chain bones follow append parents outside the closure, one with a track and one
    without"""
    from reze_engine_amd import synth
    sc = _scene("chain(17) sampled", [17], _all(0, 17), V=1000, I=len(SAMPLED_FRAMES), inst_loop=4, inst_block=512, seed=3017)
    chain, spares = sc["chains"][0], sc["spares"]
    _append(sc, np.random.default_rng(3018), [chain[5], chain[12]], [spares[0], spares[1]])
    keyed = np.zeros(sc["B"], dtype=bool)
    keyed[chain] = True
    keyed[chain[9]] = False                                # a closure bone the motion leaves at rest
    keyed[spares[0]] = True                                # the append parent with a track; spares[1] has none
    sc["clip"] = synth.make_motion(sc["B"], 0, seed=3019, keyed=keyed, base=synth.make_motion_base(sc["B"], seed=3020), flip=0.3, trans=0.15)
    sc["frames"] = np.array(SAMPLED_FRAMES, dtype=np.float32)
    sc["q"] = sc["lt"] = None
    sc["tracked_parent"], sc["untracked_parent"] = spares[0], spares[1]
    return sc


_BUILDERS = {}
for _L in (1, 2, 4, 5, 16, 17, 64, 65):
    _BUILDERS["chain%d" % _L] = (lambda L: lambda: _chain(L))(_L)
_BUILDERS.update({
    "tip17": lambda: _chain(17, tip=True),
    "tip64": lambda: _chain(64, tip=True),
    # 256 threads, 8 poses per workgroup, four chains of 16: stride 64, 512 items = 2 x BLOCK in a full group
    "items256_tail3": lambda: _scene("4 x 16 bones at 256 threads, I = 19", [16] * 4, sum((_all(c, 16) for c in range(4)), []), V=1000, I=19, inst_loop=8, inst_block=256, seed=4019),
    "items256_tail1": lambda: _scene("4 x 16 bones at 256 threads, I = 17", [16] * 4, sum((_all(c, 16) for c in range(4)), []), V=999, I=17, inst_loop=8, inst_block=256, seed=4017, pin0=True),
    "items256_over": lambda: _scene("17 + 3 x 16 bones at 256 threads", [17, 16, 16, 16], sum((_all(c, n) for c, n in enumerate((17, 16, 16, 16))), []), V=1000, I=17, inst_loop=8,
                                    inst_block=256, seed=4065),
    # 512 threads, two chains of 64: stride 128, 1024 items = 2 x BLOCK, three rounds
    "items512": lambda: _scene("2 x 64 bones at 512 threads", [64, 64], _all(0, 64) + _all(1, 64), V=2000, I=9, inst_loop=8, inst_block=512, seed=5128),
    "chain17_1024": lambda: _chain(17, block=1024),
    # 1024 threads: the LDS budget (156 KB) binds before the item limit. A flat forest of n roots, all named: 8 x 3 n x 48 B
    "forest138": lambda: _scene("forest of 138 roots at 1024 threads", [1] * 138, [(c, 0) for c in range(138)], V=1999, I=9, inst_loop=8, inst_block=1024, seed=6138, pin0=True),
    "forest139": lambda: _scene("forest of 139 roots at 1024 threads", [1] * 139, [(c, 0) for c in range(139)], V=1999, I=9, inst_loop=8, inst_block=1024, seed=6139, pin0=True),
    "append17": _append_scene,
    "sampled17": _sampled_scene,
})
NAMES = tuple(_BUILDERS)
CHAIN_NAMES = tuple("chain%d" % L for L in (1, 2, 4, 5, 16, 17, 64, 65))


def scene(name):
    if name not in _memo:
        _memo[name] = _BUILDERS[name]()
    return _memo[name]
