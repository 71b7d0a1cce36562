"""The scenes of tests/crowd_scenes.py held to the numbers they claim, without a device: the plan arithmetic of a device-animated crowd
restated in numpy — the run split of inst_runs under the scene's grid_cap, the bones every run names (rz_run_subsets_kernel), their
closure under "parent of", the record stride and the doubling rounds of ensure_subfk, the item and LDS admission tests of make_plan
(reze-engine_amd/csrc/plan.cpp) — applied to the scene's mesh and skeleton arrays. tests/test_gpu_crowd_front.py asserts the
"effective_*" keys of the library against the same claims; this file is what keeps that from being circular."""
import numpy as np
import pytest

import crowd_scenes as cs


def inst_runs(V, I, G, grid_cap):
    """plan.cpp inst_runs with a caller's grid_cap: (vertices per run, runs)"""
    groups = (I + G - 1) // G
    gxi = max(1, grid_cap // groups)
    per = ((V + gxi - 1) // gxi + 63) // 64 * 64
    return per, (V + per - 1) // per


def named_bones(joints, V, B, per, runs):
    """rz_run_subsets_kernel: the ascending list of bones the joints of a run's vertices name, any weight — over whole quads, the padding
    vertices of the last quad carrying joints 0"""
    v_lim = (V + 3) // 4 * 4
    j = np.zeros((v_lim, 4), dtype=np.int64)
    j[:V] = np.minimum(joints.astype(np.int64), B - 1)
    return [sorted(set(j[r * per:min(v_lim, (r + 1) * per)].ravel().tolist())) for r in range(runs)]


def closure_of(named, parents):
    inside = set()
    for b in named:
        while b >= 0 and b not in inside:
            inside.add(b)
            b = int(parents[b])
    return sorted(inside)


def depth_of(b, parents):
    d = 0
    while parents[b] >= 0:
        b, d = int(parents[b]), d + 1
    return d


def plan(sc):
    """what plan.cpp makes of the scene: a dict with the fields of the scene's `expect`"""
    t = sc["tuning"]
    V, B, I, blk = sc["V"], sc["B"], sc["I"], t["inst_block"]
    G = min(t["inst_loop"], I)
    groups = (I + G - 1) // G
    per, runs = inst_runs(V, I, G, t["grid_cap"])
    named = named_bones(sc["mesh"]["joints"], V, B, per, runs)
    closures = [closure_of(n, sc["parents"]) for n in named]
    sub_max = max(len(n) for n in named)
    stride = max(len(c) for c in closures)
    max_depth = max(depth_of(b, sc["parents"]) for c in closures for b in c)
    rounds, span = 0, 1
    while span < max_depth + 1:                               # ensure_subfk's loop
        rounds, span = rounds + 1, span * 4
    budget = (80 if blk == 256 else 156) * 1024
    subsets = sub_max < B and sub_max <= blk and G * sub_max * 48 <= budget       # the bone-subset form behind rz_fk_kernel (finished rows: 48 B)
    lds = G * (2 * stride + sub_max) * 48
    failed = [what for what, bad in (("rounds", rounds > 3 or stride > 0xfff), ("items", G * stride > 2 * blk), ("lds", lds > budget)) if bad]
    return dict(runs=runs, per=per, named=tuple(len(n) for n in named), closure=tuple(len(c) for c in closures), stride=stride,
                rounds=rounds if rounds <= 3 else None, longest=max_depth + 1, G=G, block=blk, groups=groups,
                items=tuple(min(G, I - g * G) * stride for g in range(groups)), lds=lds, fused=subsets and not failed,
                refused=None if not failed else "+".join(failed)), subsets, named, closures


@pytest.mark.parametrize("name", cs.NAMES)
def test_every_scene_has_the_numbers_it_claims(name):
    sc = cs.scene(name)
    got, subsets, named, closures = plan(sc)
    assert subsets, "the bone-subset form itself must be planned"
    assert got == sc["expect"], (got, sc["expect"])
    assert [n for n in named] == [list(r) for r in sc["run_bones"]]
    e = sc["expect"]
    assert e["runs"] * e["groups"] == sc["tuning"]["grid_cap"]
    assert sc["V"] <= 4096 and sc["I"] <= 19 and max(e["named"]) < sc["B"]
    assert np.all(sc["mesh"]["weights"].astype(np.int64).sum(axis=1) == 255)
    p = sc["parents"]
    assert all(b < p[b] or p[b] == 0 for b in range(sc["B"]) if p[b] >= 0), "children come before their parents (bone 0 may be pinned to a root)"
    assert all(p[b] < 0 and b not in closures[0] and b not in closures[1] for b in sc["spares"])
    ib = sc["inv_bind"].reshape(-1, 4, 4)
    assert np.abs(ib[:, 3, :3]).max() > 0.1, "inverse bind matrices are not the identity"


def test_the_working_points_the_scenes_stand_on():
    """rounds 0 1 1 2 2 3 3 and the fall-back for chains of 1 2 4 5 16 17 64 65 bones; item counts at, under and over 2 x BLOCK; the LDS
    budget at 1024 threads; padding records; tail groups under BLOCK items; a V that is no multiple of 4"""
    E = {n: cs.scene(n)["expect"] for n in cs.NAMES}
    assert [E[n]["rounds"] for n in cs.CHAIN_NAMES] == [0, 1, 1, 2, 2, 3, 3, None]
    assert [E[n]["stride"] for n in cs.CHAIN_NAMES] == [1, 2, 4, 5, 16, 17, 64, 65]
    assert [E[n]["fused"] for n in cs.CHAIN_NAMES] == [True] * 7 + [False]
    for n in cs.CHAIN_NAMES:
        assert E[n]["items"] == (4 * E[n]["stride"], E[n]["stride"]) and E[n]["G"] == 4        # a full group and a tail of one pose
    for n, L in (("tip17", 17), ("tip64", 64)):
        assert E[n]["named"] == (1, 3) and E[n]["closure"] == (L, 3) and E[n]["rounds"] == 3 and E[n]["fused"]
    assert E["items256_tail3"]["items"] == (512, 512, 192) and E["items256_tail3"]["stride"] == 64 and E["items256_tail3"]["block"] == 256
    assert E["items256_tail1"]["items"] == (512, 512, 64) and E["items256_tail1"]["rounds"] == 2
    assert E["items256_over"]["items"][0] == 520 and E["items256_over"]["rounds"] == 3
    assert E["items512"]["items"] == (1024, 128) and E["items512"]["stride"] == 128 and E["items512"]["rounds"] == 3 and E["items512"]["block"] == 512
    assert E["chain17_1024"]["block"] == 1024 and E["chain17_1024"]["rounds"] == 3 and E["chain17_1024"]["fused"]
    assert E["forest138"]["rounds"] == 0 and E["forest138"]["stride"] == 138 and E["forest138"]["fused"]
    assert E["forest138"]["lds"] <= 156 * 1024 < E["forest139"]["lds"] and E["forest139"]["items"][0] <= 2 * 1024
    # the fall-back scenes fail exactly one admission test each
    assert {n: E[n]["refused"] for n in cs.NAMES if not E[n]["fused"]} == {"chain65": "rounds", "items256_over": "items", "forest139": "lds"}
    # padding records: run 1's closure is shorter than the stride wherever the first tree is deeper than the few bones run 1 names
    for n in cs.NAMES:
        if E[n]["longest"] > cs.TOP or len(cs.scene(n)["chains"]) > 1:
            assert E[n]["closure"][1] < E[n]["stride"], n
    assert any(cs.scene(n)["V"] % 4 for n in cs.NAMES)
    assert any(e["fused"] and e["items"][-1] <= e["block"] < e["items"][0] for e in E.values())      # a tail group whose second items are all dead


@pytest.mark.parametrize("name", [n for n in cs.NAMES if not n.startswith("tip")])
def test_every_bone_of_run_0_is_named_by_four_rigid_vertices(name):
    """positions and normals are the only outputs that see the front (world matrices read back afterwards come from rz_fk_kernel), and
    a blend averages a wrong matrix down: every level keeps vertices of its own"""
    sc = cs.scene(name)
    j, w, per = sc["mesh"]["joints"], sc["mesh"]["weights"], sc["expect"]["per"]
    rigid = (w[:per, 0] == 255) & (j[:per] == j[:per, :1]).all(axis=1)
    count = np.bincount(j[:per, 0][rigid], minlength=sc["B"])
    assert all(count[b] >= 4 for b in sc["run_bones"][0]), name
    assert (~rigid).sum() >= 64, "and some four-bone blends"
    if sc["expect"]["longest"] >= 4:
        assert (np.sort(j[:per][~rigid], axis=1)[:, 1:] != np.sort(j[:per][~rigid], axis=1)[:, :-1]).all(), "of four distinct bones"


def test_the_tip_only_scenes_give_one_bone_a_palette_slot():
    for n in ("tip17", "tip64"):
        sc = cs.scene(n)
        per = sc["expect"]["per"]
        assert set(sc["mesh"]["joints"][:per].ravel().tolist()) == {sc["chains"][0][-1]}


def test_append_parents_lie_outside_every_closure():
    for n in ("append17", "sampled17"):
        sc = cs.scene(n)
        _, _, _, closures = plan(sc)
        used = [b for b in sc["append_bones"]]
        assert used and all(b in closures[0] for b in used)
        assert all(sc["ap"][b] >= 0 and sc["ap"][b] not in closures[0] and sc["ap"][b] not in closures[1] for b in used)
        assert np.abs(sc["ratio"][used]).max() <= 1.2
    sc = cs.scene("append17")
    used = sc["append_bones"]
    assert sc["mv"][used].sum() == len(used) // 2 and len(used) >= 8
    assert np.abs(sc["ratio"][used]).max() > 1.0 and sc["ratio"][used].min() < 0 < sc["ratio"][used].max()       # clamped and negative ratios occur


def test_the_sampled_scene_has_uneven_keys_and_frames_beyond_both_ends():
    sc = cs.scene("sampled17")
    clip, f = sc["clip"], sc["frames"]
    off, kf = clip["key_off"], clip["key_frame"]
    firsts, lasts = kf[off[:-1]], kf[off[1:] - 1]
    assert f[0] < firsts.min() and f[-1] > lasts.max() and len(f) == sc["I"]
    assert any(firsts.min() < x < lasts.min() for x in f[1:-1])
    assert clip["key_interp"] is not None and len(set(np.diff(kf[off[0]:off[1]]).tolist())) > 1
    tracked = set(clip["track_bone"].tolist())
    assert sc["tracked_parent"] in tracked and sc["untracked_parent"] not in tracked
    assert {int(sc["ap"][b]) for b in sc["append_bones"]} == {sc["tracked_parent"], sc["untracked_parent"]}
    assert sum(b in tracked for b in sc["chains"][0]) == 16
