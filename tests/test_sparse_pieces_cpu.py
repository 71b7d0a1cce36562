"""What the GPU bars of tests/test_gpu_sparse_pieces.py rest on, checked without a GPU for every scene of tests/sparse_piece_scenes.py:
the scene has the shape it claims against its piece size (recomputed from the CSR the upload builds, not from the generator's lists),
every live entry moves its vertex by at least 50 x the parity bar, and the float64 reference with one entry dropped or doubled at a piece
edge misses the true reference by that much — so a frame that passes the bar staged, walked and weighted every single entry once."""
import numpy as np
import pytest

import sparse_piece_scenes as sps
from helpers import POS_TOL

MARGIN = 50.0


def pieces(e0, e1, P):
    return [(c0, min(e1, c0 + P)) for c0 in range(e0, e1, P)]


def per_round(s):
    return sps.round_ranges(s["ptr"], s["V"])


@pytest.mark.parametrize("name,P", sps.DESIGNS)
def test_the_csr_is_the_uploads_and_the_inputs_are_distinct(name, P):
    s = sps.scene(name, P)
    ptr, src, morph = s["ptr"], s["src"], s["morph"]
    # the upload's loops, literally (csrc/upload.cpp: count, prefix sum, scatter by ascending morph then file order)
    V = s["V"]
    cnt = np.zeros(V + 1, dtype=np.int64)
    for v in s["idx"]:
        if v < V:
            cnt[v + 1] += 1
    want_ptr = np.cumsum(cnt)
    cur, want_src, want_m = want_ptr[:-1].copy(), np.zeros(want_ptr[-1], dtype=np.int64), np.zeros(want_ptr[-1], dtype=np.int64)
    for m in range(sps.M):
        for e in range(int(s["off"][m]), int(s["off"][m + 1])):
            v = int(s["idx"][e])
            if v < V:
                want_src[cur[v]], want_m[cur[v]] = e, m
                cur[v] += 1
    assert np.array_equal(ptr, want_ptr) and np.array_equal(src, want_src) and np.array_equal(morph, want_m)
    assert len(s["idx"]) - len(src) == 3                                       # the three strays are dropped, nothing else
    assert np.array_equal(np.diff(ptr), s["rows"])
    if name == "long_row" and P >= 32:                                          # rows longer than the morph count: duplicates inside one morph
        v = int(np.argmax(s["rows"]))
        assert s["rows"][v] > sps.M and np.bincount(morph[ptr[v]:ptr[v + 1]]).max() >= 2
    for v in range(V):                                                          # ascending morph inside every row
        assert np.all(np.diff(morph[ptr[v]:ptr[v + 1]]) >= 0)
    assert len(np.unique(s["d3"], axis=0)) == len(s["d3"])
    nz = s["mw"][s["mw"] != 0]
    assert len(np.unique(np.abs(nz))) == len(nz) and np.all(np.abs(nz) >= 0.5) and np.all(np.abs(nz) <= 1.0)
    assert (s["mw"] == 0).sum() == sps.M // 4 and s["off"][sps.EMPTY_MORPH] == s["off"][sps.EMPTY_MORPH + 1] and s["mw"][sps.EMPTY_MORPH] != 0
    assert (s["mw2"] != 0).sum() == 3
    # the plan of so small a mesh: one 64-vertex step per wave at morph_split = 4, so the rounds are the kernel's steps
    assert sps.kernel_steps(V, 4) == [[(v0, min(64, (V + 3) // 4 * 4 - v0))] for v0 in range(0, V, 64)]        # (the last one: 3 vertices and their quad's padding)
    assert V == (sps.V if name != "tall" else sps.TALL_ROUNDS * 64 + 3) and sps.step_quads(sps.V, 4) == (2, 16)


@pytest.mark.parametrize("name,P", sps.DESIGNS)
def test_the_scene_has_the_shape_it_claims(name, P):
    s = sps.scene(name, P)
    ptr = s["ptr"]
    rr = per_round(s)
    totals = [e1 - e0 for _v0, _n, e0, e1 in rr]
    assert len(rr) == (sps.TALL_ROUNDS if name == "tall" else sps.ROUNDS) + 1 and rr[-1][1] == 3      # a ragged last round
    if name == "exact":
        assert totals[:5] == [P - 1, P, P + 1, 2 * P, 0]
        assert [len(pieces(e0, e1, P)) for _v0, _n, e0, e1 in rr[:5]] == [1, 1, 2, 2, 0]
        assert pieces(rr[2][2], rr[2][3], P)[1][1] - pieces(rr[2][2], rr[2][3], P)[1][0] == 1      # a piece of ONE entry
    elif name == "straddle":
        assert np.all(s["rows"][:64] == 5) and max(totals) >= 4 * P
        phases = set()
        for _v0, _n, e0, e1 in rr:
            ps = pieces(e0, e1, P)
            if e1 - e0 >= 4 * P:
                assert len(ps) >= 4                                            # the first piece asked for up front, three or more inside the loop
            for c0, _c1 in ps[1:]:                                             # every boundary: inside exactly one row, or between two
                cross = np.flatnonzero((ptr[:-1] < c0) & (ptr[1:] > c0))
                v = int(np.searchsorted(ptr, c0, side="right") - 1)
                phase = c0 - int(ptr[v])
                assert len(cross) == (1 if phase else 0)
                phases.add(phase)
        assert phases >= {1, 2, 3, 4}                                          # a boundary at every place inside a 5-entry row
    elif name == "long_row":
        L = 3 * P + 5
        for rnd, lane, near in ((0, 0, (1, 2)), (2, 63, (62, 61))):
            v0, _n, e0, e1 = rr[rnd]
            v = v0 + lane
            assert ptr[v + 1] - ptr[v] == L and [int(s["rows"][v0 + k]) for k in near] == [0, 1]
            span = [k for k, (c0, c1) in enumerate(pieces(e0, e1, P)) if max(c0, ptr[v]) < min(c1, ptr[v + 1])]
            assert len(span) >= 4 and span == list(range(span[0], span[-1] + 1))
        assert ptr[rr[0][0]] == rr[0][2]                                       # lane 0's row starts its round's first piece
    elif name == "holes":
        assert totals[0] == 0 and totals[2] == 0 and totals[4] == 0 and totals[1] > 0 and totals[3] > 0
        assert totals[5] > 2 * 16 and ptr[sps.V] == ptr[sps.V - 1] + s["rows"][-1] and s["rows"][-1] > 0      # the array ends with the last live lane's row
        assert ptr[sps.V] == len(s["src"])
    elif name == "tall":
        V = s["V"]
        ends = np.minimum(np.arange(0, V + 128, 1), V)

        def n_pieces(v0, n):
            e0, e1 = int(ptr[min(v0, V)]), int(ptr[ends[v0 + n]])
            return len(pieces(e0, e1, P))
        # 256-vertex steps, one workgroup: every wave's first step is four live rounds, in three waves every one of them takes two pieces
        # or more (bounds loaded round by round, pieces staged inside the loop only), and a second, ragged step follows
        steps = sps.kernel_steps(V, 1, grid_cap=1)
        four = [st for st in steps if len(st) == 4 and all(n_pieces(v0, n) >= 2 for v0, n in st)]
        assert len(steps) == 7 and len(four) >= 2 and sum(len(st) == 1 and st[0][1] == 32 for st in steps) == 3
        assert any(len(st) == 4 and st[-1][1] < 64 for st in steps)              # ... and a step whose fourth round is ragged
        # 64-vertex steps, one workgroup: second and later steps of a wave (the steady-state form) with four pieces or more, the first
        # asked for at the top of the step; and a wave that meets the empty round in mid-run
        steps = sps.kernel_steps(V, 4, grid_cap=1)
        per = sps.step_quads(V, 4, grid_cap=1)[1] * 4
        later = [st for st in steps if st[0][0] % per != 0]
        assert len(later) >= 8 and sum(n_pieces(*st[0]) >= 4 for st in later) >= 4 and any(n_pieces(*st[0]) == 0 for st in later)
        assert sum(int(x) == 3 * P + 5 for x in s["rows"]) == 3
    elif name == "bursts":
        assert totals[0] >= 64 * 9 and totals[1] >= 64 * 9
        for t in totals[:2]:
            assert (t + 255) // 256 >= 3                                       # sp_stage's i += 256 loop, three times in one piece at the plan's own size
        # all sixteen XOR patterns of sp_slot — (i >> 4) & 15 — carry live entries in the first 256 of the round
        v0, _n, e0, e1 = rr[0]
        live = s["mw"][s["morph"][e0:e0 + 256]] != 0
        assert all(live[16 * k:16 * k + 16].any() for k in range(16))
        assert sorted(i ^ ((i >> 4) & 15) for i in range(256)) == list(range(256))       # (a permutation inside every 16)


@pytest.mark.parametrize("name,P", sps.DESIGNS)
def test_every_entry_matters(name, P):
    """||S_v (w d_e)|| >= 50 x POS_TOL x max(||P_ref(v)||, 1) for every kept entry of a morph with a nonzero weight, both weight vectors"""
    s = sps.scene(name, P)
    ptr, src, morph = s["ptr"], s["src"], s["morph"]
    vert = np.repeat(np.arange(s["V"]), np.diff(ptr))
    for mw in (s["mw"], s["mw2"]):
        pref, _n, S3 = sps.skin64(s, sps.morph64(s, mw))
        w = mw.astype(np.float64)[morph]
        moved = np.linalg.norm(np.einsum("eij,ej->ei", S3[vert], w[:, None] * s["d3"].astype(np.float64)[src]), axis=1)
        bar = MARGIN * POS_TOL * np.maximum(np.linalg.norm(pref, axis=1), 1.0)[vert]
        livee = w != 0
        assert livee.any()
        worst = (moved[livee] / bar[livee]).min()
        assert worst >= 1.0, "%s P=%d: an entry moves its vertex by only %.2f x the margin" % (name, P, worst)


@pytest.mark.parametrize("name,P", sps.DESIGNS)
def test_mutants_miss_the_reference(name, P):
    """one entry dropped, or taken twice, at the first, the last and a middle position of a piece — the long row's included, and the very
    last entry of the array: each is off the true reference by >= 50 x the bar at its vertex"""
    s = sps.scene(name, P)
    ptr, morph = s["ptr"], s["morph"]
    live = s["mw"].astype(np.float64)[morph] != 0
    pref, nref = sps.reference64(s)
    denom = np.maximum(np.linalg.norm(pref, axis=1), 1.0)
    picks = {}
    for _v0, _n, e0, e1 in per_round(s):
        for c0, c1 in pieces(e0, e1, P):
            for kind, e in (("first", c0), ("last", c1 - 1), ("middle", (c0 + c1) // 2)):
                if kind not in picks and live[e]:
                    picks[kind] = e
    assert set(picks) == {"first", "last", "middle"}
    end = len(live) - 1
    while not live[end]:
        end -= 1
    if name == "holes":
        assert end >= len(live) - 2                # the array's last entry (or, where its morph is off, the one before)
    picks["array end"] = end
    if name == "long_row":
        v = int(np.argmax(s["rows"]))
        e0 = per_round(s)[v // 64][2]
        for where, at in (("long row, piece start", 0), ("long row, piece end", P - 1)):      # a live entry of the long row on either side of a boundary
            inside = [e for e in range(int(ptr[v]), int(ptr[v + 1])) if live[e] and (e - e0) % P == at]
            assert inside, where
            picks[where] = inside[-1]
    for what, e in picks.items():
        v = int(np.searchsorted(ptr, e, side="right") - 1)
        for mutant in (dict(skip=e), dict(twice=e)):
            pm, _nm = sps.reference64(s, **mutant)
            err = np.linalg.norm(pm - pref, axis=1) / denom
            assert err[v] >= MARGIN * POS_TOL, "%s P=%d %s %r: %.2e" % (name, P, what, mutant, err[v])
            assert np.count_nonzero(err) == 1


def test_piece_sizes_cover_the_designs():
    """every designed piece size is one the GPU test runs (the plan's own, 2048 here, as 0)"""
    assert {P for _n, P in sps.DESIGNS} <= {p or sps.AUTO_PIECE for p in sps.PIECES}
    assert min(64 * sps.M, 2048) == sps.AUTO_PIECE
