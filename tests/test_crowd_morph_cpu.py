"""The scenes of tests/crowd_morph_scenes.py held to the shapes they claim, and the definition held to float64 — without a GPU. What
tests/test_gpu_crowd_morphs.py then finds on the device is about the kernels, not about a scene that is not what it says.

The plan arithmetic restated here is plan.cpp's (inst_runs, make_plan's LDS admission) and kernels/crowd.hip's
(csrc/lds_layout.h: rzlds::crowd / rzlds::crowd_front with the weight block of G x Mpad x 4 B)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import crowd_morph_scenes as cms
from helpers import assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def test_the_launch_shape_the_scenes_assume():
    # plan.cpp inst_runs with grid_cap = runs x groups: per = round_up(ceil(V / runs), 64)
    assert cms.GROUPS == 3 and cms.GROUP_SIZES == tuple(min(cms.G, cms.I - g * cms.G) for g in range(cms.GROUPS))
    gxi = cms.TUNING["grid_cap"] // cms.GROUPS
    per = ((cms.V + gxi - 1) // gxi + 63) // 64 * 64
    assert gxi == cms.RUNS and per == cms.PER and (cms.V + per - 1) // per == cms.RUNS
    assert cms.V % 4 == 3 and cms.V4 == cms.V + 1                           # the last quad is padded
    assert cms.PER > 2 * 256 and cms.V4 - cms.PER > 2 * 256                 # more than one 256-vertex step in either run
    assert cms.PER % 64 == 0                                                # wave steps are aligned blocks of 64 vertices at every workgroup size
    # the bone-subset form needs run lists shorter than the skeleton
    named = [len(x) for x in cms.run_bones()]
    assert max(named) < cms.B and min(named) >= 2, named
    assert 12 <= cms.B <= 40


@pytest.mark.parametrize("name", cms.NAMES + ("nofit",))
def test_weights_and_deltas_are_what_the_module_says(name):
    s = cms.scene(name)
    mw = s["mw"]
    assert mw.shape == (s["I"], s["M"]) and mw.dtype == np.float32
    nz = mw[mw != 0]
    assert len(np.unique(nz)) == len(nz), "weights repeat"
    others = np.delete(mw, min(cms.ZERO_INSTANCE, s["I"] - 1), axis=0)
    assert 0.15 <= (others == 0).mean() <= 0.35 and (nz < 0).any() and (nz > 1).any()      # a quarter off (drawn over all instances)
    assert not mw[min(cms.ZERO_INSTANCE, s["I"] - 1)].any()
    d = s["d3"]
    assert len(np.unique(d.reshape(-1))) == d.size, "deltas repeat"
    assert np.isfinite(d).all() and (np.abs(d).max() < 0.06)
    assert np.array_equal(np.diff(s["ptr"]), s["rows"]) and s["ptr"][-1] == (s["idx"] < cms.V).sum()


def test_scattered_most_wave_steps_have_no_row_some_have_one():
    s = cms.scene("scattered")
    per_step = cms.wave_step_rows(s["rows"])
    assert len(per_step) == cms.WAVE_STEPS == 21
    assert (per_step == 0).sum() > cms.WAVE_STEPS // 2, per_step
    assert (per_step == 1).sum() >= 3 and (per_step > 1).any(), per_step
    assert {cms.run_of(v) for v in np.flatnonzero(s["rows"])} == {0, 1}          # rows in both runs


def test_face_straddles_a_wave_and_a_step_boundary_and_has_a_long_row():
    s = cms.scene("face")
    v0, n = cms.FACE
    assert n == 130 and v0 < 256 < 320 < v0 + n and v0 // 256 != (v0 + n - 1) // 256       # wave boundaries 256 and 320; 256 is a workgroup-step boundary at 256 threads
    assert cms.run_of(v0) == cms.run_of(v0 + n - 1) == 0
    rows = s["rows"]
    assert np.array_equal(np.flatnonzero(rows), np.arange(v0, v0 + n))
    assert rows[cms.FACE_LONG] == 72 > 64 and (np.delete(rows[v0:v0 + n], cms.FACE_LONG - v0) == s["M"]).all()       # every morph touches all of them
    # the duplicates lie apart in the file, and the upload keeps them in file order inside (vertex, morph)
    e = np.arange(s["ptr"][cms.FACE_LONG], s["ptr"][cms.FACE_LONG + 1])
    assert np.array_equal(s["morph"][e], np.repeat(np.arange(6), 12)) and (np.diff(s["src"][e]) > 1).all()


def test_edges_single_entry_rows_where_the_module_says():
    s = cms.scene("edges")
    rows = s["rows"]
    assert sorted(np.flatnonzero(rows).tolist()) == sorted(cms.EDGE_VERTS) and rows.max() == 1
    lanes = {v: v % 64 for v in cms.EDGE_VERTS}
    assert lanes[128] == 0 and lanes[191] == 63 and 128 // 64 == 191 // 64
    assert 0 % cms.PER == 0 and (cms.PER - 1) // cms.PER == 0 and cms.PER // cms.PER == 1       # first / last of run 0, first of run 1
    assert cms.V - 1 in cms.EDGE_VERTS and cms.run_of(cms.V - 1) == 1 and cms.V4 - 1 == cms.V     # V - 1 is the last real vertex of run 1; one padding vertex behind it


def test_empty_targets_with_no_row():
    s = cms.scene("empty")
    assert s["M"] == 3 and len(s["idx"]) == 3 and (s["idx"] >= cms.V).all() and s["off"][1] == s["off"][2]
    assert not s["rows"].any() and s["ptr"][-1] == 0


def test_lds_of_every_form_against_the_two_budgets():
    named = max(len(x) for x in cms.run_bones())
    for name in cms.NAMES:
        s = cms.scene(name)
        g = min(s["tuning"]["inst_loop"], s["I"])
        for blk in (256, 512, 1024):
            # subset form behind a front (48 B per bone), in one launch (112), whole palettes behind a front (48) and in one launch (64)
            for bones, per_bone in ((named, 48), (named, 112), (cms.B, 48), (cms.B, 64)):
                assert cms.lds_bytes(g, bones, per_bone, s["M"]) <= cms.BUDGET[blk], (name, blk, bones, per_bone)
    many = cms.scene("many")
    assert many["M"] == 300 and many["tuning"]["inst_loop"] == 8 and 8 * 300 * 4 == 9600 and 8 * cms.mpad(300) * 4 == 9856
    # the combination that must not fit: the weights alone leave less than two bones per pose under the larger budget, and whole palettes
    # would have to shrink the group — which a crowd with targets does not do (plan.cpp: it keeps the generic kernel)
    nf = cms.scene("nofit")
    g = min(nf["tuning"]["inst_loop"], nf["I"])
    assert g == 64 and nf["M"] == 600
    weights = g * cms.mpad(600) * 4
    assert weights == 155648 and weights > cms.BUDGET[256]
    assert weights + g * 2 * 48 > cms.BUDGET[512] and cms.lds_bytes(g, cms.B, 48, 600) > cms.BUDGET[512]
    assert cms.lds_bytes(g, named, 48, 600) > cms.BUDGET[1024]


@pytest.mark.parametrize("name", cms.NAMES)
def test_the_float32_chain_stays_inside_the_bars_of_the_float64_definition(name):
    """both from the scene's arrays: before any GPU run the scenes are ones the definition itself passes (bars: helpers.assert_parity,
    what tests/test_gpu_sparse_pieces.py uses)"""
    s = cms.scene(name)
    worst = np.zeros(2)
    for inst in sorted({0, 3, cms.ZERO_INSTANCE, s["I"] - 1}):
        p32, n32, _ = cms.sps.skin64(s, cms.chain32(s, s["mw"][inst]), s["mesh"]["worlds"][inst])
        p64, n64 = cms.reference64(s, inst)
        worst = np.maximum(worst, assert_parity(p32.astype(np.float32), n32.astype(np.float32), p64, n64, "%s instance %d" % (name, inst)))
        if inst == cms.ZERO_INSTANCE or name == "empty":
            base, _, _ = cms.sps.skin64(s, s["mesh"]["pos"], s["mesh"]["worlds"][inst])
            assert np.array_equal(p64, base)                # all-zero weights / no row: the unmorphed mesh
    print("crowd morph scenes | %s: float32 chain against float64: positions %.3e normals %.3e (bars 1e-4)" % (name, worst[0], worst[1]))
    # a mutant the bars must see: one entry with a non-zero weight dropped, out of the longest row that has one
    if s["rows"].any():
        inst = 0
        live = np.flatnonzero(s["mw"][inst][s["morph"]] != 0)
        vert = np.repeat(np.arange(cms.V), s["rows"])
        e = int(live[np.argmax(s["rows"][vert[live]])])
        bad, _, _ = cms.sps.skin64(s, cms.sps.morph64(s, s["mw"][inst], skip=e), s["mesh"]["worlds"][inst])
        p64, _ = cms.reference64(s, inst)
        err = np.linalg.norm(bad - p64, axis=1) / np.maximum(np.linalg.norm(p64, axis=1), 1.0)
        assert err.max() > 1e-3, "a dropped entry would pass the bar (%.3e)" % err.max()


@needs_node
def test_engine_option_with_a_recording_addon():
    """Engine { crowdMorphs } against a stand-in for the addon: inst_morphs = 1 on the shard behind setInstanceCount and on a fork right
    behind rz_fork; no such call without the option"""
    r = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "js", "crowd_morphs_engine_mock.js")], timeout=60).decode().strip().splitlines()[-1])
    assert r["on"] == ["setInstances:11", "setTuning:inst_morphs=1"]
    assert r["fork"] == ["setInstances:11", "setTuning:inst_morphs=1", "fork", "setTuning:inst_morphs=1:fork"]
    assert r["off"] == ["setInstances:11", "fork"]


def test_the_shipped_js_and_the_typings_carry_the_option():
    host = os.path.join(ROOT, "reze-engine_amd", "host")
    for f in ("engine.js", "index.d.ts", os.path.join("src", "engine.ts"), os.path.join("src", "types.d.ts")):
        assert "crowdMorphs" in open(os.path.join(host, f)).read(), f
