"""The LDS ledger (reze-engine_amd/csrc/lds_layout.h) on the CPU. tests/lds_layout_main.cpp includes the header alone (and physics_table.h for
the physics stage's limit), is built under AddressSanitizer and UBSan and prints every family's regions over a small grid; the tests hold the
regions to order, alignment and their totals, the totals to the formulas the other tests keep in Python, and the generic frame to its known
edges. A last test reads the sources: the CU's LDS size and the opt-in above 48 KB are spelled once."""
import glob
import os
import re
import subprocess

import pytest

import crowd_morph_scenes as cms
import physics_scenes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reze-engine_amd", "csrc")
CU = 160 * 1024
# regions a kernel reads or writes with 16-byte LDS accesses (float4 rows, LDS-DMA bursts, ds_write_b128 of parked quads) start 16-aligned
ALIGNED = {"palette", "scratch", "parked", "pieces", "second", "palettes", "slots", "A", "B", "rows", "dq"}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_layout") / "lds_layout_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "lds_layout_main.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.rstrip().endswith("ok all"), out[-3000:]
    return out.splitlines()


def layouts(lines, family):
    """(arguments, [(region, offset, bytes)], extras, total) of every line of one family"""
    for line in lines:
        if not line.startswith(family + " "):
            continue
        head, body = line.split(" : ")
        args = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
        regions, extras, total = [], {}, None
        for part in (s.split() for s in body.split(";")):
            if part[0] == "total":
                total = int(part[1])
            elif part[0] in ("alias", "work", "scalars", "staged_off", "poses_bytes"):
                extras[part[0]] = tuple(int(x) for x in part[1:])
            else:
                regions.append((part[0], int(part[1]), int(part[2])))
        yield args, regions, extras, total


def round16(n):
    return (n + 15) // 16 * 16


def test_limits_are_todays(lines):
    """the named limits carry the values the plan and the refusals have always used; the physics stage's limit is the shared one"""
    words = lines[0].split()
    assert words[0] == "limits"
    got = dict(zip(words[1::2], words[2::2]))
    assert [int(got[k]) for k in ("cu", "optin", "half", "crowd", "reserve")] == [CU, 48 * 1024, 80 * 1024, 156 * 1024, 8192]
    assert words[-2] == "physics" and int(words[-1]) == ps.LDS_LIMIT == CU
    assert lines[0].split(" fit ")[1].split()[:2] == ["12", "4096"] and lines[0].split(" piece ")[1].split()[:3] == ["4096", "1024", "16"]
    assert (CU - 8192) // 48 == 3242           # what rz_upload_skeleton admits


@pytest.mark.parametrize("family", ["solve", "frame", "crowd", "crowd_front", "after", "qdef"])
def test_regions_are_ordered_aligned_and_sum_to_the_total(lines, family):
    """every region starts where the one in front of it ends (no gap, no overlap), regions of 16-byte accesses start 16-byte aligned, and
    total() is the end of the last region — for the generic frame the end of the work area, whose size is the larger of the step scratch +
    parked outputs + pieces and the fused solve's scratch, which aliases it from its first byte"""
    n = 0
    for args, regions, extras, total in layouts(lines, family):
        n += 1
        end = 0
        for name, off, size in regions:
            assert off == end, (family, args, name, off, end)
            if name in ALIGNED and size:
                assert off % 16 == 0, (family, args, name, off)
            end = off + size
        if family == "frame":
            work0 = regions[3][1]
            assert regions[3][0] == "scratch" and extras["alias"][0] == work0 and work0 % 16 == 0
            assert extras["work"][0] == max(end - work0, extras["alias"][1]), (args, extras)
            assert bool(extras["alias"][1]) == bool(args["fused"])
            end = work0 + extras["work"][0]
        assert total == end, (family, args, total, end)
    assert n >= 3


def expected_regions(family, a):
    """every region of a layout restated from its arguments alone: [(name, offset, bytes)]"""
    if family == "solve":
        sizes = [("palette", a["B"] * 48), ("scratch", round16(a["B"] * 60)), ("weights", round16(a["n"] * 4) if a["ik"] else a["n"] * 4), ("second", a["B"] * 48 if a["ik"] else 0)]
    elif family == "frame":
        sizes = [("palette", a["B"] * 48), ("idx", a["pad"] * 4), ("w", a["pad"] * 4), ("scratch", 4 * a["planes"] * a["vw"] * 4), ("parked", 4 * a["out_cap"] * 24),
                 ("pieces", 4 * a["sp_cap"] * 16)]
    elif family == "crowd":
        sizes = [("slots", a["G"] * a["bones"] * (48 if a["dma"] else 112 if a["subsets"] else 64)), ("weights", a["G"] * a["morph_pad"] * 4)]
    elif family == "crowd_front":
        sizes = [("A", a["G"] * a["closure"] * 48), ("B", a["G"] * a["closure"] * 48), ("palettes", a["G"] * a["named"] * 48), ("weights", a["G"] * a["morph_pad"] * 4)]
    elif family == "after":
        sizes = [("rows", a["B"] * 48), ("skip", round16(a["n"]))]
    else:
        sizes = [("dq", a["B"] * 32)]
    out, off = [], 0
    for name, size in sizes:
        out.append((name, off, size))
        off += size
    return out


@pytest.mark.parametrize("family", ["solve", "frame", "crowd", "crowd_front", "after", "qdef"])
def test_every_region_is_where_the_arguments_put_it(lines, family):
    """offsets and sizes as the layout returns them against the same regions restated here from the arguments; the scalars two kernels
    add in place of a struct field (rz_fk_kernel: palette_bytes, solve_scratch; the MORPH crowd kernels: crowd_poses_bytes) equal that
    field, and crowd().staged_off, which the one hand-written carve is named after, is G x bones x 48: behind the palette region"""
    for a, regions, extras, _ in layouts(lines, family):
        assert regions == expected_regions(family, a), (family, a, regions)
        if family == "solve":
            assert extras["scalars"] == (a["B"] * 48, round16(a["B"] * 60))
        if family == "crowd":
            assert extras["staged_off"] == (a["G"] * a["bones"] * 48,) and extras["poses_bytes"] == (regions[1][1],)
        if family == "frame" and a["fused"]:
            assert extras["alias"] == (a["B"] * 48 + a["pad"] * 8, round16(a["B"] * 60) + max(a["M"], 1) * 4 + 16)


def test_totals_equal_the_independent_formulas(lines):
    """crowd forms: crowd_morph_scenes.lds_bytes and crowd_scenes' G x (2 stride + named) x 48; physics: physics_scenes.lds_bytes;
    after-physics: B x 48 + round16(n); solve: 108 B per bone (156 with IK) + the weights; QDEF: 32 B per bone"""
    for a, _, _, total in layouts(lines, "crowd"):
        per_bone = 48 if a["dma"] else 112 if a["subsets"] else 64
        assert a["slot"] == per_bone
        assert total == a["G"] * a["bones"] * per_bone + a["G"] * a["morph_pad"] * 4
        if a["morph_pad"] == cms.mpad(a["morph_pad"] - 8) and a["morph_pad"]:
            assert total == cms.lds_bytes(a["G"], a["bones"], per_bone, a["morph_pad"] - 8)
    for a, _, _, total in layouts(lines, "crowd_front"):
        assert total == a["G"] * (2 * a["closure"] + a["named"]) * 48 + a["G"] * a["morph_pad"] * 4
    for a, _, _, total in layouts(lines, "after"):
        assert total == a["B"] * 48 + round16(a["n"])
    for a, _, _, total in layouts(lines, "qdef"):
        assert total == a["B"] * 32
    for a, _, _, total in layouts(lines, "solve"):
        w = a["n"] * 4
        assert total == a["B"] * 48 + round16(a["B"] * 60) + (round16(w) + a["B"] * 48 if a["ik"] else w)
    seen = 0
    for line in lines:
        if line.startswith("physics "):
            head, body = line.split(" : ")
            a = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
            plain, springs = (int(x) for x in body.split())
            assert plain == ps.lds_bytes(a["nb"], a["nj"]), a
            assert springs == a["nb"] * 96 + (a["nj"] * 24 if a["nj"] > a["block"] else 0), a
            seen += 1
    assert seen >= 40 and ps.lds_bytes(ps.MOST_BODIES, 0) <= CU < ps.lds_bytes(ps.MOST_BODIES + 1, 0)
    fit = {tuple(int(x.split("=")[1]) for x in l.split(" : ")[0].split()[1:]): int(l.split(" : ")[1]) for l in lines if l.startswith("fused_fit ")}
    assert fit[(1479, 0)] <= CU < fit[(1480, 0)] and all(v == B * 48 + round16(B * 60) + M * 12 + 4096 for (B, M), v in fit.items())


def test_generic_frame_at_its_known_edges(lines):
    """64-vertex steps of 3 planes (3 KB of step scratch). 3 242 bones, the most rz_upload_skeleton admits, fit without write batching and
    not with the smallest buffer (64 vertices per wave); 3 200 bones with sparse targets (60 - 64 morphs: lists of 72) fit only with
    out_cap = 0, then with a piece of 16 and of 64 entries per wave; and the fused solve's alias sets the work area exactly where it is
    the larger region"""
    frames = {tuple(sorted(a.items())): (extras, total) for a, _, extras, total in layouts(lines, "frame")}

    def total(**a):
        return frames[tuple(sorted(dict(dict(pad=0, planes=3, vw=64, out_cap=0, sp_cap=0, fused=0, M=0), **a).items()))]

    assert total(B=3242)[1] == 3242 * 48 + 3072 <= CU < total(B=3242, out_cap=64)[1] == 3242 * 48 + 3072 + 6144
    sparse = dict(B=3200, pad=72, M=64)
    assert total(sp_cap=16, **sparse)[1] == 3200 * 48 + 576 + 3072 + 1024 <= CU and total(sp_cap=64, **sparse)[1] <= CU
    assert total(sp_cap=16, out_cap=64, **sparse)[1] > CU and total(sp_cap=2048, **sparse)[1] > CU
    # the alias: 349 bones need 20 944 + 4 x 64 + 16 = 21 216 B of solve scratch and weights
    small, big = total(B=349, pad=72, M=64, fused=1), total(B=349, pad=72, M=64, fused=1, out_cap=640, sp_cap=64)
    assert small[0]["alias"][1] == round16(349 * 60) + 64 * 4 + 16 == 21216
    assert small[0]["work"][0] == 21216 > 3072 and small[1] == 349 * 48 + 576 + 21216
    assert big[0]["work"][0] == 3072 + 4 * 640 * 24 + 4096 > 21216


def test_one_spelling_of_the_limit_and_of_the_opt_in():
    """no source under csrc/ but lds_layout.h spells the CU's LDS size, and hipFuncAttributeMaxDynamicSharedMemorySize is named by
    rz_opt_in_lds (kernels/common.hip.h) alone: a new launcher calls the helper, a new fit reads the header"""
    sources = [p for p in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True)
               if os.path.isfile(p) and os.path.splitext(p)[1] in (".cpp", ".h", ".hip", ".c") and "build" not in os.path.relpath(p, CSRC).split(os.sep)]
    assert len(sources) >= 30
    for path in sources:
        text = open(path, encoding="utf-8").read()
        name = os.path.relpath(path, CSRC)
        if name != "lds_layout.h":
            assert not re.search(r"160u?\s*\*\s*1024|163840", text), f"{name}: the CU's LDS is rzlds::kCuLds (lds_layout.h)"
        uses = len(re.findall(r"hipFuncAttributeMaxDynamicSharedMemorySize", text))
        assert uses == (1 if name == os.path.join("kernels", "common.hip.h") else 0), f"{name}: launchers opt in through rz_opt_in_lds (kernels/common.hip.h)"
