"""The frame kernel's record (reze-engine_amd/csrc/frame_kernel.h) on the CPU. tests/frame_kernel_main.cpp includes the header alone, is
built under AddressSanitizer and UBSan and prints, for every input of the resolver, the record, whether the product and the all-variants
build carry the instantiation, and its full symbol. The tests hold the product's symbols to the kernels the product build compiled, all
symbols to the all-variants build's (read from the device code objects with the ROCm LLVM tools), the FKV rule to its sentence, and
DeformContext.kernel_name()'s spelling (capi.kernel_name_of) to the record's."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FRAME_SOURCES = ("deform_dense", "deform_small", "crowd", "crowd_morph")
FRAME_KERNEL = re.compile(r"^(rz_deform_(dense|small)_kernel|rz_skin_instances(_fk)?(_morph)?_kernel|rz_skin_instances_reg_kernel)<")
SMALL, DENSE, CROWD, CROWD_FK, CROWD_REG = range(5)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_kernel") / "frame_kernel_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "frame_kernel_main.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.rstrip().splitlines()[-1].startswith("ok all "), out[-3000:]
    parsed = []
    for line in out.splitlines()[:-1]:
        head, rec, built, sym = line.split(" : ")
        kv = lambda s: {k: int(v) for k, v in (w.split("=") for w in s.split())}     # noqa: E731
        parsed.append((kv(head[3:]), kv(rec), kv(built), sym))
    assert len(parsed) == int(out.split()[-1]) == 3 * 4 * 2 * 64 * 6 + 3 * 12 * 2 + 2
    return parsed


def compiled_kernels(objdir):
    """demangled frame-kernel symbols in the device code of a build's kernel objects, or a reason why they cannot be read"""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")] + [shutil.which("c++filt") or "c++filt"]
    objs = [os.path.join(objdir, s + ".o") for s in FRAME_SOURCES]
    if not all(os.path.exists(o) for o in objs):
        return None, "the kernel objects are not built (%s)" % os.path.relpath(objdir, ROOT)
    if not all(os.path.exists(t) for t in tools):
        return None, "the ROCm LLVM tools are not installed"
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            fat, elf = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "k.elf")
            subprocess.check_call([tools[0], "--dump-section", ".hip_fatbin=" + fat, o, os.path.join(tmp, "scrap.o")])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
            table = subprocess.check_output([tools[2], "--symbols", "--wide", elf]).decode().splitlines()
            syms = [w[7] for w in (l.split() for l in table) if len(w) == 8 and w[3] == "FUNC" and w[6] != "UND"]
            for d in subprocess.check_output([tools[3]] + syms).decode().splitlines():
                d = re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "").replace("void ", ""))
                if FRAME_KERNEL.match(d):
                    names.add(d)
    return names, None


def test_the_product_set_is_exactly_the_builds(rows):
    """(a) the symbols whose record says `in the product` are the frame kernels the product build compiled, no more and no fewer"""
    built, why = compiled_kernels(os.path.join(ROOT, "reze-engine_amd", "csrc", "build"))
    if built is None:
        pytest.skip(why)
    named = {sym for _, _, b, sym in rows if b["product"]}
    assert named == built, (sorted(named - built)[:5], sorted(built - named)[:5])
    assert len(built) == 96 + 48 + 12 + 6 + 12 + 4


def test_nothing_is_unreachable_and_nothing_named_is_missing(rows):
    """(b) over all inputs the symbols a build can carry are the all-variants build's frame kernels: a plan cannot name a kernel that is
    not compiled in, nothing compiled in is unreachable. The inputs NO build carries are the 1024-thread MORPH fk front alone, which
    make_plan never asks for (plan.cpp keeps rz_fk_kernel in front of such a crowd), and every product kernel is in the larger build."""
    refused = [(i, r) for i, r, b, _ in rows if not b["all"]]
    assert refused and all(r["family"] == CROWD_FK and r["morph"] and r["block"] == 1024 for _, r in refused)
    assert all(b["all"] for _, _, b, _ in rows if b["product"])
    built, why = compiled_kernels(os.path.join(ROOT, "tools", "variants", "obj"))
    if built is None:
        pytest.skip(why)
    named = {sym for _, _, b, sym in rows if b["all"]}
    assert named == built, (sorted(named - built)[:5], sorted(built - named)[:5])


def test_the_fkv_rule(rows):
    """(c) FKV is 3 exactly when the shape is one a plan selects by default (rest geometry by plain loads; dense targets: nontemporal loads,
    eight deep) and no fused consumer is on, it becomes the solve's kind 1 / 2 when such a frame is not the one-launch form and solves a
    plain pose itself, and it is 0 for everything else."""
    seen = set()
    for i, r, _, _ in rows:
        selectable = not i["geo"] and (i["mode"] != 1 or (i["nt"] and i["U"] == 8))
        want = 3 if selectable and not i["consumer"] else 0
        if want == 3 and not i["fast"] and i["fk_on"] and i["fk_kind"] in (1, 2):
            want = i["fk_kind"]
        assert r["fkv"] == want, (i, r)
        seen.add(want)
    assert seen == {0, 1, 2, 3}


def test_the_record_is_the_inputs(rows):
    """family by the plan's crowd fields first, then the morph mode; template arguments as the kernels are instantiated; crowd fields zero
    outside the crowd families; `solve` = the kernel solves the hierarchy itself"""
    for i, r, _, sym in rows:
        fam = CROWD_REG if i["ppw"] > 0 else (CROWD_FK if i["subfk"] else CROWD) if i["group"] > 0 else DENSE if i["mode"] == 1 else SMALL
        assert r["family"] == fam
        assert r["S"] == (i["S"] if i["mode"] == 1 else (4 if i["S"] == 4 else 1)) and r["U"] == i["U"] and r["mode"] == i["mode"]
        assert (r["nt"], r["nts"], r["geo"], r["fast"]) == (i["nt"], i["nts"], i["geo"], i["fast"]) and r["q24"] == (i["q24"] if fam == DENSE else 0)
        crowd = fam in (CROWD, CROWD_FK)
        assert (r["block"], r["group"], r["sub"], r["morph"]) == ((i["block"], i["group"], i["subsets"], i["morphs"]) if crowd else (0, 0, 0, 0))
        assert (r["ppw"], r["kv"]) == ((i["ppw"], 8) if fam == CROWD_REG else (0, 0)) and r["solve"] == (1 if i["fk_on"] or fam == CROWD_FK else 0)
        assert sym.startswith(("rz_deform_small_kernel<", "rz_deform_dense_kernel<", "rz_skin_instances", "rz_skin_instances_fk", "rz_skin_instances_reg_kernel<")[fam])


def tuning_keys(i, r):
    """what rz_get_tuning reports for a frame of this record (tune.cpp: kReadKeys)"""
    return {"morph_mode": i["mode"], "effective_split": r["S"], "effective_unroll": r["U"], "effective_nt": 1 if r["nt"] and r["mode"] == 1 else 0,
            "effective_nt_store": r["nts"], "effective_geo": r["geo"], "effective_fast": r["fast"], "effective_variant": r["fkv"], "effective_inst_group": r["group"],
            "effective_inst_block": r["block"], "effective_subsets": r["sub"], "effective_fuse_fk": r["solve"], "effective_inst_morphs": r["morph"],
            "effective_poses_per_wg": r["ppw"]}


def test_kernel_name_agrees_with_the_record(rows, rz):
    """(d) capi.kernel_name_of over the record's key values is the full symbol with the dense kernel's eighth argument removed and nothing
    else different; (e) the stand-in name of tests/test_bench_rehearsal.py's fake context is one of those strings"""
    names = set()
    for i, r, _, sym in rows:
        want = re.sub(r", (true|false)>$", ">", sym) if r["family"] == DENSE else sym
        assert sym.count(",") == (7 if r["family"] == DENSE else want.count(","))
        assert rz.capi.kernel_name_of(tuning_keys(i, r)) == want, (i, r)
        names.add(want)
    assert set(tuning_keys(*rows[0][:2])) == set(rz.capi.KERNEL_NAME_KEYS)
    text = open(os.path.join(ROOT, "tests", "test_bench_rehearsal.py"), encoding="utf-8").read()
    stand_in = re.search(r'def kernel_name\(self\): return "([^"]+)"', text).group(1)
    assert stand_in in names, stand_in
