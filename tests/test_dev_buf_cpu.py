"""The owners of a context's device memory (reze-engine_amd/csrc/dev_buf.h) on the CPU. tests/dev_buf_main.cpp includes only that header
and brings its own hipMalloc / hipFree (malloc behind a live-block count, with a switch that fails the n-th allocation), under
AddressSanitizer and UBSan: release, move, borrow-by-copy, the grow path's failure and success, and a table reset as a whole after an
upload that failed part-way. A second test reads the host sources: no release list, no allocation beside an owner."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reze-engine_amd", "csrc")


def build_dev_buf_tool(folder):
    """tests/dev_buf_main.cpp under ASan and UBSan, the way test_pose_ring_cpu.py builds its program; the HIP headers only declare"""
    exe = str(folder / "dev_buf_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "dev_buf_main.cpp")])
    return exe


def test_owners_release_move_borrow_and_grow(tmp_path):
    """Every case prints one ok line: reset and scope end leave no live block; a move transfers ownership; a copy of a static table aliases
    and frees nothing, the original frees once; a grow whose replacement cannot be allocated keeps pointer, capacity and contents, a
    successful one frees the old block once, one that fits allocates nothing, a set moves together or not at all; four arrays of one table
    with the third allocation failing (the rz_upload_ik shape) leave nothing live once the table is reset as a whole."""
    exe = build_dev_buf_tool(tmp_path)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out[-3000:]
    for case in ("ok release:", "ok move:", "ok copy:", "ok grow:", "ok partial upload:", "ok all:"):
        assert case in out, (case, out[-3000:])


# what a context owns outright (ctx.h: rz_ctx): every one of these has an owner type, so rz_destroy has no line for it
OWNED = ("ovr_off", "ovr_bone", "ovr_world", "fol_off", "fol_ent", "rj01", "rj23", "sub_list", "sub_count", "subfk_rec", "subfk_count",
         "palette_ring", "act_idx_ring", "act_w_ring", "act_count_ring", "out_pos", "out_nrm", "out_hull", "aabb", "g_pos", "g_nrm", "tl",
         "ev_front", "ev_skin")


def test_host_sources_keep_no_release_list():
    """The host sources (csrc/*.cpp, ctx.h) free nothing by hand and allocate device memory through an owner only (dev_buf.h is the one
    place that calls the allocator: a function's scratch is a Scratch<T>), and rz_destroy names none of the buffers a context owns: the next
    feature gets its release by giving its array an owner, not by adding a line to a list."""
    sources = sorted(glob.glob(os.path.join(CSRC, "*.cpp"))) + [os.path.join(CSRC, "ctx.h")]
    assert len(sources) >= 9
    for path in sources:
        text = open(path, encoding="utf-8").read()
        name = os.path.basename(path)
        assert "dfree(" not in text, f"{name}: dfree is gone; give the array an owner (dev_buf.h)"
        assert "hipFree(" not in text, f"{name}: hipFree outside dev_buf.h; give the array an owner"
        assert not re.search(r"hipMalloc\s*\(", text), f"{name}: hipMalloc outside dev_buf.h; allocate through an owner (Scratch for a function's scratch)"
    core = open(os.path.join(CSRC, "core.cpp"), encoding="utf-8").read()
    m = re.search(r"^int rz_destroy\(rz_ctx \*c\)\n\{(.*?)^    delete c;", core, re.S | re.M)
    assert m, "rz_destroy not found in core.cpp"
    body = m.group(1)
    named = [b for b in OWNED if re.search(r"\b%s\b" % b, body)]
    assert not named, f"rz_destroy names {named}: a buffer the context owns is released by its owner"
    assert "RzStatic{}" not in body and "RzStatic {}" not in body, "a fork's RzStatic holds aliases: nothing to overwrite before the release"
