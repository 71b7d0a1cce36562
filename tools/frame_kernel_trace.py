#!/usr/bin/env python3
"""The launched frame kernel against the named one: the only check that sees the launcher's arm, not the tuning keys.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o walk -- python tools/frame_kernel_trace.py walk DIR/expected.txt
  python tools/frame_kernel_trace.py compare DIR/expected.txt DIR profiles/frame_kernel_names.txt

walk: tests/frame_kernel_walk.py once, one frame per arm; writes per arm its name, the full symbol the kernel record gives
(csrc/frame_kernel.h) and what kernel_name() says. compare: the frame kernels of the trace, in launch order, beside those symbols."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_KERNEL = re.compile(r"(rz_deform_(dense|small)_kernel|rz_skin_instances\w*_kernel)<[^>]*>")


def walk(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import frame_kernel_walk as fkw
    import reze_engine_amd as rz
    with open(out_path, "w") as out:
        for arm in fkw.walk(rz):
            name = arm["c"].kernel_name()
            arm["c"].deform()
            arm["c"].read(0)
            out.write("%s\t%s\t%s\n" % (arm["name"], arm["symbol"], name))
            out.flush()


def compare(expected_path, trace_dir, out_path):
    want = [l.rstrip("\n").split("\t") for l in open(expected_path)]
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    got = []
    for r in rows:
        m = FRAME_KERNEL.search(r["Kernel_Name"])
        if m:
            got.append(m.group(0))
    n = max(len(want), len(got))
    differ = 0
    with open(out_path, "w") as out:
        out.write("arm | symbol of the kernel record | kernel_name() | traced frame kernel\n")
        for i in range(n):
            w = want[i] if i < len(want) else ["-", "-", "-"]
            g = got[i] if i < len(got) else "-"
            differ += w[1] != g
            out.write("%s | %s | %s | %s%s\n" % (w[0], w[1], w[2], g, "" if w[1] == g else "   <-- differs"))
        out.write("%d arms, %d traced frame kernels, %d rows differ\n" % (len(want), len(got), differ))
    print(open(out_path).read())
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(walk(sys.argv[2]) if sys.argv[1] == "walk" else compare(*sys.argv[2:5]))
