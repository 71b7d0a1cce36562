"""Compare two directories of normalised per-kernel disassembly (tools/archive/isa_dump.sh): for every kernel of the NEW directory, the kernel it
replaces in the OLD one (the hierarchy solve's six hand-written entries of kernels/front.hip became the six instantiations of
rz_fk_kernel<Stage...>; the motion stack's two, of kernels/motion.hip and kernels/motion_layers.hip, the two of rz_motion_kernel<P>),
identical or not, instruction counts, and the mnemonic histogram differences."""
import collections, difflib, os, sys
old, new = sys.argv[1], sys.argv[2]
OLD_NAME = {
    "rz_fk_kernel<>": "rz_fk_kernel",
    "rz_fk_kernel<RzIkParams>": "rz_fk_ik_kernel",
    "rz_fk_kernel<RzFollowParams>": "rz_fk_follow_kernel",
    "rz_fk_kernel<RzIkParams,RzFollowParams>": "rz_fk_ik_follow_kernel",
    "rz_fk_kernel<RzIkParams,RzIkSwitchParams>": "rz_fk_ik_sw_kernel",
    "rz_fk_kernel<RzIkParams,RzFollowParams,RzIkSwitchParams>": "rz_fk_ik_sw_follow_kernel",
    "rz_motion_kernel<RzMotionParams>": "rz_motion_blend_kernel",
    "rz_motion_kernel<RzLayerParams>": "rz_motion_layer_kernel",
}
def old_name(n): return OLD_NAME.get(n, n)
same = diff = 0
for f in sorted(os.listdir(new)):
    n = f[:-2]
    o = os.path.join(old, old_name(n) + ".s")
    if not os.path.exists(o):
        print("%-70s NEW (no counterpart)" % n); continue
    a, b = open(o).read().splitlines(), open(os.path.join(new, f)).read().splitlines()
    if a == b:
        same += 1; print("%-70s identical (%d instructions)" % (n, len(a))); continue
    diff += 1
    ha = collections.Counter(l.split()[0] for l in a if l and not l.endswith(":")); hb = collections.Counter(l.split()[0] for l in b if l and not l.endswith(":"))
    d = {k: hb[k] - ha[k] for k in set(ha) | set(hb) if hb[k] != ha[k]}
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    print("%-70s DIFFERS: %d -> %d instructions, similarity %.4f, histogram delta %s" % (n, len(a), len(b), sm.ratio(), dict(sorted(d.items())) if len(d) < 16 else "%d mnemonics" % len(d)))
print("%d identical, %d differ" % (same, diff))
