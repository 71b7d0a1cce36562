"""The reuse proof of the zero-copy and big-pose rings (reze-engine_amd/csrc/pose_ring.h) on the CPU: tests/pose_ring_main.cpp includes
only that header and walks it against a brute-force model, under AddressSanitizer and UBSan."""
import os
import subprocess


def build_pose_ring_tool(folder):
    """tests/pose_ring_main.cpp under ASan and UBSan (the way physics_scenes.build_table_tool builds the physics table program)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(folder / "pose_ring_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(root, "tests", "pose_ring_main.cpp")])
    return exe


def test_ring_reuse_proof_against_a_brute_force_model(tmp_path):
    """N = 8 and N = 32, uploads 0 .. 4 N + 3: an event is recorded exactly every N / 2 uploads; from upload N on the event polled carries a
    sequence in [u - N + 1, u - N / 2] — it covers every reader of the slot's previous tenant and is at least half a ring old — and has
    not been overwritten; after a reset the first N uploads poll nothing; corrupted books answer "inconsistent" instead of a poll."""
    exe = build_pose_ring_tool(tmp_path)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out[-3000:]
    assert "N=8 ok: 28 polls over 36 uploads" in out and "N=32 ok: 100 polls over 132 uploads" in out
