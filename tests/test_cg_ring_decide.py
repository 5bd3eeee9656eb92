"""CPU check of the host decisions of the classic CG pass about its ring of search directions (csrc/cg_decide.h), compiled with g++ (no GPU):
cg_ring_depth at its threshold (4e7 rows) and at the knob's bounds (0 = automatic, 1 .. 16 forced), the captured cycle's length, and the ring's
bookkeeping replayed over whole passes -- every iteration's update of x applied exactly once, in iteration order, wherever the pass ends."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cg_ring_decisions(tmp_path):
    exe = str(tmp_path / "host_check_cg")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_cg.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("OK")
