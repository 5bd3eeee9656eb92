"""CPU check of the trimmed patch sweep's decisions (csrc/symp_trim_decide.h), no GPU needed: tools/host_check_symp_trim.cpp, compiled with g++.

For m1, m2 in {8, 9, 12, 16, 17, 32, 33, 34, 35, 64, 65, 513} and B in {1, 2}: the swept patches and the rim rows tile the lattice plane exactly once, the
corner rows are counted once (in the line rim), row <-> rim index round-trips in both directions, no direction is trimmed to zero patches, 513 x 513 at
B = 2 gives 1024 patches and 1025 rim rows per plane, and the run-count rule of the sweep (spt_nseg, the arithmetic symp_nseg uses) gives 3 runs per patch
on 1024 patches and 768 slots where the 1105 untrimmed patches got 2."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metafem.jl_amd", "csrc")


def test_host_check_symp_trim(tmp_path):
    exe = str(tmp_path / "host_check_symp_trim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tools", "host_check_symp_trim.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("OK")
