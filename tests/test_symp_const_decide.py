"""CPU check of the constant form's decisions (csrc/symp_const_decide.h), no GPU needed: tools/host_check_symp_const.cpp, compiled with g++.

The gate (flagged share >= twice the break-even share c / (c + g), integer form against the rational one; the knob's two bits; no constant form without
usable step flags), the rotation of the runs among an XCD's waves (every run taken once per round; at the headline no wave meets the first or last
patch column more than once), and the entries a bind in
the constant form reads less than the stored form, against a hand count on the lattice (17, 33, 129) of tests/test_gpu_symp_const.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metafem.jl_amd", "csrc")


def test_host_check_symp_const(tmp_path):
    exe = str(tmp_path / "host_check_symp_const")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tools", "host_check_symp_const.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("OK")
