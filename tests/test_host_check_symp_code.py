"""CPU checks of the coded-diagonal form of the patch sweep's copy (csrc/spmv_symp.h), no GPU needed.

1. tools/host_check_symp_code.cpp, compiled with g++: the code bytes, the edge block and the 13 slots of every band tile the main part of a step without
   overlap for B = 1 and B = 2, every piece is 16-byte aligned, the default form reproduces the stored form's constants (2196 / 4068 table doubles,
   318 / 354 edge entries, SP_MAIN), the code <-> double round trip is exact for the codes -127 .. 127, and what the gate must refuse has no code.
2. The build check of the sweep: csrc/spmv_sym.hip cross-compiled for gfx950 with the resource-usage remarks on.  k_spmv_symp<0, 2, 1> (two bands, coded
   diagonal: the 512^3 headline) must use no scratch and no more LDS than the stored form's 41.2 KB, so that three one-wave workgroups stay resident per CU
   (3 x 41 200 B of the CU's 160 KB; one wave per SIMD at up to 512 registers per lane).  Recorded when this test was written: 256 VGPRs + 138 AGPRs
   (k_spmv_symp<0, 2, 0>: 256 + 144), scratch 0, LDS 41 200 B as the stored form."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metafem.jl_amd", "csrc")
LDS_STORED_B2 = 41200   # bytes per workgroup of k_spmv_symp<0, 2, 0>: 3 x (8 + 2) lines of 36 doubles of x + 4068 + 2 table doubles
LDS_PER_CU = 160 * 1024


def test_host_check_symp_code(tmp_path):
    exe = str(tmp_path / "host_check_symp_code")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tools", "host_check_symp_code.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("OK")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_coded_sweep_keeps_three_workgroups_per_cu(tmp_path):
    hipcc = _hipcc()
    assert hipcc, "hipcc is needed to build the library at all"
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          "-I", os.path.join(ROOT, "include"), "-c", os.path.join(CSRC, "spmv_sym.hip"), "-o", str(tmp_path / "spmv_sym.dev.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    usage = {}
    name = None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    sweeps = {k: v for k, v in usage.items() if k.startswith("_Z11k_spmv_sympILi0E")}
    coded = [v for k, v in sweeps.items() if "ILi0ELi2ELi1EE" in k]
    stored = [v for k, v in sweeps.items() if "ILi0ELi2ELi0EE" in k]
    assert len(coded) == 1 and len(stored) == 1, sorted(sweeps)
    c, s = coded[0], stored[0]
    print(f"\nk_spmv_symp<0, 2, 1>: {c}\nk_spmv_symp<0, 2, 0>: {s}")
    assert c["ScratchSize"] == 0
    assert s["LDS Size"] == LDS_STORED_B2
    assert c["LDS Size"] <= LDS_STORED_B2
    assert 3 * c["LDS Size"] <= LDS_PER_CU
    assert c["VGPRs"] + c.get("AGPRs", 0) <= 512   # one wave per SIMD: four one-wave workgroups' worth of registers per CU, LDS admits three
