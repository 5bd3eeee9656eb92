"""CPU check of the host decisions of the direct row assembly (csrc/mesh_direct_decide.h: batch cuts, task lists, refusals, the LDS block of a
workgroup), compiled with g++ -- plain, and once more as the same stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfem_mesh_direct_plan_create", "mfem_mesh_direct_plan_destroy", "mfem_mesh_direct_plan_stats", "mfem_mesh_assemble_elements_direct",
         "mfem_debug_mesh_direct_count", "mfem_debug_ws_bytes")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_host_check_mesh_direct(tmp_path, flags):
    exe = str(tmp_path / "host_check_mesh_direct")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_mesh_direct.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")


def test_every_direct_entry_point_is_bound_and_declared():
    """The entry points and the two debug additions stand in the headers, the ctypes signature table and the Julia binding."""
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read() + open(os.path.join(ROOT, "include", "metafem_mi355x_debug.h")).read()
    lib = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in NAMES:
        assert f" {name}(" in hdr, name
        assert f'"{name}"' in lib, name
        assert f"(:{name}, lib)" in jl, name
    assert '"mesh_direct_budget"' in hdr and '"mesh_direct_budget"' in open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "api.hip")).read()
