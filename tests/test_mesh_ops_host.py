"""CPU check of the host decisions of the table-free mesh operators (csrc/mesh_ops_decide.h: LDS block sizes, the 64 KB refusals, waves per
workgroup, table slots of the gradient operator), compiled with g++ -- and of the Python mirror's one host-side refusal."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_mesh_ops(tmp_path):
    exe = str(tmp_path / "host_check_mesh_ops")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_mesh_ops.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("OK")


def test_every_table_free_entry_point_is_bound_and_declared():
    """The seven entry points and the counter stand in the header, the ctypes signature table and the Julia binding."""
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read() + open(os.path.join(ROOT, "include", "metafem_mi355x_debug.h")).read()
    lib = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in ("mfem_mesh_var_elements", "mfem_mesh_var_facets", "mfem_mesh_res_elements", "mfem_mesh_res_facets", "mfem_mesh_kval_elements",
                 "mfem_mesh_kval_elements_rows", "mfem_mesh_kval_facets", "mfem_debug_mesh_ops_count"):
        assert f" {name}(" in hdr, name
        assert f'"{name}"' in lib, name
        assert f"(:{name}, lib)" in jl, name
