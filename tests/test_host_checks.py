"""CPU checks of host/device headers of the product, compiled with g++ (no GPU): the sum-factorised hex-8 element routines against the
stored-table form (reference semantics: 4_Update_Integrator.jl:2-33,90-154; 06_FEM_Kernel.jl:28-45,65-79) and the LDS mirror-table /
edge-block bookkeeping of the wave-private symmetric sweep, replayed on small lattices; the step / slot tables of the symmetric lattice-tile layouts
(every stencil pair listed exactly once: a product through the tables against the entry-by-entry product); the host decisions of the solve
driver, of the CSR SpMV (which kernel, which tile, which inspections) of the sliced solver layout (csrc/sell_decide.h: which form, which
keys, which padding, which instantiation) and of the symmetric lattice tiles (csrc/lat_decide.h: knob words, eligibility, the lattice of row 0,
geometry and sizes, the split of a slab's launch, the gather grid, the symmetry gate), branch by branch; the host decisions of the hex-27
thermal assembly (csrc/hex27_decide.h: knob word, path choice, workspace, ring, grids, face schedule, LDS size) against the expressions of the
driver they were cut out of, their own properties, and the macros the kernel lays its LDS block out with; the host decisions of the fused
hex-8 assembly (csrc/hex8_decide.h: both knob words, kernel choice and flag words, sweep segments and grids, face predicates, block-to-tile
maps, boundary enumeration, reference tables) in the same three parts."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["host_check_hex8", "host_check_symp", "host_check_lat", "host_check_solve", "host_check_csr", "host_check_sell",
                                  "host_check_lat_decide", "host_check_hex27", "host_check_hex8_decide"])
def test_host_check(name, tmp_path):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("OK")
