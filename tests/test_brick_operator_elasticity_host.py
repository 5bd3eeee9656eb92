"""CPU: the host side of the matrix-free hex-8 brick operator on elasticity.  tools/host_check_brick_operator_elasticity.cpp walks the new decisions
of csrc/brick_operator_decide.h for lattices from 1^3 to 1025^3 (every control point owned exactly once, the partial sums within
MFEM_MAX_PARTIALS, the kernel per Gauss rule) and compares the diagonal formula, evaluated on the CPU, with the diagonal of element matrices built
from unit vectors through sf_elasticity_fe; compiled plain and as the same stand-alone program under the address and undefined-behaviour
sanitizers.  Every new entry point is declared in the header, bound in _lib.py and bound in julia/MI355X.jl."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mfem_brick_operator_create_elasticity", "mfem_brick_operator_set_elasticity_params"]
DEBUG_ENTRY_POINTS = ["mfem_debug_brick_operator_apply_dot"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_operator_elasticity(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_operator_elasticity")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_operator_elasticity.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")


def test_entry_points_are_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x_debug.h")).read(), flags=re.S)
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert f'"{name}":' in lib_py, name
        assert f"(:{name}, lib)" in jl, name
    for name in DEBUG_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", dbg), name
        assert f'"{name}":' in lib_py, name
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 8 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver


def test_ctypes_rows_resolve(mf):
    from metafem_jl_amd import _lib

    for name in ENTRY_POINTS + DEBUG_ENTRY_POINTS:
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.mfem_abi_version() >= 8
    assert _lib.lib.mfem_brick_operator_set_elasticity_params(0, None) == -1  # (host only: no handle -> MFEM_ERR_INVALID)


def test_the_python_interface_is_there(mf):
    assert issubclass(mf.ElasticityBrickOperator, mf.BrickOperator)
    assert callable(mf.Brick.elasticity_operator) and callable(mf.ElasticityDomain)
