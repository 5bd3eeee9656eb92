"""CPU: the host side of the matrix-free hex-8 brick operator.  tools/host_check_brick_operator.cpp walks csrc/brick_operator_decide.h for lattices
from 1^3 to 1025^3 (every control point owned exactly once, the partial sums within MFEM_MAX_PARTIALS, the kernel per Gauss rule, the face kernel's
grid), compiled plain and as the same stand-alone program under the address and undefined-behaviour sanitizers; every new entry point is declared
in the header, bound in _lib.py and bound in julia/MI355X.jl; the refusal rule of ThermalDomain(matrix_free=True) answers without a device."""
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mfem_brick_operator_create", "mfem_brick_operator_set_params", "mfem_brick_operator_destroy", "mfem_brick_operator_apply",
                "mfem_brick_operator_diagonal"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_operator(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_operator")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_operator.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")


def test_the_cap_is_the_solver_cap():
    common = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "common.h")).read()
    decide = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_decide.h")).read()
    cap = int(re.search(r"#define MFEM_MAX_PARTIALS (\d+)", common).group(1))
    assert int(re.search(r"#define BOP_MAX_PARTIALS (\d+)", decide).group(1)) == cap == 4096


def test_entry_points_are_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    dbg = open(os.path.join(ROOT, "include", "metafem_mi355x_debug.h")).read()
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"\bint64_t\s+mfem_debug_brick_operator_count\s*\(\s*void\s*\)", dbg)
    for name in ENTRY_POINTS + ["mfem_debug_brick_operator_count"]:
        assert f'"{name}":' in lib_py, name
        assert f"(:{name}, lib)" in jl, name
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 7 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver


def test_ctypes_rows_resolve(mf):
    from metafem_jl_amd import _lib

    for name in ENTRY_POINTS + ["mfem_debug_brick_operator_count"]:
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.mfem_brick_operator_destroy(0) == 0  # (host only: no handle, nothing to do)
    assert _lib.lib.mfem_debug_brick_operator_count() >= 0


def test_refused_bricks_have_a_reason(mf):
    """The rule ThermalDomain(matrix_free=True) asks before it builds anything: the library's own (bop_refusal), on the host."""
    brick = lambda order, slab, m0: types.SimpleNamespace(itp_order=order, slab=slab, m=(m0, 5, 5))
    assert mf.brick_operator_refusal(brick(1, (0, 9), 9)) is None
    assert "hex-27" in mf.brick_operator_refusal(brick(2, (0, 9), 9))
    assert "slab" in mf.brick_operator_refusal(brick(1, (2, 9), 9))
    assert "slab" in mf.brick_operator_refusal(brick(1, (0, 8), 9))
    decide = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_decide.h")).read()
    for b in (brick(2, (0, 9), 9), brick(1, (2, 9), 9)):  # the same words as the library's message
        assert '"' + mf.brick_operator_refusal(b) + '"' in decide
