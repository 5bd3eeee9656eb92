"""CPU: the host side of the matrix-free hex-27 brick operator.  tools/host_check_brick_operator_hex27.cpp walks csrc/brick_operator_hex27_decide.h
for lattices from 1^3 to 513^3 elements (every control point owned exactly once, every adjacent element integrated by the owner, the partial sums
within MFEM_MAX_PARTIALS, the LDS block within the declared limit, the redundancy R) and compares the diagonal formula, evaluated on the CPU, with
element matrices built from unit vectors; compiled plain and as the same stand-alone program under the address and undefined-behaviour sanitizers.
The new entry point is declared in the header, bound in _lib.py and bound in julia/MI355X.jl; the refusal forecast answers without a device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mfem_brick_operator_create_hex27"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_operator_hex27(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_operator_hex27")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_operator_hex27.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    R = float(re.search(r"R\(128 x 128 x 128 elements\) = ([0-9.]+)", out.stdout).group(1))
    assert 1.0 < R <= 1.3


def test_entry_point_is_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert f'"{name}":' in lib_py, name
        assert f"(:{name}, lib)" in jl, name
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 9 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver


def test_ctypes_rows_resolve(mf):
    from metafem_jl_amd import _lib

    for name in ENTRY_POINTS:
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.mfem_abi_version() >= 9
    assert _lib.lib.mfem_brick_operator_create_hex27(None, None, None, None) == -1  # (host only: no out pointer -> MFEM_ERR_INVALID)


def test_the_python_interface_is_there(mf):
    assert issubclass(mf.Hex27BrickOperator, mf.BrickOperator) and isinstance(mf.Hex27BrickOperator, type)
    assert mf.Hex27BrickOperator in mf._OPERATORS
    assert callable(mf.Brick.thermal_operator_hex27) and callable(mf.brick_operator_hex27_refusal)
    assert "Hex27BrickOperator" in mf.__all__ and "brick_operator_hex27_refusal" in mf.__all__


def test_refusal_rule_on_stand_in_bricks(mf):
    """The rule ThermalDomain(matrix_free="any") asks before it builds anything: the library's own (bop27_refusal), on the host."""
    from types import SimpleNamespace as brick

    def b(order, slab, m0):
        return brick(itp_order=order, slab=slab, m=(m0, 5, 5))

    assert mf.brick_operator_hex27_refusal(b(2, (0, 9), 9)) is None
    assert "hex-8" in mf.brick_operator_hex27_refusal(b(1, (0, 9), 9))
    assert "slab" in mf.brick_operator_hex27_refusal(b(2, (2, 9), 9))
    assert "slab" in mf.brick_operator_hex27_refusal(b(2, (0, 8), 9))
    decide = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_hex27_decide.h")).read()
    for s in (b(1, (0, 9), 9), b(2, (2, 9), 9)):
        assert '"' + mf.brick_operator_hex27_refusal(s) + '"' in decide
    # the hex-8 forecast is unchanged: it keeps refusing an order-2 brick
    assert "hex-27" in mf.brick_operator_refusal(b(2, (0, 9), 9))
