"""CPU: the host side of the matrix-free hex-27 elasticity brick operator.  tools/host_check_brick_operator_elasticity_hex27.cpp walks
csrc/brick_operator_elasticity_hex27_decide.h (every control point owned exactly once, every adjacent element integrated by the owner, the LDS
offsets in order and within a CU's 160 KB, the waves per rule, the redundancy R) and compares the diagonal formula with element matrices built from unit
vectors; compiled plain and as the same stand-alone program under the address and undefined-behaviour sanitizers.  The two new entry points are
declared in the header, bound in _lib.py and in julia/MI355X.jl; the refusal forecast, the rule predicate included, answers without a device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mfem_brick_operator_create_elasticity_hex27", "mfem_brick_operator_residual_elasticity"]
DECIDE = os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_elasticity_hex27_decide.h")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    def run(flags):
        exe = str(tmp_path_factory.mktemp("e27") / "host_check_brick_operator_elasticity_hex27")
        subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                        os.path.join(ROOT, "tools", "host_check_brick_operator_elasticity_hex27.cpp"), "-o", exe], check=True)
        return subprocess.run([exe], capture_output=True, text=True)

    return run


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_operator_elasticity_hex27(flags, host_check):
    out = host_check(flags)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    R = float(re.search(r"R\(128 x 128 x 128 elements\) = ([0-9.]+)", out.stdout).group(1))
    assert abs(R - 1.277) < 5e-4  # as stated (the thermal operator's work items)
    waves = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"LDS\(ng = (\d)\): (\d+) waves, (\d+) bytes", out.stdout)}
    assert sorted(waves) == [1, 2, 3, 4]
    for ng, (w, nbytes) in waves.items():
        assert ng > 3 or w == 12  # the rules with 1 to 3 points run the full workgroup
        assert w == 0 or (5 <= w <= 12 and nbytes + 128 <= 160 * 1024)


def test_entry_points_are_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert f'"{name}":' in lib_py, name
        assert f"(:{name}, lib)" in jl, name
    assert re.search(r"int\s+mfem_brick_operator_create_elasticity_hex27\s*\(\s*mfem_context\s+ctx,\s*mfem_brick\s+m,\s*const\s+mfem_elasticity_params\s*\*\s*p,\s*uint64_t\s*\*\s*op", hdr)
    assert re.search(r"int\s+mfem_brick_operator_residual_elasticity\s*\(\s*mfem_context\s+ctx,\s*uint64_t\s+op,\s*const\s+double\s*\*\s*x_star,\s*double\s*\*\s*residue\s*\)", hdr)
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 14 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver
    tag = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator.h")).read()
    assert re.search(r"BOP_PHYSICS_ELASTICITY_HEX27 = 4\b", tag)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in integration, name


def test_ctypes_rows_resolve(mf):
    import ctypes as C

    from metafem_jl_amd import _lib

    for name in ENTRY_POINTS:
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES[ENTRY_POINTS[0]][1][2] == C.POINTER(_lib.ElasticityParams)
    assert _lib.lib.mfem_abi_version() >= 14
    assert _lib.lib.mfem_brick_operator_create_elasticity_hex27(None, None, None, None) == -1  # (host only: no out pointer -> MFEM_ERR_INVALID)
    assert _lib.lib.mfem_brick_operator_residual_elasticity(None, 0, None, None) == -1


def test_the_python_interface_is_there(mf):
    assert issubclass(mf.Hex27ElasticityBrickOperator, mf.BrickOperator) and mf.Hex27ElasticityBrickOperator in mf._OPERATORS
    assert callable(mf.Brick.elasticity_operator_hex27) and callable(mf.brick_operator_elasticity_hex27_refusal)
    assert callable(mf.Hex27ElasticityBrickOperator.residual) and callable(mf.Hex27ElasticityBrickOperator.set_params)
    assert "Hex27ElasticityBrickOperator" in mf.__all__ and "brick_operator_elasticity_hex27_refusal" in mf.__all__


def test_refusal_forecast_on_stand_in_bricks(mf):
    """The rule ElasticityDomain(matrix_free="any") asks before it builds anything: the library's own (bop_e27_refusal), on the host; its LDS
    arithmetic restates the header's, and the host check prints the header's values."""
    from types import SimpleNamespace as brick

    def b(order, slab, m0, itg=5):
        return brick(itp_order=order, slab=slab, m=(m0, 5, 5), itg_order=itg)

    for itg in range(1, 6):
        assert mf.brick_operator_elasticity_hex27_refusal(b(2, (0, 9), 9, itg)) is None  # the rules with 1 to 3 points are served
    assert "mfem_brick_operator_create_elasticity" in mf.brick_operator_elasticity_hex27_refusal(b(1, (0, 9), 9))
    assert "slab" in mf.brick_operator_elasticity_hex27_refusal(b(2, (2, 9), 9))
    assert "slab" in mf.brick_operator_elasticity_hex27_refusal(b(2, (0, 8), 9))
    decide = open(DECIDE).read()
    for s in (b(1, (0, 9), 9), b(2, (2, 9), 9)):
        assert '"' + mf.brick_operator_elasticity_hex27_refusal(s) + '"' in decide
    assert '"the 4-point Gauss rule (itg_order 6 to 7): the volume kernel\'s per-workgroup LDS block exceeds the 160 KB of a CU"' in decide
    # the 4-point rule follows the predicate: served exactly when some admitted number of waves fits
    served = mf.brick_operator_elasticity_hex27_waves(4) > 0
    for itg in (6, 7):
        why = mf.brick_operator_elasticity_hex27_refusal(b(2, (0, 9), 9, itg))
        assert (why is None) == served and (served or "4-point Gauss rule" in why)
    # the constants behind the forecast are the header's
    for name, key in (("E27_NI", "NI"), ("E27_NF", "NF"), ("E27_TE", "TE"), ("E27_WAVES_MAX", "WAVES_MAX"), ("E27_WAVES_MIN", "WAVES_MIN"),
                      ("E27_LDS_STATIC", "LDS_STATIC")):
        assert int(re.search(r"#define " + name + r"\s+(\d+)", decide).group(1)) == mf._e27_constants()[key], name
    # a rule the tables do not hold is named as such, with the library's words
    why = mf.brick_operator_elasticity_hex27_refusal(b(2, (0, 9), 9, 9))
    assert "outside 1 to 4 points" in why and '"' + why + '"' in decide
    # the existing forecasts are unchanged
    assert "hex-27" in mf.brick_operator_refusal(b(2, (0, 9), 9))
    assert mf.brick_operator_hex27_refusal(b(2, (0, 9), 9)) is None


def test_forecast_bytes_equal_the_headers(mf, host_check):
    out = host_check(["-O2"]).stdout
    for m in re.finditer(r"LDS\(ng = (\d)\): (\d+) waves, (\d+) bytes \(per wave \d+, shared \d+\); 8 waves: (\d+), 12 waves: (\d+)", out):
        ng, w, nbytes, b8, b12 = (int(v) for v in m.groups())
        assert mf.brick_operator_elasticity_hex27_waves(ng) == w
        assert mf.brick_operator_elasticity_hex27_lds_bytes(ng, 8) == b8 and mf.brick_operator_elasticity_hex27_lds_bytes(ng, 12) == b12
        assert w == 0 or mf.brick_operator_elasticity_hex27_lds_bytes(ng, w) == nbytes
