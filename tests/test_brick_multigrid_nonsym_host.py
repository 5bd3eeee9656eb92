"""CPU: the host side of the nonsymmetric thermal hierarchy (mfem_brick_multigrid_create_nonsymmetric) and of gmres! with the V-cycle.
tools/host_check_brick_multigrid_nonsym.cpp walks the new functions of csrc/brick_multigrid_decide.h -- the gate mg_solve_refusal_nonsym row by
row against mg_solve_refusal_hex27, which setups refuse a Nitsche term, and the product formula of a pass against a host model of the pass's loop --
compiled plain and as the same stand-alone program under the address and undefined-behaviour sanitizers; its gate rows are compared with a Python
restatement; header, ctypes and Julia agree on the new names and the ABI constant, and the built library exports them."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mfem_brick_multigrid_create_nonsymmetric"
FLAG = "mfem_brick_multigrid_nonsymmetric"
CG, GMRES, LEFT_NONE = 0, 4, 0  # MFEM_SOLVER_CG, MFEM_SOLVER_GMRES, MFEM_LEFT_NONE


def _admitted(brick, kind, attached, nonsym, method, left, comm, nitsche):
    """the gate in words: kind 1 hex-8 thermal, 2 hex-8 elasticity, 3 hex-27 thermal.  cg! as before this hierarchy; gmres! on a hex-8 thermal
    operator with a nonsymmetric hierarchy attached, the Nitsche term on or off; never with a left preconditioner or a communicator"""
    if not brick or left != LEFT_NONE or comm:
        return False
    if method == CG:
        return not nitsche and (kind == 1 or (kind in (2, 3) and attached))
    if method == GMRES:
        return kind == 1 and attached and nonsym
    return False


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_multigrid_nonsym(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_multigrid_nonsym")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_multigrid_nonsym.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    if flags != ["-O2"]:
        return
    rows = [tuple(int(v) for v in m.group(1).split()) for m in re.finditer(r"^GATE (.*)$", out.stdout, flags=re.M)]
    assert len(rows) == 320 and len(set(r[:8] for r in rows)) == 320
    for r in rows:
        assert r[8] == int(_admitted(*r[:8])), r
    new = [r for r in rows if r[8] and r[4] == GMRES]
    assert sorted(new) == [(1, 1, 1, 1, GMRES, LEFT_NONE, 0, 0, 1), (1, 1, 1, 1, GMRES, LEFT_NONE, 0, 1, 1)]  # the new rows, Nitsche off and on


def test_the_existing_gate_functions_keep_their_text():
    """mg_solve_refusal, _fields and _hex27 are byte for byte what they were: the new gate wraps them"""
    dec = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_multigrid_decide.h")).read()
    assert dec.count("static inline const char* mg_solve_refusal_nonsym(") == 1
    body = dec[dec.index("static inline const char* mg_solve_refusal_nonsym("):]
    assert "return mg_solve_refusal_hex27(brick_operator, thermal_hex8, elasticity_hex8, thermal_hex27, hierarchy_attached, method, left_precond, has_comm, nitsche_on);" in body
    for words in ("the multigrid preconditioner needs MFEM_SOLVER_CG: the cycle is a symmetric operator, the other methods are not offered it",
                  "the multigrid preconditioner needs a symmetric K: a Nitsche (fixed_faces) term is active",
                  "mfem_brick_multigrid_create_hex27 (no default hierarchy is made for hex-27)"):
        assert dec.count(words) == 1
    assert "mg_gmres_pass_products" in dec and dec.index("mg_pass_products") < dec.index("mg_gmres_pass_products")


def test_abi_constants():
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 13 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver


def test_entry_points_are_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*mfem_context ctx,\s*uint64_t op,\s*const mfem_multigrid_options\* opts,\s*uint64_t\* mg", hdr)
    assert re.search(r"\bint\s+" + FLAG + r"\s*\(\s*uint64_t mg\s*\)", hdr)
    for name in (NAME, FLAG):
        assert f'"{name}":' in lib_py
        assert f"(:{name}, lib)" in jl


def test_entry_points_resolve_in_the_built_library(mf, tmp_path):
    import inspect

    from metafem_jl_amd import _lib

    fn = getattr(_lib.lib, NAME)
    assert fn.argtypes == _lib.SIGNATURES[NAME][1] == _lib.SIGNATURES["mfem_brick_multigrid_create"][1]
    assert _lib.lib.mfem_abi_version() >= 13
    out = C.c_uint64(5)
    assert fn(None, 0, None, C.byref(out)) == -1 and out.value == 0  # (host only: a null context is MFEM_ERR_INVALID, nothing is created)
    assert getattr(_lib.lib, FLAG)(0) == -1
    assert "nonsymmetric" in inspect.signature(mf.BrickOperator.multigrid).parameters
    assert inspect.signature(mf.BrickOperator.multigrid).parameters["nonsymmetric"].default is False
    assert not hasattr(mf.BrickOperator, "_multigrid_create")
    assert C.sizeof(_lib.MultigridInfo) == 376  # (the flag has its own entry point: the struct keeps its layout)
