"""CPU: the host side of the geometric multigrid preconditioner on hex-27 thermal bricks (mfem_brick_multigrid_create_hex27).
tools/host_check_brick_multigrid_hex27.cpp walks the new functions of csrc/brick_multigrid_decide.h -- the level plan (p-coarsening once, then the
halving rule), the level-0 lattice and the bytes, every refusal string including the rule with fewer than 3 Gauss points per direction, and that
mg_plan, mg_solve_refusal and mg_solve_refusal_fields answer as before -- compiled plain and as the same stand-alone program under the address and
undefined-behaviour sanitizers; its digest of every plan up to 20^3 and its line for 128^3 are compared with a Python restatement; header, ctypes
and Julia agree on the new name and the ABI constant, and the built library exports it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mfem_brick_multigrid_create_hex27"


def _plan8(n, max_levels=12):
    levels = [tuple(n)]
    while len(levels) < max_levels and all(v % 2 == 0 and v // 2 >= 2 for v in levels[-1]):
        levels.append(tuple(v // 2 for v in levels[-1]))
    return levels


def _plan27(n, max_levels=12):
    return [tuple(n)] + (_plan8(n, max_levels - 1) if max_levels >= 2 else [])


def _bytes(levels):
    """info.bytes of a hex-27 hierarchy in closed form: 16 bytes of flags; level 0 three vectors of (2 nx + 1)(2 ny + 1)(2 nz + 1) doubles, every
    hex-8 level five of (nx + 1)(ny + 1)(nz + 1), each padded to 32 doubles, its three coordinate arrays and the lattice tables of its brick"""
    total = 16
    for l, ne in enumerate(levels):
        pts = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1) if l else (2 * ne[0] + 1) * (2 * ne[1] + 1) * (2 * ne[2] + 1)
        total += (5 if l else 3) * ((pts + 31) // 32 * 32) * 8
        if l:
            total += 3 * pts * 8 + sum(16 * (e + 1) + 8 for e in ne)
    return total


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_multigrid_hex27(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_multigrid_hex27")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_multigrid_hex27.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    if flags != ["-O2"]:
        return
    count, digest = 0, 0
    for nx in range(1, 21):
        for ny in range(1, 21):
            for nz in range(1, 21):
                lv = _plan27((nx, ny, nz))
                digest = (digest * 1000003 + len(lv) * 1315423911 + _bytes(lv)) & 0xFFFFFFFFFFFFFFFF
                count += 1
    m = re.search(r"^PLANS27 (\d+) (\d+)$", out.stdout, flags=re.M)
    assert (int(m.group(1)), int(m.group(2))) == (count, digest)
    size, nlev, nbytes = [int(v) for v in re.search(r"^PLAN27 (.*)$", out.stdout, flags=re.M).group(1).split()]
    lv = _plan27((size,) * 3)
    assert size == 128 and nlev == len(lv) == 8 and nbytes == _bytes(lv)


def test_python_plan_restates_the_header(mf):
    for n in [(1, 1, 1), (2, 1, 3), (8, 12, 6), (16, 16, 16), (3, 5, 7)]:
        for ml in (1, 2, 3, 12):
            assert mf.multigrid_plan_hex27(n, ml) == _plan27(n, ml), (n, ml)
    assert mf.multigrid_plan_hex27((8, 12, 6)) == [(8, 12, 6), (8, 12, 6), (4, 6, 3)]
    assert mf.multigrid_plan_hex27((16, 16, 16), 1) == [(16, 16, 16)]
    assert mf.multigrid_plan((16, 24, 12)) == [(16, 24, 12), (8, 12, 6), (4, 6, 3)]  # (the hex-8 plan answers as before)


def test_abi_constants():
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    dec = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_multigrid_decide.h")).read()
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 12 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver
    assert re.search(r"#define MG_HEX27_MIN_NG 3\b", dec)
    assert re.search(r"MFEM_PRECOND_MULTIGRID = 3\b", hdr)
    assert "nx[0] == nx[1]" in hdr  # (the header says what mfem_multigrid_info reports on such a hierarchy)


def test_entry_point_is_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*mfem_context ctx,\s*uint64_t op,\s*const mfem_multigrid_options\* opts,\s*uint64_t\* mg", hdr)
    assert f'"{NAME}":' in lib_py
    assert f"(:{NAME}, lib)" in jl


def test_entry_point_resolves_in_the_built_library(mf, tmp_path):
    import ctypes as C

    from metafem_jl_amd import _lib

    fn = getattr(_lib.lib, NAME)
    assert fn.argtypes == _lib.SIGNATURES[NAME][1] == _lib.SIGNATURES["mfem_brick_multigrid_create"][1]
    assert _lib.lib.mfem_abi_version() >= 12
    out = C.c_uint64(5)
    assert fn(None, 0, None, C.byref(out)) == -1 and out.value == 0  # (host only: a null context is MFEM_ERR_INVALID, nothing is created)
    import inspect

    # (the name is set on each operator in __init__, not on the class: the GPU file checks it on an operator)
    assert f'self._multigrid_create = "{NAME}"' in inspect.getsource(mf.Hex27BrickOperator.__init__)
    assert mf.ElasticityBrickOperator._multigrid_create == "mfem_brick_multigrid_create_elasticity"
    assert not hasattr(mf.BrickOperator, "_multigrid_create")
    # the structs kept their layout
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "metafem_mi355x.h"\nint main(void) { printf("%zu %zu\\n", sizeof(mfem_multigrid_options), '
                   'sizeof(mfem_multigrid_info)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe], text=True).split()] == [32, 376]
    assert (C.sizeof(_lib.MultigridOptions), C.sizeof(_lib.MultigridInfo)) == (32, 376)
