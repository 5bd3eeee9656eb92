"""CPU: the host side of the geometric multigrid preconditioner on hex-8 elasticity bricks (mfem_brick_multigrid_create_elasticity).
tools/host_check_brick_multigrid_elasticity.cpp walks the field-aware functions of csrc/brick_multigrid_decide.h (the bytes of a 3-field hierarchy,
the field offsets and the padding, the stream bytes, the solve gate's truth table), compiled plain and as the same stand-alone program under the
address and undefined-behaviour sanitizers; its digest of every plan up to 32^3 and its lines for 128^3, 256^3 and 512^3 are compared with a Python
restatement; header, ctypes and Julia agree on the new name and the ABI constant, and the built library exports it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mfem_brick_multigrid_create_elasticity"


def _plan(n, max_levels=12):
    levels = [tuple(n)]
    while len(levels) < max_levels and all(v % 2 == 0 and v // 2 >= 2 for v in levels[-1]):
        levels.append(tuple(v // 2 for v in levels[-1]))
    return levels


def _bytes(levels, fields=3):
    """info.bytes of a hierarchy with `fields` field-major fields, in closed form: 16 bytes of flags; per level 3 (level 0) or 5 vectors of
    fields x points doubles, the VECTOR padded to 32 doubles; per coarse level its three coordinate arrays and the lattice tables of its brick"""
    total = 16
    for l, ne in enumerate(levels):
        pts = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
        total += (5 if l else 3) * ((fields * pts + 31) // 32 * 32) * 8
        if l:
            total += 3 * pts * 8 + sum(16 * (e + 1) + 8 for e in ne)
    return total


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_multigrid_elasticity(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_multigrid_elasticity")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_multigrid_elasticity.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    if flags != ["-O2"]:
        return
    count, digest = 0, 0
    for nx in range(1, 33):
        for ny in range(1, 33):
            for nz in range(1, 33):
                lv = _plan((nx, ny, nz))
                digest = (digest * 1000003 + len(lv) * 1315423911 + _bytes(lv)) & 0xFFFFFFFFFFFFFFFF
                count += 1
    m = re.search(r"^PLANS3 (\d+) (\d+)$", out.stdout, flags=re.M)
    assert (int(m.group(1)), int(m.group(2))) == (count, digest)
    lines = [[int(v) for v in line.split()] for line in re.findall(r"^PLAN3 (.*)$", out.stdout, flags=re.M)]
    assert [f[0] for f in lines] == [128, 256, 512]
    for size, nlev, nbytes in lines:
        lv = _plan((size,) * 3)
        assert nlev == len(lv) and nbytes == _bytes(lv), size


def test_abi_constants():
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    dec = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_multigrid_decide.h")).read()
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 11 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver
    assert re.search(r"#define MG_ELASTICITY_FIELDS 3\b", dec)
    assert re.search(r"MFEM_PRECOND_MULTIGRID = 3\b", hdr)


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
    assert _lib.lib.mfem_abi_version() >= 11
    out = C.c_uint64(5)
    assert fn(None, 0, None, C.byref(out)) == -1 and out.value == 0  # (host only: a null context is MFEM_ERR_INVALID, nothing is created)
    assert mf.ElasticityBrickOperator._multigrid_create == NAME and not hasattr(mf.Hex27BrickOperator, "_multigrid_create")
    # the structs kept their layout
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "metafem_mi355x.h"\nint main(void) { printf("%zu %zu\\n", sizeof(mfem_multigrid_options), '
                   'sizeof(mfem_multigrid_info)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe], text=True).split()] == [32, 376]
    assert (C.sizeof(_lib.MultigridOptions), C.sizeof(_lib.MultigridInfo)) == (32, 376)
