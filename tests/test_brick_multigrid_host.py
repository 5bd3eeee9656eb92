"""CPU: the host side of the geometric multigrid preconditioner on hex-8 thermal bricks.  tools/host_check_brick_multigrid.cpp walks
csrc/brick_multigrid_decide.h (the level plans, the transfer kernels' grids, the bytes, the products, the Chebyshev coefficients, the solve gate),
compiled plain and as the same stand-alone program under the address and undefined-behaviour sanitizers; its digest of every plan up to 64^3 and its
lines for 512^3, 768^3, 1000^3 and 1024^3 are compared with a Python restatement; header, ctypes and Julia agree on the new names and constants."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mfem_brick_multigrid_create", "mfem_brick_multigrid_setup", "mfem_brick_multigrid_apply", "mfem_brick_multigrid_info",
                "mfem_brick_multigrid_destroy"]
DECIDE = os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_multigrid_decide.h")


def _plan(n, max_levels=12):
    levels = [tuple(n)]
    while len(levels) < max_levels and all(v % 2 == 0 and v // 2 >= 2 for v in levels[-1]):
        levels.append(tuple(v // 2 for v in levels[-1]))
    return levels


def _bytes(levels):
    """info.bytes in closed form: 16 bytes of flags; per level 3 (level 0) or 5 vectors padded to 32 doubles; per coarse level its three coordinate
    arrays and the lattice tables of its brick (16 bytes per lattice index and 8 more, per dimension)"""
    total = 16
    for l, ne in enumerate(levels):
        n = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
        total += (5 if l else 3) * ((n + 31) // 32 * 32) * 8
        if l:
            total += 3 * n * 8 + sum(16 * (e + 1) + 8 for e in ne)
    return total


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_multigrid(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_multigrid")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_brick_multigrid.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    if flags != ["-O2"]:
        return
    # the Python restatement: every plan up to 64^3 through the digest, the large bricks line by line
    count, digest = 0, 0
    for nx in range(1, 65):
        for ny in range(1, 65):
            for nz in range(1, 65):
                lv = _plan((nx, ny, nz))
                digest = (digest * 1000003 + len(lv) * 1315423911 + _bytes(lv)) & 0xFFFFFFFFFFFFFFFF
                count += 1
    m = re.search(r"^PLANS (\d+) (\d+)$", out.stdout, flags=re.M)
    assert (int(m.group(1)), int(m.group(2))) == (count, digest)
    seen = 0
    for line in re.findall(r"^PLAN (.*)$", out.stdout, flags=re.M):
        f = [int(v) for v in line.split()]
        lv = _plan((f[0],) * 3)
        assert f[1] == len(lv) and f[2] == _bytes(lv) and f[3:] == [e[0] for e in lv], line
        seen += 1
    assert seen == 4
    assert [len(_plan((s,) * 3)) for s in (512, 768, 1000, 1024)] == [9, 9, 4, 10]


def test_python_plan_is_the_librarys(mf):
    for n in [(16, 24, 12), (16, 16, 16), (32, 32, 32), (8, 8, 8), (6, 10, 14), (9, 14, 15), (4, 4, 4), (2, 2, 2), (1024, 1024, 1024)]:
        assert mf.multigrid_plan(n) == _plan(n)
    assert mf.multigrid_plan((64, 64, 64), 3) == _plan((64, 64, 64), 3)


def test_constants_agree_between_header_decide_and_julia():
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    dec = open(DECIDE).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    cap = int(re.search(r"#define MFEM_MG_MAX_LEVELS (\d+)", hdr).group(1))
    assert cap == int(re.search(r"#define MG_MAX_LEVELS (\d+)", dec).group(1)) == 12
    assert int(re.search(r"const MG_MAX_LEVELS = (\d+)", jl).group(1)) == cap
    assert re.search(r"MFEM_PRECOND_MULTIGRID = 3\b", hdr) and re.search(r"const PRECOND_MULTIGRID = Int32\(3\)", jl)
    assert re.search(r"int32_t nx\[12\];", hdr) and "NTuple{12, Int32}" in jl
    for name, want in (("MG_DEFAULT_SMOOTHER_DEGREE", "2"), ("MG_DEFAULT_COARSE_DEGREE", "32"), ("MG_DEFAULT_SMOOTHING_RANGE", "4.0"),
                       ("MG_DEFAULT_COARSE_RANGE", "300.0"), ("MG_DEFAULT_EIG_STEPS", "20"), ("MG_MIN_EIG_STEPS", "10"), ("MG_EIG_SAFETY", "1.1")):
        assert re.search(r"#define " + name + r" " + re.escape(want) + r"\b", dec), name
    ver = int(re.search(r"#define MFEM_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 10 and int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == ver


def test_entry_points_are_declared_and_bound_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read(), flags=re.S)
    lib_py = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert f'"{name}":' in lib_py, name
        assert f"(:{name}, lib)" in jl, name
    for mirror in ("mfem_multigrid_options", "mfem_multigrid_info"):
        assert f"# == {mirror}" in jl, mirror


def test_ctypes_rows_resolve_and_structs_have_the_c_layout(mf, tmp_path):
    import ctypes as C

    from metafem_jl_amd import _lib

    for name in ENTRY_POINTS + ["mfem_debug_brick_multigrid_transfer", "mfem_debug_brick_multigrid_coords"]:
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.mfem_brick_multigrid_destroy(0) == 0  # (host only: no handle, nothing to do)
    assert _lib.lib.mfem_abi_version() >= 10 and mf.Pr_Multigrid_ == 3 and _lib.MG_MAX_LEVELS == 12
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "metafem_mi355x.h"\nint main(void) { printf("%zu %zu\\n", sizeof(mfem_multigrid_options), '
                   'sizeof(mfem_multigrid_info)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    so, si = (int(v) for v in subprocess.check_output([exe], text=True).split())
    assert (C.sizeof(_lib.MultigridOptions), C.sizeof(_lib.MultigridInfo)) == (so, si)
