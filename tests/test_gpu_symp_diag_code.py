"""The coded-diagonal form of the patch sweep's copy (csrc/spmv_symp.h; k_symp_fill<RP, true, true> writes it, k_spmv_symp<MODE, B, 1> reads it): the scaled
CG (cg_variant 4) binds S^-1 A S^-1, whose diagonal a_ii * (t_i * t_i), t_i = 1 / sqrt|a_ii|, is -1.0 up to a few roundings (the thermal K is negative
definite; +1.0 for a positive definite matrix) and travels as one signed byte per row, bits(v) - bits(unit), the unit +-1.0 with the sign of the first swept
row's diagonal.  The sweep rebuilds the same double, so EVERY comparison here is coded form against the stored form forced by bit 21 of the
"ell" knob in the same build, bit for bit: y, the partial sums of the fused dot product, x, the solver statistics.

Lattices = (planes, lines, points per line) = elements + 1; layout_min_rows = (0, 0); the band count forced by bits 24 / 25.

RIM: the lattices the issue lists -- lines of 31, 32, 33, 65 points; 3, 4, 5, 8, 9 lines; 3 and 7 planes.  The slot-major layout the sweep belongs to is planned
only where padding every row to 27 slots costs at most 10 % (ell_plan_columns) and the sweep needs four whole swept planes (symp_plan): none of these 40
lattices gets there (3 lines alone: 1 - 2 / 9 = 0.78), so on them the comparison holds between two runs of the per-row kernels and the test only pins that
the knob and the entry point leave those alone.  SWEPT therefore adds lattices on which the sweep does run (asserted), with the same rim features: lines of
31 / 32 / 33 / 34 / 65 points (an odd line length: a lone valid point in the last lane pair; 33, 65: a last patch column of one point), 9 lines (8 + 1: band 1
of the last patch row empty), 12 (a full band 0 and a full band 1 / three full four-line strips), 14 (8 + 4 + 2: a partly filled band), 17 (8 + 8 + 1),
4 .. 32 swept planes in one run and 190 swept planes cut into several runs.

Values: the assembled thermal matrix rescaled symmetrically as in test_scaled_cg_matches_the_jacobi_recurrence (T K T, t in [1, 30], t_r * t_c formed
first).  The host forms the same scaled diagonals (IEEE products in the fill's order) and asserts that at least three distinct codes occur and that one is
non-zero -- otherwise the test would prove nothing.

Tolerance of the one non-bitwise comparison (cg_variant 4 against 3): 1e-9 * max |x|, what test_scaled_cg_matches_the_jacobi_recurrence uses."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_COND, H, TENV = 0.6, 25.0, 293.15
B1, B2, STORED, CHECK_PASS = 1 << 24, 1 << 25, 1 << 21, 1 << 30

RIM = [(planes, points) for planes in (3, 7) for points in (31, 32, 33, 65)]
RIM_LINES = (3, 4, 5, 8, 9)
SWEPT = [(20, 17, 65), (40, 12, 34), (40, 17, 33), (40, 17, 31), (40, 16, 32), (40, 14, 33), (200, 9, 65)]


class Sys:
    pass


_CACHE = {}


def _system(mf, lat):
    """Brick, pattern, T K T, the host's 1 / sqrt|a_ii| and the codes of the scaled diagonals, vectors -- made once per lattice, never changed."""
    import torch

    if lat in _CACHE:
        return _CACHE[lat]
    S = Sys()
    S.lat = lat
    S.brick = mf.make_Brick((1.0, 0.7, 1.3), tuple(v - 1 for v in lat))
    S.A = S.brick.pattern(1)
    S.n = n = S.A.n
    assert n == lat[0] * lat[1] * lat[2]
    K = S.brick.assemble_thermal(S.A, K_COND, H, TENV, 0x3F)
    t = 1.0 + 29.0 * mf.FEM_rand(n, 3, 0)
    S.rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (S.A.rowptr[1:] - S.A.rowptr[:-1]).long())
    cols = S.A.colidx.long() - int(S.A.index_base)
    S.K = K * (t[S.rows] * t[cols])
    S.diag_idx = torch.nonzero(cols == S.rows).flatten()
    assert S.diag_idx.numel() == n
    S.diag_idx_h = S.diag_idx.cpu().numpy()
    S.ssym, S.codes = _scaling(S, S.K)
    S.x = mf.FEM_rand(n, 5, 0) - 0.5
    S.w = mf.FEM_rand(n, 6, 0) - 0.5
    S.y0 = mf.FEM_rand(n, 7, 0) - 0.5
    S.b = mf.FEM_rand(n, 11, 0) - 0.5
    _CACHE[lat] = S
    return S


def _scaling(S, K):
    """(1 / sqrt|a_ii| on the device, codes of a_ii * (t_i * t_i) on the host) for the values K"""
    import torch

    d = K[S.diag_idx].cpu().numpy()
    t = 1.0 / np.sqrt(np.abs(d))
    v = d * (t * t)
    planes, m1, m2 = S.lat
    PL = m1 * m2
    first = min(-(-(-(-(PL + m2 + 1) // 128) * 128) // PL) * PL, S.n - 1)   # the first swept row (first whole plane inside the regular 128-row blocks)
    unit = np.float64(-1.0 if d[first] < 0 else 1.0).view(np.int64)
    with np.errstate(over="ignore"):
        codes = v.view(np.int64) - unit   # (a value of the other sign: 2^63 away, wraps to a huge magnitude)
    return torch.tensor(t, device="cuda"), codes


def _no_code(codes):
    return (codes < -127) | (codes > 127)   # (not abs: the other sign's distance wraps to -2^63)


class _lift:
    def __enter__(self):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_layout_min_rows(0, 0)

    def __exit__(self, *exc):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_ell(1)
        _lib.lib.mfem_debug_set_cg_ring(0)
        _lib.lib.mfem_debug_set_graphs(1, 0)
        _lib.lib.mfem_debug_set_layout_min_rows(262144, 1000000)


def _sweep_planned(S):
    from metafem_jl_amd import _lib

    ent, sym = C.c_int64(), C.c_int32()
    _lib.check(_lib.lib.mfem_csr_solver_layout_entries(S.brick.ctx._h, S.A._h, C.byref(ent), C.byref(sym)))
    return sym.value == 2


def _layout_mode(S):
    from metafem_jl_amd import _lib

    mode = C.c_int32()
    _lib.check(_lib.lib.mfem_csr_solver_layout(S.brick.ctx._h, S.A._h, C.byref(mode), None, None, None))
    return mode.value


def _product(S, K, ssym, word, alpha, beta, dotw):
    """(form, bytes of y, bytes of the partial sums) of one product of the scaled layout under knob word `word`"""
    import torch
    from metafem_jl_amd import _lib

    _lib.check(_lib.lib.mfem_debug_set_ell(1 | word))
    y = S.y0.clone()
    part = np.zeros(4096, dtype=np.float64)
    npart, form = C.c_int32(0), C.c_int32(-7)
    _lib.check(_lib.lib.mfem_debug_spmv_scaled_layout(S.brick.ctx._h, S.A._h, K.data_ptr(), ssym.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta,
                                                      dotw.data_ptr() if dotw is not None else None, part.ctypes.data, 4096, C.byref(npart), C.byref(form)))
    torch.cuda.synchronize()
    return form.value, y.cpu().numpy().tobytes(), part[:npart.value].tobytes()


def _compare_products(S, K, ssym, swept, want_form=1):
    """coded against forced stored for B = 1, 2, (alpha, beta) = (1, 0), (-1, 1), dotw == x and dotw != x"""
    for bands in (B1, B2):
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
            for dotw in (S.x, S.w):
                fc, yc, pc = _product(S, K, ssym, bands, alpha, beta, dotw)
                fs, ys, ps = _product(S, K, ssym, bands | STORED, alpha, beta, dotw)
                assert fs == (0 if swept else -1) and fc == (want_form if swept else -1), (S.lat, bands, fc, fs)
                assert len(pc) > 0 and yc == ys and pc == ps, (S.lat, hex(bands), alpha, beta, dotw is S.x)


@pytest.mark.parametrize("planes,points", RIM, ids=[f"{p}x{q}" for p, q in RIM])
def test_the_issues_rim_lattices(mf, planes, points):
    """Check 1 on the lattices the issue lists (see the module docstring: the sweep's planning rules keep it off all of them)"""
    from metafem_jl_amd import _lib

    with _lift():
        for lines in RIM_LINES:
            S = _system(mf, (planes, lines, points))
            assert len(set(S.codes.tolist())) >= 3 and np.any(S.codes != 0) and not np.any(_no_code(S.codes)), (S.lat, sorted(set(S.codes.tolist())))
            if _layout_mode(S) == 2:
                _compare_products(S, S.K, S.ssym, _sweep_planned(S))
                continue
            # no diagonal-slotted layout, so no scaled copy either: the plain product and the scaled CG's fall-back under both knob words
            for bands in (B1, B2):
                for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
                    ys = []
                    for word in (bands, bands | STORED):
                        _lib.check(_lib.lib.mfem_debug_set_ell(1 | word))
                        y = S.y0.clone()
                        _lib.check(_lib.lib.mfem_spmv_solver_layout(S.brick.ctx._h, S.A._h, S.K.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta))
                        ys.append(y.cpu().numpy().tobytes())
                    assert ys[0] == ys[1]
                a, b = _solve(mf, S, S.K, bands, 4, 12, 8, True), _solve(mf, S, S.K, bands | STORED, 4, 12, 8, True)
                assert a[2] == 0 and b[2] == 0 and _same(a, b)


@pytest.mark.parametrize("lat", SWEPT, ids=["x".join(map(str, v)) for v in SWEPT])
def test_coded_product_is_bitwise_the_stored_product(mf, lat):
    """Check 1 where the sweep runs: the bind reports the coded form, the forced bind the stored one; y and the partial sums are the same bytes; the coded form
    also with the symmetry verdict from the check pass (bit 30: MODE 1 follows the coded layout) and with the tail rows in a launch of their own (bit 26)."""
    from metafem_jl_amd import _lib

    S = _system(mf, lat)
    codes = sorted(set(S.codes.tolist()))
    print(f"\n{lat}: codes {codes}, zero in {float(np.mean(S.codes == 0)):.2f} of the rows")
    assert len(codes) >= 3 and np.any(S.codes != 0) and not np.any(_no_code(S.codes))
    with _lift():
        assert _sweep_planned(S)
        c0 = int(_lib.lib.mfem_debug_symp_coded_count())
        _compare_products(S, S.K, S.ssym, True)
        assert int(_lib.lib.mfem_debug_symp_coded_count()) == c0 + 8   # one per coded bind, none per forced bind
        f0, y0, p0 = _product(S, S.K, S.ssym, B2, 1.0, 0.0, S.x)
        for word in (B2 | CHECK_PASS, B2 | 1 << 26, B1 | CHECK_PASS):
            f, y, p = _product(S, S.K, S.ssym, word, 1.0, 0.0, S.x)
            assert f == 1 and y == y0, hex(word)
        for word in (B2 | 1 << 29, B2 | 1 << 27):   # not the fast fill: the stored form, the same product
            f, y, p = _product(S, S.K, S.ssym, word, 1.0, 0.0, S.x)
            assert f == 0 and y == y0 and p == p0, hex(word)
        # the byte accounting answers for the form of the last bind: two bytes instead of two doubles of diagonal per lane pair and step
        byts = {}
        for word in (B2, B2 | STORED):
            _product(S, S.K, S.ssym, word, 1.0, 0.0, S.x)
            _lib.check(_lib.lib.mfem_debug_set_ell(1 | word))
            b = C.c_int64()
            _lib.check(_lib.lib.mfem_csr_solver_layout_bytes(S.brick.ctx._h, S.A._h, C.byref(b)))
            byts[word] = b.value
        pairs = sum(1 for j in range(lat[1]) for k in range(0, lat[2], 2))
        nplanes_lo, nplanes_hi = lat[0] - 6, lat[0] - 2
        saved = byts[B2 | STORED] - byts[B2]
        print(f"design bytes: stored {byts[B2 | STORED]}, coded {byts[B2]}")
        assert 13 * pairs * nplanes_lo <= saved <= 14 * pairs * nplanes_hi + 8, (saved, pairs)


def _solve(mf, S, K, word, variant, iters, ring, graphs):
    from metafem_jl_amd import _lib

    _lib.check(_lib.lib.mfem_debug_set_ell(1 | word))
    _lib.check(_lib.lib.mfem_debug_set_graphs(1 if graphs else 0, 0))
    _lib.check(_lib.lib.mfem_debug_set_cg_ring(ring))
    c0, s0 = int(_lib.lib.mfem_debug_symp_coded_count()), int(_lib.lib.mfem_debug_sym_spmv_count())
    x, st = mf.iterative_Solve(S.A, K, S.b, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=iters, max_pass=1, fixed_iterations=True, cg_variant=variant)
    stats = (st.passes, st.iterations, st.final_res, st.initial_res, st.converged, st.spmv_count)
    return x, stats, int(_lib.lib.mfem_debug_symp_coded_count()) - c0, int(_lib.lib.mfem_debug_sym_spmv_count()) - s0


def _same(a, b):
    return a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and repr(a[1]) == repr(b[1])   # (bytes and repr: a NaN equals itself)


@pytest.mark.parametrize("bands", [B1, B2], ids=["B1", "B2"])
def test_cg_on_the_coded_copy_is_bitwise_cg_on_the_stored_copy(mf, bands):
    """Check 2: cg_variant 4 and 0 (auto: scaled from 64 iterations per pass on), 12 and 40 fixed iterations (and 64 for auto), ring depth 1 and 8, captured
    cycles on and off -- x and the statistics of the coded bind equal the forced stored bind's; variant 4 against variant 3 to 1e-9."""
    S = _system(mf, (40, 17, 33))
    with _lift():
        x3 = {it: _solve(mf, S, S.K, bands, 3, it, 1, True)[0] for it in (12, 40)}
        for variant, iters in ((4, 12), (4, 40), (0, 12), (0, 40), (0, 64)):
            scaled = variant == 4 or iters >= 64
            for ring in (1, 8):
                for graphs in (True, False):
                    coded = _solve(mf, S, S.K, bands, variant, iters, ring, graphs)
                    stored = _solve(mf, S, S.K, bands | STORED, variant, iters, ring, graphs)
                    assert coded[2] == (1 if scaled else 0) and stored[2] == 0 and coded[3] > 0 and stored[3] > 0, (variant, iters, coded[2:], stored[2:])
                    assert _same(coded, stored), (variant, iters, ring, graphs, coded[1], stored[1])
                    assert coded[1][1] == iters
            if variant == 4:
                err = float((coded[0] - x3[iters]).abs().max()) / float(x3[iters].abs().max())
                print(f"\ncg_variant 4 against 3 after {iters} iterations: {err:.3e}")
                assert err <= 1e-9


def _rows_for_the_gate(S):
    """a swept interior row; a row of the first swept plane (where every run of plane p0 starts); a row on a patch rim (line 8, column 32: the first cell of a
    patch for either band count)"""
    planes, m1, m2 = S.lat
    PL = m1 * m2
    lo = -(-(PL + m2 + 1) // 128) * 128
    p0 = -(-lo // PL)
    return {"interior": (planes // 2) * PL + 5 * m2 + 13, "first swept plane": p0 * PL + 2 * m2 + 7, "patch rim": (planes // 2 + 1) * PL + 8 * m2 + 32}


@pytest.mark.parametrize("where", ["interior", "first swept plane", "patch rim"])
def test_a_diagonal_without_a_code_sends_the_bind_to_the_stored_form(mf, where):
    """Check 3: the sign of one swept row's diagonal flipped (the other sign than the unit: 2^63 ulps away) -> the bind reports the stored form and the results are the forced stored bind's, product and CG; a following
    solve with the good values ON THE SAME BUFFERS is coded again and repeats the first solve bit for bit (captured cycles on: the graph key follows)."""
    import torch

    S = _system(mf, (40, 17, 33))
    r = _rows_for_the_gate(S)[where]
    assert S.lat[1] * S.lat[2] * 2 <= r < S.n - S.lat[1] * S.lat[2] * 2
    Kw = S.K.clone()
    k = int(S.diag_idx_h[r])
    good = float(Kw[k])
    with _lift():
        first = {bands: _solve(mf, S, Kw, bands, 4, 12, 8, True) for bands in (B1, B2)}
        assert all(v[2] == 1 for v in first.values())
        Kw[k] = -good
        ssym_bad, codes_bad = _scaling(S, Kw)
        assert bool(_no_code(codes_bad)[r]) and int(np.sum(_no_code(codes_bad))) == 1
        _compare_products(S, Kw, ssym_bad, True, want_form=0)
        for bands in (B1, B2):
            refused = _solve(mf, S, Kw, bands, 4, 12, 8, True)
            forced = _solve(mf, S, Kw, bands | STORED, 4, 12, 8, True)
            assert refused[2] == 0 and refused[3] > 0 and forced[3] > 0, (refused[2:], forced[2:])   # the sweep ran, on the stored form
            assert _same(refused, forced)
            assert not _same(refused, first[bands])
        Kw[k] = good
        torch.cuda.synchronize()
        for bands in (B1, B2):
            again = _solve(mf, S, Kw, bands, 4, 12, 8, True)
            assert again[2] == 1 and _same(again, first[bands])
        _compare_products(S, Kw, S.ssym, True)


def test_unsymmetric_values_never_get_the_coded_form(mf):
    """Check 4: with unsymmetric values cg_variant 4 falls back to the classic recurrence on the per-row kernel as before -- no coded bind, no sweep, the
    forced run's bytes -- and the product entry point reports that the bind did not end on the sweep; a bind without the scaling is never coded."""
    from metafem_jl_amd import _lib

    S = _system(mf, (40, 17, 33))
    planes, m1, m2 = S.lat
    row = 9 * m1 * m2 + 6 * m2 + 14
    Ku = S.K.clone()
    Ku[int(S.A.rowptr[row]) - int(S.A.index_base) + 20] *= 1.0 + 1e-3
    with _lift():
        for bands in (B1, B2):
            a = _solve(mf, S, Ku, bands, 4, 30, 1, True)
            b = _solve(mf, S, Ku, bands | STORED, 4, 30, 1, True)
            assert a[2] == 0 and a[3] == 0 and b[3] == 0 and _same(a, b)
            assert _product(S, Ku, S.ssym, bands, 1.0, 0.0, S.x)[0] == -1
            # symmetric values, no scaling (cg_variant 3 reads the diagonal from the copy): the sweep on the stored form
            c = _solve(mf, S, S.K, bands, 3, 12, 1, True)
            assert c[2] == 0 and c[3] > 0
        c0 = int(_lib.lib.mfem_debug_symp_coded_count())
        y = S.y0.clone()
        _lib.check(_lib.lib.mfem_debug_set_ell(1 | B2))
        _lib.check(_lib.lib.mfem_spmv_solver_layout(S.brick.ctx._h, S.A._h, S.K.data_ptr(), S.x.data_ptr(), y.data_ptr(), 1.0, 0.0))
        assert int(_lib.lib.mfem_debug_symp_coded_count()) == c0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_on_one_gpu():
    """Check 5: two slabs on cuda:0 through the host-callback communicator: every rank's x and statistics of the scaled CG on the coded copy against the
    forced stored copy, bit for bit (tests/symp_diag_code_worker.py compares and reports)"""
    world, port = 2, _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    logs = [tempfile.TemporaryFile() for _ in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "symp_diag_code_worker.py"), str(world), str(r), str(port)], stdout=logs[r],
                              stderr=subprocess.STDOUT, env=env) for r in range(world)]
    deadline = time.monotonic() + 300
    try:
        for p in procs:
            try:
                p.wait(timeout=max(deadline - time.monotonic(), 0.1))
            except subprocess.TimeoutExpired:
                break
            if p.returncode != 0:  # a dead rank leaves the other waiting in a collective
                deadline = min(deadline, time.monotonic() + 20)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, f) in enumerate(zip(procs, logs)):
        f.seek(0)
        out = f.read().decode(errors="replace")
        f.close()
        line = [ln for ln in out.splitlines() if ln.startswith("DIAG_CODE_REPORT ")]
        rep = json.loads(line[-1][len("DIAG_CODE_REPORT "):]) if line else None
        assert p.returncode == 0 and rep is not None and rep["compared"] > 0 and not rep["failed"] and rep["coded_binds"] >= rep["compared"], (
            f"rank {r}: rc={p.returncode}, report {rep}\n--- output tail ---\n" + out[-3000:])
