"""The trimmed form of the wave-private patch sweep (csrc/symp_trim_decide.h): the sweep covers whole patches only -- a remainder of at most 2 points per
lattice line and of one line per plane leaves it -- and the rim rows are computed row by row from a compact copy (k_symp_rim_fill, symp_rim_unit).

Conventions of tests/test_gpu_symp_bands.py: layout_min_rows = (0, 0), bands forced by bits 24 / 25 of the "ell" knob, random bitwise-symmetric values and
one assembled thermal K with Robin faces.  The trim is decided by size (mfem_symp_trim_wanted: from 1.6e7 swept rows on, the sizes it was measured at), so
on these small lattices bit 3 forces it and bit 2 forces the untrimmed form; mfem_debug_symp_trim_count tells that a bind really ended with rim rows.

Lattices (planes, lines, points per line):
  (40, 17, 33)  both rims and the corner; one patch column remains
  (200, 9, 65)  one patch row remains at B = 2; several runs per patch
  (20, 17, 65)
  (40, 12, 34)  a 2-point rim; at B = 2 the 4-line remainder stays swept
  (40, 12, 35)  the 3-point remainder stays swept: no rim at all
  (20, 5, 3), (4, 9, 34)  unswept: must be left alone

Bounds.  Product against the oracle's CSR product mul(y0, A, x, alpha, beta): |y - y_ref| <= 2 * 27 * eps * (|alpha| |A| |x| + |beta| |y0|) elementwise -- for
(alpha, beta) = (1, 0) the rounding bound of two 27-term sums in different orders, 2 * 27 * eps * (|A| |x|); the scaling by alpha and the added beta y0 each
round once more on either side, far inside the same factor.  Fused x . y against dot(x, y): n * eps * |x|_2 * |y|_2 (two n-term sums in different orders).
CG: the comparison tests/test_gpu_jacobi_solve.py applies to its patch-sweep cases -- max |x - x_oracle| / max |x_oracle| <= 1e-10 after k steps, equal
iteration and pass counts.  Two ranks: every rank's x of the trimmed solve against its own solve by the plain per-row kernel, the same 1e-10 (both run the
same recurrence on the same products; only the order of the partial sums of p . Ap differs)."""
import ctypes as C
import importlib.util
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
EPS = 2.0 ** -52
B1, B2, PLAIN, CHECK_PASS, STORED = 1 << 24, 1 << 25, 1 << 22, 1 << 30, 1 << 21
UNTRIMMED, TRIM = 1 << 2, 1 << 3
SP_L, SP_W = 4, 32

SWEPT = [(40, 17, 33), (200, 9, 65), (20, 17, 65), (40, 12, 34), (40, 12, 35)]
UNSWEPT = [(20, 5, 3), (4, 9, 34)]
CASES = [(lat, "random") for lat in SWEPT + UNSWEPT] + [((40, 17, 33), "thermal")]


def _bands_module():
    spec = importlib.util.spec_from_file_location("_symp_bands_for_trim", os.path.join(HERE, "test_gpu_symp_bands.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SB = _bands_module()   # its systems (brick, pattern, values, x, the oracle's products: made once per lattice), knob helpers
KS = SB.KS


def _extents(lat, B):
    """(ms1, ms2) of csrc/symp_trim_decide.h, restated"""
    _, m1, m2 = lat
    L = SP_L * B
    ms1 = m1 - m1 % L if 1 <= m1 % L <= 1 and m1 >= L + m1 % L else m1
    ms2 = m2 - m2 % SP_W if 1 <= m2 % SP_W <= 2 and m2 >= SP_W + m2 % SP_W else m2
    return ms1, ms2


def _has_rim(lat, B):
    return lat in SWEPT and _extents(lat, B) != (lat[1], lat[2])


def _trim_count():
    from metafem_jl_amd import _lib

    return int(_lib.lib.mfem_debug_symp_trim_count())


def _product(S, K, word, alpha=1.0, beta=0.0, dot=False, y0=None):
    """(y, sweep launched?, binds that ended with rim rows, x . y) of one product through the solver layout under knob word `word`"""
    import torch
    from metafem_jl_amd import _lib

    SB._set_ell(word)
    try:
        y = torch.full((S.n,), 3.0, dtype=torch.float64, device="cuda") if y0 is None else y0.clone()
        before, t0 = _lib.lib.mfem_debug_sym_spmv_count(), _trim_count()
        d = C.c_double(0.0)
        if dot:
            _lib.check(_lib.lib.mfem_spmv_solver_layout_dot(S.brick.ctx._h, S.A._h, K.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta, C.byref(d)))
        else:
            _lib.check(_lib.lib.mfem_spmv_solver_layout(S.brick.ctx._h, S.A._h, K.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta))
        torch.cuda.synchronize()
        return y, _lib.lib.mfem_debug_sym_spmv_count() > before, _trim_count() - t0, d.value
    finally:
        SB._set_ell(0)


@pytest.mark.parametrize("lat,values", CASES, ids=["x".join(map(str, v)) + "-" + w for v, w in CASES])
def test_trimmed_product_is_bitwise_the_plain_product(mf, lat, values):
    """y of the trimmed sweep is bitwise y of the plain per-row kernel (bit 22) and of the untrimmed sweep, for both band counts and however the copy is
    made (k_symp_fill, the row tiles of bit 29, the two-pass bind of bit 27), with the check pass (bit 30) and with the rim and tail rows in launches of
    their own (bit 26); against the oracle within the rounding bound for (alpha, beta) = (1, 0) and (-1, 1); the fused x . y against dot(x, y)."""
    import torch
    from oracle import solvers

    S = SB._system(mf, lat)
    K = S.Kr if values == "random" else S.Kt
    K_h = S.Kr_h if values == "random" else S.Kt_h
    y_ref, bound = S.ref[values]
    y0 = mf.FEM_rand(S.n, 7, 0) - 0.5
    y0_h = y0.cpu().numpy()
    Ah = solvers.csr(S.rowptr, S.col, K_h, S.n)
    y_ref_ab = solvers.mul(y0_h.copy(), Ah, S.x_h, -1.0, 1.0)
    with SB._lift():
        swept = SB._sweep_planned(S)
        assert swept == (lat in SWEPT), lat
        y_plain, ran, _, _ = _product(S, K, PLAIN)
        assert not ran
        for B, bw in ((1, B1), (2, B2)):
            rim = _has_rim(lat, B)
            yt, rant, nt, dt = _product(S, K, bw | TRIM, dot=True)
            yu, ranu, nu, _ = _product(S, K, bw | UNTRIMMED)
            yd, rand, nd, _ = _product(S, K, bw)   # by size: these lattices keep every row in a patch
            assert rant == ranu == rand == swept and nt == (1 if rim else 0) and nu == 0 and nd == 0, (lat, B, rant, ranu, nt, nu, nd)
            assert torch.equal(yt, y_plain) and torch.equal(yu, y_plain) and torch.equal(yd, y_plain), (lat, B)
            for word in (bw | TRIM | 1 << 29, bw | TRIM | 1 << 27, bw | TRIM | CHECK_PASS, bw | TRIM | 1 << 26, bw | TRIM | 1 << 27 | CHECK_PASS):
                yv, ranv, nv, _ = _product(S, K, word)
                assert ranv == swept and nv == (1 if rim else 0) and torch.equal(yv, y_plain), (lat, hex(word))
            y_h = yt.cpu().numpy()
            excess = float((np.abs(y_h - y_ref) - 2 * 27 * EPS * bound).max())
            yab, ranab, _, _ = _product(S, K, bw | TRIM, alpha=-1.0, beta=1.0, y0=y0)
            excess_ab = float((np.abs(yab.cpu().numpy() - y_ref_ab) - 2 * 27 * EPS * (bound + np.abs(y0_h))).max())
            dref = float(np.dot(S.x_h, y_h))
            tol = S.n * EPS * float(np.linalg.norm(S.x_h)) * float(np.linalg.norm(y_h))
            print(f"\n{lat} {values} B = {B}: rim {rim}, max |y - y_ref| = {np.abs(y_h - y_ref).max():.3e}, excess over the bound {excess:.3e} / (-1, 1): {excess_ab:.3e}; "
                  f"fused x . y {dt!r}, dot(x, y) {dref!r}, tolerance {tol:.3e}")
            assert ranab == swept
            assert excess <= 0.0 and excess_ab <= 0.0
            assert abs(dt - dref) <= tol


def _entry(S, r, c):
    lo, hi = int(S.rowptr[r]), int(S.rowptr[r + 1])
    k = lo + int(np.searchsorted(S.col[lo:hi], c))
    assert S.col[k] == c
    return k


@pytest.mark.parametrize("bands", [B1, B2], ids=["B1", "B2"])
def test_symmetry_verdicts_look_at_swept_pairs_only(mf, bands):
    """The fill's fingerprint and the check pass (bit 30) agree: both accept the symmetric values, both refuse after one off-diagonal entry of a pair of two
    swept rows is moved by an ulp, both accept when only entries towards rim rows are moved -- the sweep does not mirror those pairs (the swept row reads
    its own entry: an upper slot, or the edge block's copy of a lower one; the rim row its own 27 slots) -- and the product is then still the plain
    kernel's, bit for bit, and the oracle's on the perturbed matrix."""
    import torch
    from oracle import solvers

    S = SB._system(mf, (40, 17, 33))
    planes, m1, m2 = S.lat
    PL = m1 * m2
    ms1, ms2 = _extents(S.lat, 1 if bands == B1 else 2)
    assert (ms1, ms2) == (16, 32)

    def moved(pairs):
        Kf_h = S.Kr_h.copy()
        for r, c in pairs:
            k = _entry(S, r, c)
            Kf_h[k] = np.nextafter(Kf_h[k], np.inf)
            assert Kf_h[k] != S.Kr_h[k]
        return Kf_h, torch.tensor(Kf_h, device="cuda")

    r = 9 * PL + 2 * m2 + 20                                # plane 9, line 2, column 20; its neighbour on line 1: both swept, one patch
    _, K_ss = moved([(r, r - m2)])
    a = 9 * PL + 5 * m2 + (ms2 - 1)                         # a swept row in the last swept column ...
    b = 9 * PL + (ms1 - 1) * m2 + 7                         # ... and one on the last swept line
    rim_pairs = [(a, a + 1), (a, a - PL + 1), (a, a + PL + m2 + 1),       # towards the column rim: slots 14, 5 (an edge-block entry), 26
                 (b, b + m2), (b, b - PL + m2 - 1), (b + 1, b + 1 + m2)]  # towards the line rim: slots 16, 6, 16
    Kr_h, K_sr = moved(rim_pairs)
    with SB._lift():
        assert SB._sweep_planned(S)
        for check in (0, CHECK_PASS):
            word = bands | TRIM | check
            _, ran, nt, _ = _product(S, S.Kr, word)
            assert ran and nt == 1, hex(word)
            _, ran, nt, _ = _product(S, K_ss, word)
            assert not ran and nt == 0, hex(word)
            y, ran, nt, _ = _product(S, K_sr, word)
            assert ran and nt == 1, hex(word)
            y_plain, ranp, _, _ = _product(S, K_sr, PLAIN)
            assert not ranp and torch.equal(y, y_plain), hex(word)
            Ah = solvers.csr(S.rowptr, S.col, Kr_h, S.n)
            y_ref = solvers.mul(np.zeros(S.n), Ah, S.x_h)
            assert np.all(np.abs(y.cpu().numpy() - y_ref) <= 2 * 27 * EPS * (abs(Ah) @ np.abs(S.x_h)))
        # the untrimmed sweep holds the rim rows in patches of their own: its fingerprint looks at these pairs and refuses
        assert not _product(S, K_sr, bands | UNTRIMMED)[1]


SOLVES = [(B2, 4, 0), (B2, 4, STORED), (B2, 3, 0), (B1, 4, 0), (B1, 1, 0)]


@pytest.mark.parametrize("bands,variant,stored", SOLVES, ids=[f"B{1 if b == B1 else 2}-v{v}-{'stored' if s else 'coded'}" for b, v, s in SOLVES])
def test_cg_on_the_trimmed_sweep_matches_the_oracle(mf, bands, variant, stored):
    """CG with Pr_Jacobi! -- cg_variant 4 on S^-1 A S^-1 with the coded and the stored diagonal, variants 3 and 1 on the unscaled copy -- on the trimmed sweep
    against the oracle's Jacobi CG after k steps, as tests/test_gpu_jacobi_solve.py compares its patch-sweep cases."""
    import torch
    from metafem_jl_amd import _lib
    from oracle import solvers

    S = SB._system(mf, (40, 17, 33))
    b = KS.mf_rand(S.n)
    k = KS._k("cg", 0)
    maxiter = KS._maxiter("cg", 0, k)
    info = solvers.SolveInfo()
    with np.errstate(all="ignore"):
        xo = solvers.solve_cg_jacobi(S.rowptr, S.col, S.Kt_h, b.cpu().numpy(), 1e-300, maxiter, max_pass=1, info=info, guard_zero=True)
    with SB._lift():
        SB._set_ell(bands | TRIM | stored)
        try:
            s0, t0, c0 = _lib.lib.mfem_debug_sym_spmv_count(), _trim_count(), int(_lib.lib.mfem_debug_symp_coded_count())
            x, st = mf.iterative_Solve(S.A, S.Kt, b, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=maxiter, max_pass=1, cg_variant=variant,
                                       fixed_iterations=True)
            torch.cuda.synchronize()
            assert _lib.lib.mfem_debug_sym_spmv_count() > s0 and _trim_count() > t0
            assert (int(_lib.lib.mfem_debug_symp_coded_count()) > c0) == (variant == 4 and not stored)
        finally:
            SB._set_ell(0)
    xd = x.cpu().numpy()
    err = float(np.abs(xd - xo).max() / np.abs(xo).max())
    print(f"\ncg_variant {variant}: err = {err:.3e}, iterations {st.iterations}/{info.iters}")
    assert np.all(np.isfinite(xd))
    assert err <= KS.TOL_X
    assert st.passes == info.passes == 1
    assert st.iterations == info.iters


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_on_one_gpu():
    """The split SpMV: two slabs on cuda:0 through the host-callback communicator, as tests/test_gpu_cg_ring.py runs them (tests/symp_trim_worker.py compares
    and reports)."""
    world, port = 2, _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    logs = [tempfile.TemporaryFile() for _ in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "symp_trim_worker.py"), str(world), str(r), str(port)], stdout=logs[r],
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
        line = [ln for ln in out.splitlines() if ln.startswith("SYMP_TRIM_REPORT ")]
        rep = json.loads(line[-1][len("SYMP_TRIM_REPORT "):]) if line else None
        assert p.returncode == 0 and rep is not None and rep["compared"] > 0 and not rep["failed"], (
            f"rank {r}: rc={p.returncode}, report {rep}\n--- output tail ---\n" + out[-3000:])
