"""The constant form of the wave-private patch sweep (csrc/symp_const_decide.h; k_spmv_symp_const<B, DC>): the fill flags every patch step whose matrix
values all equal, bit for bit, the values of one reference row, and the sweep computes a flagged step from its kernel arguments alone: the 27 products of
every row with the reference row's values, rounded and added in slot order, without matrix loads, mirror tables or edge block.  Those are the very doubles
the stored form multiplies by (the row's own slots were compared by the fill, the mirrored ones are bitwise equal to them by the bind's fingerprint), so
EVERY product comparison here is bitwise.

Conventions of tests/test_gpu_symp_trim.py: layout_min_rows = (0, 0), bands forced by bits 24 / 25 of the "ell" knob, the trim by bits 2 / 3.  Bit 4 forces
the stored form (no step flags are made), bit 5 the constant form whatever the share of flagged steps, bit 21 the stored diagonal, bit 22 the plain per-row
kernel.  The gate (spc_gate: 44 % of the steps, from the two measurements beside it) keeps the stored form on this small fixture, where 25 - 56 % of the
steps are interior, unless the share reaches it; the tests bind the constant form with bit 5 and pin the gate's own answer beside it.

Fixture: the assembled thermal K with Robin terms on all six faces on Brick((0.125, 0.25, 1.0), (16, 32, 128)): h = 2^-7 in every direction, lattice
(planes, lines, points) = (17, 33, 129), 72 369 rows -- the smallest dyadic lattice with interior patches in both in-plane directions for B = 2 (4 patch
rows of 8 lines, 4 patch columns of 32 points, two interior each way).  The regular 128-row blocks hold the whole planes [2, 15): 13 swept planes.

Expected flagged steps, from the geometry alone: whole patches whose lines lie in [g, m1 - 1 - g] and points in [g, m2 - 1 - g], times the swept planes in
[g, planes - 1 - g].  For the scaled copies S^-1 A S^-1 the margin is g = 2: a row's entry towards column c carries t_c = 1 / sqrt|a_cc|, and the diagonal of a
node on the boundary (Robin term, fewer elements) differs, so all 27 neighbours must be interior nodes.  The UNSCALED copy is constant one node further out,
g = 1: a row of a node next to the boundary gathers the same eight element matrices in the same order, and the Robin terms touch only entries between
two boundary nodes -- with patches starting at multiples of 4, 8 and 32 the wider range adds the last whole patch row (B = 1) and patch column of this
lattice.  Both counts are > 0 for every parametrisation (asserted).

CG: x against the oracle's Jacobi CG to the 1e-10 of tests/test_gpu_symp_trim.py; constant form against forced stored form byte for byte."""
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
B1, B2, PLAIN, STORED_DIAG = 1 << 24, 1 << 25, 1 << 22, 1 << 21
UNTRIMMED, TRIM = 1 << 2, 1 << 3
FORCE_STORED, FORCE_CONST = 1 << 4, 1 << 5
SP_L, SP_W = 4, 32
LAT = (17, 33, 129)
SIDES = (0.125, 0.25, 1.0)


def _bands_module():
    spec = importlib.util.spec_from_file_location("_symp_bands_for_const", os.path.join(HERE, "test_gpu_symp_bands.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SB = _bands_module()
KS = SB.KS


class Sys:
    pass


_CACHE = {}


def _system(mf):
    """Brick, pattern, K, its 1 / sqrt|a_ii|, T K T and its scaling, x -- made once, never changed."""
    import torch

    if "S" in _CACHE:
        return _CACHE["S"]
    S = Sys()
    S.lat = LAT
    S.brick = mf.make_Brick(SIDES, tuple(v - 1 for v in LAT))
    S.A = S.brick.pattern(1)
    S.n = n = S.A.n
    assert n == LAT[0] * LAT[1] * LAT[2] == 72369
    S.rowptr = S.A.rowptr.cpu().numpy().astype(np.int64) - S.A.index_base
    S.col = S.A.colidx.cpu().numpy().astype(np.int32) - S.A.index_base
    S.K = S.brick.assemble_thermal(S.A, KS.K_COND, KS.H, KS.TENV, 0x3F)
    S.K_h = S.K.cpu().numpy()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (S.A.rowptr[1:] - S.A.rowptr[:-1]).long())
    cols = S.A.colidx.long() - int(S.A.index_base)
    S.diag_idx = torch.nonzero(cols == rows).flatten()
    assert S.diag_idx.numel() == n
    S.ssym = _ssym(S, S.K)
    t = 1.0 + 29.0 * mf.FEM_rand(n, 3, 0)
    S.KT = S.K * (t[rows] * t[cols])       # T K T, t in [1, 30]: the existing tests' matrix -- no two rows alike
    S.ssymT = _ssym(S, S.KT)
    S.x = mf.FEM_rand(n, 5, 0) - 0.5
    S.y0 = mf.FEM_rand(n, 7, 0) - 0.5
    _CACHE["S"] = S
    return S


def _ssym(S, K):
    import torch

    return torch.tensor(1.0 / np.sqrt(np.abs(K[S.diag_idx].cpu().numpy())), device="cuda")


def _swept_planes():
    """[p0, p1): the whole planes inside the regular 128-row blocks (every row r with r - (PL + m2 + 1) >= 0 and r + PL + m2 + 1 < n), as symp_plan"""
    planes, m1, m2 = LAT
    PL, n = m1 * m2, planes * m1 * m2
    b_lo, b_hi = -(-(PL + m2 + 1) // 128), (n - (PL + m2 + 1)) // 128
    return -(-(b_lo * 128) // PL), (b_hi * 128) // PL


def _extents(B, trim):
    """(ms1, ms2) of csrc/symp_trim_decide.h, restated"""
    _, m1, m2 = LAT
    L = SP_L * B
    if not trim:
        return m1, m2
    ms1 = m1 - m1 % L if 1 <= m1 % L <= 1 and m1 >= L + m1 % L else m1
    ms2 = m2 - m2 % SP_W if 1 <= m2 % SP_W <= 2 and m2 >= SP_W + m2 % SP_W else m2
    return ms1, ms2


def _steps(B, trim):
    ms1, ms2 = _extents(B, trim)
    L = SP_L * B
    p0, p1 = _swept_planes()
    return -(-ms1 // L) * -(-ms2 // SP_W) * (p1 - p0)


def _expected(B, trim, g):
    """flagged steps by geometry (csrc/symp_const_decide.h: spc_expected, restated with the margin g of the module docstring)"""
    planes, m1, m2 = LAT
    ms1, ms2 = _extents(B, trim)
    L = SP_L * B
    p0, p1 = _swept_planes()
    pr = sum(1 for j0 in range(0, ms1, L) if j0 + L <= ms1 and j0 >= g and j0 + L - 1 <= m1 - 1 - g)
    pc = sum(1 for k0 in range(0, ms2, SP_W) if k0 + SP_W <= ms2 and k0 >= g and k0 + SP_W - 1 <= m2 - 1 - g)
    pp = sum(1 for p in range(p0, p1) if g <= p <= planes - 1 - g)
    return pr * pc * pp


def _counts():
    from metafem_jl_amd import _lib

    return int(_lib.lib.mfem_debug_symp_const_count()), int(_lib.lib.mfem_debug_symp_const_steps())


def _product(S, K, ssym, word, alpha=1.0, beta=0.0):
    """(y, sweep launched?, constant binds, flagged steps of the bind, design entries of that bind) of one product under knob word `word`: on the copy the
    scaled CG binds (ssym given; bit 21: with its diagonal stored) or on the unscaled copy (ssym None)"""
    import torch
    from metafem_jl_amd import _lib

    SB._set_ell(word)
    try:
        y = S.y0.clone()
        s0, (c0, _) = _lib.lib.mfem_debug_sym_spmv_count(), _counts()
        if ssym is None:
            _lib.check(_lib.lib.mfem_spmv_solver_layout(S.brick.ctx._h, S.A._h, K.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta))
        else:
            form = C.c_int32(-7)
            _lib.check(_lib.lib.mfem_debug_spmv_scaled_layout(S.brick.ctx._h, S.A._h, K.data_ptr(), ssym.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta,
                                                              None, None, 0, None, C.byref(form)))
        torch.cuda.synchronize()
        c1, steps = _counts()
        ent, sym = C.c_int64(), C.c_int32()
        _lib.check(_lib.lib.mfem_csr_solver_layout_entries(S.brick.ctx._h, S.A._h, C.byref(ent), C.byref(sym)))   # (answers for the last bind, under this word)
        return y, _lib.lib.mfem_debug_sym_spmv_count() > s0, c1 - c0, steps, ent.value
    finally:
        SB._set_ell(0)


def _ne(B):
    L = SP_L * B
    return 9 * SP_W + 6 * (L - 1) + 3 * L


FORMS = ["coded", "stored", "unscaled"]
PRODUCTS = [(b, f, t) for b in (1, 2) for f in FORMS for t in (True, False)]


@pytest.mark.parametrize("B,form,trim", PRODUCTS, ids=[f"B{b}-{f}-{'trimmed' if t else 'untrimmed'}" for b, f, t in PRODUCTS])
def test_constant_form_is_bitwise_the_stored_form(mf, B, form, trim):
    """Check 1: y of the constant form = y of the forced stored form = y of the plain per-row kernel, the flagged steps are the geometric count, the bind
    counter advanced, and the design entries fall by what the flagged steps no longer read (13 or 14 slots of 64 B lane pairs, the edge block, the codes;
    one flag byte per step comes on top)."""
    import torch

    S = _system(mf)
    ssym = None if form == "unscaled" else S.ssym
    g = 1 if form == "unscaled" else 2
    base = (B1 if B == 1 else B2) | (TRIM if trim else UNTRIMMED) | (STORED_DIAG if form == "stored" else 0)
    word = base | FORCE_CONST
    want = _expected(B, trim, g)
    assert 0 < want < _steps(B, trim)
    with SB._lift():
        assert SB._sweep_planned(S)
        yp, ranp, _, _, _ = _product(S, S.K, ssym, PLAIN)
        assert not ranp
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
            yc, ranc, nc, steps, ent_c = _product(S, S.K, ssym, word, alpha, beta)
            ys, rans, ns, steps_s, ent_s = _product(S, S.K, ssym, word | FORCE_STORED, alpha, beta)
            print(f"\nB = {B} {form} trim {trim} ({alpha}, {beta}): flagged {steps} of {_steps(B, trim)} steps (geometry: {want}), constant binds {nc} / {ns}, "
                  f"entries {ent_c} / {ent_s}")
            assert ranc and rans
            assert steps == want and nc == 1
            assert steps_s == 0 and ns == 0
            assert torch.equal(yc.view(torch.int64), ys.view(torch.int64))
            if (alpha, beta) == (1.0, 0.0):
                assert torch.equal(yc.view(torch.int64), yp.view(torch.int64))
            per_step = (26 if form == "coded" else 28) * 64 * B + _ne(B) + (16 * B if form == "coded" else 0)
            assert ent_s - ent_c == want * per_step - -(-_steps(B, trim) // 8)
        # the tail rows in a launch of their own (bit 26) leave the form and the product alone; with the symmetry verdict from the check pass (bit 30: it lets
        # +0.0 meet -0.0 in a mirrored pair, the flagged steps' path needs the pairs bitwise equal) the steps are flagged and the stored form is kept
        for extra, binds in ((1 << 26, 1), (1 << 30, 0)):
            yv, ranv, nv, stv, _ = _product(S, S.K, ssym, word | extra)
            assert ranv and nv == binds and stv == want and torch.equal(yv.view(torch.int64), yp.view(torch.int64)), hex(extra)
        # by the gate alone: the constant form from 44 % flagged steps on (integer form of spc_gate: 2 c / (c + g), c = 736, g = 2594)
        yg, rang, ng, stg, _ = _product(S, S.K, ssym, base)
        assert rang and stg == want and ng == (1 if want * (736 + 2594) >= 2 * 736 * _steps(B, trim) else 0)
        assert torch.equal(yg.view(torch.int64), yp.view(torch.int64))
        # no direct fill (the row tiles of bit 29, the two-pass bind of bit 27): no flags, the stored form, the same product
        for extra in (1 << 29, 1 << 27):
            yv, ranv, nv, stv, _ = _product(S, S.K, ssym, word | extra)
            assert ranv and nv == 0 and stv == 0 and torch.equal(yv.view(torch.int64), yp.view(torch.int64)), hex(extra)


def _entry(S, r, c):
    lo, hi = int(S.rowptr[r]), int(S.rowptr[r + 1])
    k = lo + int(np.searchsorted(S.col[lo:hi], c))
    assert S.col[k] == c
    return k


@pytest.mark.parametrize("B", [1, 2], ids=["B1", "B2"])
def test_one_ulp_unflags_exactly_the_steps_that_hold_it(mf, B):
    """Check 2: K moved by one ulp at (r, c) and (c, r) -- the same ulp: the copy stays symmetric -- with r an interior row of an interior patch in a middle
    swept plane (not the reference row) and c its +plane neighbour (two steps hold r or c) or its +line neighbour in the same patch (one step): the flagged
    count falls by exactly that, an unflagged step runs between flagged ones of the same run, and y stays the plain kernel's bit for bit.  A diagonal entry moved
    by one ulp: y alone (how many steps it unflags depends on how the scaled entries round)."""
    import torch

    S = _system(mf)
    planes, m1, m2 = LAT
    PL = m1 * m2
    r = 8 * PL + 12 * m2 + 40           # plane 8 of the swept [2, 15); line 12: patch rows 8..15 (B = 2), 12..15 (B = 1); point 40: patch column 32..63
    assert r != (2 + 13 // 2) * PL + (32 // 2) * m2 + 128 // 2    # the reference row: centre of the swept region
    word = (B1 if B == 1 else B2) | TRIM | FORCE_CONST
    want = _expected(B, True, 2)

    def moved(pairs):
        Kf_h = S.K_h.copy()
        for a, b in pairs:
            k = _entry(S, a, b)
            Kf_h[k] = np.nextafter(Kf_h[k], np.inf)
            assert Kf_h[k] != S.K_h[k]
        return torch.tensor(Kf_h, device="cuda")

    with SB._lift():
        for c, held in ((r + PL, 2), (r + m2, 1)):
            Kf = moved([(r, c), (c, r)])
            yp, ranp, _, _, _ = _product(S, Kf, S.ssym, PLAIN)
            yc, ranc, nc, steps, _ = _product(S, Kf, S.ssym, word)
            print(f"\nB = {B}: entry ({r}, {c}) moved by an ulp: flagged {steps} (unmoved: {want})")
            assert ranc and not ranp and nc == 1
            assert steps == want - held
            assert torch.equal(yc.view(torch.int64), yp.view(torch.int64))
        Kd = moved([(r, r)])
        yp, _, _, _, _ = _product(S, Kd, S.ssym, PLAIN)
        yc, ranc, _, steps, _ = _product(S, Kd, S.ssym, word)
        print(f"B = {B}: diagonal of row {r} moved by an ulp: flagged {steps}")
        assert ranc and torch.equal(yc.view(torch.int64), yp.view(torch.int64))


@pytest.mark.parametrize("B", [1, 2], ids=["B1", "B2"])
def test_nothing_to_flag_keeps_the_stored_form(mf, B):
    """Check 3: T K T, t in [1, 30] -- no step is flagged and the bind keeps the stored form (the counter stands still); with the constant form forced
    (bit 5) the CS = 1 kernel runs with zero flagged steps and gives the stored form's y bit for bit."""
    import torch

    S = _system(mf)
    word = (B1 if B == 1 else B2) | TRIM
    with SB._lift():
        yp, ranp, _, _, _ = _product(S, S.KT, S.ssymT, PLAIN)
        ys, rans, ns, steps, _ = _product(S, S.KT, S.ssymT, word)
        assert rans and not ranp and ns == 0 and steps == 0
        assert torch.equal(ys.view(torch.int64), yp.view(torch.int64))
        yf, ranf, nf, stepsf, _ = _product(S, S.KT, S.ssymT, word | FORCE_CONST)
        assert ranf and nf == 1 and stepsf == 0
        assert torch.equal(yf.view(torch.int64), ys.view(torch.int64))
        yu, ranu, nu, stepsu, _ = _product(S, S.KT, None, word | FORCE_CONST)   # the unscaled copy, stored diagonal
        yq, _, _, _, _ = _product(S, S.KT, None, PLAIN)
        assert ranu and nu == 1 and stepsu == 0 and torch.equal(yu.view(torch.int64), yq.view(torch.int64))


def _oracle_cg(S, b_h, iters):
    from oracle import solvers

    if "xo" not in _CACHE:
        info = solvers.SolveInfo()
        with np.errstate(all="ignore"):
            xo = solvers.solve_cg_jacobi(S.rowptr, S.col, S.K_h, b_h, 1e-300, iters, max_pass=1, info=info, guard_zero=True)
        _CACHE["xo"] = (xo, info)
    return _CACHE["xo"]


@pytest.mark.parametrize("variant", [4, 1], ids=["v4", "v1"])
def test_cg_on_the_constant_form(mf, variant):
    """Check 4: 60 iterations of cg! with Pr_Jacobi! -- cg_variant 4 on the coded S^-1 A S^-1, variant 1 on the unscaled copy -- x and the solver statistics
    of the constant form are the forced stored form's byte for byte; x matches the oracle's Jacobi CG to 1e-10."""
    import torch
    from metafem_jl_amd import _lib

    S = _system(mf)
    b = KS.mf_rand(S.n)
    iters = 60
    xo, info = _oracle_cg(S, b.cpu().numpy(), iters)
    out = {}
    with SB._lift():
        for word in (B2 | TRIM | FORCE_CONST, B2 | TRIM | FORCE_STORED):
            SB._set_ell(word)
            try:
                s0, (c0, _) = _lib.lib.mfem_debug_sym_spmv_count(), _counts()
                x, st = mf.iterative_Solve(S.A, S.K, b, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=iters, max_pass=1, cg_variant=variant,
                                           fixed_iterations=True)
                torch.cuda.synchronize()
                assert _lib.lib.mfem_debug_sym_spmv_count() > s0
                out[word] = (x.cpu().numpy(), (st.passes, st.iterations, st.final_res, st.initial_res, st.converged, st.spmv_count), _counts()[0] - c0, _counts()[1])
            finally:
                SB._set_ell(0)
    xc, stc, nc, steps = out[B2 | TRIM | FORCE_CONST]
    xs, sts, ns, steps_s = out[B2 | TRIM | FORCE_STORED]
    err = float(np.abs(xc - xo).max() / np.abs(xo).max())
    print(f"\ncg_variant {variant}: err = {err:.3e}, iterations {stc[1]}/{info.iters}, flagged steps {steps}, constant binds {nc} / {ns}")
    assert nc >= 1 and ns == 0 and steps == _expected(2, True, 2 if variant == 4 else 1) and steps_s == 0
    assert xc.tobytes() == xs.tobytes() and repr(stc) == repr(sts)
    assert np.all(np.isfinite(xc))
    assert err <= KS.TOL_X
    assert stc[0] == info.passes == 1 and stc[1] == info.iters


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_on_one_gpu():
    """Check 5: two slabs on cuda:0 through the host-callback communicator, as tests/test_gpu_symp_trim.py runs them (tests/symp_const_worker.py compares
    and reports): every rank's x of the constant-form solve against its own plain-kernel solve."""
    world, port = 2, _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    logs = [tempfile.TemporaryFile() for _ in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "symp_const_worker.py"), str(world), str(r), str(port)], stdout=logs[r],
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
        line = [ln for ln in out.splitlines() if ln.startswith("SYMP_CONST_REPORT ")]
        rep = json.loads(line[-1][len("SYMP_CONST_REPORT "):]) if line else None
        assert p.returncode == 0 and rep is not None and rep["compared"] > 0 and not rep["failed"] and rep["const_binds"] > 0, (
            f"rank {r}: rc={p.returncode}, report {rep}\n--- output tail ---\n" + out[-3000:])
