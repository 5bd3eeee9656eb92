"""The schedule of the patch sweep's runs and its per-run p . Ap sums (csrc/symp_sched_decide.h; k_spmv_symp_const<B, DC, SCH> walks a table of run ids, both
kernels store one partial sum per run).  A run's sum is formed by the wave that sweeps it, from zero, in step order, and stored at partials[run id]; the tail
and rim units keep one sum per workgroup behind the runs'.  So y, the array of partial sums and every CG iterate must be the same BIT FOR BIT whichever wave
sweeps which run: under the decision's own schedule (mode 0 of the "symp_sched" knob), the identity schedule (1), two seeds of the pseudo-random one (2),
and between the forced constant (bit 5 of the "ell" knob) and the forced stored form (bit 4), which always runs the identity schedule.

Conventions and first fixture of tests/test_gpu_symp_const.py: layout_min_rows = (0, 0), bands by bits 24 / 25, the trim by bit 3, bit 22 the plain per-row
kernel; the assembled thermal K with Robin terms on all six faces, h = 2^-7 in every direction.
  (17, 33, 129) on sides (0.125, 0.25, 1.0): 13 swept planes, one run per patch, 16 patches for B = 2 (32 for B = 1), 72 369 rows
  (49, 33, 129) on sides (0.375, 0.25, 1.0): 45 swept planes, two runs per patch (run boundaries inside the sweep), 208 593 rows
The grid is capped at 8 workgroups (second argument of the knob) so that every wave sweeps several runs: one wave per XCD, whose list the schedules cut
(shares by cost against equal shares) and order differently.  Uncapped, the small lattices have a wave per run; the runs' sums must still be the same bytes.

CG: x against the oracle's Jacobi CG to the 1e-10 of tests/test_gpu_symp_const.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
B1, B2, PLAIN = 1 << 24, 1 << 25, 1 << 22
TRIM, FORCE_STORED, FORCE_CONST = 1 << 3, 1 << 4, 1 << 5
SP_L, SP_W = 4, 32
CAP = 8
AUTO, IDENTITY, RANDOM_A, RANDOM_B = 0, 1, 2 | (1 << 8), 2 | (2 << 8)
MODES = [AUTO, IDENTITY, RANDOM_A, RANDOM_B]
FIXTURES = {"one_run": ((17, 33, 129), (0.125, 0.25, 1.0), 13, 1), "two_runs": ((49, 33, 129), (0.375, 0.25, 1.0), 45, 2)}  # lattice, sides, swept planes, runs per patch
# 16 x 34 patches of 4 lines (B = 1) = 544 runs on 8 workgroups: at least one list holds 68 runs, more than the 64 run ids of one gathered load
LONG = {"long_lists": ((17, 65, 1089), (0.125, 0.5, 8.5), 13, 1)}
EPS = 2.0 ** -52


def _bands_module():
    spec = importlib.util.spec_from_file_location("_symp_bands_for_sched", os.path.join(HERE, "test_gpu_symp_bands.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SB = _bands_module()
KS = SB.KS


class Sys:
    pass


_CACHE = {}


def _system(mf, name):
    """Brick, pattern, K, 1 / sqrt|a_ii|, x, b -- made once per fixture, never changed."""
    import torch

    if name in _CACHE:
        return _CACHE[name]
    lat, sides, planes, nseg = {**FIXTURES, **LONG}[name]
    S = Sys()
    S.lat, S.planes, S.nseg = lat, planes, nseg
    S.brick = mf.make_Brick(sides, tuple(v - 1 for v in lat))
    S.A = S.brick.pattern(1)
    S.n = n = S.A.n
    assert n == lat[0] * lat[1] * lat[2]
    S.rowptr = S.A.rowptr.cpu().numpy().astype(np.int64) - S.A.index_base
    S.col = S.A.colidx.cpu().numpy().astype(np.int32) - S.A.index_base
    S.K = S.brick.assemble_thermal(S.A, KS.K_COND, KS.H, KS.TENV, 0x3F)
    S.K_h = S.K.cpu().numpy()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (S.A.rowptr[1:] - S.A.rowptr[:-1]).long())
    cols = S.A.colidx.long() - int(S.A.index_base)
    diag = torch.nonzero(cols == rows).flatten()
    assert diag.numel() == n
    S.ssym = torch.tensor(1.0 / np.sqrt(np.abs(S.K[diag].cpu().numpy())), device="cuda")
    S.x = mf.FEM_rand(n, 5, 0) - 0.5
    S.y0 = mf.FEM_rand(n, 7, 0) - 0.5
    S.b = KS.mf_rand(n)
    _CACHE[name] = S
    return S


def _nruns(S, B):
    """runs of the trimmed sweep by geometry: whole patches of 4 B lines x 32 points, times the runs per patch"""
    _, m1, m2 = S.lat
    return (m1 // (SP_L * B)) * (m2 // SP_W) * S.nseg


def _set_sched(a, cap):
    from metafem_jl_amd import _lib

    _lib.check(_lib.lib.mfem_debug_set(b"symp_sched", int(a), int(cap)))


def _counts():
    from metafem_jl_amd import _lib

    return int(_lib.lib.mfem_debug_symp_const_count()), int(_lib.lib.mfem_debug_symp_sched_count()), int(_lib.lib.mfem_debug_sym_spmv_count())


def _product(S, word, mode, cap, alpha=1.0, beta=0.0):
    """(y bytes, partial sums, [constant binds, schedule tables built, sweep launches]) of one product of the scaled layout with the fused x . y"""
    import torch
    from metafem_jl_amd import _lib

    SB._set_ell(word)
    _set_sched(mode, cap)
    try:
        y = S.y0.clone()
        part = np.zeros(4096, dtype=np.float64)
        npart, form = C.c_int32(0), C.c_int32(-7)
        c0 = _counts()
        _lib.check(_lib.lib.mfem_debug_spmv_scaled_layout(S.brick.ctx._h, S.A._h, S.K.data_ptr(), S.ssym.data_ptr(), S.x.data_ptr(), y.data_ptr(), alpha, beta,
                                                          S.x.data_ptr(), part.ctypes.data, 4096, C.byref(npart), C.byref(form)))
        torch.cuda.synchronize()
        c1 = _counts()
        return y.cpu().numpy(), part[:npart.value].copy(), [b - a for a, b in zip(c0, c1)]
    finally:
        SB._set_ell(0)
        _set_sched(0, 0)


CASES = [(f, b) for f in FIXTURES for b in (1, 2)]


@pytest.mark.parametrize("fixture,B", CASES, ids=[f"{f}-B{b}" for f, b in CASES])
def test_every_schedule_gives_the_same_bytes(mf, fixture, B):
    """y = the plain kernel's and the partial sums are one array of bytes under modes 0, 1 and 2 (two seeds) of the constant form and in the stored form; the
    sums are per run (their count is runs + workgroups) and add up to x . y; without the cap the runs' sums are still the same bytes."""
    S = _system(mf, fixture)
    base = (B1 if B == 1 else B2) | TRIM
    nruns = _nruns(S, B)
    with SB._lift():
        assert SB._sweep_planned(S)
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
            yp, _, cp = _product(S, PLAIN, AUTO, CAP, alpha, beta)
            assert cp[2] == 0
            ref = None
            for mode in MODES:
                y, part, c = _product(S, base | FORCE_CONST, mode, CAP, alpha, beta)
                print(f"\n{fixture} B = {B} ({alpha}, {beta}) mode {mode:#x}: {part.size} partial sums ({nruns} runs), binds/tables/launches {c}")
                assert c[0] == 1 and c[2] == 1 and c[1] == (0 if mode == IDENTITY else 1)
                assert part.size == nruns + CAP
                assert y.tobytes() == yp.tobytes()
                if ref is None:
                    ref = part
                assert part.tobytes() == ref.tobytes(), f"mode {mode:#x}"
            for mode in (AUTO, RANDOM_A):   # the stored form has no flags to schedule by: the identity schedule whatever the knob says
                ys, parts, cs = _product(S, base | FORCE_STORED, mode, CAP, alpha, beta)
                assert cs[0] == 0 and cs[1] == 0 and cs[2] == 1
                assert ys.tobytes() == yp.tobytes() and parts.tobytes() == ref.tobytes()
            # the sums add up to x . y: two n-term sums in different orders (the bound of tests/test_gpu_symp_bands.py)
            x_h = S.x.cpu().numpy()
            assert abs(ref.sum() - float(x_h @ yp)) <= S.n * EPS * np.linalg.norm(x_h) * np.linalg.norm(yp)
            # no cap: more workgroups, other lists, the same sums per run; the rows outside the swept planes in a launch of their own (bit 26): the same again
            for word, cap in ((base | FORCE_CONST, 0), (base | FORCE_CONST | (1 << 26), CAP), (base | FORCE_STORED | (1 << 26), 0)):
                yu, partu, _ = _product(S, word, AUTO, cap, alpha, beta)
                assert yu.tobytes() == yp.tobytes() and partu.size > nruns and partu[:nruns].tobytes() == ref[:nruns].tobytes(), (hex(word), cap)


def test_lists_longer_than_one_gathered_load(mf):
    """544 runs under the cap of 8 workgroups: whatever the schedule, some wave's list is longer than 64 runs, so the sweep refills its run ids from the table
    in mid-list (the decision's own schedule and both seeds).  y = the plain kernel's, the sums per run are one array of bytes under every mode and in the
    stored form, and the sums add up to x . y."""
    S = _system(mf, "long_lists")
    base = B1 | TRIM
    nruns = _nruns(S, 1)
    assert nruns == 544 and nruns > 64 * CAP
    with SB._lift():
        assert SB._sweep_planned(S)
        yp, _, cp = _product(S, PLAIN, AUTO, CAP)
        assert cp[2] == 0
        ys, ref, cs = _product(S, base | FORCE_STORED, AUTO, CAP)
        assert cs[2] == 1 and cs[1] == 0 and ref.size == nruns + CAP and ys.tobytes() == yp.tobytes()
        for mode in MODES:
            y, part, c = _product(S, base | FORCE_CONST, mode, CAP)
            assert c[0] == 1 and c[2] == 1 and c[1] == (0 if mode == IDENTITY else 1), (hex(mode), c)
            assert y.tobytes() == yp.tobytes() and part.size == nruns + CAP and part.tobytes() == ref.tobytes(), hex(mode)
        x_h = S.x.cpu().numpy()
        assert abs(ref.sum() - float(x_h @ yp)) <= S.n * EPS * np.linalg.norm(x_h) * np.linalg.norm(yp)


def _oracle_cg(S, iters):
    from oracle import solvers

    if not hasattr(S, "xo"):
        info = solvers.SolveInfo()
        with np.errstate(all="ignore"):
            S.xo = solvers.solve_cg_jacobi(S.rowptr, S.col, S.K_h, S.b.cpu().numpy(), 1e-300, iters, max_pass=1, info=info, guard_zero=True)
        S.info = info
    return S.xo, S.info


@pytest.mark.parametrize("fixture", list(FIXTURES))
def test_cg_under_every_schedule(mf, fixture):
    """60 iterations of cg! with Pr_Jacobi! (cg_variant 4, B = 2 and B = 1): x and the statistics are the same bytes under modes 0, 1 and 2 of the constant form,
    in the stored form, and in a second solve under mode 0; x matches the oracle's Jacobi CG to 1e-10."""
    import torch
    from metafem_jl_amd import _lib

    S = _system(mf, fixture)
    iters = 60
    xo, info = _oracle_cg(S, iters)
    with SB._lift():
        for bands in (B2, B1):
            out = []
            for word, mode in [(FORCE_CONST, m) for m in MODES] + [(FORCE_CONST, AUTO), (FORCE_STORED, AUTO)]:
                SB._set_ell(bands | TRIM | word)
                _set_sched(mode, CAP)
                try:
                    c0 = _counts()
                    x, st = mf.iterative_Solve(S.A, S.K, S.b, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=iters, max_pass=1, cg_variant=4,
                                               fixed_iterations=True)
                    torch.cuda.synchronize()
                    c = [b - a for a, b in zip(c0, _counts())]
                    assert c[2] > 0 and (c[0] >= 1) == (word == FORCE_CONST) and (c[1] >= 1) == (word == FORCE_CONST and mode != IDENTITY), (hex(word), mode, c)
                    out.append((x.cpu().numpy(), repr((st.passes, st.iterations, st.final_res, st.initial_res, st.converged, st.spmv_count))))
                finally:
                    SB._set_ell(0)
                    _set_sched(0, 0)
            x0, st0 = out[0]
            err = float(np.abs(x0 - xo).max() / np.abs(xo).max())
            print(f"\n{fixture} bands {bands:#x}: err = {err:.3e}, {st0}")
            for k, (x, st) in enumerate(out[1:], 1):
                assert x.tobytes() == x0.tobytes() and st == st0, f"solve {k}"
            assert np.all(np.isfinite(x0)) and err <= KS.TOL_X
            assert st0.startswith(f"({info.passes}, {info.iters},") and info.passes == 1
