"""The Jacobi scalings inside a solve, on every solver layout, on matrices whose diagonals are degenerate.

Every other Krylov test runs on FEM matrices whose diagonals are all stored, positive and nonzero, so the guarded rule of csrc/jacobi.hip (a row
without a stored diagonal, or with a stored +-0.0, keeps d = 1) and the scalings folded into the layout binds (dsc, ssym) are only ever seen through
well-behaved values.  Here each case runs k steps (k from the scale tests' _k, converge_tol = 1e-300, max_pass = 1) and is compared with oracle.solvers
run with guard_zero=True, the same seed and shadow vectors: max |x - x_oracle| / max |x_oracle| <= TOL_X = 1e-10, equal iteration and pass counts,
and the SpMV counters must show the layout and sweep the case was written for.

Systems (means of tests/test_gpu_krylov_scale.py: knobs under a context manager, layout_min_rows = (0, 0), the SpMV counters):

  Dz    hex-8 thermal (9, 61, 61), n = 38 440: the stored diagonal set to exactly 0.0 on 1 % of the rows and negated on another 1 % (seeded; the edit
        is symmetric, so the symmetric sweeps accept the values).  One brick serves modes 0, 1, 2 and 3: the workgroup-tile sweep needs 8 chunks of 512
        rows per lattice plane (62 x 62 points) and a run of 4 such planes between the boundary planes, the patch sweep 4 whole planes, and the slot-major
        copy of mode 1 is planned from 13 824 rows on (its padding rule); smaller than every one-field case of
        test_solver_layouts_agree_with_the_csr_kernel_on_odd_shapes but (64, 5, 5), on which neither sweep is planned.
  Dm    the same pattern with the diagonal ENTRY removed from 1 % of the rows, handed over as a caller-supplied CSR (int32 / int64 rowptr, base 0 / 1);
        the values are the assembled ones.  In mode 2 the blocks that hold an edited row are irregular: k_ell_diag's explicit-column branch serves them.
  Tz8   3-field hex-8 elasticity (3, 3, 3), n = 192, and
  Tz27  hex-27 thermal (3, 3, 3), n = 343: the Dz edit (at least 2 rows each) on the smallest bricks of tests/test_gpu_lat8.py / test_gpu_lat27.py --
        the lattice tiles, modes 5 and 4.

Conditions on the inputs, checked on the host with the values one MI355X assembled (_sensitivity and _discrimination below; the asserts in _build
hold in every run):
  * no row and no column of any system is empty (asserted in _build), so no row or column norm is zero;
  * sensitivity -- the oracle's x_k with every value multiplied by 1 +- 2^-52 (seeded signs) against the unperturbed x_k, relative: cg! (k = 3)
    <= 1.7e-14 on every system; bicgstabl(2) (k = 2) <= 6.2e-14 on every system and scaling.  idrs!(4) over TWO cycles exceeded the 1e-12 the
    comparison needs (9.6e-13 on Dz with Pr_Jacobi!, 5.3e-13 with the column norms, but 4.2e-12 on Dz with Pl_Jacobi alone, 3.7e-12 on Dm, 8.9e-12 on
    Tz27 and 1.5e-10 on Tz8, where the device then differed from the oracle by 7.7e-9), so every idrs! case here runs ONE cycle (K_MAX): <= 9.1e-14 then (Tz8;
    8.0e-14 on Dz with the column norms, <= 2.5e-14 elsewhere).  The maximum over all (system, solver, k) used is 9.1e-14;
  * discrimination -- on Dz, Tz8 and Tz27 the oracle with the UNGUARDED rule gives non-finite iterates for every solver and scaling that takes |diag|;
    with d of one non-degenerate row replaced by 1 its x_k moves by 2.2e-2 .. 1.0 relative (cg!, bicgstabl, one-cycle idrs!), at least 2e8 TOL_X.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _scale_module():
    spec = importlib.util.spec_from_file_location("_krylov_scale_means", os.path.join(HERE, "test_gpu_krylov_scale.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KS = _scale_module()
TOL_X, SEED, LIFT = KS.TOL_X, KS.SEED, KS.LIFT
EDIT_SEED = 0x0D1A6



# -- systems --------------------------------------------------------------------------------------------------------------------------------------------
class Sys:
    """Host CSR (base 0, sorted rows) + device values and right-hand side; new_handle(rp, base) makes a pattern handle."""

    def __init__(self, name, ctx, rowptr, col, K_h, new_handle, keep=()):
        import torch

        self.name, self.ctx, self.rowptr, self.col, self.K_h, self.new_handle, self.keep = name, ctx, rowptr, col, K_h, new_handle, keep
        self.n = rowptr.size - 1
        self.K = torch.tensor(K_h, device="cuda")
        self.b = KS.mf_rand(self.n)
        self.b_h = self.b.cpu().numpy()
        self.rows = np.repeat(np.arange(self.n), np.diff(rowptr))
        assert np.diff(rowptr).min() > 0 and np.bincount(col, minlength=self.n).min() > 0   # no empty row, no empty column


def _edit_rows(n):
    """(rows whose diagonal becomes 0.0, rows whose diagonal is negated / -- for Dm -- whose diagonal entry is removed): 1 % each, at least 2."""
    m = max(2, round(0.01 * n))
    pick = np.random.default_rng(EDIT_SEED).choice(n, size=2 * m, replace=False)
    return np.sort(pick[:m]), np.sort(pick[m:])


def _caller_csr(mf, ctx, rowptr, col, n):
    import torch

    def new(rp="int64", base=0):
        return mf.FEM_SpMat_CSR(torch.tensor((rowptr + base).astype(rp), device="cuda"), torch.tensor((col + base).astype(np.int32), device="cuda"),
                                n, index_base=base, ctx=ctx)
    return new


def _build(mf, name):
    if name in ("Dz", "Dm"):
        b = mf.make_Brick((1.0, 1.0, 1.0), (9, 61, 61))
        A = b.pattern(1)
        K = b.assemble_thermal(A, KS.K_COND, KS.H, KS.TENV, 0x3F)
    elif name == "Tz8":
        b = mf.make_Brick((1.0, 0.7, 1.3), (3, 3, 3), 1, 3)
        A = b.pattern(3)
        K = b.assemble_elasticity(A, KS.LAM, KS.MU, KS.TAU, KS.X0)
    elif name == "Tz27":
        b = mf.make_Brick((1.0, 1.0, 1.0), (3, 3, 3), 2, 5)
        A = b.pattern(1)
        K = b.assemble_thermal(A, KS.K_COND, KS.H, KS.TENV, 0x3F)
    else:
        raise KeyError(name)
    nf = 3 if name == "Tz8" else 1
    rowptr = A.rowptr.cpu().numpy().astype(np.int64) - A.index_base
    col = A.colidx.cpu().numpy().astype(np.int32) - A.index_base
    K_h = K.cpu().numpy().copy()
    n = A.n
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    dslot = np.flatnonzero(rows == col)
    assert dslot.size == n and np.all(K_h[dslot] != 0.0)   # the assembly stores every diagonal, none of them zero
    first, second = _edit_rows(n)
    if name == "Dm":
        keep = np.ones(col.size, dtype=bool)
        keep[dslot[second]] = False
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64)
        col, K_h = col[keep], K_h[keep]
        return Sys(name, b.ctx, rowptr, col, K_h, _caller_csr(mf, b.ctx, rowptr, col, n), keep=(b,))
    K_h[dslot[first]] = 0.0
    K_h[dslot[second]] = -K_h[dslot[second]]
    return Sys(name, b.ctx, rowptr, col, K_h, lambda rp="int64", base=0: b.pattern(nf), keep=(b,))


@pytest.fixture(scope="module")
def systems(mf):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _build(mf, name)
        return cache[name]

    yield get
    cache.clear()


# -- the oracle -----------------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_x(rowptr, col, K_h, b_h, solver, s, k, pr, pl, guard=True, jacobi=None):
    """x_k and SolveInfo of oracle.solvers with the device call's arguments.  jacobi: a replacement for solvers.jacobi_by_diagonal (discrimination)."""
    from oracle import solvers

    info = solvers.SolveInfo()
    maxiter = KS._maxiter(solver, s, k)
    jd0 = solvers.jacobi_by_diagonal
    if jacobi is not None:
        solvers.jacobi_by_diagonal = jacobi
    try:
        with np.errstate(all="ignore"):
            if solver == "cg":
                assert pr == "jacobi" and pl is None
                x = solvers.solve_cg_jacobi(rowptr, col, K_h, b_h, 1e-300, maxiter, max_pass=1, info=info, guard_zero=guard)
            else:
                sv = {"bicgstabl": solvers.bicgstabl_gs, "idrs": solvers.idrs}[solver]
                prf = {None: None, "jacobi": lambda A: solvers.pr_jacobi(A, guard_zero=guard),
                       "colnorm": lambda A: solvers.pr_jacobi(A, normalized_by_column=True)}[pr]
                plf = {None: None, "diag": lambda A: solvers.pl_jacobi(A, guard_zero=guard),
                       "rownorm": lambda A: solvers.pl_jacobi(A, normalized_by_row=True)}[pl]
                x = solvers.iterative_solve(rowptr, col, K_h, b_h, 1e-300, Sv_func=sv, Pr_func=prf, Pl_func=plf, max_pass=1, maxiter=maxiter, s=s,
                                            seed=SEED, info=info)
    finally:
        solvers.jacobi_by_diagonal = jd0
    return x, info


def _oracle(S, case):
    key = (S.name, case.solver, case.s, case.k, case.pr, case.pl)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_x(S.rowptr, S.col, S.K_h, S.b_h, *key[1:])
    return _ORACLE[key]


def _sensitivity(S, case):
    """max |x_k(K (1 +- 2^-52)) - x_k(K)| / max |x_k(K)|, seeded signs."""
    x0, _ = _oracle(S, case)
    sign = np.where(np.random.default_rng(EDIT_SEED + 1).random(S.K_h.size) < 0.5, -1.0, 1.0)
    x1, _ = _oracle_x(S.rowptr, S.col, S.K_h * (1.0 + sign * 2.0 ** -52), S.b_h, case.solver, case.s, case.k, case.pr, case.pl)
    return float(np.abs(x1 - x0).max() / np.abs(x0).max())


def _discrimination(S, case):
    """(are the unguarded oracle's iterates finite?, relative move of x_k when d of one non-degenerate row is replaced by 1)."""
    from oracle import solvers

    x0, _ = _oracle(S, case)
    try:
        xu, _ = _oracle_x(S.rowptr, S.col, S.K_h, S.b_h, case.solver, case.s, case.k, case.pr, case.pl, guard=False)
    except ValueError:   # (scipy's triangular solve of idrs! refuses the non-finite coefficients)
        xu = np.full(S.n, np.nan)
    jd = solvers.jacobi_by_diagonal
    first, second = _edit_rows(S.n)
    row = int(np.setdiff1d(np.arange(S.n), np.concatenate([first, second]))[S.n // 3])

    def one_wrong(A, guard_zero=False):
        d = jd(A, guard_zero)
        d[row] = 1.0
        return d

    x1, _ = _oracle_x(S.rowptr, S.col, S.K_h, S.b_h, case.solver, case.s, case.k, case.pr, case.pl, jacobi=one_wrong)
    return bool(np.all(np.isfinite(xu))), float(np.abs(x1 - x0).max() / np.abs(x0).max())


K_MAX = {"idrs": 1}


# -- one case -------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, sysname, solver, s=0, pr="jacobi", pl=None, cg_variant=0, knobs=None, expect=(), fmt=("int64", 0)):
        # k from the scale tests' _k, but ONE cycle for idrs!: over two cycles the oracle itself moves by up to 1.5e-10 under a 2^-52 perturbation of
        # these values (Tz8; 8.9e-12 on Tz27, 4.2e-12 on Dz with the left scaling alone, 3.7e-12 on Dm), more than the 1e-12 the comparison allows
        self.sysname, self.solver, self.s, self.k, self.pr, self.pl = sysname, solver, s, min(KS._k(solver, s), K_MAX.get(solver, 99)), pr, pl
        self.cg_variant, self.knobs, self.expect, self.fmt = cg_variant, dict(knobs or {}), set(expect), fmt
        kn = ",".join(f"{a}={b}" for a, b in self.knobs.items())
        self.id = f"{sysname}-{solver}{s or ''}-v{cg_variant}-{pr}-{pl}" + (f"-[{kn}]" if kn else "") + (f"-{fmt[0]}-base{fmt[1]}" if sysname == "Dm" else "")


RAN = {}


def _run_case(mf, systems, case):
    import torch
    from metafem_jl_amd import _lib

    S = systems(case.sysname)
    lib = _lib.lib
    with KS._knobs(**case.knobs):
        A = S.new_handle(*case.fmt)   # (a fresh pattern: some knobs are read when a pattern's layout is planned)
        mode, padded, regular, ent, sym = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(lib.mfem_csr_solver_layout(S.ctx._h, A._h, C.byref(mode), None, C.byref(padded), C.byref(regular)))
        _lib.check(lib.mfem_csr_solver_layout_entries(S.ctx._h, A._h, C.byref(ent), C.byref(sym)))
        kw = dict(Sv_func=getattr(mf, KS.SOLVERS[case.solver]),
                  Pr_func={None: mf.Identity, "jacobi": mf.Pr_Jacobi_, "colnorm": mf.Pr_Jacobi_colnorm_}[case.pr],
                  Pl_func={None: mf.Identity, "diag": mf.Pl_Jacobi_, "rownorm": mf.Pl_Jacobi_rownorm_}[case.pl],
                  maxiter=KS._maxiter(case.solver, case.s, case.k), max_pass=1, s=case.s, seed=SEED, cg_variant=case.cg_variant,
                  fixed_iterations=case.solver == "cg")
        c0 = KS._counters(lib)
        x, st = mf.iterative_Solve(A, S.K, S.b, 1e-300, **kw)
        torch.cuda.synchronize()
        c1 = KS._counters(lib)
    d = {key: c1[key] - c0[key] for key in c0}
    xd = x.cpu().numpy()
    xo, info = _oracle(S, case)
    err = float(np.abs(xd - xo).max() / np.abs(xo).max())
    tags = set()
    if d["lat27"] > 0:
        tags.add("mode4")
    elif d["lat8"] > 0:
        tags.add("mode5")
    else:
        tags.add(f"mode{mode.value}")
        if mode.value == 2:
            tags.add({1: "sym_sweep", 2: "symp"}.get(sym.value, "sym?") if d["sym"] > 0 else "plain")
            if 0 < regular.value < padded.value:
                tags.add("irregular_blocks")
    print(f"\n{case.id}: n={S.n} served={sorted(tags)} regular={regular.value}/{padded.value} d={d} err={err:.3e} it={st.iterations}/{info.iters} "
          f"passes={st.passes}/{info.passes}")
    RAN[case.id] = tags
    assert case.expect <= tags, (case.id, sorted(tags))
    assert np.all(np.isfinite(xd))
    assert err <= TOL_X, (case.id, err)
    assert st.passes == info.passes == 1
    assert st.iterations == info.iters, (st.iterations, info.iters)


# -- the cases ------------------------------------------------------------------------------------------------------------------------------------------
NOT5 = dict(LIFT, lat8=0)   # one field: idrs! / bicgstabl_GS! with Pr_Jacobi! would take the tiles of mode 5 once the size limits are lifted
M2 = dict(NOT5)                                # mode 2, the kernel the bind chooses: the patch sweep where the values are symmetric
M2_PLAIN = dict(NOT5, ell=1 | 1 << 22)         # ... with the symmetric sweeps off
M2_TILE = dict(NOT5, ell=1 | 1 << 23)          # ... with the workgroup-tile sweep
M1 = dict(NOT5, ell=3)
M3 = dict(NOT5, ell=0)
KRY = [("idrs", 4), ("bicgstabl", 2)]

CASES = []
# cg! with Pr_Jacobi! (|diag| taken by k_jacobi_diag_table on mode 0 / 3, by k_ell_diag from the bound copy on modes 1 / 2)
CASES += [Case("Dz", "cg", expect={"mode0"}), Case("Dz", "cg", knobs=M2_PLAIN, expect={"mode2", "plain"}),
          Case("Dz", "cg", knobs=M2_TILE, expect={"mode2", "sym_sweep"}), Case("Dz", "cg", knobs=M2, expect={"mode2", "symp"}),
          Case("Dz", "cg", knobs=M1, expect={"mode1"}), Case("Dz", "cg", knobs=M3, expect={"mode3"})]
# the CG variants on mode 2: 1-3 read k_ell_diag, 4 runs on the symmetrically scaled copy (ssym in the DIA bind)
CASES += [Case("Dz", "cg", cg_variant=v, knobs=M2, expect={"mode2", "symp"}) for v in (1, 2, 3, 4)]
CASES += [Case("Dz", "cg", cg_variant=v, knobs=M2_PLAIN, expect={"mode2", "plain"}) for v in (3, 4)]
CASES += [Case("Dz", "cg", cg_variant=4, knobs=M2_TILE, expect={"mode2", "sym_sweep"})]
# k_ell_diag's padding-slot case: rows without a diagonal entry
CASES += [Case("Dm", "cg", knobs=M1, expect={"mode1"}, fmt=("int32", 0)), Case("Dm", "cg", knobs=M2, expect={"mode2", "irregular_blocks"}, fmt=("int64", 1)),
          Case("Dm", "cg", cg_variant=4, knobs=M2, expect={"mode2", "irregular_blocks"}, fmt=("int32", 0))]
# the scaling folded into each bind (dsc)
for _sv, _s in KRY:
    CASES += [Case("Dz", _sv, _s, expect={"mode0"}), Case("Dz", _sv, _s, knobs=M2, expect={"mode2"}), Case("Dz", _sv, _s, knobs=M1, expect={"mode1"}),
              Case("Dz", _sv, _s, knobs=M3, expect={"mode3"})]
    CASES += [Case("Dm", _sv, _s, expect={"mode0"}, fmt=("int32", 1)), Case("Dm", _sv, _s, knobs=M1, expect={"mode1"}, fmt=("int64", 0)),
              Case("Dm", _sv, _s, knobs=M2, expect={"mode2", "irregular_blocks"}, fmt=("int32", 0)),
              Case("Dm", _sv, _s, knobs=M3, expect={"mode3"}, fmt=("int32", 1))]
    CASES += [Case("Tz8", _sv, _s, knobs=LIFT, expect={"mode5"}), Case("Tz27", _sv, _s, knobs=LIFT, expect={"mode4"})]
CASES += [Case("Tz8", "cg", knobs=LIFT, expect={"mode5"}), Case("Tz27", "cg", knobs=LIFT, expect={"mode4"})]
# column norms as the right scaling
CASES += [Case("Dz", "idrs", 4, pr="colnorm", expect={"mode0"}), Case("Dz", "idrs", 4, pr="colnorm", knobs=M2, expect={"mode2"}),
          Case("Dz", "idrs", 4, pr="colnorm", knobs=M3, expect={"mode3"})]
# left scalings (mfem_mat_div_rows on the working copy: int64 / base 0 on Dz, int32 and base 1 on Dm), with and without the right one
for _sv, _s, _pl in (("idrs", 4, "diag"), ("bicgstabl", 2, "rownorm")):
    for _pr in ("jacobi", None):
        CASES += [Case("Dz", _sv, _s, pr=_pr, pl=_pl, expect={"mode0"}), Case("Dz", _sv, _s, pr=_pr, pl=_pl, knobs=M2, expect={"mode2"}),
                  Case("Dm", _sv, _s, pr=_pr, pl=_pl, expect={"mode0"}, fmt=("int32", 1) if _sv == "idrs" else ("int64", 1)),
                  Case("Dm", _sv, _s, pr=_pr, pl=_pl, knobs=M2, expect={"mode2", "irregular_blocks"}, fmt=("int32", 0))]

REQUIRED = {"mode0", "mode1", "mode2", "mode3", "mode4", "mode5", "plain", "sym_sweep", "symp", "irregular_blocks"}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_scaled_solves_match_the_guarded_oracle(mf, systems, case):
    _run_case(mf, systems, case)


def test_every_layout_served_a_case(mf, systems):
    """Independent of test selection: the cases the session did not run are run here first."""
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        if c.id not in RAN:
            _run_case(mf, systems, c)
    ran = set().union(*RAN.values())
    assert REQUIRED <= ran, sorted(REQUIRED - ran)


@pytest.mark.parametrize("sysname,fmt", [("Dz", ("int64", 0)), ("Dm", ("int32", 1)), ("Dm", ("int64", 0))])
def test_scale_in_place_leaves_the_scaled_values(mf, systems, sysname, fmt):
    """scale_in_place with Pr_Jacobi! and Pl_Jacobi on the CSR path: the caller's values become (K / d[col]) / dl[row] bit for bit, d from K and dl from
    the column-scaled matrix (left_precond), both by the guarded rule."""
    import scipy.sparse as sp
    import torch
    from oracle import solvers

    S = systems(sysname)
    A = S.new_handle(*fmt)
    K = S.K.clone()
    x, st = mf.iterative_Solve(A, K, S.b, 1e-300, Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, Pl_func=mf.Pl_Jacobi_, maxiter=KS._maxiter("idrs", 4, 1),
                               max_pass=1, s=4, seed=SEED, scale_in_place=True)
    torch.cuda.synchronize()
    M = sp.csr_matrix((S.K_h.copy(), S.col, S.rowptr), shape=(S.n, S.n))
    d = solvers.jacobi_by_diagonal(M, guard_zero=True)
    M.data = M.data / d[S.col]
    dl = solvers.jacobi_by_diagonal(M, guard_zero=True)
    first, second = _edit_rows(S.n)
    assert np.all(d[first if sysname == "Dz" else second] == 1.0) and np.count_nonzero(d == 1.0) == first.size
    assert np.array_equal(K.cpu().numpy(), M.data / dl[S.rows])
    assert np.array_equal(S.K.cpu().numpy(), S.K_h)   # (the system's own values were not touched)
