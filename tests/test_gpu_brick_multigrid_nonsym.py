"""GPU: the multigrid V-cycle on hex-8 thermal bricks WITH Nitsche (fixed_faces) faces -- the nonsymmetric hierarchy of
mfem_brick_multigrid_create_nonsymmetric -- and right-preconditioned restarted GMRES with it (gmres_ + Pr_Multigrid_, csrc/krylov_gmres_mg.hip).

The twin is the Twin of tests/test_gpu_brick_multigrid.py with problems.thermal_fixed on the fixed faces of every level and lambda_max per level taken
from the device's info; its solver is right-preconditioned GMRES(s) with the residual estimate tested at every step.  Constants: k = 0.6, itg 3 unless
said otherwise, h = 25 on the Robin faces, Tw = 1173.15.

Rows (MG / Jacobi steps of a CPU twin at 1e-8 |b| / sqrt(n), b = A uniform(-1, 1) seed 3, distorted bricks):
  0  unit 8^3, Robin 0,1,2,3,5, fixed 4, h_penalty 1000            3 levels   8 / 30
  1  unit 16^3, the same faces                                     4 levels   9 / 46
  2  (1,1.5,.75) 16x24x12, Robin 1,2,3, fixed 0,4, h_penalty 1000  3 levels   8 / 58
  3  unit 16^3, all six fixed, h_penalty 1e5                       4 levels   9 / 35
  4  unit 16^3, Robin 5, fixed 4, h_penalty 10                     4 levels   5 / 95
  5  unit 32^3, faces of row 0                                     5 levels   8 / 96
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_brick_multigrid import NU, NU_C, Twin, _bits, _distort, interpolation, plan

pytestmark = pytest.mark.gpu

K_COND, TENV, TW, H_ROBIN = 0.6, 293.15, 1173.15, 25.0
XB, XU = (1.0, 1.5, 0.75), (1.0, 1.0, 1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brick_multigrid_nonsym_sha256.json")


def _dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


# ---- what must not move: computed by code that exists before and after the nonsymmetric hierarchy ---------------------------------------------------
def unmoved_digests(mf):
    """SHA-256 of a symmetric thermal hierarchy's apply(r) and cg_ solve at 32^3 and 33^3 (five levels / one level) and of plain gmres_ solves on a
    small Nitsche operator.  tests/golden/brick_multigrid_nonsym_sha256.json holds them as the commit before the nonsymmetric hierarchy gave them."""
    out = {}
    for n in (32, 33):
        brick = mf.make_Brick(XU, (n, n, n), 1, 3)
        op = brick.thermal_operator(K_COND, H_ROBIN, TENV, 0x3F)
        mg = op.multigrid().setup()
        r = _dev(np.random.default_rng(5).uniform(-1.0, 1.0, op.n))
        b = _dev(np.random.default_rng(3).uniform(-1.0, 1.0, op.n))
        out[f"apply_{n}"] = _sha(mg.apply(r))
        tol = 1e-8 * float(b.norm()) / np.sqrt(op.n)
        x, st = mf.iterative_Solve(op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)
        assert st.converged == 1
        out[f"cg_{n}"] = _sha(x)
        mg.close()
        op.close()
    brick = mf.make_Brick(XU, (6, 5, 4), 1, 3)
    nit = brick.thermal_operator(K_COND, H_ROBIN, TENV, 0x2F, fixed_faces=0x10, h_penalty=1000.0, Tw=TW)
    b = _dev(np.random.default_rng(3).uniform(-1.0, 1.0, nit.n))
    for name, pr, s in (("gmres_jacobi", mf.Pr_Jacobi_, 0), ("gmres_identity_s7", 0, 7)):
        x, st = mf.iterative_Solve(nit, None, b, 1e-10, Sv_func=mf.gmres_, Pr_func=pr, maxiter=400, max_pass=5, s=s)
        assert st.converged == 1
        out[name] = _sha(x)
    nit.close()
    return out


def test_what_must_not_move(mf):
    want = json.load(open(GOLDEN))
    got = unmoved_digests(mf)
    assert got == want


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------------------
R5 = [0, 1, 2, 3, 5]
# x, n, Robin faces, fixed faces, h_penalty
ROWS = [
    (XU, (8, 8, 8), R5, [4], 1000.0),
    (XU, (16, 16, 16), R5, [4], 1000.0),
    (XB, (16, 24, 12), [1, 2, 3], [0, 4], 1000.0),
    (XU, (16, 16, 16), [], [0, 1, 2, 3, 4, 5], 1e5),
    (XU, (16, 16, 16), [5], [4], 10.0),
    (XU, (32, 32, 32), R5, [4], 1000.0),
]
ROW_IDS = ["8", "16", "16x24x12", "16-six-fixed", "16-hp10", "32"]
SMALLEST = (XU, (4, 4, 4), R5, [4], 1000.0)     # the smallest brick with two levels
TWO_LEVELS = (XB, (6, 10, 14), [1, 2, 3], [4], 1000.0)
ONE_LEVEL = (XU, (9, 14, 15), R5, [4], 1000.0)  # the coarse Chebyshev alone


def oracle_level(x, n, itg, coords, robin, fixed, hp):
    """K of one level on the given coordinates: tests/test_gpu_brick_multigrid.py's, with problems.thermal_fixed on the fixed faces"""
    import scipy.sparse as sp
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    msh.coords[:] = coords
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = []
    if robin:
        bnd.append((fac.select(np.isin(fac.element_eindex, robin)), problems.thermal_convection(H_ROBIN, TENV)))
    if fixed:
        bnd.append((fac.select(np.isin(fac.element_eindex, fixed)), problems.thermal_fixed(3, hp, TW, K_COND)))
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, K_COND), bnd)
    od.controlpoints["s"] = np.zeros(msh.ncp)
    od.update_time()
    od.K_linear_func()
    return sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)


class NTwin(Twin):
    """The Twin with the Nitsche rows on every level (A_l = -K_l is no longer symmetric) and right-preconditioned restarted GMRES in place of PCG."""

    def __init__(self, x, n, itg, robin, fixed, hp, max_levels=12):
        from oracle import mesh as om, reference_element as re_

        self.levels = plan(n, max_levels)
        disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
        c = _distort(om.lattice_mesh(x, n, disc).coords.copy())
        self.coords, self.A, self.dinv, self.P, self.K = [], [], [], [], []
        for l, ne in enumerate(self.levels):
            if l:
                pf = self.levels[l - 1]
                c = c.reshape(pf[0] + 1, pf[1] + 1, pf[2] + 1, 3)[::2, ::2, ::2].reshape(-1, 3).copy()
            K = oracle_level(x, ne, itg, c, robin, fixed, hp)
            d = K.diagonal()
            assert (d < 0).all()
            self.coords.append(c)
            self.K.append(K)
            self.A.append((-K).tocsr())
            self.dinv.append(1.0 / np.abs(d))
            if l:
                self.P.append(interpolation(ne))
        self.lam = None

    def asymmetry(self):
        A = self.A[0]
        return float(abs(A - A.T).max() / abs(A).max())

    def gmres(self, b, tol, s=20, maxiter=200, fixed=False, x0=None, **kw):
        """A M^-1 u = b, x = M^-1 u, M^-1 = the cycle; CGS2; the estimate |g_(k+1)| tested at every step, the true residual at the end of a restart
        -> (x, steps, restarts, |b - A x| / sqrt(n))"""
        A, n = self.A[0], b.size
        M = lambda v: self.cycle(v, **kw)
        nrm = lambda v: float(np.linalg.norm(v)) / np.sqrt(n)
        x = np.zeros(n) if x0 is None else x0.copy()
        r = b - A @ x
        it = restarts = 0
        if nrm(r) == 0.0 or (not fixed and nrm(r) <= tol) or maxiter <= 0:
            return x, 0, 0, nrm(r)
        while True:
            beta = float(np.linalg.norm(r))
            Q = np.zeros((n, s + 1))
            H = np.zeros((s + 1, s))
            Q[:, 0] = r / beta
            width = 0
            for k in range(s):
                w = A @ M(Q[:, k])
                for _ in range(2):
                    h = Q[:, :k + 1].T @ w
                    w = w - Q[:, :k + 1] @ h
                    H[:k + 1, k] += h
                H[k + 1, k] = np.linalg.norm(w)
                if H[k + 1, k] > 0.0:
                    Q[:, k + 1] = w / H[k + 1, k]
                it += 1
                width = k + 1
                e1 = np.zeros(width + 1)
                e1[0] = beta
                y = np.linalg.lstsq(H[:width + 1, :width], e1, rcond=None)[0]
                est = float(np.linalg.norm(e1 - H[:width + 1, :width] @ y))
                if (not fixed and est / np.sqrt(n) <= tol) or it >= maxiter or H[k + 1, k] == 0.0:
                    break
            x = x + M(Q[:, :width] @ y)
            r = b - A @ x
            restarts += 1
            if nrm(r) == 0.0 or (not fixed and nrm(r) <= tol) or it >= maxiter:
                return x, it, restarts, nrm(r)


# ---- shared, built once, never changed ---------------------------------------------------------------------------------------------------------------
class _Built:
    pass


_CACHE = {}


def _built(mf, row, itg=3, shared=True, **opts):
    import torch

    key = (row[0], row[1], tuple(row[2]), tuple(row[3]), row[4], itg, tuple(sorted(opts.items())))
    if shared and key in _CACHE:
        return _CACHE[key]
    x, n, robin, fixed, hp = row
    S = _Built()
    S.row, S.itg = row, itg
    S.twin = NTwin(x, n, itg, robin, fixed, hp)
    S.brick = mf.make_Brick(x, n, 1, itg)
    for d in range(3):
        S.brick.coords_view(d).copy_(_dev(S.twin.coords[0][:, d]))
    S.params = dict(fixed_faces=_bits(fixed), h_penalty=hp, Tw=TW)
    S.op = S.brick.thermal_operator(K_COND, H_ROBIN, TENV, _bits(robin), **S.params)
    S.mg = S.op.multigrid(nonsymmetric=True, **opts).setup()
    S.info = S.mg.info()
    S.twin.lam = list(S.info["lambda_max"])
    S.n = S.op.n
    S.u = np.random.default_rng(3).uniform(-1.0, 1.0, S.n)
    S.b = S.twin.A[0] @ S.u       # b = A uniform(-1, 1), seed 3
    S.r = np.random.default_rng(5).uniform(-1.0, 1.0, S.n)
    torch.cuda.synchronize()
    if shared:
        _CACHE[key] = S
    return S


def _tol(S, rel=1e-8):
    return rel * float(np.linalg.norm(S.b)) / np.sqrt(S.n)


def _gmres(mf, S, tol=None, b=None, **kw):
    """K x = -b  <=>  A x = b (A = -K): the solve's iterate is the twin's"""
    kw.setdefault("maxiter", 200)
    kw.setdefault("max_pass", 1)
    return mf.iterative_Solve(S.op, None, _dev(-(S.b if b is None else b)), _tol(S) if tol is None else tol, Sv_func=mf.gmres_, Pr_func=mf.Pr_Multigrid_, **kw)


def _assembled_residual(mf, S, x, b=None):
    """|b - K x| / sqrt(n) on the ASSEMBLED K (assemble_thermal with fixed_faces, the CSR kernel)"""
    key = "_assembled"
    if not hasattr(S, key):
        A = S.brick.pattern(1)
        setattr(S, key, (A, S.brick.assemble_thermal(A, K_COND, H_ROBIN, TENV, _bits(S.row[2]), **S.params)))
    A, Kv = getattr(S, key)
    bb = _dev(-(S.b if b is None else b))
    return float((bb - mf.mul_(_dev(np.zeros(S.n)), A, Kv, x)).norm()) / np.sqrt(S.n)


# ---- 1. the cycle against the twin -------------------------------------------------------------------------------------------------------------------
CYCLE_CASES = [(SMALLEST, 3), (ROWS[0], 3), (ROWS[2], 3), (TWO_LEVELS, 3), (ONE_LEVEL, 3), (ROWS[3], 3), (ROWS[4], 3), (ROWS[0], 5), (ROWS[0], 7)]
CYCLE_IDS = ["4", "8", "16x24x12-fixed04", "6x10x14", "9x14x15", "16-six-fixed", "16-hp10", "8-itg5", "8-itg7"]


@pytest.mark.parametrize("row,itg", CYCLE_CASES, ids=CYCLE_IDS)
def test_cycle_equals_the_twin(mf, row, itg):
    """apply(r) on a random r against the twin with the Nitsche rows on every level: 1e-10 of max |z|, the bound of the symmetric hierarchy's test"""
    S = _built(mf, row, itg)
    assert S.info["levels"] == len(S.twin.levels) and [tuple(e) for e in S.info["ne"]] == S.twin.levels
    assert S.info["sign"] == -1 and S.info["nonsymmetric"] is True
    assert S.twin.asymmetry() > 1e-5  # (the Nitsche rows are there: 9.7e-5 on the six-fixed row, 4.8e-3 .. 1.7e-1 on the others)
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r)
    err = np.abs(z - want).max() / np.abs(want).max()
    print(f"{row[1]} itg {itg}: {S.info['levels']} levels, asymmetry {S.twin.asymmetry():.1e}, lambda {S.twin.lam}, |z - z_twin| / max|z| = {err:.2e}")
    assert np.isfinite(z).all()
    assert err <= 1e-10


@pytest.mark.parametrize("row", [ROWS[0], ONE_LEVEL], ids=["8", "9x14x15"])
def test_cycle_is_linear_and_a_fixed_operator(mf, row):
    """linear to 1e-12, the bound of the symmetric hierarchy's test; two applies of one r give the same bits.  Symmetry is not asserted: the cycle of
    a nonsymmetric K is not symmetric."""
    S = _built(mf, row)
    rng = np.random.default_rng(23)
    M = lambda v: S.mg.apply(_dev(v)).cpu().numpy()
    u, v = rng.uniform(-1, 1, S.n), rng.uniform(-1, 1, S.n)
    Mu, Mv = M(u), M(v)
    lin = np.abs(M(2.0 * u - 3.0 * v) - (2.0 * Mu - 3.0 * Mv)).max() / np.abs(2.0 * Mu - 3.0 * Mv).max()
    print(f"{row[1]}: linearity {lin:.1e}, symmetry defect (not asserted) {abs(v @ Mu - u @ Mv) / abs(v @ Mu):.1e}")
    assert lin <= 1e-12
    assert M(u).tobytes() == Mu.tobytes()


# ---- 2. the solves -------------------------------------------------------------------------------------------------------------------------------------
_SOLVED = {}


def _solve_row(mf, i):
    if i in _SOLVED:
        return _SOLVED[i]
    import scipy.sparse.linalg as spl

    S = _built(mf, ROWS[i])
    tol = _tol(S)
    sol, st = _gmres(mf, S)
    _, st_j = mf.iterative_Solve(S.op, None, _dev(-S.b), tol, Sv_func=mf.gmres_, Pr_func=mf.Pr_Jacobi_, maxiter=2000, max_pass=1)
    res = _assembled_residual(mf, S, sol)
    _, it_twin, _, _ = S.twin.gmres(S.b, tol)
    want = S.u if i == 5 else spl.spsolve(S.twin.A[0].tocsc(), S.b)  # (32^3: the u of b = A u)
    err = np.abs(sol.cpu().numpy() - want).max() / np.abs(want).max()
    out = dict(converged=st.converged, it=st.iterations, jacobi=st_j.iterations, jacobi_converged=st_j.converged, res=res, tol=tol, twin=it_twin, err=err)
    print(f"row {i} {ROWS[i][1]}: {S.info['levels']} levels, MG {st.iterations} (twin {it_twin}) / Jacobi {st_j.iterations} steps, residual {res:.2e} "
          f"(tol {tol:.2e}), |x - x_direct| / |x| = {err:.1e}, spmv {st.spmv_count}")
    _SOLVED[i] = out
    return out


@pytest.mark.parametrize("i", range(len(ROWS)), ids=ROW_IDS)
def test_solve_converges_in_the_twins_steps(mf, i):
    R = _solve_row(mf, i)
    assert R["converged"] == 1
    assert R["res"] <= 2 * R["tol"]
    assert R["it"] <= R["twin"] + 1
    assert R["it"] < R["jacobi"]
    assert R["err"] <= 1e-6


def test_steps_do_not_grow_with_the_mesh(mf):
    assert _solve_row(mf, 5)["it"] <= _solve_row(mf, 1)["it"] + 1


# ---- 3. restarts and edges -----------------------------------------------------------------------------------------------------------------------------
EDGES = [("s4", dict(s=4)), ("s1", dict(s=1, maxiter=400)), ("maxiter-inside-a-restart", dict(s=4, maxiter=6)),
         ("fixed-7-steps", dict(s=4, maxiter=7, fixed_iterations=True))]


@pytest.mark.parametrize("name,kw", EDGES, ids=[e[0] for e in EDGES])
def test_restarts_and_edges(mf, name, kw):
    """The device takes the twin's count of steps.  A run that converges meets the residual bound on the assembled K; a run that the cap or
    fixed_iterations ends has not converged, so its iterate and its residual are compared with the twin's after the same steps instead (1e-8 and
    1e-6: the twin's sums are numpy's)."""
    S = _built(mf, ROWS[1])
    tol = _tol(S)
    sol, st = _gmres(mf, S, **kw)
    fixed = bool(kw.get("fixed_iterations"))
    xt, it_twin, restarts_twin, res_twin = S.twin.gmres(S.b, tol, s=kw["s"], maxiter=kw.get("maxiter", 200), fixed=fixed)
    res = _assembled_residual(mf, S, sol)
    print(f"{name}: {st.iterations} steps (twin {it_twin} in {restarts_twin} restarts), residual {res:.2e} (twin {res_twin:.2e}, tol {tol:.2e})")
    if name in ("s4", "s1"):
        assert st.converged == 1 and restarts_twin >= 2
        assert st.iterations <= it_twin + 1 and res <= 2 * tol
    else:
        assert st.iterations == it_twin == kw["maxiter"]
        assert np.abs(sol.cpu().numpy() - xt).max() <= 1e-8 * np.abs(xt).max()
        assert abs(res - res_twin) <= 1e-6 * res_twin


def test_a_converged_start_and_a_zero_right_hand_side(mf):
    S = _built(mf, ROWS[0])
    before = S.mg.info()
    sol, st = _gmres(mf, S, tol=10.0 * float(np.linalg.norm(S.b)))
    assert st.iterations == 0 and st.converged == 1 and S.mg.info()["cycles"] == before["cycles"]
    assert float(sol.abs().max()) == 0.0
    sol, st = _gmres(mf, S, b=np.zeros(S.n), tol=1e-12)
    assert st.iterations == 0 and S.mg.info()["cycles"] == before["cycles"]
    assert float(sol.abs().max()) == 0.0
    sol, st = _gmres(mf, S, b=np.zeros(S.n), tol=1e-12, maxiter=5, fixed_iterations=True)  # (nothing to normalise: no step is taken)
    assert st.iterations == 0 and bool(sol.isfinite().all()) and float(sol.abs().max()) == 0.0


# ---- 4. the counts -------------------------------------------------------------------------------------------------------------------------------------
def _count_check(mf, S, nu, nu_c, s, **kw):
    """spmv_count and the deltas of info against brick_multigrid_decide.h: mg_gmres_pass_products -- it (1 + c) + restarts (c + 1) from a zero
    start, one more for the wrapper's true residual; cycles = it + restarts on every level"""
    L = S.info["levels"]
    per_cycle = [(nu_c - 1) if l == L - 1 else 2 * nu for l in range(L)]
    c = per_cycle[0]
    before = S.mg.info()
    sol, st = _gmres(mf, S, s=s, **kw)
    after = S.mg.info()
    it = st.iterations
    cycles = after["cycles"] - before["cycles"]
    restarts = cycles - it
    assert restarts >= -(-it // s) and (it == 0 or restarts >= 1)
    assert st.spmv_count == it * (1 + c) + restarts * (c + 1) + 1
    assert [a - b_ for a, b_ in zip(after["products"], before["products"])] == [pc * cycles for pc in per_cycle]
    assert after["setups"] == before["setups"] + 1
    return st, restarts


def test_product_counts(mf):
    S = _built(mf, ROWS[0])
    st, restarts = _count_check(mf, S, NU, NU_C, 20)
    assert st.converged == 1 and st.iterations >= 1 and restarts == 1
    st, restarts = _count_check(mf, S, NU, NU_C, 4, maxiter=7, fixed_iterations=True)
    assert st.iterations == 7 and restarts == 2
    st, restarts = _count_check(mf, S, NU, NU_C, 3)
    assert st.converged == 1 and restarts >= 2
    S1 = _built(mf, ONE_LEVEL)
    st, restarts = _count_check(mf, S1, NU, NU_C, 20)
    assert st.converged == 1


def test_product_counts_with_other_degrees(mf):
    S = _built(mf, ROWS[0], smoother_degree=3, coarse_degree=8)
    st, _ = _count_check(mf, S, 3, 8, 20)
    assert st.converged == 1
    st, restarts = _count_check(mf, S, 3, 8, 4, maxiter=7, fixed_iterations=True)
    assert st.iterations == 7 and restarts == 2
    st, restarts = _count_check(mf, S, 3, 8, 3)
    assert st.converged == 1 and restarts >= 2
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r, nu=3, nu_c=8)
    assert np.abs(z - want).max() / np.abs(want).max() <= 1e-10


# ---- 5. bits -------------------------------------------------------------------------------------------------------------------------------------------
def test_two_solves_and_a_recreated_hierarchy_give_the_same_bits(mf):
    S = _built(mf, ROWS[0], shared=False)
    solve = lambda: _gmres(mf, S, s=5)[0].cpu().numpy().tobytes()
    a = solve()
    assert solve() == a
    S.mg.close()
    assert S.op._mg is None
    S.op.multigrid(nonsymmetric=True)
    assert solve() == a
    S.op.close()


# ---- 6. live parameters --------------------------------------------------------------------------------------------------------------------------------
def test_the_nitsche_term_is_switched_live(mf):
    x, n, robin, fixed, hp = ROWS[0]
    S = _built(mf, ROWS[0], shared=False)
    b = _dev(-S.b)
    tol = _tol(S)
    cg = dict(Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)
    with pytest.raises(mf.MetaFEMError, match="Nitsche"):
        mf.iterative_Solve(S.op, None, b, tol, **cg)
    S.op.set_params(K_COND, H_ROBIN, TENV, _bits(robin))  # off
    got, st = mf.iterative_Solve(S.op, None, b, tol, **cg)
    assert st.converged == 1
    brick = mf.make_Brick(x, n, 1, 3)
    for d in range(3):
        brick.coords_view(d).copy_(_dev(S.twin.coords[0][:, d]))
    plain = brick.thermal_operator(K_COND, H_ROBIN, TENV, _bits(robin))
    plain.multigrid()
    assert plain._mg.info()["nonsymmetric"] is False
    want, _ = mf.iterative_Solve(plain, None, b, tol, **cg)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    sol, st = _gmres(mf, S)  # (gmres_ takes the hierarchy with the term off as well)
    assert st.converged == 1
    S.op.set_params(K_COND, H_ROBIN, TENV, _bits(robin), **S.params)  # on again
    with pytest.raises(mf.MetaFEMError, match="Nitsche"):
        mf.iterative_Solve(S.op, None, b, tol, **cg)
    sol, st = _gmres(mf, S)
    assert st.converged == 1 and _assembled_residual(mf, S, sol) <= 2 * tol
    plain.close()
    S.op.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_missing_and_touch_nothing(mf):
    import torch
    from metafem_jl_amd import _lib

    lib = _lib.lib
    n = (4, 4, 4)
    brick = mf.make_Brick(XU, n, 1, 3)
    ctx = brick.ctx
    N = brick.ncp
    NAME = "mfem_brick_multigrid_create_nonsymmetric"

    def refused(handle, nn, want_rc, method=mf.gmres_, left=0):
        x = torch.full((nn,), 777.0, dtype=torch.float64, device="cuda")
        bb = torch.ones(nn, dtype=torch.float64, device="cuda")
        o = _lib.SolveOptions(method=method, precond=mf.Pr_Multigrid_, l_or_s=0, maxiter=50, max_pass=1, check_every=8, converge_tol=1e-8, seed=1,
                              fixed_iterations=0, scale_in_place=0, left_precond=left, cg_variant=0)
        st = _lib.SolveStats()
        count = lib.mfem_debug_brick_operator_count()
        rc = lib.mfem_solve_operator(ctx._h, handle, bb.data_ptr(), x.data_ptr(), C.byref(o), C.byref(st))
        msg = lib.mfem_last_error().decode()
        torch.cuda.synchronize()
        assert rc == want_rc, (rc, msg)
        assert len(msg) > 20
        assert bool((x == 777.0).all())
        assert lib.mfem_debug_brick_operator_count() == count
        return msg

    nit = brick.thermal_operator(K_COND, H_ROBIN, TENV, 0x2F, fixed_faces=0x10, h_penalty=1000.0, Tw=TW)
    op = brick.thermal_operator(K_COND, H_ROBIN, TENV, 0x3F)
    assert NAME in refused(nit._h, N, -3)                      # no hierarchy: none is made by default
    assert nit._mg is None
    plain = op.multigrid()
    assert NAME in refused(op._h, N, -3)                       # a plain hierarchy
    el = brick.elasticity_operator(1.0, 1.0, 10.0, 0x10)
    assert "elasticity" in refused(el._h, 3 * N, -3)
    b27 = mf.make_Brick(XU, (2, 2, 2), 2, 3)
    h27 = b27.thermal_operator_hex27(K_COND, H_ROBIN, TENV, 0x3F)
    assert "hex-27" in refused(h27._h, b27.ncp, -3)
    cube = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.float64, device="cuda")  # one hex-8 element
    mop = mf.MeshOperator(ctx, 3, 8, 1, 8, 1, cube, torch.arange(1, 9, dtype=torch.int32, device="cuda"), 1)
    assert "brick operator" in refused(mop._h, mop.n, -3)
    mg = nit.multigrid(nonsymmetric=True)
    assert "left" in refused(nit._h, N, -3, left=1)
    assert "MFEM_SOLVER_CG" in refused(nit._h, N, -3, method=mf.idrs_)
    assert "Nitsche" in refused(nit._h, N, -3, method=mf.cg_)
    ar = _lib.ALLREDUCE_CB(lambda user, buf, count: 0)
    ex = _lib.EXCHANGE_CB(lambda user, a, b_, c, d, count: 0)
    ops = _lib.CommHostOps(None, ar, ex, 0, 0)
    comm = C.c_void_p()
    _lib.check(lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(comm)))
    try:
        _lib.check(lib.mfem_context_set_comm(ctx._h, comm, N, (n[1] + 1) * (n[2] + 1), 1))
        assert "communicator" in refused(nit._h, N, -3)
    finally:
        lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        lib.mfem_comm_destroy(comm)
    # the new entry point
    create = lib.mfem_brick_multigrid_create_nonsymmetric
    out = C.c_uint64(5)
    count = lib.mfem_debug_brick_operator_count()
    assert create(ctx._h, el._h, None, C.byref(out)) == -3 and out.value == 0
    assert create(ctx._h, h27._h, None, C.byref(out)) == -3
    assert create(ctx._h, mop._h, None, C.byref(out)) == -3
    assert create(None, nit._h, None, C.byref(out)) == -1
    assert create(ctx._h, 0, None, C.byref(out)) == -1
    assert create(ctx._h, nit._h, None, None) == -1
    other = mf.Context(0)
    fresh = brick.thermal_operator(K_COND, H_ROBIN, TENV, 0x2F, fixed_faces=0x10, h_penalty=1000.0, Tw=TW)
    assert create(other._h, fresh._h, None, C.byref(out)) == -1              # a foreign context
    assert create(ctx._h, nit._h, None, C.byref(out)) == -1                  # a second hierarchy on one operator
    assert create(ctx._h, op._h, None, C.byref(out)) == -1                   # ... of either kind
    assert out.value == 0 and lib.mfem_debug_brick_operator_count() == count  # (no product was launched)
    assert lib.mfem_brick_multigrid_nonsymmetric(0) == -1
    with pytest.raises(mf.MultigridRefused):
        el.multigrid(nonsymmetric=True)
    with pytest.raises(mf.MultigridRefused):
        h27.multigrid(nonsymmetric=True)
    # what was refused before is refused still, and every handle is usable
    assert lib.mfem_brick_multigrid_create(ctx._h, fresh._h, None, C.byref(out)) == -3
    with pytest.raises(mf.MultigridRefused):
        fresh.multigrid()
    assert mg.info()["nonsymmetric"] is True and plain.info()["nonsymmetric"] is False
    b = torch.ones(N, dtype=torch.float64, device="cuda")
    sol, st = mf.iterative_Solve(nit, None, b, 1e-9, Sv_func=mf.gmres_, Pr_func=mf.Pr_Multigrid_, maxiter=100, max_pass=1)
    assert st.converged == 1
    sol, st = mf.iterative_Solve(op, None, b, 1e-9, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=100, max_pass=1)
    assert st.converged == 1


# ---- 8. the domain -------------------------------------------------------------------------------------------------------------------------------------
def test_thermal_domain_with_fixed_faces_and_multigrid_any(mf):
    x0 = mf.FACE_BITS["x0"]
    hist = []
    for kw in (dict(), dict(matrix_free=True, multigrid="any")):
        dom = mf.ThermalDomain(mf.make_Brick(XB, (16, 24, 12), 1, 3), K_COND, H_ROBIN, TENV, mf.ALL_FACES & ~x0, fixed_faces=x0, h_penalty=1000.0, Tw=TW, **kw)
        dom.s.fill_(1600.0)
        dom.converge_tol = 1e-9
        hist.append((dom.update_OneStep(), dom.x.cpu().numpy(), dom))
    d_mg = hist[1][2]
    assert d_mg.multigrid and d_mg.multigrid_reason is None and d_mg.K_linear is None
    assert d_mg.A._mg is d_mg.mg and d_mg.mg.info()["nonsymmetric"] is True and d_mg.mg.info()["cycles"] > 0
    assert len(hist[0][0]) == len(hist[1][0])
    for a, b in zip(hist[0][0], hist[1][0]):
        assert abs(a - b) <= 1e-8 * hist[0][0][0]
    assert hist[1][0][-1] < 1e-9
    err = np.abs(hist[0][1] - hist[1][1]).max() / np.abs(hist[0][1]).max()
    print(f"histories {hist[0][0]} / {hist[1][0]}, |x - x_default| / |x| = {err:.1e}")
    assert err <= 1e-8
    # without fixed faces "any" is True; True with fixed faces keeps falling back
    dom = mf.ThermalDomain(mf.make_Brick(XU, (4, 4, 4), 1, 3), K_COND, H_ROBIN, TENV, matrix_free=True, multigrid="any")
    assert dom.multigrid and dom.mg.info()["nonsymmetric"] is False
    dom = mf.ThermalDomain(mf.make_Brick(XU, (4, 4, 4), 1, 3), K_COND, H_ROBIN, TENV, mf.ALL_FACES & ~x0, fixed_faces=x0, h_penalty=1000.0, Tw=TW,
                           matrix_free=True, multigrid=True)
    assert not dom.multigrid and "nonsymmetric" in dom.multigrid_reason
    dom = mf.ThermalDomain(mf.make_Brick(XU, (4, 4, 4), 1, 3), K_COND, H_ROBIN, TENV, mf.ALL_FACES & ~x0, fixed_faces=x0, h_penalty=1000.0, Tw=TW,
                           multigrid="any")
    assert not dom.multigrid and "assembled" in dom.multigrid_reason
