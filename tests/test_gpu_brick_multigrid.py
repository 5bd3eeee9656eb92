"""GPU: the geometric multigrid V-cycle on hex-8 thermal bricks (mfem_brick_multigrid_*, csrc/brick_multigrid.hip) and cg! with it as the
preconditioner (Pr_Multigrid_, csrc/krylov_cg_mg.hip).

The file carries a NUMPY TWIN of the scheme: the level matrices are the oracle's (built as _oracle of tests/test_gpu_brick_operator.py builds them,
on coordinates injected from the next finer level), P is the Kronecker product of the 1-D interpolation, restriction is P', the smoother is the
Chebyshev recurrence in D^-1 A with the residual carried, and lambda_max per level is the DEVICE's own (info), so that the device has to agree with
the twin step by step.  Constants: k = 0.6, h = 25 (or 1), Tenv = 293.15; "distorted" is _distort of that file.

Rows of the table (MG / Jacobi iterations the twin needs at 1e-8 |b| / sqrt(n), b = A uniform(-1, 1) seed 3, measured on a CPU):
  0  (1,1.5,.75) 16x24x12 distorted, all faces      3 levels   5 / 41
  1  unit 16^3 distorted, face 4 only, h = 1         4 levels   5 / 78
  2  unit 32^3 distorted, face 4 only, h = 1         5 levels   5 / 144
  3  (1,1.5,.75) 8^3 distorted, all faces (aspect 2) 3 levels  10 / 29
  4  (1,1.5,.75) 6x10x14 distorted, faces 0, 3       2 levels  12 / 80
  5  unit 9x14x15 distorted, all faces               1 level    6 / 36
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_COND, TENV = 0.6, 293.15
ALL = [0, 1, 2, 3, 4, 5]
XB, XU = (1.0, 1.5, 0.75), (1.0, 1.0, 1.0)
NU, RANGE_S, NU_C, RANGE_C = 2, 4.0, 32, 300.0
# x, n, Robin faces, h
ROWS = [
    (XB, (16, 24, 12), ALL, 25.0),
    (XU, (16, 16, 16), [4], 1.0),
    (XU, (32, 32, 32), [4], 1.0),
    (XB, (8, 8, 8), ALL, 25.0),
    (XB, (6, 10, 14), [0, 3], 25.0),
    (XU, (9, 14, 15), ALL, 25.0),
]
SMALLEST = (XU, (4, 4, 4), ALL, 25.0)  # the smallest brick with two levels
ROW_IDS = ["x".join(map(str, r[1])) for r in ROWS]


def _distort(c):  # (tests/test_gpu_brick_operator.py: _distort)
    out = c.copy()
    out[:, 0] += 0.03 * np.sin(3 * c[:, 1]) * np.cos(2 * c[:, 2])
    out[:, 1] += 0.02 * np.sin(2 * c[:, 0] + c[:, 2])
    out[:, 2] += 0.025 * c[:, 0] * c[:, 1]
    return out


def _bits(faces):
    return sum(1 << f for f in faces)


def plan(n, max_levels=12):
    levels = [tuple(n)]
    while len(levels) < max_levels and all(v % 2 == 0 and v // 2 >= 2 for v in levels[-1]):
        levels.append(tuple(v // 2 for v in levels[-1]))
    return levels


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------------------
def _interp_1d(mc):
    import scipy.sparse as sp

    mf_ = 2 * mc - 1
    P = sp.lil_matrix((mf_, mc))
    for i in range(mf_):
        if i % 2 == 0:
            P[i, i // 2] = 1.0
        else:
            P[i, i // 2] = 0.5
            P[i, i // 2 + 1] = 0.5
    return P.tocsr()


def interpolation(ne_coarse):
    import scipy.sparse as sp

    return sp.kron(sp.kron(_interp_1d(ne_coarse[0] + 1), _interp_1d(ne_coarse[1] + 1)), _interp_1d(ne_coarse[2] + 1)).tocsr()


def oracle_level(x, n, itg, coords, robin, h):
    """(K, the oracle's domain) of one level on the given coordinates"""
    import scipy.sparse as sp
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    msh.coords[:] = coords
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = [(fac.select(np.isin(fac.element_eindex, robin)), problems.thermal_convection(h, TENV))] if robin else []
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, K_COND), bnd)
    od.controlpoints["s"] = np.zeros(msh.ncp)
    od.update_time()
    od.K_linear_func()
    return sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2), od


class Twin:
    """levels: A_l = -K_l (the thermal K is negative definite), dinv_l, P_l (level l + 1 -> l), the coordinates per level"""

    def __init__(self, x, n, itg, robin, h, distorted=True, max_levels=12):
        from oracle import mesh as om, reference_element as re_

        self.levels = plan(n, max_levels)
        disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
        c = om.lattice_mesh(x, n, disc).coords.copy()
        if distorted:
            c = _distort(c)
        self.coords, self.A, self.dinv, self.P, self.K = [], [], [], [], []
        for l, ne in enumerate(self.levels):
            if l:  # injection: coarse point (i, j, k) takes fine point (2 i, 2 j, 2 k)
                pf = self.levels[l - 1]
                c = c.reshape(pf[0] + 1, pf[1] + 1, pf[2] + 1, 3)[::2, ::2, ::2].reshape(-1, 3).copy()
            K, _ = oracle_level(x, ne, itg, c, robin, h)
            d = K.diagonal()
            assert (d < 0).all()
            self.coords.append(c)
            self.K.append(K)
            self.A.append((-K).tocsr())
            self.dinv.append(1.0 / np.abs(d))
            if l:
                self.P.append(interpolation(ne))
        self.lam = None  # lambda_max per level: set from the device's info

    def true_lambda(self, l):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl

        s = np.sqrt(self.dinv[l])
        S = sp.diags(s)
        M = (S @ self.A[l] @ S).tocsr()
        if M.shape[0] < 400:
            return float(np.linalg.eigvalsh(M.toarray())[-1])
        return float(spl.eigsh(M, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0])

    def cheb(self, l, b, nu, lo, hi, z=None, r=None):
        """-> (z, r, d): r = b - A z carried by recurrence up to the last step's start (the caller brings it up to date)"""
        A, dinv = self.A[l], self.dinv[l]
        theta, delta = (hi + lo) / 2.0, (hi - lo) / 2.0
        sigma = theta / delta
        rho = 1.0 / sigma
        if z is None:
            r = b.copy()
            d = dinv * r / theta
            z = d.copy()
        else:
            d = dinv * r / theta
            z = z + d
        for _ in range(1, nu):
            rho_new = 1.0 / (2.0 * sigma - rho)
            r = r - A @ d
            d = rho_new * rho * d + (2.0 * rho_new / delta) * (dinv * r)
            z = z + d
            rho = rho_new
        return z, r, d

    def cycle(self, b, l=0, nu=NU, nu_c=NU_C, range_s=RANGE_S, range_c=RANGE_C):
        hi = 1.1 * self.lam[l]
        kw = dict(nu=nu, nu_c=nu_c, range_s=range_s, range_c=range_c)
        if l == len(self.levels) - 1:
            return self.cheb(l, b, nu_c, hi / range_c, hi)[0]
        z, r, d = self.cheb(l, b, nu, hi / range_s, hi)
        r = r - self.A[l] @ d
        e = self.cycle(self.P[l].T @ r, l + 1, **kw)
        pe = self.P[l] @ e
        z = z + pe
        r = r - self.A[l] @ pe
        return self.cheb(l, b, nu, hi / range_s, hi, z=z, r=r)[0]

    def pcg(self, b, tol, maxiter=500, jacobi=False, **kw):
        """classic PCG on A x = b from x = 0; stops on |r| / sqrt(n) <= tol; -> (x, iterations)"""
        A = self.A[0]
        M = (lambda v: self.dinv[0] * v) if jacobi else (lambda v: self.cycle(v, **kw))
        n = b.size
        x = np.zeros(n)
        r = b.copy()
        if np.linalg.norm(r) / np.sqrt(n) <= tol:
            return x, 0
        z = M(r)
        p = z.copy()
        rz = r @ z
        for it in range(1, maxiter + 1):
            Ap = A @ p
            alpha = rz / (p @ Ap)
            x += alpha * p
            r -= alpha * Ap
            if np.linalg.norm(r) / np.sqrt(n) <= tol:
                return x, it
            z = M(r)
            rz_new = r @ z
            p = z + (rz_new / rz) * p
            rz = rz_new
        return x, maxiter


# ---- shared, built once, never changed ---------------------------------------------------------------------------------------------------------------
class _Built:
    pass


_CACHE = {}


def _dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _built(mf, row, itg=3, shared=True, **opts):
    import torch

    key = (row[0], row[1], tuple(row[2]), row[3], itg, tuple(sorted(opts.items())))
    if shared and key in _CACHE:
        return _CACHE[key]
    x, n, robin, h = row
    S = _Built()
    S.row, S.itg = row, itg
    S.twin = Twin(x, n, itg, robin, h, max_levels=opts.get("max_levels", 12) or 12)
    S.brick = mf.make_Brick(x, n, 1, itg)
    for d in range(3):
        S.brick.coords_view(d).copy_(_dev(S.twin.coords[0][:, d]))
    S.op = S.brick.thermal_operator(K_COND, h, TENV, _bits(robin))
    S.mg = S.op.multigrid(**opts).setup()
    S.info = S.mg.info()
    S.twin.lam = list(S.info["lambda_max"])
    S.n = S.op.n
    rng = np.random.default_rng(3)
    S.u = rng.uniform(-1.0, 1.0, S.n)
    S.b = S.twin.A[0] @ S.u       # b = A uniform(-1, 1), seed 3
    S.r = np.random.default_rng(5).uniform(-1.0, 1.0, S.n)
    torch.cuda.synchronize()
    if shared:
        _CACHE[key] = S
    return S


def _tol(S, rel=1e-8):
    return rel * float(np.linalg.norm(S.b)) / np.sqrt(S.n)


# ---- 1. the cycle against the twin -------------------------------------------------------------------------------------------------------------------
CYCLE_CASES = [(ROWS[0], 3), (ROWS[1], 3), (ROWS[3], 3), (ROWS[4], 3), (ROWS[5], 3), (ROWS[0], 5), (ROWS[0], 7), (SMALLEST, 3)]


@pytest.mark.parametrize("row,itg", CYCLE_CASES, ids=["x".join(map(str, r[1])) + f"-itg{g}" for r, g in CYCLE_CASES])
def test_cycle_equals_the_twin(mf, row, itg):
    """apply(r) on a random r against the twin: 1e-10 of max |z| -- 100 x the project's product-against-oracle bound of 1e-11, for a chain of up to
    2 nu levels + nu_c products in which no step amplifies."""
    S = _built(mf, row, itg)
    assert S.info["levels"] == len(S.twin.levels) and [tuple(e) for e in S.info["ne"]] == S.twin.levels
    assert S.info["sign"] == -1
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r)
    err = np.abs(z - want).max() / np.abs(want).max()
    print(f"{row[1]} itg {itg}: {S.info['levels']} levels, |z - z_twin| / max|z| = {err:.2e}")
    assert np.isfinite(z).all()
    assert err <= 1e-10


# ---- 2. the transfers alone ----------------------------------------------------------------------------------------------------------------------------
def _tile_constants():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "metafem.jl_amd", "csrc", "brick_multigrid_decide.h")).read()
    val = lambda name: int(re.search(r"#define " + name + r" (\d+)", text).group(1))
    return val("MG_TILE_J"), val("MG_TILE_K")


def _transfer_bricks():
    """Fine element counts whose lattices sit around the tiles of both kernels.  A fine lattice has an odd number of points (2 mc - 1), so the
    prolongation's tile of TK points is met one short and one past (TK - 1 and TK + 1 points; TK itself is even: no fine lattice has it); the coarse
    lattice (the restriction's) takes every count: on, one short of and one past the tile.  A tile is one lattice plane thick: every plane is an edge."""
    TJ, TK = _tile_constants()
    out = []
    for mc2 in (TK - 1, TK, TK + 1):            # restriction, along k: coarse points
        out.append((4, 4, 2 * (mc2 - 1)))
    for mc1 in (TJ - 1, TJ, TJ + 1):            # restriction, along j
        out.append((4, 2 * (mc1 - 1), 6))
    for mf2 in (TK - 1, TK + 1):                # prolongation, along k: fine points (odd)
        out.append((4, 4, mf2 - 1))
    for mf1 in (TJ + 1, 2 * TJ - 1, 2 * TJ + 1):  # prolongation, along j (a brick that coarsens has at least 5 points: the tile's multiples)
        out.append((6, mf1 - 1, 4))
    out.append((4, 6, 10))                      # nx != ny != nz
    return sorted(set(out))


@pytest.mark.parametrize("n", _transfer_bricks(), ids=lambda n: "x".join(map(str, n)))
def test_transfers_equal_the_sparse_interpolation(mf, n):
    import torch
    from metafem_jl_amd import _lib

    assert all(v % 2 == 0 and v >= 4 for v in n), n
    brick = mf.make_Brick(XU, n, 1, 3)
    c0 = [brick.coords_view(d) for d in range(3)]
    rng = np.random.default_rng(17)
    for d in range(3):  # (any coordinates: the injection is checked bit for bit)
        c0[d].add_(_dev(0.1 / max(n) * rng.uniform(-1.0, 1.0, brick.ncp)))  # (a tenth of the smallest element edge: no element inverts)
    op = brick.thermal_operator(K_COND, 25.0, TENV, 0x3F)
    mg = op.multigrid(max_levels=2).setup()
    nc = tuple(v // 2 for v in n)
    assert mg.info()["levels"] == 2 and tuple(mg.info()["ne"][1]) == nc
    P = interpolation(nc)
    nf_pts, nc_pts = P.shape
    e, r, u = rng.uniform(-1, 1, nc_pts), rng.uniform(-1, 1, nf_pts), rng.uniform(-1, 1, nf_pts)
    h = _lib.lib
    pe = torch.full((nf_pts,), float("nan"), dtype=torch.float64, device="cuda")
    ptr = torch.full((nc_pts,), float("nan"), dtype=torch.float64, device="cuda")
    ptu = torch.empty_like(ptr)
    _lib.check(h.mfem_debug_brick_multigrid_transfer(op.ctx._h, mg._h, 0, 0, _dev(e).data_ptr(), pe.data_ptr()))
    _lib.check(h.mfem_debug_brick_multigrid_transfer(op.ctx._h, mg._h, 0, 1, _dev(r).data_ptr(), ptr.data_ptr()))
    _lib.check(h.mfem_debug_brick_multigrid_transfer(op.ctx._h, mg._h, 0, 1, _dev(u).data_ptr(), ptu.data_ptr()))
    pe, ptr, ptu = pe.cpu().numpy(), ptr.cpu().numpy(), ptu.cpu().numpy()
    e1 = np.abs(pe - P @ e).max() / np.abs(P @ e).max()
    e2 = np.abs(ptr - P.T @ r).max() / np.abs(P.T @ r).max()
    # (relative to the size of the terms, sum |u_i (P e)_i|: the two sums are rounded by numpy, and u . P e itself is the small remainder of terms
    # of either sign -- dividing by it would measure that cancellation, not the kernels)
    adj = abs(u @ pe - ptu @ e) / (np.abs(u) @ np.abs(pe))
    print(f"{n}: P e {e1:.1e}, P' r {e2:.1e}, <u, P e> - <P' u, e> {adj:.1e}")
    assert e1 <= 1e-14 and e2 <= 1e-14 and adj <= 1e-14
    # the injected coordinates are bitwise the fine ones
    for d in range(3):
        cp = h.mfem_debug_brick_multigrid_coords(mg._h, 1, d)
        got = mf._tensor_from_ptr(cp, nc_pts, torch.float64, op.ctx.device, owner=mg).cpu().numpy()
        want = c0[d].cpu().numpy().reshape(n[0] + 1, n[1] + 1, n[2] + 1)[::2, ::2, ::2].reshape(-1)
        assert got.tobytes() == want.tobytes(), d
    assert h.mfem_debug_brick_multigrid_coords(mg._h, 2, 0) is None


# ---- 3. the estimate -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [ROWS[0], ROWS[1], ROWS[3]], ids=[ROW_IDS[0], ROW_IDS[1], ROW_IDS[3]])
def test_estimate_brackets_the_true_eigenvalue(mf, row):
    S = _built(mf, row)
    lam = S.info["lambda_max"]
    for l in range(S.info["levels"]):
        true = S.twin.true_lambda(l)
        print(f"{row[1]} level {l} {S.twin.levels[l]}: estimate {lam[l]:.6f}, true {true:.6f}, share {lam[l] / true:.4f}")
        assert 1.1 * lam[l] >= true
        assert lam[l] <= true * (1.0 + 1e-10)
    again = S.mg.setup().info()["lambda_max"]
    assert np.array(again).tobytes() == np.array(lam).tobytes()


# ---- 4. operator properties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [ROWS[0], ROWS[5]], ids=[ROW_IDS[0], ROW_IDS[5]])
def test_cycle_is_symmetric_positive_and_linear(mf, row):
    S = _built(mf, row)
    rng = np.random.default_rng(23)
    M = lambda v: S.mg.apply(_dev(v)).cpu().numpy()
    for _ in range(5):
        r = rng.uniform(-1, 1, S.n)
        assert r @ M(r) > 0.0
    u, v = rng.uniform(-1, 1, S.n), rng.uniform(-1, 1, S.n)
    Mu, Mv = M(u), M(v)
    sym = abs(v @ Mu - u @ Mv) / abs(v @ Mu)
    lin = np.abs(M(2.0 * u - 3.0 * v) - (2.0 * Mu - 3.0 * Mv)).max() / np.abs(2.0 * Mu - 3.0 * Mv).max()
    print(f"{row[1]}: symmetry defect {sym:.1e}, linearity {lin:.1e}")
    assert sym <= 1e-12 and lin <= 1e-12


# ---- 5. the solve --------------------------------------------------------------------------------------------------------------------------------------
_ITER = {}


def _solve_row(mf, i):
    """one solve per table row, shared by the tests below: MG and Jacobi on the same operator, the twin's count, the assembled matrix's residual"""
    if i in _ITER:
        return _ITER[i]
    S = _built(mf, ROWS[i])
    x, n, robin, h = ROWS[i]
    tol = _tol(S)
    b = _dev(-S.b)  # K x = -b  <=>  A x = b (A = -K): the solve's iterate is the twin's, negated...
    sol, st = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)
    _, st_j = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=2000, max_pass=1)
    A = S.brick.pattern(1)
    Kv = S.brick.assemble_thermal(A, K_COND, h, TENV, _bits(robin))
    res = float((b - mf.mul_(_dev(np.zeros(S.n)), A, Kv, sol)).norm()) / np.sqrt(S.n)
    _, it_twin = S.twin.pcg(S.b, tol)
    direct = _direct_solve(S.twin.A[0], S.b)  # K x = -b  <=>  A x = b
    err = np.abs(sol.cpu().numpy() - direct).max() / np.abs(direct).max()
    out = dict(st=(st.converged, st.iterations, st.spmv_count, st.passes), jacobi=st_j.iterations, res=res, tol=tol, twin=it_twin, err=err,
               levels=S.info["levels"])
    print(f"row {i} {n}: {out['levels']} levels, MG {st.iterations} (twin {it_twin}) / Jacobi {st_j.iterations} iterations, residual {res:.2e} (tol {tol:.2e}), "
          f"|x - x_direct| / |x| = {err:.1e}")
    _ITER[i] = out
    return out


def _direct_solve(A, b):
    """the oracle's matrix factorised directly: banded Cholesky (LAPACK dpbsv) of the positive definite A = -K, whose band is one lattice plane and
    a line wide -- a second at 32^3, where a general sparse LU takes ten"""
    import scipy.linalg as sl

    Ac = A.tocoo()
    low = Ac.row >= Ac.col
    bw = int((Ac.row[low] - Ac.col[low]).max())
    ab = np.zeros((bw + 1, A.shape[0]))
    ab[Ac.row[low] - Ac.col[low], Ac.col[low]] = Ac.data[low]
    return sl.solveh_banded(ab, b, lower=True)


@pytest.mark.parametrize("i", range(len(ROWS)), ids=ROW_IDS)
def test_solve_converges_in_the_twins_iterations(mf, i):
    R = _solve_row(mf, i)
    converged, iterations = R["st"][0], R["st"][1]
    assert converged == 1
    assert R["res"] <= 2 * R["tol"]
    assert iterations <= R["twin"] + 1
    if i in (0, 1, 2, 4):
        assert 3 * iterations <= R["jacobi"]
    assert R["err"] <= 1e-6


def test_iterations_do_not_grow_with_the_mesh(mf):
    assert _solve_row(mf, 2)["st"][1] <= _solve_row(mf, 1)["st"][1] + 1


# ---- 6. the counts -------------------------------------------------------------------------------------------------------------------------------------
def _count_check(mf, S, nu, nu_c, **kw):
    L = S.info["levels"]
    per_cycle = [(nu_c - 1) if l == L - 1 else 2 * nu for l in range(L)]
    b = _dev(-S.b)
    before = S.mg.info()
    sol, st = mf.iterative_Solve(S.op, None, b, kw.pop("tol", _tol(S)), Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, max_pass=1, **kw)
    after = S.mg.info()
    it = st.iterations
    cycles = after["cycles"] - before["cycles"]
    assert cycles == it  # the first before iteration 1, none after the last
    assert st.spmv_count == (it + per_cycle[0] * it + 1 if it >= 1 else 1)
    assert [a - b_ for a, b_ in zip(after["products"], before["products"])] == [c * cycles for c in per_cycle]
    assert after["setups"] == before["setups"] + 1  # a solve always runs the setup
    return st


def test_product_counts_multi_level_and_one_level(mf):
    for row in (ROWS[0], ROWS[5]):
        S = _built(mf, row)
        st = _count_check(mf, S, NU, NU_C, maxiter=200)
        assert st.converged == 1 and st.iterations >= 1
        st = _count_check(mf, S, NU, NU_C, maxiter=3, fixed_iterations=True)
        assert st.iterations == 3
        st = _count_check(mf, S, NU, NU_C, maxiter=200, tol=10.0 * float(np.linalg.norm(S.b)))  # the start has converged: it = 0, no cycle
        assert st.iterations == 0 and st.converged == 1


def test_product_counts_with_other_degrees(mf):
    S = _built(mf, ROWS[0], smoother_degree=3, coarse_degree=8)
    st = _count_check(mf, S, 3, 8, maxiter=200)
    assert st.converged == 1
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r, nu=3, nu_c=8)
    assert np.abs(z - want).max() / np.abs(want).max() <= 1e-10


# ---- 7. bits ---------------------------------------------------------------------------------------------------------------------------------------------
def test_two_solves_and_a_recreated_hierarchy_give_the_same_bits(mf):
    S = _built(mf, ROWS[3], shared=False)  # (its hierarchy is closed below)
    b = _dev(-S.b)
    solve = lambda: mf.iterative_Solve(S.op, None, b, _tol(S), Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)[0].cpu().numpy().tobytes()
    a = solve()
    assert solve() == a
    S.mg.close()
    assert S.op._mg is None
    assert solve() == a  # (the solve creates a default hierarchy)
    S.op.close()


# ---- 8. liveness -----------------------------------------------------------------------------------------------------------------------------------------
def test_parameters_and_coordinates_are_read_live(mf):
    import torch

    x, n, robin, h = ROWS[3]
    tw = Twin(x, n, 3, robin, h)

    def fresh(k, hh, coords):
        brick = mf.make_Brick(x, n, 1, 3)
        for d in range(3):
            brick.coords_view(d).copy_(_dev(coords[:, d]))
        return brick, brick.thermal_operator(k, hh, TENV, _bits(robin))

    b = _dev(-(tw.A[0] @ np.random.default_rng(3).uniform(-1, 1, tw.A[0].shape[0])))
    tol = 1e-8 * float(b.norm()) / np.sqrt(b.numel())
    kw = dict(Sv_func=mf.cg_, maxiter=300, max_pass=1)
    brick, op = fresh(K_COND, h, tw.coords[0])
    jac_before = mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Jacobi_, **kw)[0].cpu().numpy().tobytes()
    first = mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Multigrid_, **kw)[0]
    assert mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Jacobi_, **kw)[0].cpu().numpy().tobytes() == jac_before
    # new parameters, then new coordinates: the attached hierarchy against a fresh operator's
    moved = tw.coords[0] * np.array([1.0, 1.02, 0.97])
    op.set_params(2.0 * K_COND, 3.0, TENV, _bits(robin))
    _, op2 = fresh(2.0 * K_COND, 3.0, tw.coords[0])
    got = mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Multigrid_, **kw)[0]
    want = mf.iterative_Solve(op2, None, b, tol, Pr_func=mf.Pr_Multigrid_, **kw)[0]
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert got.cpu().numpy().tobytes() != first.cpu().numpy().tobytes()
    for d in range(3):
        brick.coords_view(d).copy_(_dev(moved[:, d]))
    _, op3 = fresh(2.0 * K_COND, 3.0, moved)
    got = mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Multigrid_, **kw)[0]
    want = mf.iterative_Solve(op3, None, b, tol, Pr_func=mf.Pr_Multigrid_, **kw)[0]
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    torch.cuda.synchronize()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_missing_and_touch_nothing(mf):
    import torch
    from metafem_jl_amd import _lib

    lib = _lib.lib
    n = (4, 4, 4)
    brick = mf.make_Brick(XU, n, 1, 3)
    ctx = brick.ctx
    N = brick.ncp
    b = torch.ones(N, dtype=torch.float64, device="cuda")

    def refused(handle, nn, want_rc, method=mf.cg_, left=0, solve_csr=None):
        x = torch.full((nn,), 777.0, dtype=torch.float64, device="cuda")
        bb = torch.ones(nn, dtype=torch.float64, device="cuda")
        o = _lib.SolveOptions(method=method, precond=mf.Pr_Multigrid_, l_or_s=0, maxiter=50, max_pass=1, check_every=8, converge_tol=1e-8, seed=1,
                              fixed_iterations=0, scale_in_place=0, left_precond=left, cg_variant=0)
        st = _lib.SolveStats()
        count = lib.mfem_debug_brick_operator_count()
        if solve_csr is not None:
            A, vals = solve_csr
            rc = lib.mfem_solve(ctx._h, A._h, vals.data_ptr(), bb.data_ptr(), x.data_ptr(), C.byref(o), C.byref(st))
        else:
            rc = lib.mfem_solve_operator(ctx._h, handle, bb.data_ptr(), x.data_ptr(), C.byref(o), C.byref(st))
        msg = lib.mfem_last_error().decode()
        torch.cuda.synchronize()
        assert rc == want_rc, (rc, msg)
        assert len(msg) > 20
        assert bool((x == 777.0).all())
        assert lib.mfem_debug_brick_operator_count() == count
        return msg

    op = brick.thermal_operator(K_COND, 25.0, TENV, 0x3F)
    nit = brick.thermal_operator(K_COND, 25.0, TENV, 0x1F, fixed_faces=0x20, h_penalty=1000.0, Tw=1173.15)
    assert "Nitsche" in refused(nit._h, N, -3)
    assert "MFEM_SOLVER_CG" in refused(op._h, N, -3, method=mf.idrs_)
    assert "left" in refused(op._h, N, -3, left=1)
    el = brick.elasticity_operator(1.0, 1.0, 10.0, 0x10)
    assert "elasticity" in refused(el._h, 3 * N, -3)
    b27 = mf.make_Brick(XU, (2, 2, 2), 2, 3)
    h27 = b27.thermal_operator_hex27(K_COND, 25.0, TENV, 0x3F)
    assert "hex-27" in refused(h27._h, b27.ncp, -3)
    A = brick.pattern(1)
    vals = brick.assemble_thermal(A, K_COND, 25.0, TENV, 0x3F)
    assert "brick operator" in refused(None, N, -3, solve_csr=(A, vals))
    # a mesh operator
    cube = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.float64, device="cuda")  # one hex-8 element
    mop = mf.MeshOperator(ctx, 3, 8, 1, 8, 1, cube, torch.arange(1, 9, dtype=torch.int32, device="cuda"), 1)
    assert "brick operator" in refused(mop._h, mop.n, -3)
    assert lib.mfem_brick_multigrid_create(ctx._h, mop._h, None, C.byref(C.c_uint64())) == -3
    # a host communicator
    ar = _lib.ALLREDUCE_CB(lambda user, buf, count: 0)
    ex = _lib.EXCHANGE_CB(lambda user, a, b_, c, d, count: 0)
    ops = _lib.CommHostOps(None, ar, ex, 0, 0)
    comm = C.c_void_p()
    _lib.check(lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(comm)))
    try:
        _lib.check(lib.mfem_context_set_comm(ctx._h, comm, N, (n[1] + 1) * (n[2] + 1), 1))
        assert "communicator" in refused(op._h, N, -3)
    finally:
        lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        lib.mfem_comm_destroy(comm)
    # the hierarchy's own entry points
    out = C.c_uint64()
    assert lib.mfem_brick_multigrid_create(ctx._h, nit._h, None, C.byref(out)) == -3 and out.value == 0
    assert lib.mfem_brick_multigrid_create(ctx._h, el._h, None, C.byref(out)) == -3
    assert lib.mfem_brick_multigrid_create(ctx._h, h27._h, None, C.byref(out)) == -3
    assert lib.mfem_brick_multigrid_create(ctx._h, op._h, None, None) == -1
    assert lib.mfem_brick_multigrid_create(None, op._h, None, C.byref(out)) == -1
    assert lib.mfem_brick_multigrid_create(ctx._h, 0, None, C.byref(out)) == -1
    bad = _lib.MultigridOptions(0, 0, 0.5, 0.0, 0, 0)
    assert lib.mfem_brick_multigrid_create(ctx._h, op._h, C.byref(bad), C.byref(out)) == -1
    few = _lib.MultigridOptions(0, 0, 0.0, 0.0, 5, 0)
    assert lib.mfem_brick_multigrid_create(ctx._h, op._h, C.byref(few), C.byref(out)) == -1
    mg = op.multigrid()
    assert lib.mfem_brick_multigrid_create(ctx._h, op._h, None, C.byref(out)) == -1  # one per operator
    r = torch.ones(N, dtype=torch.float64, device="cuda")
    z = torch.zeros_like(r)
    assert lib.mfem_brick_multigrid_apply(ctx._h, mg._h, r.data_ptr(), z.data_ptr()) == -1  # no setup yet
    other = mf.Context(0)
    assert lib.mfem_brick_multigrid_setup(other._h, mg._h) == -1  # a hierarchy of another context
    assert lib.mfem_brick_multigrid_apply(other._h, mg._h, r.data_ptr(), z.data_ptr()) == -1
    assert lib.mfem_brick_multigrid_setup(ctx._h, 0) == -1
    assert lib.mfem_brick_multigrid_apply(ctx._h, mg._h, None, z.data_ptr()) == -1
    assert lib.mfem_brick_multigrid_info(mg._h, None) == -1
    # every handle is still usable
    mg.setup()
    assert float(mg.apply(r) @ r) > 0.0
    sol, st = mf.iterative_Solve(op, None, b, 1e-10, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=100, max_pass=1)
    assert st.converged == 1
    sol, st = mf.iterative_Solve(nit, None, b, 1e-8, Sv_func=mf.idrs_, s=4)
    assert st.converged == 1
    with pytest.raises(mf.MultigridRefused):
        nit.multigrid()
    with pytest.raises(mf.MetaFEMError):
        mf.iterative_Solve(A, vals, b, 1e-8, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_)
    mg.close()
    op.close()


# ---- 10. the domain ------------------------------------------------------------------------------------------------------------------------------------
def test_thermal_domain_with_multigrid(mf):
    x, n, robin, h = ROWS[0]
    hist = []
    for kw in (dict(), dict(matrix_free=True, multigrid=True)):
        dom = mf.ThermalDomain(mf.make_Brick(x, n, 1, 3), K_COND, h, TENV, **kw)
        dom.s.fill_(1600.0)
        dom.converge_tol = 1e-9
        hist.append((dom.update_OneStep(), dom.x.cpu().numpy(), dom))
    d_mg = hist[1][2]
    assert d_mg.multigrid and d_mg.multigrid_reason is None and d_mg.K_linear is None and d_mg.K_total is None
    assert isinstance(d_mg.A, mf.BrickOperator) and d_mg.A._mg is d_mg.mg and d_mg.mg.info()["cycles"] > 0
    assert len(hist[0][0]) == len(hist[1][0])
    for a, b in zip(hist[0][0], hist[1][0]):  # (the entries behind the first are the solvers' own residuals, below the tolerance both)
        assert abs(a - b) <= 1e-8 * hist[0][0][0]
    assert hist[1][0][-1] < 1e-9
    err = np.abs(hist[0][1] - hist[1][1]).max() / np.abs(hist[0][1]).max()
    print(f"histories {hist[0][0]} / {hist[1][0]}, |x - x_default| / |x| = {err:.1e}")
    assert err <= 1e-8
    x0 = mf.FACE_BITS["x0"]
    dom = mf.ThermalDomain(mf.make_Brick(x, (4, 4, 4), 1, 3), K_COND, h, TENV, mf.ALL_FACES & ~x0, fixed_faces=x0, h_penalty=1000.0, Tw=1173.15,
                           matrix_free=True, multigrid=True)
    assert not dom.multigrid and "nonsymmetric" in dom.multigrid_reason
    dom.s.fill_(1600.0)
    assert dom.update_OneStep()[-1] < dom.converge_tol  # the default solver runs
    dom = mf.ThermalDomain(mf.make_Brick(x, (4, 4, 4), 1, 3), K_COND, h, TENV, multigrid=True)
    assert not dom.multigrid and "assembled" in dom.multigrid_reason
