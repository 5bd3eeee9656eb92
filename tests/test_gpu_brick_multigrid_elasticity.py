"""GPU: the geometric multigrid V-cycle on hex-8 ELASTICITY bricks (mfem_brick_multigrid_create_elasticity, csrc/brick_multigrid.hip: three
field-major fields per lattice point) and cg! with it as the preconditioner (Pr_Multigrid_ on an ElasticityBrickOperator with a hierarchy attached).

The file carries the NUMPY TWIN of tests/test_gpu_brick_multigrid.py on the oracle's elasticity level matrices (problems.elasticity_domain +
problems.elasticity_penalty, built as _oracle of tests/test_gpu_brick_operator_elasticity.py builds them, on coordinates injected from the next finer
level): P = I_3 (x) the Kronecker product of the 1-D interpolation, restriction P', the Chebyshev recurrence in D^-1 A with the residual carried,
A = -K, and lambda_max per level the DEVICE's own (info), so that the device has to agree with the twin step by step.  Constants: E = 1,
Poisson 0.3, tau = 1000; every brick is distorted by _distort of that file.

MG / Jacobi iterations the twin needs at 1e-8 |b| / sqrt(n), b = A uniform(-1, 1) seed 3 (measured on a CPU with hi = 1.1 x 0.98 x the true
lambda_max; orientation only -- the tests compare with the twin fed the device's estimates):
  unit 8^3 x0                 3 levels  11 / 120
  unit 16^3 x0                4 levels  10 / 226
  (3,1,2) 24x8x16 x0|z1       3 levels  11 / 194
  (1,1.5,.75) 16x24x12 x0     3 levels  11 / 241
  unit 9x14x15 x0             1 level   10 / 190
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_MOD, POISSON = 1.0, 0.3
LAM, MU = E_MOD * POISSON / ((1 + POISSON) * (1 - 2 * POISSON)), E_MOD / (2 * (1 + POISSON))
TAU = 1000.0
FACE_NAMES = ["z0", "y0", "x1", "y1", "x0", "z1"]  # oracle face id f == bit f of the mask
XU, X312, XB, XK = (1.0, 1.0, 1.0), (3.0, 1.0, 2.0), (1.0, 1.5, 0.75), (1.0, 1.0, 32.5)
NU_S, RANGE_S, NU_C, RANGE_C = 2, 4.0, 32, 300.0
# x, n, penalty faces
SOLVE_ROWS = [
    (XU, (8, 8, 8), "x0"),
    (XU, (16, 16, 16), "x0"),
    (X312, (24, 8, 16), "x0|z1"),
    (XB, (16, 24, 12), "x0"),
    (XU, (9, 14, 15), "x0"),
]
SOLVE_IDS = ["x".join(map(str, r[1])) for r in SOLVE_ROWS]
K130 = (XK, (4, 4, 130), "x0")  # 131 fine and 66 coarse points along k: both transfer kernels cross the 64-point tile, short last tiles of 3 and 2


def _ids(names):
    return [FACE_NAMES.index(s) for s in names.split("|")] if names else []


def _bits(mf, names):
    b = 0
    for s in (names.split("|") if names else []):
        b |= mf.FACE_BITS[s]
    return b


def _distort(c, x):  # (tests/test_gpu_brick_operator_elasticity.py: _distort)
    return c + 0.03 * np.stack([np.sin(2 * c[:, 1]), np.cos(2 * c[:, 2]) - 1, c[:, 0] * c[:, 1] / x[0]], axis=1)


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


def interpolation(ne_coarse, fields=3):
    """I_fields (x) the trilinear interpolation from the coarse lattice: field-major vectors"""
    import scipy.sparse as sp

    P = sp.kron(sp.kron(_interp_1d(ne_coarse[0] + 1), _interp_1d(ne_coarse[1] + 1)), _interp_1d(ne_coarse[2] + 1))
    return sp.kron(sp.identity(fields), P).tocsr()


def oracle_level(x, n, itg, coords, pen, tau, lam=LAM, mu=MU):
    """K of one level on the given coordinates"""
    import scipy.sparse as sp
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    msh.coords = coords.copy()
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = [(fac.select(np.isin(fac.element_eindex, _ids(pen))), problems.elasticity_penalty(3, tau))] if pen else []
    od = fem.FEMDomain(msh, disc, 3, problems.elasticity_domain(3, lam, mu), bnd)
    od.update_time()
    od.K_linear_func()
    return sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)


def lattice_coords(x, n):
    from oracle import mesh as om, reference_element as re_

    return om.lattice_mesh(x, n, re_.initialize_classical_element(3, "CUBE", 1, 1, 3)).coords.copy()


class Twin:
    """levels: A_l = -K_l (the elasticity K with a penalty face is negative definite), dinv_l, P_l (level l + 1 -> l), the coordinates per level"""

    def __init__(self, x, n, itg, pen, tau=TAU, max_levels=12):
        self.levels = plan(n, max_levels)
        c = _distort(lattice_coords(x, n), x)
        self.coords, self.A, self.dinv, self.P = [], [], [], []
        for l, ne in enumerate(self.levels):
            if l:  # injection: coarse point (i, j, k) takes fine point (2 i, 2 j, 2 k)
                pf = self.levels[l - 1]
                c = c.reshape(pf[0] + 1, pf[1] + 1, pf[2] + 1, 3)[::2, ::2, ::2].reshape(-1, 3).copy()
            K = oracle_level(x, ne, itg, c, pen, tau)
            d = K.diagonal()
            assert (d < 0).all()
            self.coords.append(c)
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

    def cycle(self, b, l=0, nu=NU_S, nu_c=NU_C, range_s=RANGE_S, range_c=RANGE_C):
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

    def pcg(self, b, tol, maxiter=500, **kw):
        """classic PCG on A x = b from x = 0; stops on |r| / sqrt(n) <= tol; -> (x, iterations)"""
        A = self.A[0]
        n = b.size
        x = np.zeros(n)
        r = b.copy()
        if np.linalg.norm(r) / np.sqrt(n) <= tol:
            return x, 0
        z = self.cycle(r, **kw)
        p = z.copy()
        rz = r @ z
        for it in range(1, maxiter + 1):
            Ap = A @ p
            alpha = rz / (p @ Ap)
            x += alpha * p
            r -= alpha * Ap
            if np.linalg.norm(r) / np.sqrt(n) <= tol:
                return x, it
            z = self.cycle(r, **kw)
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


def _set_coords(brick, coords):
    for d in range(3):
        brick.coords_view(d).copy_(_dev(coords[:, d]))


def _built(mf, row, itg=3, shared=True, **opts):
    import torch

    key = (row, itg, tuple(sorted(opts.items())))
    if shared and key in _CACHE:
        return _CACHE[key]
    x, n, pen = row
    S = _Built()
    S.row, S.itg = row, itg
    S.twin = Twin(x, n, itg, pen, max_levels=opts.get("max_levels", 12) or 12)
    S.brick = mf.make_Brick(x, n, 1, itg)
    _set_coords(S.brick, S.twin.coords[0])
    S.op = S.brick.elasticity_operator(LAM, MU, TAU, _bits(mf, pen))
    S.mg = S.op.multigrid(**opts).setup()
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


# ---- 1. the transfers alone --------------------------------------------------------------------------------------------------------------------------
TRANSFER_BRICKS = [(XU, (4, 4, 4)), (XU, (6, 4, 4)), (XU, (16, 24, 12)), (XK, (4, 4, 130))]


@pytest.mark.parametrize("x,n", TRANSFER_BRICKS, ids=["x".join(map(str, b[1])) for b in TRANSFER_BRICKS])
def test_transfers_equal_the_sparse_interpolation_exactly(mf, x, n):
    """Small integers in, different per field: with the power-of-two weights every product and every partial sum is exact in double (at most 27
    terms of at most 9 / 8 ... 9 each), whatever the order -- the device's result EQUALS the sparse product.  One nonzero field stays in its field."""
    import torch
    from metafem_jl_amd import _lib

    op = mf.make_Brick(x, n, 1, 3).elasticity_operator(LAM, MU, TAU, mf.FACE_BITS["x0"])
    mg = op.multigrid(max_levels=2)
    nc = tuple(v // 2 for v in n)
    assert mg.info()["levels"] == 2 and tuple(mg.info()["ne"][1]) == nc
    P = interpolation(nc)
    nf3, nc3 = P.shape
    pf, pc = nf3 // 3, nc3 // 3
    assert nf3 == op.n and pf == (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
    rng = np.random.default_rng(17)
    e = np.concatenate([rng.integers(lo, hi, pc) for lo, hi in ((-9, 10), (10, 20), (-30, -20))]).astype(np.float64)
    r = np.concatenate([rng.integers(lo, hi, pf) for lo, hi in ((-9, 10), (10, 20), (-30, -20))]).astype(np.float64)
    h = _lib.lib

    def transfer(restriction, v):
        out = torch.full((nc3 if restriction else nf3,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(h.mfem_debug_brick_multigrid_transfer(op.ctx._h, mg._h, 0, restriction, _dev(v).data_ptr(), out.data_ptr()))
        return out.cpu().numpy()

    pe, ptr = transfer(0, e), transfer(1, r)
    assert np.array_equal(pe, P @ e)
    assert np.array_equal(ptr, P.T @ r)
    assert transfer(0, e).tobytes() == pe.tobytes() and transfer(1, r).tobytes() == ptr.tobytes()  # the same bits on every run
    for f in range(3):  # no field leaks into another
        ef, rf = np.zeros_like(e), np.zeros_like(r)
        ef[f * pc:(f + 1) * pc] = e[f * pc:(f + 1) * pc]
        rf[f * pf:(f + 1) * pf] = r[f * pf:(f + 1) * pf]
        got_p, got_r = transfer(0, ef), transfer(1, rf)
        for g in range(3):
            if g == f:
                assert np.array_equal(got_p[g * pf:(g + 1) * pf], pe[g * pf:(g + 1) * pf]) and np.abs(got_p[g * pf:(g + 1) * pf]).max() > 0
                assert np.array_equal(got_r[g * pc:(g + 1) * pc], ptr[g * pc:(g + 1) * pc])
            else:
                assert not got_p[g * pf:(g + 1) * pf].any() and not got_r[g * pc:(g + 1) * pc].any()
    mg.close()
    op.close()


# ---- 2. the cycle against the twin -------------------------------------------------------------------------------------------------------------------
CYCLE_CASES = [((XU, (4, 4, 4), "x0"), 3), ((XU, (8, 8, 8), "x0"), 3), ((X312, (12, 4, 8), "x0|z1"), 2), ((XU, (4, 4, 4), "x0"), 5),
               ((XU, (9, 14, 15), "x0"), 3), (K130, 3)]


@pytest.mark.parametrize("row,itg", CYCLE_CASES, ids=["x".join(map(str, r[1])) + f"-itg{g}" for r, g in CYCLE_CASES])
def test_cycle_equals_the_twin(mf, row, itg):
    """apply(r) on a random r against the twin: 1e-10 of max |z|, the project's bound for the cycle (the thermal one measured 1.2e-15)."""
    S = _built(mf, row, itg)
    assert S.info["levels"] == len(S.twin.levels) and [tuple(e) for e in S.info["ne"]] == S.twin.levels
    assert S.info["sign"] == -1
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r)
    err = np.abs(z - want).max() / np.abs(want).max()
    print(f"{row[1]} itg {itg}: {S.info['levels']} levels, |z - z_twin| / max|z| = {err:.2e}")
    assert z.shape == (3 * S.brick.ncp,) and np.isfinite(z).all()
    assert err <= 1e-10


# ---- 3. properties ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [SOLVE_ROWS[0], SOLVE_ROWS[4]], ids=[SOLVE_IDS[0], SOLVE_IDS[4]])
def test_cycle_is_symmetric_positive_and_linear(mf, row):
    S = _built(mf, row)
    rng = np.random.default_rng(23)
    M = lambda v: S.mg.apply(_dev(v)).cpu().numpy()
    for _ in range(5):
        r = rng.uniform(-1, 1, S.n)
        assert r @ M(r) > 0.0
    u, v = rng.uniform(-1, 1, S.n), rng.uniform(-1, 1, S.n)
    Mu, Mv = M(u), M(v)
    sym = abs(v @ Mu - u @ Mv) / (np.abs(u) @ np.abs(Mv))  # (relative to the size of the terms, as the thermal test measures an adjoint defect)
    lin = np.abs(M(2.0 * u - 3.0 * v) - (2.0 * Mu - 3.0 * Mv)).max() / np.abs(2.0 * Mu - 3.0 * Mv).max()
    print(f"{row[1]}: symmetry defect {sym:.1e}, linearity {lin:.1e}")
    assert sym <= 1e-12 and lin <= 1e-12


@pytest.mark.parametrize("row", [SOLVE_ROWS[0], (X312, (12, 4, 8), "x0|z1")], ids=["8x8x8", "12x4x8"])
def test_estimate_does_not_exceed_the_true_eigenvalue(mf, row):
    S = _built(mf, row, 3 if row[1] == (8, 8, 8) else 2)
    lam = S.info["lambda_max"]
    for l in range(S.info["levels"]):
        true = S.twin.true_lambda(l)
        print(f"{row[1]} level {l} {S.twin.levels[l]}: estimate {lam[l]:.6f}, true {true:.6f}, share {lam[l] / true:.4f}")
        assert lam[l] <= true * (1.0 + 1e-10)
        if row[1] == (8, 8, 8):
            assert lam[l] >= 0.9 * true
    again = S.mg.setup().info()["lambda_max"]
    assert np.array(again).tobytes() == np.array(lam).tobytes()


# ---- 4. the solve --------------------------------------------------------------------------------------------------------------------------------------
_ITER = {}


def _solve_row(mf, i):
    """one solve per row, shared: MG and Jacobi on the same operator, the twin's count, the assembled matrix's residual on the CSR kernel"""
    if i in _ITER:
        return _ITER[i]
    S = _built(mf, SOLVE_ROWS[i])
    x, n, pen = SOLVE_ROWS[i]
    tol = _tol(S)
    b = _dev(-S.b)  # K x = -b  <=>  A x = b (A = -K)
    sol, st = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)
    _, st_j = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=4000, max_pass=1)
    A = S.brick.pattern(3)
    Kv = S.brick.assemble_elasticity(A, LAM, MU, TAU, _bits(mf, pen))
    res = float((b - mf.mul_(_dev(np.zeros(S.n)), A, Kv, sol)).norm()) / np.sqrt(S.n)
    _, it_twin = S.twin.pcg(S.b, tol)
    err = np.abs(sol.cpu().numpy() - S.u).max() / np.abs(S.u).max()
    out = dict(st=(st.converged, st.iterations, st.spmv_count, st.passes), jacobi=(st_j.converged, st_j.iterations), res=res, tol=tol, twin=it_twin,
               err=err, levels=S.info["levels"])
    print(f"row {i} {n}: {out['levels']} levels, MG {st.iterations} (twin {it_twin}) / Jacobi {st_j.iterations} iterations, residual {res:.3e} "
          f"(tol {tol:.3e}), |x - u| / |u| = {err:.1e}")
    _ITER[i] = out
    return out


@pytest.mark.parametrize("i", range(len(SOLVE_ROWS)), ids=SOLVE_IDS)
def test_solve_converges_in_the_twins_iterations(mf, i):
    R = _solve_row(mf, i)
    converged, iterations = R["st"][0], R["st"][1]
    assert converged == 1
    assert R["res"] <= R["tol"]
    assert iterations <= R["twin"] + 1
    assert R["jacobi"][0] == 1 and 3 * iterations <= R["jacobi"][1]
    assert R["err"] <= 1e-4  # (x = u up to |A^-1| tol: the residual above is the check, this guards the sign convention)


def test_iterations_do_not_grow_with_the_mesh(mf):
    """the device alone (the oracle does not reach 32^3 in seconds): unit cubes of 8^3 and 32^3 elements, distorted, b = K uniform(-1, 1) seed 3"""
    import torch

    its = {}
    for m in (8, 32):
        brick = mf.make_Brick(XU, (m, m, m), 1, 3)
        c = np.stack([brick.coords_view(d).cpu().numpy() for d in range(3)], axis=1)
        _set_coords(brick, _distort(c, XU))
        op = brick.elasticity_operator(LAM, MU, TAU, mf.FACE_BITS["x0"])
        op.multigrid()
        u = _dev(np.random.default_rng(3).uniform(-1.0, 1.0, op.n))
        b = op.mul_(torch.empty_like(u), u)
        tol = 1e-8 * float(b.norm()) / np.sqrt(op.n)
        _, st = mf.iterative_Solve(op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)
        assert st.converged == 1
        its[m] = st.iterations
        op.close()
    print(f"iterations: 8^3 {its[8]}, 32^3 {its[32]}")
    assert its[32] <= its[8] + 2


# ---- 5. the counts and the bits ------------------------------------------------------------------------------------------------------------------------
def _count_check(mf, S, nu, nu_c, **kw):
    L = S.info["levels"]
    per_cycle = [(nu_c - 1) if l == L - 1 else 2 * nu for l in range(L)]  # (mg_cycle_products)
    b = _dev(-S.b)
    before = S.mg.info()
    sol, st = mf.iterative_Solve(S.op, None, b, kw.pop("tol", _tol(S)), Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, max_pass=1, **kw)
    after = S.mg.info()
    it = st.iterations
    cycles = after["cycles"] - before["cycles"]
    assert cycles == it  # the first before iteration 1, none after the last
    assert st.spmv_count == (it + per_cycle[0] * it + 1 if it >= 1 else 1)  # x0 + it + 2 nu it + 1 with x0 = 0
    assert [a - b_ for a, b_ in zip(after["products"], before["products"])] == [c * cycles for c in per_cycle]
    assert after["setups"] == before["setups"] + 1  # a solve always runs the setup
    return st


def test_product_counts_multi_level_and_one_level(mf):
    for row in (SOLVE_ROWS[0], SOLVE_ROWS[4]):
        S = _built(mf, row)
        st = _count_check(mf, S, NU_S, NU_C, maxiter=200)
        assert st.converged == 1 and st.iterations >= 1
        st = _count_check(mf, S, NU_S, NU_C, maxiter=3, fixed_iterations=True)
        assert st.iterations == 3
        st = _count_check(mf, S, NU_S, NU_C, maxiter=200, tol=10.0 * float(np.linalg.norm(S.b)))  # the start has converged: it = 0, no cycle
        assert st.iterations == 0 and st.converged == 1


def test_product_counts_with_other_degrees(mf):
    S = _built(mf, SOLVE_ROWS[0], smoother_degree=3, coarse_degree=8)
    st = _count_check(mf, S, 3, 8, maxiter=200)
    assert st.converged == 1
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r, nu=3, nu_c=8)
    assert np.abs(z - want).max() / np.abs(want).max() <= 1e-10


def test_two_solves_and_a_recreated_hierarchy_give_the_same_bits(mf):
    S = _built(mf, SOLVE_ROWS[0], shared=False)  # (its hierarchy is closed below)
    b = _dev(-S.b)
    solve = lambda: mf.iterative_Solve(S.op, None, b, _tol(S), Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)[0].cpu().numpy().tobytes()
    a = solve()
    assert solve() == a
    S.mg.close()
    assert S.op._mg is None
    with pytest.raises(mf.MetaFEMError, match="mfem_brick_multigrid_create_elasticity"):  # (no default hierarchy for elasticity)
        solve()
    S.op.multigrid()
    assert solve() == a
    S.op.close()


# ---- 6. liveness -----------------------------------------------------------------------------------------------------------------------------------------
def test_parameters_and_coordinates_are_read_live(mf):
    x, n, pen = SOLVE_ROWS[0]
    c0 = _distort(lattice_coords(x, n), x)
    moved = c0 * np.array([1.0, 1.02, 0.97])
    pen2 = "x0|y1"

    def fresh(lam, mu, tau, faces, coords):
        brick = mf.make_Brick(x, n, 1, 3)
        _set_coords(brick, coords)
        op = brick.elasticity_operator(lam, mu, tau, _bits(mf, faces))
        op.multigrid()
        return brick, op

    b = _dev(np.random.default_rng(3).uniform(-1, 1, 3 * c0.shape[0]))
    tol = 1e-8 * float(b.norm()) / np.sqrt(b.numel())
    solve = lambda op: mf.iterative_Solve(op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=300, max_pass=1)[0].cpu().numpy().tobytes()
    brick, op = fresh(LAM, MU, TAU, pen, c0)
    first = solve(op)
    op.set_params(2.0 * LAM, 0.5 * MU, 3.0 * TAU, _bits(mf, pen2))
    _set_coords(brick, moved)
    _, op2 = fresh(2.0 * LAM, 0.5 * MU, 3.0 * TAU, pen2, moved)
    got, want = solve(op), solve(op2)
    assert got == want
    assert got != first


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_missing_and_touch_nothing(mf):
    import torch
    from metafem_jl_amd import _lib

    lib = _lib.lib
    INVALID, UNSUPPORTED = -1, -3
    n = (4, 4, 4)
    brick = mf.make_Brick(XU, n, 1, 3)
    ctx = brick.ctx
    N = 3 * brick.ncp
    x0 = mf.FACE_BITS["x0"]

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

    def create_refused(handle, want_rc=UNSUPPORTED, opts=None):
        out = C.c_uint64(9)
        count = lib.mfem_debug_brick_operator_count()
        assert lib.mfem_brick_multigrid_create_elasticity(ctx._h, handle, opts, C.byref(out)) == want_rc
        assert out.value == 0 and lib.mfem_debug_brick_operator_count() == count
        return lib.mfem_last_error().decode()

    # no hierarchy attached: the refusal stands, and names the entry point
    bare = brick.elasticity_operator(LAM, MU, TAU, x0)
    msg = refused(bare._h, N, UNSUPPORTED)
    assert "elasticity" in msg and "mfem_brick_multigrid_create_elasticity" in msg
    assert lib.mfem_brick_multigrid_create(ctx._h, bare._h, None, C.byref(C.c_uint64())) == UNSUPPORTED  # (the thermal name keeps refusing it)
    # a singular K at create
    no_tau = brick.elasticity_operator(LAM, MU, 0.0, x0)
    no_face = brick.elasticity_operator(LAM, MU, TAU, 0)
    assert "tau" in create_refused(no_tau._h) and "penalty_faces" in create_refused(no_face._h)
    for op_ in (no_tau, no_face):
        with pytest.raises(mf.MultigridRefused):
            op_.multigrid()
        assert op_._mg is None
    # the other operator kinds
    thermal = brick.thermal_operator(0.6, 25.0, 293.15, 0x3F)
    b27 = mf.make_Brick(XU, (2, 2, 2), 2, 3)
    h27 = b27.thermal_operator_hex27(0.6, 25.0, 293.15, 0x3F)
    cube = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.float64, device="cuda")  # one hex-8 element
    mop = mf.MeshOperator(ctx, 3, 8, 1, 8, 1, cube, torch.arange(1, 9, dtype=torch.int32, device="cuda"), 1)
    assert "thermal" in create_refused(thermal._h) and "hex-27" in create_refused(h27._h) and "mesh operator" in create_refused(mop._h)
    create_refused(0, INVALID)
    assert lib.mfem_brick_multigrid_create_elasticity(ctx._h, bare._h, None, None) == INVALID
    create_refused(bare._h, INVALID, C.byref(_lib.MultigridOptions(0, 0, 0.5, 0.0, 0, 0)))
    # with a hierarchy attached: every other combination
    op = brick.elasticity_operator(LAM, MU, TAU, x0)
    mg = op.multigrid()
    create_refused(op._h, INVALID)  # one per operator
    assert "MFEM_SOLVER_CG" in refused(op._h, N, UNSUPPORTED, method=mf.idrs_)
    assert "left" in refused(op._h, N, UNSUPPORTED, left=1)
    ar = _lib.ALLREDUCE_CB(lambda user, buf, count: 0)
    ex = _lib.EXCHANGE_CB(lambda user, a, b_, c, d, count: 0)
    ops = _lib.CommHostOps(None, ar, ex, 0, 0)
    comm = C.c_void_p()
    _lib.check(lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(comm)))
    try:
        _lib.check(lib.mfem_context_set_comm(ctx._h, comm, N, 1, 1))
        assert "communicator" in refused(op._h, N, UNSUPPORTED)
    finally:
        lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        lib.mfem_comm_destroy(comm)
    A = brick.pattern(3)
    vals = brick.assemble_elasticity(A, LAM, MU, TAU, x0)
    assert "mfem_solve_operator" in refused(None, N, UNSUPPORTED, solve_csr=(A, vals))
    # tau = 0 after a valid create: refused at the setup and inside a solve
    mg.setup()
    setups = mg.info()["setups"]
    op.set_params(LAM, MU, 0.0, x0)
    count = lib.mfem_debug_brick_operator_count()
    assert lib.mfem_brick_multigrid_setup(ctx._h, mg._h) == UNSUPPORTED and "tau" in lib.mfem_last_error().decode()
    with pytest.raises(mf.MultigridRefused):
        mg.setup()
    assert lib.mfem_debug_brick_operator_count() == count and mg.info()["setups"] == setups
    r = torch.ones(N, dtype=torch.float64, device="cuda")
    z = torch.full_like(r, 777.0)
    assert lib.mfem_brick_multigrid_apply(ctx._h, mg._h, r.data_ptr(), z.data_ptr()) == INVALID  # (the refused setup left no usable levels)
    torch.cuda.synchronize()
    assert bool((z == 777.0).all())
    assert "tau" in refused(op._h, N, UNSUPPORTED)
    op.set_params(LAM, MU, TAU, 0)
    assert "penalty_faces" in refused(op._h, N, UNSUPPORTED)
    # every handle is still usable
    op.set_params(LAM, MU, TAU, x0)
    mg.setup()
    assert float(mg.apply(r) @ r) > 0.0
    b = torch.ones(N, dtype=torch.float64, device="cuda")
    for o_ in (op, thermal):
        bb = b[: o_.n]
        sol, st = mf.iterative_Solve(o_, None, bb, 1e-10, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=100, max_pass=1)
        assert st.converged == 1
    sol, st = mf.iterative_Solve(bare, None, b, 1e-8, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=2000)
    assert st.converged == 1
    sol, st = mf.iterative_Solve(no_tau, None, b, 1e-8, Sv_func=mf.cg_, maxiter=5, fixed_iterations=True)  # (a singular K still serves products)
    assert st.iterations == 5
    mg.close()
    op.close()


# ---- 8. the domain ---------------------------------------------------------------------------------------------------------------------------------------
def test_elasticity_domain_with_multigrid(mf, monkeypatch):
    """The cantilever of tests/test_gpu_brick_operator_elasticity.py: the unit cube of 8 x 6 x 5 elements held by the penalty on x0, sigma_11 = 0.01
    pulled on x1, both domains at converge_tol = 1e-15 (normalised residual; |b| / sqrt(n) is 5e-5).  That file bounds |K^-1| by ~500: an x with
    residual r is off by at most 500 sqrt(n) 1e-15 = 1.7e-11 against displacements of 1e-2 -- 2e-9 relative per domain, under the 1e-8 asked for."""
    import torch

    x, n = XU, (8, 6, 5)
    pen, tra = mf.FACE_BITS["x0"], mf.FACE_BITS["x1"]
    sig = (0.01, 0.0, 0.0, 0.0, 0.0, 0.0)
    hist = []
    for kw in (dict(), dict(matrix_free=True, multigrid=True)):
        dom = mf.ElasticityDomain(mf.make_Brick(x, n), LAM, MU, TAU, pen, tra, sig, **kw)
        dom.converge_tol = 1e-15
        hist.append((dom.update_OneStep(), dom.x.cpu().numpy(), dom))
    d_mg = hist[1][2]
    assert d_mg.multigrid and d_mg.multigrid_reason is None and d_mg.K_linear is None and d_mg.K_total is None
    assert isinstance(d_mg.A, mf.ElasticityBrickOperator) and d_mg.A._mg is d_mg.mg and d_mg.mg.info()["cycles"] > 0
    scale = np.abs(hist[0][1]).max()
    err = np.abs(hist[0][1] - hist[1][1]).max() / scale
    print(f"histories {hist[0][0]} / {hist[1][0]}, |x - x_default| / |x| = {err:.1e} (max|x| = {scale:.3e})")
    assert hist[1][0][-1] < d_mg.converge_tol
    assert scale > 1e-3
    assert err <= 1e-8
    # no penalty face: the reason is set and the default solver runs
    dom = mf.ElasticityDomain(mf.make_Brick(x, (4, 4, 4)), LAM, MU, TAU, 0, tra, sig, matrix_free=True, multigrid=True)
    assert not dom.multigrid and "penalty" in dom.multigrid_reason and dom.matrix_free and not hasattr(dom, "mg")
    calls = []  # (K is singular: no convergence is claimed, only that the default solver -- idrs_(8) without the cycle -- is the one that runs)
    monkeypatch.setattr(mf, "iterative_Solve", lambda A, K, res, tol, **kw: (calls.append(kw), (torch.zeros_like(res), None))[1])
    dom.update_OneStep(max_iter=0)
    assert len(calls) == 1 and calls[0]["Sv_func"] == mf.idrs_ and "Pr_func" not in calls[0]
    monkeypatch.undo()
    dom = mf.ElasticityDomain(mf.make_Brick(x, (4, 4, 4)), LAM, MU, TAU, pen, tra, sig, multigrid=True)
    assert not dom.multigrid and "assembled" in dom.multigrid_reason
