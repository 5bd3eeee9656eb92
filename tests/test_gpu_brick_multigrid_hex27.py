"""GPU: the geometric multigrid V-cycle on hex-27 thermal bricks (mfem_brick_multigrid_create_hex27, csrc/brick_multigrid.hip), the signed diagonal
it reads (k_brick27_diagonal_sweep, csrc/brick_operator_hex27_diagonal.hip) and cg! with the cycle as the preconditioner.

The twin is Twin of tests/test_gpu_brick_multigrid.py with another level 0: the oracle's ORDER-2 K (initialize_classical_element(3, "CUBE", 2, 1,
itg)) on the lattice 2 n + 1; level 1 is the oracle's hex-8 K on the same elements, on the coordinates taken [::2, ::2, ::2] (the corner nodes),
and the hex-8 levels below it follow the halving rule.  P between levels 0 and 1 is the same Kronecker interpolation (mf = 2 mc - 1): the embedding
Q1 in Q2.  lambda_max per level is the DEVICE's own (info).  Constants: k = 0.6, Tenv = 293.15, nu = 2 on range 4, 32 coarse steps on range 300,
_distort'ed coordinates, b = A uniform(-1, 1) seed 3, stopped at 1e-8 |b| / sqrt(n).

Rows (MG / Jacobi iterations of the twin with 0.98 x the true lambda_max, measured on a CPU):
  0  (1,1.5,.75) 8x12x6, all faces, h = 25, itg 5    27 -> 8x12x6 -> 4x6x3        5 / 50
  1  the same, itg 7                                                                5 / 50
  2  unit 8^3, face 4, h = 1, itg 5                   27 -> 8^3 -> 4^3 -> 2^3       6 / 100
  3  unit 16^3, face 4, h = 1, itg 5 (35 937 rows)    27 -> 16^3 -> ... -> 2^3      6 / 175
  4  unit 4^3, all faces, h = 25, itg 5               27 -> 4^3 -> 2^3              5 / 25
  5  (1,1.5,.75) 3x5x7, faces 0 and 3, h = 25, itg 5  27 -> 3x5x7                   13 / 91
  6  (1,1.5,.75) 6^3, all faces, h = 25, itg 7        27 -> 6^3 -> 3^3              8 / 48
  7  unit 1x1x1, all faces, h = 25, itg 5             27 -> 1^3                     5 / 14
  8  unit 2x1x3, all faces, h = 25, itg 5             27 -> 2x1x3                   7 / 21
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_brick_multigrid import ALL, K_COND, NU, NU_C, TENV, XB, XU, Twin, _bits, _dev, _direct_solve, _distort, interpolation, oracle_level, plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# x, n, Robin faces, h, itg, the table's MG count
ROWS = [
    (XB, (8, 12, 6), ALL, 25.0, 5, 5),
    (XB, (8, 12, 6), ALL, 25.0, 7, 5),
    (XU, (8, 8, 8), [4], 1.0, 5, 6),
    (XU, (16, 16, 16), [4], 1.0, 5, 6),
    (XU, (4, 4, 4), ALL, 25.0, 5, 5),
    (XB, (3, 5, 7), [0, 3], 25.0, 5, 13),
    (XB, (6, 6, 6), ALL, 25.0, 7, 8),
    (XU, (1, 1, 1), ALL, 25.0, 5, 5),
    (XU, (2, 1, 3), ALL, 25.0, 5, 7),
]
ROW_IDS = ["x".join(map(str, r[1])) + f"-itg{r[4]}" for r in ROWS]


def plan27(n, max_levels=12):
    return [tuple(n)] + (plan(n, max_levels - 1) if max_levels >= 2 else [])


def oracle_level27(x, n, itg, coords, robin, h):
    """the oracle's order-2 K on the given coordinates (the lattice 2 n + 1)"""
    import scipy.sparse as sp
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 2, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    msh.coords[:] = coords
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = [(fac.select(np.isin(fac.element_eindex, robin)), problems.thermal_convection(h, TENV))] if robin else []
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, K_COND), bnd)
    od.controlpoints["s"] = np.zeros(msh.ncp)
    od.update_time()
    od.K_linear_func()
    return sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)


def coords27(x, n, itg, distorted=True):
    from oracle import mesh as om, reference_element as re_

    c = om.lattice_mesh(x, n, re_.initialize_classical_element(3, "CUBE", 2, 1, itg)).coords.copy()
    return _distort(c) if distorted else c


class Twin27(Twin):
    """Twin with the hex-27 level on top: levels holds ELEMENT counts (levels[0] == levels[1]), cycle / cheb / pcg are Twin's"""

    def __init__(self, x, n, itg, robin, h, distorted=True, max_levels=12):
        self.levels = plan27(n, max_levels)
        c = coords27(x, n, itg, distorted)
        self.coords, self.A, self.dinv, self.P, self.K = [], [], [], [], []
        lattice = tuple(2 * v + 1 for v in n)
        for l, ne in enumerate(self.levels):
            if l:  # injection: coarse point (i, j, k) takes fine point (2 i, 2 j, 2 k); 0 -> 1: the corner nodes of the hex-27 elements
                c = c.reshape(*lattice, 3)[::2, ::2, ::2].reshape(-1, 3).copy()
                lattice = tuple(v + 1 for v in ne)
                K = oracle_level(x, ne, itg, c, robin, h)[0]
            else:
                K = oracle_level27(x, ne, itg, c, robin, h)
            d = K.diagonal()
            assert (d < 0).all()
            self.coords.append(c)
            self.K.append(K)
            self.A.append((-K).tocsr())
            self.dinv.append(1.0 / np.abs(d))
            if l:
                self.P.append(interpolation(ne))
                assert self.P[-1].shape == (self.A[l - 1].shape[0], self.A[l].shape[0])
        self.lam = None


class _Built:
    pass


_CACHE = {}


def _built(mf, row, shared=True, **opts):
    import torch

    key = (row[0], row[1], tuple(row[2]), row[3], row[4], tuple(sorted(opts.items())))
    if shared and key in _CACHE:
        return _CACHE[key]
    x, n, robin, h, itg = row[:5]
    S = _Built()
    S.row = row
    S.twin = Twin27(x, n, itg, robin, h, max_levels=opts.get("max_levels", 12) or 12)
    S.brick = mf.make_Brick(x, n, 2, itg)
    for d in range(3):
        S.brick.coords_view(d).copy_(_dev(S.twin.coords[0][:, d]))
    S.op = S.brick.thermal_operator_hex27(K_COND, h, TENV, _bits(robin))
    S.mg = S.op.multigrid(**opts).setup()
    S.info = S.mg.info()
    S.twin.lam = list(S.info["lambda_max"])
    S.n = S.op.n
    S.u = np.random.default_rng(3).uniform(-1.0, 1.0, S.n)
    S.b = S.twin.A[0] @ S.u
    S.r = np.random.default_rng(5).uniform(-1.0, 1.0, S.n)
    torch.cuda.synchronize()
    if shared:
        _CACHE[key] = S
    return S


def _tol(S, rel=1e-8):
    return rel * float(np.linalg.norm(S.b)) / np.sqrt(S.n)


def _signed_diagonal(op):
    import torch
    from metafem_jl_amd import _lib

    d = torch.zeros(op.n, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.mfem_debug_brick_operator_signed_diagonal(op.ctx._h, op._h, d.data_ptr()))
    return d.cpu().numpy()


# ---- 1. the cycle against the twin -------------------------------------------------------------------------------------------------------------------
CYCLE_ROWS = [0, 1, 2, 4, 5, 7, 8]


@pytest.mark.parametrize("i", CYCLE_ROWS, ids=[ROW_IDS[i] for i in CYCLE_ROWS])
def test_cycle_equals_the_twin(mf, i):
    """apply(r) on a random r against the twin: 1e-10 of max |z|, the project's bound for a cycle (tests/test_gpu_brick_multigrid.py)."""
    S = _built(mf, ROWS[i])
    assert S.info["levels"] == len(S.twin.levels) and [tuple(e) for e in S.info["ne"]] == S.twin.levels
    assert S.info["levels"] >= 2 and tuple(S.info["ne"][0]) == tuple(S.info["ne"][1]) == tuple(ROWS[i][1])
    assert S.info["sign"] == -1
    assert S.twin.levels == mf.multigrid_plan_hex27(ROWS[i][1])
    assert S.op._multigrid_create == "mfem_brick_multigrid_create_hex27"
    z = S.mg.apply(_dev(S.r)).cpu().numpy()
    want = S.twin.cycle(S.r)
    err = np.abs(z - want).max() / np.abs(want).max()
    print(f"{ROW_IDS[i]}: {S.info['levels']} levels, |z - z_twin| / max|z| = {err:.2e}")
    assert np.isfinite(z).all()
    assert err <= 1e-10


def test_info_bytes_are_exact(mf):
    for i in (0, 7):
        S = _built(mf, ROWS[i])
        total = 16
        for l, ne in enumerate(S.twin.levels):
            pts = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1) if l else (2 * ne[0] + 1) * (2 * ne[1] + 1) * (2 * ne[2] + 1)
            total += (5 if l else 3) * ((pts + 31) // 32 * 32) * 8
            if l:
                total += 3 * pts * 8 + sum(16 * (e + 1) + 8 for e in ne)
        assert S.info["bytes"] == total


# ---- 2. the transfers between levels 0 and 1 ----------------------------------------------------------------------------------------------------------
# (the prolongation's tile is 64 fine points along k: 63 and 65 points sit one short of and one past it; 1x1x1 is the smallest lattice, 3^3 -> 2^3)
@pytest.mark.parametrize("n", [(1, 1, 1), (2, 3, 31), (3, 2, 32), (3, 5, 7)], ids=lambda n: "x".join(map(str, n)))
def test_transfers_between_the_hex27_level_and_the_hex8_level_below(mf, n):
    import torch
    from metafem_jl_amd import _lib

    c = coords27(XB, n, 5)
    brick = mf.make_Brick(XB, n, 2, 5)
    for d in range(3):
        brick.coords_view(d).copy_(_dev(c[:, d]))
    op = brick.thermal_operator_hex27(K_COND, 25.0, TENV, 0x3F)
    mg = op.multigrid(max_levels=2).setup()
    info = mg.info()
    assert info["levels"] == 2 and tuple(info["ne"][0]) == tuple(info["ne"][1]) == n
    P = interpolation(n)
    nf_pts, nc_pts = P.shape
    assert nf_pts == brick.ncp == (2 * n[0] + 1) * (2 * n[1] + 1) * (2 * n[2] + 1) and nc_pts == (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
    rng = np.random.default_rng(17)
    e, r = rng.integers(-8, 9, nc_pts).astype(np.float64), rng.integers(-8, 9, nf_pts).astype(np.float64)
    h = _lib.lib
    pe = torch.full((nf_pts,), float("nan"), dtype=torch.float64, device="cuda")
    ptr = torch.full((nc_pts,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(h.mfem_debug_brick_multigrid_transfer(op.ctx._h, mg._h, 0, 0, _dev(e).data_ptr(), pe.data_ptr()))
    _lib.check(h.mfem_debug_brick_multigrid_transfer(op.ctx._h, mg._h, 0, 1, _dev(r).data_ptr(), ptr.data_ptr()))
    # integer input, weights that are powers of two: every product and sum is exact, so the sparse Kronecker interpolation is met bit for bit
    assert np.array_equal(pe.cpu().numpy(), P @ e)
    assert np.array_equal(ptr.cpu().numpy(), P.T @ r)
    for d in range(3):  # the hex-8 level's coordinates are the even lattice points of the hex-27 brick, bit for bit
        cp = h.mfem_debug_brick_multigrid_coords(mg._h, 1, d)
        got = mf._tensor_from_ptr(cp, nc_pts, torch.float64, op.ctx.device, owner=mg).cpu().numpy()
        want = c[:, d].reshape(2 * n[0] + 1, 2 * n[1] + 1, 2 * n[2] + 1)[::2, ::2, ::2].reshape(-1)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), d
    assert h.mfem_debug_brick_multigrid_coords(mg._h, 2, 0) is None


# ---- 3. the signed diagonal ------------------------------------------------------------------------------------------------------------------------------
# element counts of 1, 8 and 9 per direction (a tile of 8 element columns ends, the next holds one), 34 planes (the segments of the sweep end inside
# the brick and a halo plane is integrated for the carry), an undistorted brick (the affine shortcut), the three rules
DIAG_CASES = [((1, 1, 1), 5, True, 0x3F), ((9, 8, 1), 5, True, 0x3F), ((1, 9, 8), 5, True, 0x15), ((8, 1, 9), 7, True, 0x3F), ((34, 2, 2), 5, True, 0x3F),
              ((3, 9, 2), 5, False, 0x3F), ((2, 3, 2), 3, True, 0x3F), ((5, 4, 3), 5, True, 0)]


@pytest.mark.parametrize("n,itg,distorted,mask", DIAG_CASES, ids=["x".join(map(str, c[0])) + f"-itg{c[1]}" + ("" if c[2] else "-affine") + f"-{c[3]:02x}" for c in DIAG_CASES])
def test_signed_diagonal_equals_the_oracles(mf, n, itg, distorted, mask):
    """K_ii with its sign against the oracle's K: 1e-12 of max |d|, the bound tests/test_gpu_brick_operator_hex27.py uses for op.diagonal()"""
    robin = [f for f in range(6) if mask >> f & 1]
    c = coords27(XB, n, itg, distorted)
    want = oracle_level27(XB, n, itg, c, robin, 25.0).diagonal()
    brick = mf.make_Brick(XB, n, 2, itg)
    for d in range(3):
        brick.coords_view(d).copy_(_dev(c[:, d]))
    op = brick.thermal_operator_hex27(K_COND, 25.0, TENV, mask)
    got = _signed_diagonal(op)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{n} itg {itg} faces {mask:#x}: |d - d_oracle| / max|d| = {err:.2e}")
    assert (got < 0).all()
    assert err <= 1e-12
    assert _signed_diagonal(op).tobytes() == got.tobytes()  # no atomics: the same bits on every run
    absd = op.diagonal().cpu().numpy()  # (Pr_Jacobi_'s kernel, untouched: |K_ii|)
    assert np.abs(absd + got).max() <= 1e-12 * np.abs(want).max()


def test_signed_diagonal_on_every_face_with_and_without_robin(mf):
    n, itg = (2, 3, 2), 5
    c = coords27(XB, n, itg)
    brick = mf.make_Brick(XB, n, 2, itg)
    for d in range(3):
        brick.coords_view(d).copy_(_dev(c[:, d]))
    op = brick.thermal_operator_hex27(K_COND, 25.0, TENV, 0)
    for mask in [1 << f for f in range(6)] + [0x3F ^ (1 << f) for f in range(6)]:
        robin = [f for f in range(6) if mask >> f & 1]
        op.set_params(K_COND, 25.0, TENV, mask)
        want = oracle_level27(XB, n, itg, c, robin, 25.0).diagonal()
        got = _signed_diagonal(op)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), hex(mask)


def _sha_brick(mf, n, itg, distorted, mask):
    """the bricks whose mfem_brick_operator_diagonal bits tools/brick_multigrid_hex27_time.py --record-diagonal recorded on the parent commit: the
    library's own coordinates, moved by a formula in torch (no oracle)"""
    import torch

    brick = mf.make_Brick(XB, n, 2, itg)
    if distorted:
        c = [brick.coords_view(d).clone() for d in range(3)]
        brick.coords_view(0).add_(0.03 * torch.sin(3 * c[1]) * torch.cos(2 * c[2]))
        brick.coords_view(1).add_(0.02 * torch.sin(2 * c[0] + c[2]))
        brick.coords_view(2).add_(0.025 * c[0] * c[1])
    return brick, brick.thermal_operator_hex27(K_COND, 25.0, TENV, mask)


def test_jacobi_diagonal_keeps_the_parents_bits(mf):
    """mfem_brick_operator_diagonal (Pr_Jacobi_'s kernel) is not touched by the sweep: SHA-256 of its result, recorded on the parent commit"""
    import torch

    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "brick_multigrid_hex27_diagonal_sha256.json")))
    assert len(golden["cases"]) >= 3
    for case in golden["cases"]:
        brick, op = _sha_brick(mf, tuple(case["n"]), case["itg"], case["distorted"], case["robin_faces"])
        mg = op.multigrid().setup()  # (with a hierarchy attached and set up: the sweep has run on this operator)
        d = op.diagonal().cpu().numpy()
        assert hashlib.sha256(d.tobytes()).hexdigest() == case["sha256"], case
        x = torch.linspace(-1.0, 1.0, op.n, dtype=torch.float64, device="cuda")  # (and the product's bits beside it)
        y = op.mul_(torch.empty_like(x), x).cpu().numpy()
        assert hashlib.sha256(y.tobytes()).hexdigest() == case["product_sha256"], case
        mg.close()


# ---- 4. the solves ---------------------------------------------------------------------------------------------------------------------------------------
_ITER = {}


def _solve_row(mf, i):
    if i in _ITER:
        return _ITER[i]
    S = _built(mf, ROWS[i])
    tol = _tol(S)
    b = _dev(-S.b)  # K x = -b  <=>  A x = b (A = -K)
    sol, st = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)
    _, it_twin = S.twin.pcg(S.b, tol)
    # b = A u by construction, so a direct solve returns u up to its own rounding.  The banded Cholesky of the oracle's matrix runs on every row but
    # 16^3 (35 937 rows under a band of 2 200: 40 s on a CPU) and has to return u to 1e-9 there; at 16^3 u itself stands for it.
    direct = S.u
    if S.n < 20000:
        direct = _direct_solve(S.twin.A[0], S.b)
        assert np.abs(direct - S.u).max() <= 1e-9 * np.abs(S.u).max()
    err = np.abs(sol.cpu().numpy() - direct).max() / np.abs(direct).max()
    out = dict(converged=st.converged, it=st.iterations, spmv=st.spmv_count, twin=it_twin, err=err, levels=S.info["levels"])
    print(f"row {i} {ROW_IDS[i]}: {out['levels']} levels, MG {st.iterations} (twin {it_twin}, table {ROWS[i][5]}) iterations, |x - x_direct| / |x| = {err:.1e}")
    _ITER[i] = out
    return out


@pytest.mark.parametrize("i", range(len(ROWS)), ids=ROW_IDS)
def test_solve_needs_exactly_the_twins_iterations(mf, i):
    R = _solve_row(mf, i)
    assert R["converged"] == 1
    assert R["it"] == R["twin"]
    assert R["twin"] <= ROWS[i][5] + 2  # (the table used 0.98 x the true lambda_max; the device's estimate differs slightly)
    assert R["err"] <= 1e-6
    assert R["spmv"] == R["it"] + 2 * NU * R["it"] + 1  # x0 = 0


def test_iterations_do_not_grow_with_the_mesh(mf):
    assert _solve_row(mf, 3)["it"] <= _solve_row(mf, 2)["it"]


def _count_check(mf, S, nu, nu_c, **kw):
    L = S.info["levels"]
    per_cycle = [(nu_c - 1) if l == L - 1 else 2 * nu for l in range(L)]
    before = S.mg.info()
    sol, st = mf.iterative_Solve(S.op, None, _dev(-S.b), kw.pop("tol", _tol(S)), Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, max_pass=1, **kw)
    after = S.mg.info()
    it = st.iterations
    cycles = after["cycles"] - before["cycles"]
    assert cycles == it
    assert st.spmv_count == (it + 2 * nu * it + 1 if it >= 1 else 1)
    assert [a - b_ for a, b_ in zip(after["products"], before["products"])] == [c * cycles for c in per_cycle]
    assert after["setups"] == before["setups"] + 1  # a solve always runs the setup
    return st


def test_product_counts_with_nu_3_and_on_a_two_level_plan(mf):
    S = _built(mf, ROWS[0])
    st = _count_check(mf, S, NU, NU_C, maxiter=200)
    assert st.converged == 1 and st.iterations >= 1
    assert _count_check(mf, S, NU, NU_C, maxiter=3, fixed_iterations=True).iterations == 3
    assert _count_check(mf, S, NU, NU_C, maxiter=200, tol=10.0 * float(np.linalg.norm(S.b))).iterations == 0
    S3 = _built(mf, ROWS[4], smoother_degree=3, coarse_degree=8)
    assert _count_check(mf, S3, 3, 8, maxiter=200).converged == 1
    z = S3.mg.apply(_dev(S3.r)).cpu().numpy()
    want = S3.twin.cycle(S3.r, nu=3, nu_c=8)
    assert np.abs(z - want).max() / np.abs(want).max() <= 1e-10
    S2 = _built(mf, ROWS[0], max_levels=2)
    assert S2.info["levels"] == 2
    assert _count_check(mf, S2, NU, NU_C, maxiter=200).converged == 1
    z = S2.mg.apply(_dev(S2.r)).cpu().numpy()
    want = S2.twin.cycle(S2.r)
    assert np.abs(z - want).max() / np.abs(want).max() <= 1e-10


# ---- 5. bits, liveness, symmetry ---------------------------------------------------------------------------------------------------------------------------
def test_two_solves_and_a_recreated_hierarchy_give_the_same_bits(mf):
    S = _built(mf, ROWS[4], shared=False)  # (its hierarchy is closed below)
    b = _dev(-S.b)
    solve = lambda: mf.iterative_Solve(S.op, None, b, _tol(S), Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=200, max_pass=1)[0].cpu().numpy().tobytes()
    a = solve()
    assert solve() == a
    S.mg.close()
    assert S.op._mg is None
    with pytest.raises(mf.MetaFEMError, match="mfem_brick_multigrid_create_hex27"):  # no default hierarchy is made for hex-27
        solve()
    S.op.multigrid()
    assert solve() == a
    S.op.close()


def test_parameters_and_coordinates_are_read_live(mf):
    x, n, robin, h, itg = ROWS[4][:5]
    c0 = coords27(x, n, itg)

    def fresh(k, hh, coords):
        brick = mf.make_Brick(x, n, 2, itg)
        for d in range(3):
            brick.coords_view(d).copy_(_dev(coords[:, d]))
        op = brick.thermal_operator_hex27(k, hh, TENV, _bits(robin))
        op.multigrid()
        return brick, op

    b = _dev(np.random.default_rng(3).uniform(-1, 1, c0.shape[0]))
    tol = 1e-8 * float(b.norm()) / np.sqrt(b.numel())
    kw = dict(Sv_func=mf.cg_, maxiter=300, max_pass=1)
    brick, op = fresh(K_COND, h, c0)
    jac_before = mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Jacobi_, **kw)[0].cpu().numpy().tobytes()
    first = mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Multigrid_, **kw)[0]
    assert mf.iterative_Solve(op, None, b, tol, Pr_func=mf.Pr_Jacobi_, **kw)[0].cpu().numpy().tobytes() == jac_before
    moved = c0 * np.array([1.0, 1.02, 0.97])
    op.set_params(2.0 * K_COND, 3.0, TENV, _bits(robin))
    _, op2 = fresh(2.0 * K_COND, 3.0, c0)
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


@pytest.mark.parametrize("i", [0, 5], ids=[ROW_IDS[0], ROW_IDS[5]])
def test_cycle_is_symmetric_positive_and_linear(mf, i):
    S = _built(mf, ROWS[i])
    rng = np.random.default_rng(23)
    M = lambda v: S.mg.apply(_dev(v)).cpu().numpy()
    for _ in range(5):
        r = rng.uniform(-1, 1, S.n)
        assert r @ M(r) > 0.0
    u, v = rng.uniform(-1, 1, S.n), rng.uniform(-1, 1, S.n)
    Mu, Mv = M(u), M(v)
    sym = abs(v @ Mu - u @ Mv) / abs(v @ Mu)
    lin = np.abs(M(2.0 * u - 3.0 * v) - (2.0 * Mu - 3.0 * Mv)).max() / np.abs(2.0 * Mu - 3.0 * Mv).max()
    print(f"{ROW_IDS[i]}: symmetry defect {sym:.1e}, linearity {lin:.1e}")
    assert sym <= 1e-12 and lin <= 1e-12


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_missing_and_touch_nothing(mf):
    import torch
    from metafem_jl_amd import _lib

    lib = _lib.lib
    n = (2, 2, 2)
    b27 = mf.make_Brick(XU, n, 2, 5)
    ctx = b27.ctx
    N = b27.ncp

    def refused(handle, nn, method=mf.cg_, left=0):
        x = torch.full((nn,), float("nan"), dtype=torch.float64, device="cuda")  # the canary
        bb = torch.ones(nn, dtype=torch.float64, device="cuda")
        o = _lib.SolveOptions(method=method, precond=mf.Pr_Multigrid_, l_or_s=0, maxiter=50, max_pass=1, check_every=8, converge_tol=1e-8, seed=1,
                              fixed_iterations=0, scale_in_place=0, left_precond=left, cg_variant=0)
        st = _lib.SolveStats()
        count = lib.mfem_debug_brick_operator_count()
        rc = lib.mfem_solve_operator(ctx._h, handle, bb.data_ptr(), x.data_ptr(), C.byref(o), C.byref(st))
        msg = lib.mfem_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -3, (rc, msg)
        assert bool(torch.isnan(x).all())
        assert lib.mfem_debug_brick_operator_count() == count
        return msg

    def create_refused(fn, handle, want_rc=-3):
        out = C.c_uint64(7)
        count = lib.mfem_debug_brick_operator_count()
        rc = getattr(lib, fn)(ctx._h, handle, None, C.byref(out))
        msg = lib.mfem_last_error().decode()
        assert rc == want_rc and out.value == 0, (fn, rc, msg)
        assert lib.mfem_debug_brick_operator_count() == count
        return msg

    op = b27.thermal_operator_hex27(K_COND, 25.0, TENV, 0x3F)
    nit = b27.thermal_operator_hex27(K_COND, 25.0, TENV, 0x1F, fixed_faces=0x20, h_penalty=1000.0, Tw=1173.15)
    b3 = mf.make_Brick(XU, n, 2, 3)  # two Gauss points per direction
    op3 = b3.thermal_operator_hex27(K_COND, 25.0, TENV, 0x3F)
    b8 = mf.make_Brick(XU, (4, 4, 4), 1, 3)
    th8 = b8.thermal_operator(K_COND, 25.0, TENV, 0x3F)
    el8 = b8.elasticity_operator(1.0, 1.0, 10.0, 0x10)
    cube = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.float64, device="cuda")  # one hex-8 element
    mop = mf.MeshOperator(ctx, 3, 8, 1, 8, 1, cube, torch.arange(1, 9, dtype=torch.int32, device="cuda"), 1)
    NEW = "mfem_brick_multigrid_create_hex27"
    # Pr_Multigrid_ on hex-27 with no hierarchy: hex-27 and the entry point are named
    msg = refused(op._h, N)
    assert "hex-27" in msg and NEW in msg
    # the create call: wrong kinds, Nitsche, the under-integrated rule
    assert "mfem_brick_multigrid_create" in create_refused(NEW, th8._h) and "thermal" in create_refused(NEW, th8._h)
    assert "mfem_brick_multigrid_create_elasticity" in create_refused(NEW, el8._h)
    assert "mesh operator" in create_refused(NEW, mop._h)
    assert "Nitsche" in create_refused(NEW, nit._h)
    m3 = create_refused(NEW, op3._h)
    assert "fewer than 3 Gauss points" in m3 and "near-null modes" in m3
    # wrong-kind handles in the other directions
    assert "hex-27" in create_refused("mfem_brick_multigrid_create", op._h) and NEW in create_refused("mfem_brick_multigrid_create", op._h)
    assert "hex-27" in create_refused("mfem_brick_multigrid_create_elasticity", op._h)
    create_refused("mfem_brick_multigrid_create", el8._h)
    create_refused("mfem_brick_multigrid_create_elasticity", th8._h)
    # MFEM_ERR_INVALID as for the other two create calls
    out = C.c_uint64()
    assert lib.mfem_brick_multigrid_create_hex27(ctx._h, op._h, None, None) == -1
    assert lib.mfem_brick_multigrid_create_hex27(None, op._h, None, C.byref(out)) == -1
    assert lib.mfem_brick_multigrid_create_hex27(ctx._h, 0, None, C.byref(out)) == -1
    bad = _lib.MultigridOptions(0, 0, 0.5, 0.0, 0, 0)
    assert lib.mfem_brick_multigrid_create_hex27(ctx._h, op._h, C.byref(bad), C.byref(out)) == -1
    other = mf.Context(0)
    assert lib.mfem_brick_multigrid_create_hex27(other._h, op._h, None, C.byref(out)) == -1
    with pytest.raises(mf.MultigridRefused):
        nit.multigrid()
    with pytest.raises(mf.MultigridRefused, match="fewer than 3 Gauss points"):
        op3.multigrid()
    assert refused(op3._h, N) and refused(nit._h, N)  # (no hierarchy could be attached: the gate names the entry point)
    # with a hierarchy attached: the gate's own rows, then the parameters changed under it
    mg = op.multigrid()
    assert lib.mfem_brick_multigrid_create_hex27(ctx._h, op._h, None, C.byref(out)) == -1  # one per operator
    assert "MFEM_SOLVER_CG" in refused(op._h, N, method=mf.idrs_)
    assert "left" in refused(op._h, N, left=1)
    ar = _lib.ALLREDUCE_CB(lambda user, buf, count: 0)
    ex = _lib.EXCHANGE_CB(lambda user, a, b_, c, d, count: 0)
    ops = _lib.CommHostOps(None, ar, ex, 0, 0)
    comm = C.c_void_p()
    _lib.check(lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(comm)))
    try:
        _lib.check(lib.mfem_context_set_comm(ctx._h, comm, N, (2 * n[1] + 1) * (2 * n[2] + 1), 1))
        assert "communicator" in refused(op._h, N)
    finally:
        lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        lib.mfem_comm_destroy(comm)
    op.set_params(K_COND, 25.0, TENV, 0x1F, fixed_faces=0x20, h_penalty=1000.0, Tw=1173.15)  # a Nitsche term under an attached hierarchy
    assert "Nitsche" in refused(op._h, N)
    with pytest.raises(mf.MultigridRefused, match="Nitsche"):
        mg.setup()
    op.set_params(K_COND, 25.0, TENV, 0x3F)
    # every handle is still usable
    r = torch.ones(N, dtype=torch.float64, device="cuda")
    mg.setup()
    assert float(mg.apply(r) @ r) > 0.0
    sol, st = mf.iterative_Solve(op, None, r, 1e-10, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_, maxiter=100, max_pass=1)
    assert st.converged == 1
    sol, st = mf.iterative_Solve(nit, None, r, 1e-8, Sv_func=mf.idrs_, s=4)
    assert st.converged == 1
    y = op3.mul_(torch.full_like(r, float("nan")), r)
    assert bool(torch.isfinite(y).all())
    mg.close()


# ---- 7. the domain -----------------------------------------------------------------------------------------------------------------------------------------
def test_thermal_domain_with_multigrid_on_a_hex27_brick(mf):
    x, n, h = XB, (4, 3, 3), 25.0
    hist = []
    for kw in (dict(), dict(matrix_free="any", multigrid=True)):
        dom = mf.ThermalDomain(mf.make_Brick(x, n, 2, 5), K_COND, h, TENV, **kw)
        dom.s.fill_(1600.0)
        dom.converge_tol = 1e-9
        hist.append((dom.update_OneStep(), dom.x.cpu().numpy(), dom))
    d_mg = hist[1][2]
    assert d_mg.multigrid and d_mg.multigrid_reason is None and d_mg.K_linear is None and d_mg.K_total is None
    assert isinstance(d_mg.A, mf.Hex27BrickOperator) and d_mg.A._mg is d_mg.mg and d_mg.mg.info()["cycles"] > 0
    assert hist[1][0][-1] < 1e-9
    err = np.abs(hist[0][1] - hist[1][1]).max() / np.abs(hist[0][1]).max()
    print(f"histories {hist[0][0]} / {hist[1][0]}, |x - x_default| / |x| = {err:.1e}")
    assert err <= 1e-8
    x0 = mf.FACE_BITS["x0"]
    dom = mf.ThermalDomain(mf.make_Brick(x, (2, 2, 2), 2, 5), K_COND, h, TENV, mf.ALL_FACES & ~x0, fixed_faces=x0, h_penalty=1000.0, Tw=1173.15,
                           matrix_free="any", multigrid=True)
    assert not dom.multigrid and "nonsymmetric" in dom.multigrid_reason
    dom.s.fill_(1600.0)
    assert dom.update_OneStep()[-1] < dom.converge_tol  # the default solver runs
    dom = mf.ThermalDomain(mf.make_Brick(x, (2, 2, 2), 2, 3), K_COND, h, TENV, matrix_free="any", multigrid=True)
    assert not dom.multigrid and "fewer than 3 Gauss points" in dom.multigrid_reason
    dom = mf.ThermalDomain(mf.make_Brick(x, (2, 2, 2), 2, 5), K_COND, h, TENV, multigrid=True)
    assert not dom.multigrid and "assembled" in dom.multigrid_reason
