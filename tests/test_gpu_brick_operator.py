"""GPU: the matrix-free hex-8 brick operator (mfem_brick_operator_*: csrc/brick_operator.hip, its kernels: csrc/brick_operator_thermal.hip) against the assembled K of
mfem_brick_assemble_thermal on the CSR kernel and against the oracle's K -- product, diagonal, reproducibility, reductions across many
workgroups, every admitted solver through mfem_solve_operator, the refusals, and ThermalDomain(matrix_free=True)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
H_PEN, TW = 1000.0, 1173.15
X = (1.0, 1.5, 0.75)
ALL = [0, 1, 2, 3, 4, 5]

# n, itg, distorted, Robin faces, fixed faces
CASES = [
    ((1, 1, 1), 3, False, ALL, []),
    ((2, 1, 3), 1, True, [5], [3]),
    ((9, 14, 15), 3, True, ALL, []),           # 10 planes = 3 segments of 4; 15 and 16 points: a full tile and a one-point tile
    ((5, 16, 30), 5, True, [0, 1, 2, 3, 5], [4]),  # 17 x 31 points: 2 x 3 tiles
    ((4, 4, 3), 7, True, [2], [4, 5]),
    ((3, 4, 2), 5, True, [], ALL),
]
IDS = ["x".join(map(str, c[0])) + f"-itg{c[1]}" for c in CASES]


def _distort(c):
    out = c.copy()
    out[:, 0] += 0.03 * np.sin(3 * c[:, 1]) * np.cos(2 * c[:, 2])
    out[:, 1] += 0.02 * np.sin(2 * c[:, 0] + c[:, 2])
    out[:, 2] += 0.025 * c[:, 0] * c[:, 1]
    return out


def _bits(faces):
    return sum(1 << f for f in faces)


def _oracle(x, n, itg, distorted, robin, fixed):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    if distorted:
        msh.coords[:] = _distort(msh.coords)
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = []
    if robin:
        bnd.append((fac.select(np.isin(fac.element_eindex, robin)), problems.thermal_convection(H, TENV)))
    if fixed:
        bnd.append((fac.select(np.isin(fac.element_eindex, fixed)), problems.thermal_fixed(3, H_PEN, TW, K_COND)))
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, K_COND), bnd)
    od.controlpoints["s"] = np.full(msh.ncp, SRC)
    return od


class _Built:
    pass


_CACHE = {}


def _built(mf, case):
    """brick, operator, assembled (A, K) and the oracle's K of a case: computed once, shared, never changed"""
    import scipy.sparse as sp
    import torch

    key = (case[0], case[1])
    if key in _CACHE:
        return _CACHE[key]
    n, itg, distorted, robin, fixed = case
    od = _oracle(X, n, itg, distorted, robin, fixed)
    od.update_time()
    od.K_linear_func()
    S = _Built()
    S.Ko = sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)
    S.brick = mf.make_Brick(X, n, 1, itg)
    if distorted:
        for d in range(3):
            S.brick.coords_view(d).copy_(torch.tensor(od.mesh.coords[:, d], device="cuda"))
    S.kw = dict(fixed_faces=_bits(fixed), h_penalty=H_PEN, Tw=TW)
    S.A = S.brick.pattern(1)
    S.K = S.brick.assemble_thermal(S.A, K_COND, H, TENV, _bits(robin), **S.kw)
    S.op = S.brick.thermal_operator(K_COND, H, TENV, _bits(robin), **S.kw)
    S.n = S.A.n
    rng = np.random.default_rng(11)
    S.x = rng.uniform(-1.0, 1.0, S.n)
    S.y0 = rng.uniform(-1.0, 1.0, S.n)
    _CACHE[key] = S
    return S


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")


# ---- 1. product ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_equals_csr_kernel_and_oracle(mf, case):
    import torch

    S = _built(mf, case)
    assert isinstance(S.op, mf.BrickOperator) and S.op.n == S.n
    x = _dev(S.x)
    for alpha, beta in ((1.0, 0.0), (-0.7, 0.3)):
        y_in = torch.full_like(x, float("nan")) if beta == 0.0 else _dev(S.y0)  # beta == 0: y must not be read
        got = mf.mul_(y_in, S.op, None, x, alpha, beta).cpu().numpy()
        want_csr = mf.mul_(_dev(S.y0), S.A, S.K, x, alpha, beta).cpu().numpy()
        want_or = alpha * (S.Ko @ S.x) + beta * S.y0
        e_csr = np.abs(got - want_csr).max() / np.abs(want_csr).max()
        e_or = np.abs(got - want_or).max() / np.abs(want_or).max()
        print(f"{case[0]} itg {case[1]} ({alpha}, {beta}): vs CSR kernel {e_csr:.2e}, vs oracle {e_or:.2e}")
        assert np.isfinite(got).all()
        assert e_csr <= 1e-12, (alpha, beta)
        assert e_or <= 1e-11, (alpha, beta)


@pytest.mark.parametrize("case", [CASES[2], CASES[3], CASES[4]], ids=[IDS[2], IDS[3], IDS[4]])
def test_product_with_a_column_scaling(mf, case):
    """The solvers on A D^-1 hand d = |diag K| to the product, which reads x_j / d_j: idrs!(8) with Pr_Jacobi! on b = K x0, the residual of its x
    recomputed with the CSR kernel on the assembled K."""
    S = _built(mf, case)
    x0 = _dev(S.x)
    b = mf.mul_(_dev(S.y0), S.A, S.K, x0)
    tol = 1e-8 * float(b.abs().max())
    sol, st = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, s=8, maxiter=2000, max_pass=4)
    res = float((b - mf.mul_(_dev(S.y0), S.A, S.K, sol)).norm()) / np.sqrt(S.n)
    print(f"{case[0]}: idrs!(8) + Pr_Jacobi!: {st.iterations} iterations, residual {res:.2e} (tol {tol:.2e})")
    assert st.converged == 1 and res <= 2 * tol


# ---- 2. diagonal --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_diagonal_equals_jacobi_by_diagonal_of_the_assembled_matrix(mf, case):
    S = _built(mf, case)
    d = S.op.diagonal().cpu().numpy()
    want = mf.jacobi_by_diagonal(S.A, S.K).cpu().numpy()
    err = np.abs(d - want).max() / np.abs(want).max()
    print(f"{case[0]} itg {case[1]}: |d - d_assembled| / max|d| = {err:.2e}")
    assert err <= 1e-12


def test_zero_diagonal_keeps_the_preset(mf):
    op = mf.make_Brick(X, (3, 2, 4), 1, 3).thermal_operator(0.0)
    d = op.diagonal(preset=7.5).cpu().numpy()
    assert (d == 7.5).all()


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------------------------------
def test_two_applications_and_two_solves_give_the_same_bits(mf):
    import torch

    S = _built(mf, CASES[3])
    x = _dev(S.x)
    a = S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    assert S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == a
    b = mf.mul_(torch.empty_like(x), S.A, S.K, x)
    xs = [mf.iterative_Solve(S.op, None, b, 1e-8 * float(b.abs().max()), Sv_func=mf.idrs_, s=8, seed=0x5EED, maxiter=2000,
                             max_pass=4)[0].cpu().numpy().tobytes() for _ in range(2)]
    assert xs[0] == xs[1]


# ---- 4. reductions across many workgroups -----------------------------------------------------------------------------------------------------
def test_reductions_across_many_workgroups_with_and_without_cycle_graphs(mf):
    """n = (40, 45, 45): 41 x 46 x 46 points = 16 tiles x 11 segments.  cg! with check_every = 7: iteration count and x of the assembled path on the CSR
    kernel, to what test_cg_iterates_match_oracle_cg allows (equal counts, 1e-9 relative)."""
    import torch
    from metafem_jl_amd import _lib

    brick = mf.make_Brick((1.0, 1.0, 1.0), (40, 45, 45), 1, 3)
    A = brick.pattern(1)
    K = brick.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    op = brick.thermal_operator(K_COND, H, TENV, 0x3F)
    s = torch.full((A.n,), SRC, dtype=torch.float64, device="cuda")
    b = brick.residual_thermal(torch.zeros_like(s), K_COND, H, TENV, 0x3F, s=s)
    kw = dict(Sv_func=mf.cg_, maxiter=1000, max_pass=1, check_every=7)
    try:
        _lib.check(_lib.lib.mfem_debug_set_ell(0))  # the assembled path on the CSR kernel
        ref, st_ref = mf.iterative_Solve(A, K, b, 1e-8, **kw)
        assert st_ref.converged == 1
        for graphs in (1, 0):
            _lib.check(_lib.lib.mfem_debug_set_graphs(graphs, 0))
            got, st = mf.iterative_Solve(op, None, b, 1e-8, **kw)
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            print(f"graphs {graphs}: {st.iterations} iterations (assembled: {st_ref.iterations}), |x - x_csr| / |x| = {err:.2e}")
            assert st.converged == 1
            assert st.iterations == st_ref.iterations
            assert err <= 1e-9
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)
        _lib.lib.mfem_debug_set_ell(1)


@pytest.mark.parametrize("n,itg,items", [((80, 80, 80), 1, 21 * 21 * 11), ((4, 640, 620), 3, 43 * 42 * 2)], ids=["tiles-80x80x80-itg1", "sweep-4x640x620-itg3"])
def test_work_items_folded_onto_the_capped_grid(mf, n, itg, items):
    """More work items than the 3584 partial sums of the volume kernel: inside cg! (which asks for p . A p) a workgroup sweeps several items -- LDS
    reused across items, one dot sum across items, gridDim below the item count.  The smallest such bricks: 81^3 points in 4 x 4 x 8 tiles (4851
    items) for the tile form, and 5 planes (two 4-plane segments) of 43 x 42 tiles (3612 items) for the sweep.  Iteration count and x of the assembled
    path on the CSR kernel, as above; the unfolded product (mul_, no partial sums) against the CSR kernel too."""
    import torch
    from metafem_jl_amd import _lib

    assert items > 4096 - 512
    brick = mf.make_Brick((1.0, 1.0, 1.0), n, 1, itg)
    A = brick.pattern(1)
    K = brick.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    op = brick.thermal_operator(K_COND, H, TENV, 0x3F)
    s = torch.full((A.n,), SRC, dtype=torch.float64, device="cuda")
    b = brick.residual_thermal(torch.zeros_like(s), K_COND, H, TENV, 0x3F, s=s)
    want = mf.mul_(torch.empty_like(b), A, K, b)
    got = op.mul_(torch.full_like(b, float("nan")), b)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    tol = 1e-8 * mf.normalized_norm(b)
    kw = dict(Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=2000, max_pass=1, check_every=7)
    try:
        _lib.check(_lib.lib.mfem_debug_set_ell(0))  # the assembled path on the CSR kernel
        ref, st_ref = mf.iterative_Solve(A, K, b, tol, **kw)
    finally:
        _lib.lib.mfem_debug_set_ell(1)
    sol, st = mf.iterative_Solve(op, None, b, tol, **kw)
    err = float((sol - ref).abs().max()) / float(ref.abs().max())
    print(f"{n} itg {itg}: {items} items, {st.iterations} iterations (assembled: {st_ref.iterations}), |x - x_csr| / |x| = {err:.2e}")
    assert st_ref.converged == 1 and st.converged == 1
    assert st.iterations == st_ref.iterations
    assert err <= 1e-9
    again, _ = mf.iterative_Solve(op, None, b, tol, **kw)
    assert again.cpu().numpy().tobytes() == sol.cpu().numpy().tobytes()


def test_cached_cycle_replays_with_its_own_gauss_rule(mf):
    """Two identical Identity solves on an itg 3 operator with Nitsche faces (the face kernel reads the reference tables), cycle graphs on: the second
    replays the first one's cached cycles.  In between, operators with other rules (itg 5, 7, 1) serve products and diagonals.  One fixed pass, so that
    nothing after the pass repairs it: the same bits both times, and the assembled residual says the answer is right."""
    import torch

    S = _form(mf, nitsche=True)
    kw = dict(Sv_func=mf.idrs_, Pr_func=mf.Identity, s=8, maxiter=60, max_pass=1, fixed_iterations=True)
    first, st1 = mf.iterative_Solve(S.op, None, S.b, 1e-300, **kw)
    for itg in (5, 7, 1):
        other = mf.make_Brick(X, (3, 2, 4), 1, itg).thermal_operator(K_COND, H, TENV, _bits([0, 1]), fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)
        v = torch.ones(other.n, dtype=torch.float64, device="cuda")
        other.mul_(torch.empty_like(v), v)
        other.diagonal()
    second, st2 = mf.iterative_Solve(S.op, None, S.b, 1e-300, **kw)
    assert st1.spmv_count == st2.spmv_count
    assert second.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()
    res = float((S.b - mf.mul_(torch.empty_like(second), S.A, S.K, second)).norm()) / np.sqrt(S.n)
    assert abs(res - st2.final_res) <= 1e-6 * float(S.b.abs().max()), (res, st2.final_res)


# ---- 5. every admitted solver ---------------------------------------------------------------------------------------------------------------------
# name -> (Sv_func attribute, s)
SOLVERS = {"cg": ("cg_", 0), "bicgstabl": ("bicgstabl_GS_", 2), "idrs": ("idrs_", 8), "cgs2": ("cgs2_", 0), "gmres": ("gmres_", 0), "cgs": ("cgs_", 0),
           "tfqmr": ("tfqmr_", 0)}
MAXITER, MAX_PASS, GMRES_S, CHECKITER = 2000, 4, 20, 200


def _cap(name, maxiter):
    """the iteration count a pass returns when maxiter ends it"""
    if name in ("cg", "idrs"):
        return maxiter
    if name == "bicgstabl":
        return 1 + 2 * -(-(maxiter - 1) // 2)
    if name == "gmres":
        return 1 + GMRES_S * -(-maxiter // GMRES_S)
    return maxiter + 1


def _pass_products(name, it, maxiter):
    """products of one pass that returned `it` iterations (include/metafem_mi355x.h), without the start-of-pass and the wrapper's residual"""
    if it == 0:
        return 0
    if name in ("cg", "idrs"):
        return it
    if name in ("bicgstabl", "cgs2", "cgs"):
        return 2 * (it - 1)
    if name == "gmres":
        assert (it - 1) % GMRES_S == 0, it
        return (it - 1) + (it - 1) // GMRES_S
    checks = sum(1 for j in range(2, it + 1) if j % CHECKITER == 0 and j <= maxiter)
    return 1 + 2 * (it - 1) + checks


def _expected_products(name, st):
    cap = _cap(name, MAXITER)
    its = [cap] * (st.passes - 1) + [st.iterations - (st.passes - 1) * cap]
    return sum((1 if p > 0 else 0) + _pass_products(name, it, MAXITER) + 1 for p, it in enumerate(its))


# products the host queues per solver cycle (krylov_*.hip: the cycle each pass hands to its driver): cg! an iteration; bicgstabl_GS!(l) a sweep of
# 2 l; idrs!(s) s + 1 steps; cgs2! and cgs! an iteration of 2; gmres!(s) a restart cycle of s + 1; tfqmr! an iteration of 2 plus its checkiter residual
CYCLE_PRODUCTS = {"cg": 1, "bicgstabl": 4, "idrs": 9, "cgs2": 2, "gmres": GMRES_S + 1, "cgs": 2, "tfqmr": 3}

_FORMS = {}


def _form(mf, nitsche):
    """(8, 7, 6), itg 3: the Robin form (symmetric) or the Nitsche form (x = 0 fixed, convection elsewhere: nonsymmetric); b = K x0"""
    import torch

    if nitsche in _FORMS:
        return _FORMS[nitsche]
    S = _Built()
    S.brick = mf.make_Brick((1.0, 1.0, 1.0), (8, 7, 6), 1, 3)
    robin, S.kw = (_bits([0, 1, 2, 3, 5]), dict(fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)) if nitsche else (0x3F, {})
    S.A = S.brick.pattern(1)
    S.K = S.brick.assemble_thermal(S.A, K_COND, H, TENV, robin, **S.kw)
    S.op = S.brick.thermal_operator(K_COND, H, TENV, robin, **S.kw)
    S.n = S.A.n
    x0 = _dev(np.random.default_rng(4).uniform(-1.0, 1.0, S.n))
    S.b = mf.mul_(torch.empty_like(x0), S.A, S.K, x0)
    # test 1 bounds the product's error by 1e-12 max|K x|; the solve's tolerance stands 1e4 above that: the factor 2 below never decides
    S.tol = 1e-8 * float(S.b.abs().max())
    _FORMS[nitsche] = S
    return S


@pytest.mark.parametrize("precond", ["Identity", "Pr_Jacobi_"])
@pytest.mark.parametrize("solver", list(SOLVERS))
def test_every_solver_converges_with_the_products_of_its_formula(mf, solver, precond):
    import torch
    from metafem_jl_amd import _lib

    S = _form(mf, nitsche=solver != "cg")
    sv, s = SOLVERS[solver]
    kw = dict(Sv_func=getattr(mf, sv), Pr_func=getattr(mf, precond), s=s, maxiter=MAXITER, max_pass=MAX_PASS)
    x, st = mf.iterative_Solve(S.op, None, S.b, S.tol, **kw)
    res = float((S.b - mf.mul_(torch.empty_like(x), S.A, S.K, x)).norm()) / np.sqrt(S.n)  # the CSR kernel on the assembled K
    print(f"{solver} + {precond}: {st.iterations} iterations, {st.passes} passes, {st.spmv_count} products, residual {res:.2e} (tol {S.tol:.2e})")
    assert st.converged == 1
    assert res <= 2 * S.tol
    assert st.spmv_count == _expected_products(solver, st)
    # The counter counts the products the HOST launched (a captured cycle once, when it is captured); spmv_count counts the products that RAN on the
    # device: what the host has queued behind the stop returns at once on done_flag.  Without cycle graphs and with check_every = 1 the host reads the
    # flags after every cycle, so only the rest of the cycle that holds the stop can be queued behind it: at most CYCLE_PRODUCTS - 1 launches.  That
    # pins the counter from both sides, and to EQUALITY for cg! (a cycle is one product) -- every product is one launch of the brick operator's, no
    # product is launched twice or re-run after the stop, and no other operator serves one.
    try:
        _lib.check(_lib.lib.mfem_debug_set_graphs(0, 0))
        c0, m0 = int(_lib.lib.mfem_debug_brick_operator_count()), int(_lib.lib.mfem_debug_mesh_operator_count())
        _, st2 = mf.iterative_Solve(S.op, None, S.b, S.tol, check_every=1, **kw)
        launched = int(_lib.lib.mfem_debug_brick_operator_count()) - c0
        print(f"  without graphs, check_every = 1: {st2.spmv_count} products ran, {launched} launched")
        assert st2.converged == 1 and st2.spmv_count == _expected_products(solver, st2)
        assert st2.spmv_count <= launched <= st2.spmv_count + CYCLE_PRODUCTS[solver] - 1
        assert int(_lib.lib.mfem_debug_mesh_operator_count()) == m0
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)


def test_cg_fixed_iterations(mf):
    """cg! at 37 fixed iterations: 38 products (the 37 A p and the true residual after the pass; x0 = 0 needs none) -- and, with nothing queued behind a
    stop, 38 launches of the brick operator."""
    from metafem_jl_amd import _lib

    S = _form(mf, nitsche=False)
    try:
        _lib.check(_lib.lib.mfem_debug_set_graphs(0, 0))
        c0 = int(_lib.lib.mfem_debug_brick_operator_count())
        _, st = mf.iterative_Solve(S.op, None, S.b, 1e-30, Sv_func=mf.cg_, maxiter=37, max_pass=1, fixed_iterations=True)
        assert st.iterations == 37 and st.passes == 1 and st.spmv_count == 37 + 1
        assert int(_lib.lib.mfem_debug_brick_operator_count()) - c0 == st.spmv_count
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)
    _, st = mf.iterative_Solve(S.op, None, S.b, 1e-30, Sv_func=mf.cg_, maxiter=37, max_pass=1, fixed_iterations=True)  # (with cycle graphs)
    assert st.iterations == 37 and st.passes == 1 and st.spmv_count == 37 + 1


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mf):
    import torch
    from metafem_jl_amd import _lib

    INVALID, UNSUPPORTED = -1, -3
    S = _form(mf, nitsche=True)
    ctx = S.brick.ctx
    p = _lib.ThermalParams(K_COND, H, TENV, 0x3F, 0, 0.0, 0.0)
    h = C.c_uint64(1)
    # a hex-27 brick, a slab
    b27 = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 2, 5)
    assert _lib.lib.mfem_brick_operator_create(ctx._h, b27._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"hex-27" in _lib.lib.mfem_last_error()
    with pytest.raises(mf.MetaFEMError):
        b27.thermal_operator(K_COND)
    slab = mf.make_Brick((1.0, 1.0, 1.0), (6, 2, 2), 1, 3)
    slab.set_slab(2, 5)
    assert _lib.lib.mfem_brick_operator_create(ctx._h, slab._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"slab" in _lib.lib.mfem_last_error()
    assert b27.pattern(1).n == 125 and slab.pattern(1).n == 3 * 9  # the bricks stay usable
    for refused, word in ((b27, "hex-27"), (slab, "slab")):  # the domain is built as the default one and says why
        dom = mf.ThermalDomain(refused, K_COND, H, TENV, matrix_free=True)
        assert dom.matrix_free is False and word in dom.matrix_free_reason
        assert isinstance(dom.A, mf.FEM_SpMat_CSR) and dom.K_linear is not None and dom.K_total is dom.K_linear
    assert _lib.lib.mfem_brick_operator_create(ctx._h, None, C.byref(p), C.byref(h)) == INVALID
    assert _lib.lib.mfem_brick_operator_create(ctx._h, S.brick._h, None, C.byref(h)) == INVALID

    b = S.b
    sentinel = 123.25
    x = torch.full_like(b, sentinel)
    st = _lib.SolveStats()
    n0 = int(_lib.lib.mfem_debug_brick_operator_count())

    def solve(c=ctx, handle=S.op._h, **kw):
        opt = dict(method=mf.idrs_, precond=1, l_or_s=8, maxiter=2000, max_pass=4, check_every=32, converge_tol=S.tol, seed=1)
        opt.update(kw)
        o = _lib.SolveOptions(**opt)
        return _lib.lib.mfem_solve_operator(c._h, handle, b.data_ptr(), x.data_ptr(), C.byref(o), C.byref(st))

    assert solve(method=mf.lsqr_) == UNSUPPORTED
    assert solve(precond=mf.Pr_Jacobi_colnorm_) == UNSUPPORTED
    assert solve(left_precond=mf.Pl_Jacobi_) == UNSUPPORTED
    assert solve(scale_in_place=1) == INVALID
    assert solve(handle=0) == INVALID
    ops = _lib.CommHostOps(None, _lib.ALLREDUCE_CB(lambda *a: 1), _lib.EXCHANGE_CB(lambda *a: 1), 0, 0)
    hc = C.c_void_p()
    _lib.check(_lib.lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(hc)))
    try:
        _lib.check(_lib.lib.mfem_context_set_comm(ctx._h, hc, S.n, 1, 1))
        assert solve() == INVALID
        assert b"one rank only" in _lib.lib.mfem_last_error()
    finally:
        _lib.lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        _lib.lib.mfem_comm_destroy(hc)
    other = mf.Context(0)
    try:
        y = torch.empty_like(b)
        assert solve(c=other) == INVALID  # an operator of another context
        assert b"another context" in _lib.lib.mfem_last_error()
        assert _lib.lib.mfem_brick_operator_apply(other._h, S.op._h, b.data_ptr(), y.data_ptr(), 1.0, 0.0) == INVALID
        assert _lib.lib.mfem_brick_operator_diagonal(other._h, S.op._h, y.data_ptr()) == INVALID
        assert _lib.lib.mfem_brick_operator_create(other._h, S.brick._h, C.byref(p), C.byref(h)) == INVALID
    finally:
        other.close()
    torch.cuda.synchronize()
    assert int(_lib.lib.mfem_debug_brick_operator_count()) == n0  # nothing launched
    assert bool((x == sentinel).all())                            # nothing written
    # a brick operator's handle is not a mesh operator's
    assert _lib.lib.mfem_mesh_operator_apply(ctx._h, S.op._h, b.data_ptr(), x.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_brick_operator_apply(ctx._h, 0, b.data_ptr(), x.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_brick_operator_apply(ctx._h, S.op._h, None, x.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_brick_operator_diagonal(ctx._h, S.op._h, None) == INVALID
    assert _lib.lib.mfem_brick_operator_set_params(S.op._h, None) == INVALID
    assert _lib.lib.mfem_brick_operator_destroy(0) == 0
    # ... and every handle is still usable
    assert solve() == 0 and st.converged == 1 and not bool((x == sentinel).any())
    res = float((b - mf.mul_(torch.empty_like(x), S.A, S.K, x)).norm()) / np.sqrt(S.n)
    assert res <= 2 * S.tol


def test_set_params_changes_the_product_and_coordinates_are_read_live(mf):
    import torch

    brick = mf.make_Brick(X, (4, 3, 5), 1, 3)
    A = brick.pattern(1)
    op = brick.thermal_operator(K_COND, H, TENV, 0x3F)
    x = _dev(np.random.default_rng(2).uniform(-1.0, 1.0, A.n))
    moved = _distort(np.stack([brick.coords_view(d).cpu().numpy() for d in range(3)], axis=1))  # move the coordinates under the operator
    for d in range(3):
        brick.coords_view(d).copy_(torch.tensor(moved[:, d], device="cuda"))
    op.set_params(2.0 * K_COND, H, TENV, _bits([0, 1]), fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)
    K = brick.assemble_thermal(A, 2.0 * K_COND, H, TENV, _bits([0, 1]), fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)
    want = mf.mul_(torch.empty_like(x), A, K, x)
    got = op.mul_(torch.empty_like(x), x)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- 7. ThermalDomain(matrix_free=True) -----------------------------------------------------------------------------------------------------------
def test_matrix_free_domain_reproduces_the_direct_solve(mf):
    from oracle import solvers

    x, n = (1.0, 1.0, 1.0), (12, 10, 8)
    od = _oracle(x, n, 3, False, ALL, [])
    od.converge_tol = 1e-9
    od.linear_solver = lambda d: solvers.solver_lu_cpu(d.pattern.rowptr, d.pattern.colidx, d.K_total, d.residue)
    od.update_one_step()

    brick = mf.make_Brick(x, n)
    brick.pattern = None  # never called
    dom = mf.ThermalDomain(brick, K_COND, H, TENV, matrix_free=True)
    assert dom.matrix_free is True and dom.matrix_free_reason is None
    assert isinstance(dom.A, mf.BrickOperator) and dom.K_linear is None and dom.K_total is None
    dom.s.fill_(SRC)
    dom.converge_tol = 1e-9
    stats = []

    def solver(gf):
        dx, st = mf.iterative_Solve(gf.A, gf.K_total, gf.residue, 1e-13, Sv_func=mf.cg_, maxiter=2000, max_pass=3)
        stats.append(st)
        return dx

    dom.linear_solver = solver
    hist = dom.update_OneStep()
    got = dom.x.cpu().numpy()
    assert len(hist) == 2 and hist[1] < 1e-9
    assert stats[0].converged == 1
    err = np.max(np.abs(got - od.x)) / np.max(np.abs(od.x))
    print(f"|x - x_LU| / |x| = {err:.2e}")
    assert err <= 1e-10


def test_matrix_free_domain_holds_no_matrix(mf):
    """32^3: no pattern, no values; device bytes (torch allocations + the library's workspace) under half the default domain's.  By count: the
    matrix-free domain holds x, dx, x_star, residue, s, the solve's dx and a cg! workspace of 7 vectors = ~14 n doubles; the default one adds the 27 n
    values, and its workspace a copy of them in the solver layout: at least 75 n doubles."""
    import torch
    from metafem_jl_amd import _lib

    n = (32, 32, 32)
    used = {}
    for matrix_free in (True, False):
        ctx = mf.Context(0)
        try:
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            brick = mf.make_Brick((1.0, 1.0, 1.0), n, 1, 3, ctx=ctx)
            if matrix_free:
                brick.pattern = None  # never called
            dom = mf.ThermalDomain(brick, K_COND, H, TENV, matrix_free=matrix_free)
            dom.s.fill_(SRC)
            dom.converge_tol = 1e-9
            dom.linear_solver = lambda gf: mf.iterative_Solve(gf.A, gf.K_total, gf.residue, 1e-12, Sv_func=mf.cg_, maxiter=2000, max_pass=3)[0]
            hist = dom.update_OneStep()
            torch.cuda.synchronize()
            assert len(hist) == 2 and hist[1] < 1e-9
            if matrix_free:
                assert dom.K_linear is None and dom.K_total is None and dom.A.nnz == 0 and not hasattr(dom.A, "rowptr")
            used[matrix_free] = torch.cuda.memory_allocated() - m0 + int(_lib.lib.mfem_debug_ws_bytes(ctx._h))
            npts = dom.A.n
            del dom, brick
        finally:
            ctx.close()
    print(f"device bytes: matrix-free {used[True]} ({used[True] / 8 / npts:.1f} n doubles), default {used[False]} ({used[False] / 8 / npts:.1f} n doubles)")
    assert used[True] < 0.5 * used[False]
