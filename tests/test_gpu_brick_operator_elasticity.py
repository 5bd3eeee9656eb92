"""GPU: the matrix-free hex-8 brick operator on three-field linear elasticity (mfem_brick_operator_create_elasticity,
csrc/brick_operator_elasticity.hip) against the assembled K of mfem_brick_assemble_elasticity on the CSR kernel and against the oracle's K --
product, diagonal, reproducibility, the fold onto the capped grid, every admitted solver through mfem_solve_operator, the refusals, and
ElasticityDomain(matrix_free=True).  The oracle's K is built as tests/test_gpu_elasticity_edges.py::_oracle builds it; the bounds are those of
tests/test_gpu_brick_operator.py.  Parity cases use tau = 1 (the penalty entries do not hide the elastic ones), the solves tau = 1000."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_MOD, NU = 1.0, 0.3
LAM, MU = E_MOD * NU / ((1 + NU) * (1 - 2 * NU)), E_MOD / (2 * (1 + NU))
TAU_ONE, TAU_REF = 1.0, 1000.0
X = (3.0, 1.0, 2.0)
FACE_NAMES = ["z0", "y0", "x1", "y1", "x0", "z1"]  # oracle face id f == bit f of the product's mask
ALL6 = "z0|y0|x1|y1|x0|z1"

# n, itg, distorted, penalty faces
CASES = [
    ((1, 1, 1), 3, False, ""),
    ((2, 1, 3), 1, True, "x0"),
    ((9, 14, 15), 3, True, "x0|z1"),  # sweep: 10 planes = 3 segments of 4; 15 and 16 points: a full tile and a one-point tile
    ((5, 16, 30), 2, True, ALL6),     # sweep: 17 x 31 points = 2 x 3 tiles
    ((4, 4, 3), 7, True, "x0"),       # point form, 4-point rule
    ((3, 4, 2), 5, True, "x0|z1"),    # point form, 3-point rule
]
IDS = ["x".join(map(str, c[0])) + f"-itg{c[1]}" for c in CASES]


def _ids(names):
    return [FACE_NAMES.index(s) for s in names.split("|")] if names else []


def _bits(mf, names):
    b = 0
    for s in (names.split("|") if names else []):
        b |= mf.FACE_BITS[s]
    return b


def _distort(c, x):
    return c + 0.03 * np.stack([np.sin(2 * c[:, 1]), np.cos(2 * c[:, 2]) - 1, c[:, 0] * c[:, 1] / x[0]], axis=1)


def _oracle(x, n, pen, tau, itg, distorted):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    if distorted:
        msh.coords = _distort(msh.coords, x)
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = []
    if pen:
        bnd.append((fac.select(np.isin(fac.element_eindex, _ids(pen))), problems.elasticity_penalty(3, tau)))
    od = fem.FEMDomain(msh, disc, 3, problems.elasticity_domain(3, LAM, MU), bnd)
    od.update_time()
    od.K_linear_func()
    return od


class _Built:
    pass


_CACHE = {}


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")


def _built(mf, case):
    """brick, operator, assembled (A, K) and the oracle's K of a case: computed once, shared, never changed"""
    import scipy.sparse as sp
    import torch

    key = (case[0], case[1])
    if key in _CACHE:
        return _CACHE[key]
    n, itg, distorted, pen = case
    od = _oracle(X, n, pen, TAU_ONE, itg, distorted)
    S = _Built()
    S.Ko = sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)
    S.brick = mf.make_Brick(X, n, 1, itg)
    if distorted:
        for d in range(3):
            S.brick.coords_view(d).copy_(torch.tensor(np.ascontiguousarray(od.mesh.coords[:, d]), device="cuda"))
    S.A = S.brick.pattern(3)
    S.K = S.brick.assemble_elasticity(S.A, LAM, MU, TAU_ONE, _bits(mf, pen))
    S.op = S.brick.elasticity_operator(LAM, MU, TAU_ONE, _bits(mf, pen))
    S.n = S.A.n
    rng = np.random.default_rng(11)
    S.x = rng.uniform(-1.0, 1.0, S.n)
    S.y0 = rng.uniform(-1.0, 1.0, S.n)
    _CACHE[key] = S
    return S


def _apply_dot(op, x, y, dotw, alpha=1.0, beta=0.0):
    """one product that leaves partial sums (what a solver's cycle launches): y, the partial sums, their number"""
    import torch
    from metafem_jl_amd import _lib

    partials = torch.zeros(4096, dtype=torch.float64, device="cuda")
    np_ = C.c_int32(-1)
    _lib.check(_lib.lib.mfem_debug_brick_operator_apply_dot(op.ctx._h, op._h, x.data_ptr(), y.data_ptr(), alpha, beta, dotw.data_ptr(),
                                                            partials.data_ptr(), C.byref(np_)))
    torch.cuda.synchronize()
    return y, partials, np_.value


# ---- 1. product ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_equals_csr_kernel_and_oracle(mf, case):
    import torch

    S = _built(mf, case)
    assert isinstance(S.op, mf.BrickOperator) and S.op.n == S.n == 3 * S.brick.ncp
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
    assert d.shape == (S.n,)
    assert err <= 1e-12


def test_zero_diagonal_keeps_the_preset(mf):
    op = mf.make_Brick(X, (3, 2, 4), 1, 3).elasticity_operator(0.0, 0.0, 0.0, 0)
    d = op.diagonal(preset=7.5).cpu().numpy()
    assert d.shape == (3 * 4 * 3 * 5,) and (d == 7.5).all()


# ---- 3. reproducibility and the fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
def test_two_applications_and_two_solves_give_the_same_bits(mf, case):
    import torch

    S = _built(mf, case)
    x = _dev(S.x)
    a = S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    assert S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == a
    b = mf.mul_(torch.empty_like(x), S.A, S.K, x)
    xs = [mf.iterative_Solve(S.op, None, b, 1e-8 * float(b.abs().max()), Sv_func=mf.idrs_, s=8, seed=0x5EED, maxiter=2000,
                             max_pass=4)[0].cpu().numpy().tobytes() for _ in range(2)]
    assert xs[0] == xs[1]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_with_partial_sums_gives_the_bits_of_the_plain_one(mf, case):
    """The product a solver's cycle launches (partial sums of dotw . y: the volume kernel's, then the face kernel's) writes the y of
    mfem_brick_operator_apply bit for bit, and its sums add up to dotw . y (to the rounding of n terms)."""
    import torch

    S = _built(mf, case)
    x, w = _dev(S.x), _dev(S.y0)
    for alpha, beta in ((1.0, 0.0), (-0.7, 0.3)):
        plain = S.op.mul_(_dev(S.y0) if beta else torch.full_like(x, float("nan")), x, alpha, beta)
        y, partials, n_p = _apply_dot(S.op, x, _dev(S.y0) if beta else torch.full_like(x, float("nan")), w, alpha, beta)
        assert 1 <= n_p <= 4096
        assert y.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
        got, want = float(partials[:n_p].sum()), float((w.cpu().numpy() * y.cpu().numpy()).sum())
        bound = 4 * S.n * np.finfo(float).eps * float((w.abs() * y.abs()).sum())  # (a sum of n terms in any order)
        print(f"{case[0]} itg {case[1]} ({alpha}, {beta}): {n_p} partial sums, |sum - dotw . y| = {abs(got - want):.2e} (bound {bound:.2e})")
        assert abs(got - want) <= bound
        assert float(partials[n_p:].abs().max()) == 0.0 if n_p < 4096 else True  # nothing written behind them


@pytest.mark.parametrize("n,itg,items", [((4, 640, 620), 3, 43 * 42 * 2), ((96, 96, 99), 1, -(-97 * 97 * 100 // 256))],
                         ids=["sweep-4x640x620-itg3", "points-96x96x99-itg1"])
def test_work_items_folded_onto_the_capped_grid(mf, n, itg, items):
    """More work items than the 3584 partial sums of the volume kernel: 5 planes (two 4-plane segments) of 43 x 42 tiles = 3612 items for the sweep,
    97 x 97 x 100 points = 3676 blocks of 256 for the point form.  The folded product stays within 4096 partial sums, gives the same bits twice and
    the bits of the unfolded one; both against the CSR kernel on the assembled K (the oracle does not reach these sizes)."""
    import torch

    assert items > 4096 - 512 and items in (3612, 3676)
    brick = mf.make_Brick((1.0, 1.0, 1.0), n, 1, itg)
    pen = mf.FACE_BITS["x0"]
    A = brick.pattern(3)
    K = brick.assemble_elasticity(A, LAM, MU, TAU_ONE, pen)
    op = brick.elasticity_operator(LAM, MU, TAU_ONE, pen)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(A.n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    w = torch.rand(A.n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    want = mf.mul_(torch.empty_like(x), A, K, x)
    del K, A
    plain = op.mul_(torch.full_like(x, float("nan")), x)
    e = float((plain - want).abs().max()) / float(want.abs().max())
    print(f"{n} itg {itg}: unfolded product vs CSR kernel {e:.2e}")
    assert e <= 1e-12
    y1, p1, n1 = _apply_dot(op, x, torch.full_like(x, float("nan")), w)
    y2, p2, n2 = _apply_dot(op, x, torch.full_like(x, float("nan")), w)
    print(f"{n} itg {itg}: {items} items on {n1} partial sums")
    # two rounds: ceil(items / 2) workgroups of the volume kernel, then the face kernel's min(512, ceil(boundary points / 256))
    m = [ni + 1 for ni in n]
    boundary = m[0] * m[1] * m[2] - (m[0] - 2) * (m[1] - 2) * (m[2] - 2)
    assert n1 == n2 == -(-items // 2) + min(512, -(-boundary // 256)) and n1 <= 4096
    assert torch.equal(y1, y2) and torch.equal(p1, p2)  # the same bits twice
    assert torch.equal(y1, plain)                        # ... and the unfolded product's
    got, ref = float(p1[:n1].sum()), float((w * y1).sum())
    assert abs(got - ref) <= 4 * x.numel() * np.finfo(float).eps * float((w.abs() * y1.abs()).sum())


# ---- 4. every admitted solver ---------------------------------------------------------------------------------------------------------------------
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


_FORMS = {}


def _form(mf, itg=3):
    """(5, 4, 3) on the unit cube, penalty tau = 1000 on x0 (K is symmetric: cg! is admitted); b = K x0"""
    import torch

    if itg in _FORMS:
        return _FORMS[itg]
    S = _Built()
    S.brick = mf.make_Brick((1.0, 1.0, 1.0), (5, 4, 3), 1, itg)
    S.pen = mf.FACE_BITS["x0"]
    S.A = S.brick.pattern(3)
    S.K = S.brick.assemble_elasticity(S.A, LAM, MU, TAU_REF, S.pen)
    S.op = S.brick.elasticity_operator(LAM, MU, TAU_REF, S.pen)
    S.n = S.A.n
    x0 = _dev(np.random.default_rng(4).uniform(-1.0, 1.0, S.n))
    S.b = mf.mul_(torch.empty_like(x0), S.A, S.K, x0)
    # test 1 bounds the product's error by 1e-12 max|K x|; the solve's tolerance stands 1e4 above that: the factor 2 below never decides
    S.tol = 1e-8 * float(S.b.abs().max())
    _FORMS[itg] = S
    return S


@pytest.mark.parametrize("precond", ["Identity", "Pr_Jacobi_"])
@pytest.mark.parametrize("solver", list(SOLVERS))
def test_every_solver_converges_with_the_products_of_its_formula(mf, solver, precond):
    import torch
    from metafem_jl_amd import _lib

    S = _form(mf)
    sv, s = SOLVERS[solver]
    kw = dict(Sv_func=getattr(mf, sv), Pr_func=getattr(mf, precond), s=s, maxiter=MAXITER, max_pass=MAX_PASS)
    m0 = int(_lib.lib.mfem_debug_mesh_operator_count())
    x, st = mf.iterative_Solve(S.op, None, S.b, S.tol, **kw)
    res = float((S.b - mf.mul_(torch.empty_like(x), S.A, S.K, x)).norm()) / np.sqrt(S.n)  # the CSR kernel on the assembled K
    print(f"{solver} + {precond}: {st.iterations} iterations, {st.passes} passes, {st.spmv_count} products, residual {res:.2e} (tol {S.tol:.2e})")
    assert st.converged == 1
    assert res <= 2 * S.tol
    assert st.spmv_count == _expected_products(solver, st)
    assert int(_lib.lib.mfem_debug_mesh_operator_count()) == m0  # no other operator served a product


def test_cg_fixed_iterations_launch_the_brick_operator(mf):
    """cg! at 37 fixed iterations without cycle graphs: 38 products (the 37 A p and the true residual after the pass), each one launch of the
    brick operator's."""
    from metafem_jl_amd import _lib

    S = _form(mf)
    try:
        _lib.check(_lib.lib.mfem_debug_set_graphs(0, 0))
        c0 = int(_lib.lib.mfem_debug_brick_operator_count())
        _, st = mf.iterative_Solve(S.op, None, S.b, 1e-30, Sv_func=mf.cg_, maxiter=37, max_pass=1, fixed_iterations=True)
        assert st.iterations == 37 and st.passes == 1 and st.spmv_count == 37 + 1
        assert int(_lib.lib.mfem_debug_brick_operator_count()) - c0 == st.spmv_count
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)


def test_cached_cycle_replays_with_its_own_gauss_rule(mf):
    """Two identical Identity solves on an itg 5 operator (the point form and the face kernel read the reference tables), cycle graphs on: the second
    replays the first one's cached cycles.  In between, operators with other rules (itg 3, 7, 1) serve products and diagonals.  One fixed pass, so
    that nothing after the pass repairs it: the same bits both times, and the assembled residual says the answer is right."""
    import torch

    S = _form(mf, itg=5)
    kw = dict(Sv_func=mf.idrs_, Pr_func=mf.Identity, s=8, maxiter=60, max_pass=1, fixed_iterations=True)
    first, st1 = mf.iterative_Solve(S.op, None, S.b, 1e-300, **kw)
    for itg in (3, 7, 1):
        other = mf.make_Brick(X, (3, 2, 4), 1, itg).elasticity_operator(LAM, MU, TAU_REF, mf.FACE_BITS["x0"] | mf.FACE_BITS["z1"])
        v = torch.ones(other.n, dtype=torch.float64, device="cuda")
        other.mul_(torch.empty_like(v), v)
        other.diagonal()
    second, st2 = mf.iterative_Solve(S.op, None, S.b, 1e-300, **kw)
    assert st1.spmv_count == st2.spmv_count
    assert second.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()
    res = float((S.b - mf.mul_(torch.empty_like(second), S.A, S.K, second)).norm()) / np.sqrt(S.n)
    assert abs(res - st2.final_res) <= 1e-6 * float(S.b.abs().max()), (res, st2.final_res)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mf):
    import torch
    from metafem_jl_amd import _lib

    INVALID, UNSUPPORTED = -1, -3
    S = _form(mf)
    ctx = S.brick.ctx
    p = _lib.ElasticityParams(LAM, MU, TAU_REF, S.pen, 0, (C.c_double * 6)(*([0.0] * 6)))
    h = C.c_uint64(1)
    # a hex-27 brick, a slab: the thermal operator's messages
    b27 = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 2, 5)
    assert _lib.lib.mfem_brick_operator_create_elasticity(ctx._h, b27._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"an order-2 (hex-27) brick: the matrix-free brick operator covers hex-8 bricks" in _lib.lib.mfem_last_error()
    with pytest.raises(mf.BrickOperatorRefused):
        b27.elasticity_operator(LAM, MU)
    slab = mf.make_Brick((1.0, 1.0, 1.0), (6, 2, 2), 1, 3)
    slab.set_slab(2, 5)
    assert _lib.lib.mfem_brick_operator_create_elasticity(ctx._h, slab._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank" in _lib.lib.mfem_last_error()
    for refused, word in ((b27, "hex-27"), (slab, "slab")):  # the domain is built as the default one and says why
        dom = mf.ElasticityDomain(refused, LAM, MU, TAU_REF, S.pen, matrix_free=True)
        assert dom.matrix_free is False and word in dom.matrix_free_reason
        assert isinstance(dom.A, mf.FEM_SpMat_CSR) and dom.K_linear is not None and dom.K_total is dom.K_linear
    assert _lib.lib.mfem_brick_operator_create_elasticity(ctx._h, None, C.byref(p), C.byref(h)) == INVALID
    assert _lib.lib.mfem_brick_operator_create_elasticity(ctx._h, S.brick._h, None, C.byref(h)) == INVALID
    # a slab set after the operator was created
    late = mf.make_Brick((1.0, 1.0, 1.0), (6, 2, 2), 1, 3)
    late_op = late.elasticity_operator(LAM, MU, TAU_REF, S.pen)
    late.set_slab(2, 5)
    v = torch.full((late_op.n,), 2.5, dtype=torch.float64, device="cuda")
    assert _lib.lib.mfem_brick_operator_apply(ctx._h, late_op._h, v.data_ptr(), v.data_ptr(), 1.0, 0.0) == UNSUPPORTED
    assert b"slab" in _lib.lib.mfem_last_error()
    assert _lib.lib.mfem_brick_operator_diagonal(ctx._h, late_op._h, v.data_ptr()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((v == 2.5).all())

    # the other physics' set-params: MFEM_ERR_INVALID, nothing changed
    x = _dev(np.random.default_rng(5).uniform(-1.0, 1.0, S.n))
    before = S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    pt = _lib.ThermalParams(0.6, 25.0, 293.15, 0x3F, 0, 0.0, 0.0)
    assert _lib.lib.mfem_brick_operator_set_params(S.op._h, C.byref(pt)) == INVALID
    thermal = S.brick.thermal_operator(0.6, 25.0, 293.15, 0x3F)
    xt = x[: thermal.n].clone()
    t_before = thermal.mul_(torch.empty_like(xt), xt).cpu().numpy().tobytes()
    assert _lib.lib.mfem_brick_operator_set_elasticity_params(thermal._h, C.byref(p)) == INVALID
    assert _lib.lib.mfem_brick_operator_set_elasticity_params(S.op._h, None) == INVALID
    assert S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == before
    assert thermal.mul_(torch.empty_like(xt), xt).cpu().numpy().tobytes() == t_before

    b = S.b
    sentinel = 123.25
    xs = torch.full_like(b, sentinel)
    st = _lib.SolveStats()
    n0 = int(_lib.lib.mfem_debug_brick_operator_count())

    def solve(c=ctx, handle=S.op._h, **kw):
        opt = dict(method=mf.idrs_, precond=1, l_or_s=8, maxiter=2000, max_pass=4, check_every=32, converge_tol=S.tol, seed=1)
        opt.update(kw)
        o = _lib.SolveOptions(**opt)
        return _lib.lib.mfem_solve_operator(c._h, handle, b.data_ptr(), xs.data_ptr(), C.byref(o), C.byref(st))

    assert solve(method=mf.lsqr_) == UNSUPPORTED
    assert solve(precond=mf.Pr_Jacobi_colnorm_) == UNSUPPORTED
    assert solve(left_precond=mf.Pl_Jacobi_) == UNSUPPORTED
    assert solve(scale_in_place=1) == INVALID
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
    torch.cuda.synchronize()
    assert int(_lib.lib.mfem_debug_brick_operator_count()) == n0  # nothing launched
    assert bool((xs == sentinel).all())                           # nothing written
    # ... and the handle is still usable
    assert solve() == 0 and st.converged == 1 and not bool((xs == sentinel).any())
    res = float((b - mf.mul_(torch.empty_like(xs), S.A, S.K, xs)).norm()) / np.sqrt(S.n)
    assert res <= 2 * S.tol


def test_set_params_changes_the_product_and_coordinates_are_read_live(mf):
    import torch

    brick = mf.make_Brick(X, (4, 3, 5), 1, 3)
    A = brick.pattern(3)
    op = brick.elasticity_operator(LAM, MU, TAU_ONE, mf.FACE_BITS["x0"])
    x = _dev(np.random.default_rng(2).uniform(-1.0, 1.0, A.n))
    first = op.mul_(torch.empty_like(x), x).clone()
    cur = np.stack([brick.coords_view(d).cpu().numpy() for d in range(3)], axis=1)
    moved = _distort(cur, X)  # move the coordinates under the operator
    for d in range(3):
        brick.coords_view(d).copy_(torch.tensor(np.ascontiguousarray(moved[:, d]), device="cuda"))
    pen2 = mf.FACE_BITS["x0"] | mf.FACE_BITS["y1"]
    op.set_params(2.0 * LAM, 0.5 * MU, 3.0, pen2)
    K = brick.assemble_elasticity(A, 2.0 * LAM, 0.5 * MU, 3.0, pen2)
    want = mf.mul_(torch.empty_like(x), A, K, x)
    got = op.mul_(torch.empty_like(x), x)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((got - first).abs().max()) > 1e-3 * float(want.abs().max())  # (it did change)


# ---- 6. ElasticityDomain(matrix_free=True) -----------------------------------------------------------------------------------------------------------
def test_matrix_free_domain_reproduces_the_default_domain(mf):
    """A cantilever-like brick: the unit cube of 8 x 6 x 5 elements held by the penalty on x0, sigma_11 = 0.01 pulled on x1.  Both domains solve with
    cg! + Pr_Jacobi! to a normalized residual of 1e-12.  An x with K x = b + r differs from the exact one by at most |K^-1| |r|: the smallest
    eigenvalue of K on a unit cube with E = 1 clamped on a face is that of the continuum (order 1) times the nodal volume h^3 >= 1/512, so
    |K^-1| <= ~500, |r|_2 = sqrt(n) 1e-12 ~ 4e-11: 2e-8 absolute per solve, against displacements of order sigma / E = 1e-2.  The bound below, 1e-5
    relative, stands a further factor 5 above the two solves' sum."""
    x, n = (1.0, 1.0, 1.0), (8, 6, 5)
    pen, tra = mf.FACE_BITS["x0"], mf.FACE_BITS["x1"]
    sig = (0.01, 0.0, 0.0, 0.0, 0.0, 0.0)
    out = {}
    for matrix_free in (False, True):
        brick = mf.make_Brick(x, n)
        if matrix_free:
            brick.pattern = None  # never called
        dom = mf.ElasticityDomain(brick, LAM, MU, TAU_REF, pen, tra, sig, matrix_free=matrix_free)
        assert dom.matrix_free is matrix_free and dom.matrix_free_reason is None
        if matrix_free:
            assert isinstance(dom.A, mf.BrickOperator) and dom.A.n == 3 * brick.ncp and dom.K_linear is None and dom.K_total is None
            assert dom.A.nnz == 0 and not hasattr(dom.A, "rowptr")
        dom.converge_tol = 1e-10
        stats = []

        def solver(gf):
            dx, st = mf.iterative_Solve(gf.A, gf.K_total, gf.residue, 1e-12, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=4000, max_pass=3)
            stats.append(st)
            return dx

        dom.linear_solver = solver
        hist = dom.update_OneStep()
        print(f"matrix_free {matrix_free}: history {hist}, {stats[0].iterations} iterations")
        assert len(hist) == 2 and hist[1] < 1e-10 and stats[0].converged == 1
        out[matrix_free] = dom.x.cpu().numpy()
    scale = np.abs(out[False]).max()
    err = np.abs(out[True] - out[False]).max() / scale
    print(f"|x_matrix_free - x_default| / |x| = {err:.2e} (max|x| = {scale:.3e})")
    assert scale > 1e-3
    assert err <= 1e-5
