"""GPU: the matrix-free hex-27 brick operator (mfem_brick_operator_create_hex27, csrc/brick_operator_hex27.hip) against the assembled K of
mfem_brick_assemble_thermal on the CSR kernel and against the oracle's K -- product, diagonal, column scaling, reproducibility, the fold, rules and
cycle graphs, every admitted solver through mfem_solve_operator, the refusals, set_params and live coordinates, and
ThermalDomain(matrix_free="any").  Laid out like tests/test_gpu_brick_operator.py, with its bounds; the oracle domain is built as
tests/test_gpu_hex27_edges.py builds it, distorted by that file's smooth map.  No translated bricks: the affine gate's offset sensitivity is pinned
there (part F)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_gpu_thermal import _distort

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
H_PEN, TW = 1000.0, 1173.15
X = (3.0, 1.0, 2.0)
ALL = [0, 1, 2, 3, 4, 5]


def _const(name):
    text = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_hex27_decide.h")).read()
    return int(re.search(r"#define " + name + r"\s+(\d+)", text).group(1))


TE, LMIN = _const("B27_TE"), _const("B27_LMIN")
# one full tile plus one element in each tiled direction; along the sweep two segments plus one plane (a brick this small sweeps B27_LMIN planes a segment)
FAMILY = (2 * LMIN + 1, TE + 1, TE + 1)

# n, itg, distorted, Robin faces, fixed faces
CASES = [
    ((1, 1, 1), 5, False, ALL, []),
    ((2, 1, 3), 1, True, [5], [3]),
    (FAMILY, 5, True, [0, 1, 2, 3, 5], [4]),
    (FAMILY, 3, True, [0, 1, 2, 3, 5], [4]),
    (FAMILY, 7, True, [0, 1, 2, 3, 5], [4]),
    ((3, 4, 2), 5, True, [], ALL),
]
IDS = ["x".join(map(str, c[0])) + f"-itg{c[1]}" for c in CASES]


def _bits(faces):
    return sum(1 << f for f in faces)


def _oracle(x, n, itg, distorted, robin, fixed):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 2, 1, itg)
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


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")


def _move(brick, coords):
    import torch

    for d in range(3):
        brick.coords_view(d).copy_(torch.tensor(np.ascontiguousarray(coords[:, d]), device="cuda"))


def _built(mf, case):
    """brick, operator, assembled (A, K) and the oracle's K of a case: computed once, shared, never changed"""
    import scipy.sparse as sp

    key = (case[0], case[1])
    if key in _CACHE:
        return _CACHE[key]
    n, itg, distorted, robin, fixed = case
    od = _oracle(X, n, itg, distorted, robin, fixed)
    od.update_time()
    od.K_linear_func()
    S = _Built()
    S.Ko = sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)
    S.brick = mf.make_Brick(X, n, 2, itg)
    if distorted:
        _move(S.brick, od.mesh.coords)
    S.kw = dict(fixed_faces=_bits(fixed), h_penalty=H_PEN, Tw=TW)
    S.A = S.brick.pattern(1)
    S.K = S.brick.assemble_thermal(S.A, K_COND, H, TENV, _bits(robin), **S.kw)
    S.op = S.brick.thermal_operator_hex27(K_COND, H, TENV, _bits(robin), **S.kw)
    S.n = S.A.n
    rng = np.random.default_rng(11)
    S.x = rng.uniform(-1.0, 1.0, S.n)
    S.y0 = rng.uniform(-1.0, 1.0, S.n)
    _CACHE[key] = S
    return S


# ---- 1. product ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_equals_csr_kernel_and_oracle(mf, case):
    import torch

    S = _built(mf, case)
    assert isinstance(S.op, mf.Hex27BrickOperator) and isinstance(S.op, mf.BrickOperator) and S.op.n == S.n == S.brick.ncp
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


def test_affine_shortcut_and_general_branch_agree_on_an_affine_brick(mf):
    """The undistorted family brick takes the constant-Jacobian shortcut in every element: against the CSR kernel on the assembled K."""
    import torch

    brick = mf.make_Brick(X, FAMILY, 2, 5)
    A = brick.pattern(1)
    K = brick.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    op = brick.thermal_operator_hex27(K_COND, H, TENV, 0x3F)
    x = _dev(np.random.default_rng(3).uniform(-1.0, 1.0, A.n))
    want = mf.mul_(torch.empty_like(x), A, K, x)
    got = op.mul_(torch.full_like(x, float("nan")), x)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"affine {FAMILY}: vs CSR kernel {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_product_with_a_column_scaling(mf, case):
    """The solvers on A D^-1 hand d = |diag K| to the product, which reads x_j / d_j: idrs!(8) with Pr_Jacobi! on b = K x0, the residual of its x
    recomputed with the CSR kernel on the assembled K."""
    S = _built(mf, case)
    x0 = _dev(S.x)
    b = mf.mul_(_dev(S.y0), S.A, S.K, x0)
    tol = 1e-8 * float(b.abs().max())
    sol, st = mf.iterative_Solve(S.op, None, b, tol, Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, s=8, maxiter=2000, max_pass=4)
    res = float((b - mf.mul_(_dev(S.y0), S.A, S.K, sol)).norm()) / np.sqrt(S.n)
    print(f"{case[0]} itg {case[1]}: idrs!(8) + Pr_Jacobi!: {st.iterations} iterations, residual {res:.2e} (tol {tol:.2e})")
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


def test_zero_conductivity_without_faces_keeps_the_preset(mf):
    op = mf.make_Brick(X, (3, 2, 4), 2, 5).thermal_operator_hex27(0.0)
    d = op.diagonal(preset=7.5).cpu().numpy()
    assert (d == 7.5).all()


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------------------------------
def test_two_applications_and_two_solves_give_the_same_bits(mf):
    import torch

    S = _built(mf, CASES[2])
    x = _dev(S.x)
    a = S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    assert S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == a
    b = mf.mul_(torch.empty_like(x), S.A, S.K, x)
    xs = [mf.iterative_Solve(S.op, None, b, 1e-8 * float(b.abs().max()), Sv_func=mf.idrs_, s=8, seed=0x5EED, maxiter=2000,
                             max_pass=4)[0].cpu().numpy().tobytes() for _ in range(2)]
    assert xs[0] == xs[1]


def _apply_dot(op, x, y, alpha, beta, dotw):
    """mfem_debug_brick_operator_apply_dot: y in place, (partials, n_partials) back"""
    import torch
    from metafem_jl_amd import _lib

    partials = torch.zeros(4096, dtype=torch.float64, device="cuda")
    npart = C.c_int32(-1)
    _lib.check(_lib.lib.mfem_debug_brick_operator_apply_dot(op.ctx._h, op._h, x.data_ptr(), y.data_ptr(), alpha, beta, dotw.data_ptr(), partials.data_ptr(),
                                                          C.byref(npart)))
    return partials.cpu().numpy(), npart.value


@pytest.mark.parametrize("case", [CASES[2], CASES[5]], ids=[IDS[2], IDS[5]])
def test_apply_dot_gives_the_bits_of_apply_and_the_partial_sums_of_the_dot(mf, case):
    S = _built(mf, case)
    x, w = _dev(S.x), _dev(np.random.default_rng(5).uniform(-1.0, 1.0, S.n))
    for alpha, beta in ((1.0, 0.0), (-0.7, 0.3)):
        want = S.op.mul_(_dev(S.y0), x, alpha, beta)
        y = _dev(S.y0)
        partials, npart = _apply_dot(S.op, x, y, alpha, beta, w)
        assert 1 <= npart <= 4096
        assert y.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        dot = float((w * want).sum())
        scale = float((w * want).abs().sum())
        print(f"{case[0]} ({alpha}, {beta}): {npart} partial sums, |sum - dotw . y| / sum|dotw_i y_i| = {abs(partials[:npart].sum() - dot) / scale:.2e}")
        assert abs(partials[:npart].sum() - dot) <= 1e-13 * scale  # (n eps / 2 of the absolute sum, n < 1e4: two summation orders of the same terms)
        assert (partials[npart:] == 0.0).all()


# ---- 4. the fold -------------------------------------------------------------------------------------------------------------------------------------
def test_folded_product_equals_the_unfolded_one_bit_for_bit(mf):
    """A one-element-thick brick of 60 x 60 tiles: 3600 work items, more than the 3584 partial sums of the volume kernel.  With partial sums asked for
    a workgroup sweeps two items (LDS reused, one dot sum across them); without, one workgroup per item.  The same y, bit for bit."""
    import torch

    cap = 4096 - 512
    tiles = 60
    assert tiles * tiles > cap
    n = (1, TE * (tiles - 1) + 1, TE * (tiles - 1) + 1)
    brick = mf.make_Brick((0.1, 4.0, 4.0), n, 2, 5)
    op = brick.thermal_operator_hex27(K_COND, H, TENV, 0x3F)
    rng = np.random.default_rng(8)
    x, w, y0 = (_dev(rng.uniform(-1.0, 1.0, op.n)) for _ in range(3))
    unfolded = op.mul_(y0.clone(), x, -0.7, 0.3)
    y = y0.clone()
    partials, npart = _apply_dot(op, x, y, -0.7, 0.3, w)
    assert npart <= 4096
    assert npart < tiles * tiles  # folded
    assert torch.equal(y, unfolded) and bool(torch.isfinite(y).all())
    dot, scale = float((w * y).sum()), float((w * y).abs().sum())
    assert abs(partials[:npart].sum() - dot) <= 1e-12 * scale


# ---- 5. rules and cycle graphs -------------------------------------------------------------------------------------------------------------------------
def test_cached_cycles_keep_their_own_rule_while_the_assembly_changes_the_mutable_tables(mf):
    """Two operators with different rules (itg 5 and itg 3) are solved alternately, one fixed pass each so that nothing after it repairs a wrong
    product; between two solves a hex-27 assemble_thermal with a third rule (itg 7) re-uploads the assembly's mutable tables.  Each operator's solution
    keeps its bits, with cycle graphs (the second solve replays cached cycles) and without."""
    import torch
    from metafem_jl_amd import _lib

    Sa, Sb = _built(mf, CASES[2]), _built(mf, CASES[3])
    third = mf.make_Brick(X, (2, 2, 2), 2, 7)
    A3 = third.pattern(1)
    kw = dict(Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, s=8, maxiter=40, max_pass=1, fixed_iterations=True)
    try:
        for graphs in (1, 0):
            _lib.check(_lib.lib.mfem_debug_set_graphs(graphs, 0))
            bits = {}
            for rnd in range(3):
                for name, S in (("a", Sa), ("b", Sb)):
                    b = mf.mul_(torch.empty(S.n, dtype=torch.float64, device="cuda"), S.A, S.K, _dev(S.x))
                    sol, st = mf.iterative_Solve(S.op, None, b, 1e-300, **kw)
                    got = sol.cpu().numpy().tobytes()
                    assert bits.setdefault(name, got) == got, (graphs, rnd, name)
                    res = float((b - mf.mul_(torch.empty_like(sol), S.A, S.K, sol)).norm()) / np.sqrt(S.n)
                    assert abs(res - st.final_res) <= 1e-6 * float(b.abs().max()), (res, st.final_res)
                    third.assemble_thermal(A3, K_COND, H, TENV, 0x3F)  # (the mutable tables now hold the 4-point rule)
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)


# ---- 6. every admitted solver ---------------------------------------------------------------------------------------------------------------------
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


CYCLE_PRODUCTS = {"cg": 1, "bicgstabl": 4, "idrs": 9, "cgs2": 2, "gmres": GMRES_S + 1, "cgs": 2, "tfqmr": 3}

_FORMS = {}


def _form(mf, nitsche):
    """(4, 3, 3) elements, itg 5: the Robin form (symmetric) or the Nitsche form (x = 0 fixed, convection elsewhere: nonsymmetric); b = K x0"""
    import torch

    if nitsche in _FORMS:
        return _FORMS[nitsche]
    S = _Built()
    S.brick = mf.make_Brick((1.0, 1.0, 1.0), (4, 3, 3), 2, 5)
    robin, S.kw = (_bits([0, 1, 2, 3, 5]), dict(fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)) if nitsche else (0x3F, {})
    S.A = S.brick.pattern(1)
    S.K = S.brick.assemble_thermal(S.A, K_COND, H, TENV, robin, **S.kw)
    S.op = S.brick.thermal_operator_hex27(K_COND, H, TENV, robin, **S.kw)
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
    # without cycle graphs and with check_every = 1 at most the rest of the cycle that holds the stop is queued behind it (tests/test_gpu_brick_operator.py)
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


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mf):
    import torch
    from metafem_jl_amd import _lib

    INVALID, UNSUPPORTED = -1, -3
    S = _form(mf, nitsche=True)
    ctx = S.brick.ctx
    p = _lib.ThermalParams(K_COND, H, TENV, 0x3F, 0, 0.0, 0.0)
    h = C.c_uint64(1)
    n0 = int(_lib.lib.mfem_debug_brick_operator_count())
    # a hex-8 brick, a slab
    b8 = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 1, 3)
    assert _lib.lib.mfem_brick_operator_create_hex27(ctx._h, b8._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"hex-8" in _lib.lib.mfem_last_error() and b"mfem_brick_operator_create" in _lib.lib.mfem_last_error()
    with pytest.raises(mf.BrickOperatorRefused):
        b8.thermal_operator_hex27(K_COND)
    assert "hex-8" in mf.brick_operator_hex27_refusal(b8)
    slab = mf.make_Brick((1.0, 1.0, 1.0), (3, 2, 2), 2, 5)
    slab.set_slab(2, 4)
    h.value = 1
    assert _lib.lib.mfem_brick_operator_create_hex27(ctx._h, slab._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"slab" in _lib.lib.mfem_last_error()
    assert "slab" in mf.brick_operator_hex27_refusal(slab)
    assert b8.pattern(1).n == 27 and slab.pattern(1).n == 2 * 25  # the bricks stay usable
    # the existing names keep refusing a hex-27 brick
    assert _lib.lib.mfem_brick_operator_create(ctx._h, S.brick._h, C.byref(p), C.byref(h)) == UNSUPPORTED and b"hex-27" in _lib.lib.mfem_last_error()
    dom = mf.ThermalDomain(S.brick, K_COND, H, TENV, matrix_free=True)
    assert dom.matrix_free is False and "hex-27" in dom.matrix_free_reason
    dom = mf.ThermalDomain(slab, K_COND, H, TENV, matrix_free="any")
    assert dom.matrix_free is False and "slab" in dom.matrix_free_reason and isinstance(dom.A, mf.FEM_SpMat_CSR)
    with pytest.raises(ValueError):
        mf.ThermalDomain(S.brick, K_COND, H, TENV, matrix_free="all")
    h.value = 1
    assert _lib.lib.mfem_brick_operator_create_hex27(ctx._h, None, C.byref(p), C.byref(h)) == INVALID and h.value == 0
    assert _lib.lib.mfem_brick_operator_create_hex27(ctx._h, S.brick._h, None, C.byref(h)) == INVALID
    assert _lib.lib.mfem_brick_operator_create_hex27(ctx._h, S.brick._h, C.byref(p), None) == INVALID
    # a slab set after the operator was created: apply, diagonal and the solve answer it
    late_brick = mf.make_Brick((1.0, 1.0, 1.0), (3, 2, 2), 2, 5)
    late = late_brick.thermal_operator_hex27(K_COND, H, TENV, 0x3F)
    late_brick.set_slab(2, 4)
    v = torch.full((late.n,), 123.25, dtype=torch.float64, device="cuda")
    o = _lib.SolveOptions(method=mf.cg_, precond=1, l_or_s=0, maxiter=10, max_pass=1, check_every=1, converge_tol=1e-8, seed=1)
    st = _lib.SolveStats()
    assert _lib.lib.mfem_brick_operator_apply(ctx._h, late._h, v.data_ptr(), v.data_ptr(), 1.0, 0.0) == UNSUPPORTED and b"slab" in _lib.lib.mfem_last_error()
    assert _lib.lib.mfem_brick_operator_diagonal(ctx._h, late._h, v.data_ptr()) == UNSUPPORTED
    assert _lib.lib.mfem_solve_operator(ctx._h, late._h, v.data_ptr(), v.data_ptr(), C.byref(o), C.byref(st)) == UNSUPPORTED
    assert bool((v == 123.25).all())
    # the other physics' set-params
    e = _lib.ElasticityParams(1.0, 1.0, 0.0, 0, 0, (C.c_double * 6)(*([0.0] * 6)))
    assert _lib.lib.mfem_brick_operator_set_elasticity_params(S.op._h, C.byref(e)) == INVALID

    b = S.b
    sentinel = 123.25
    x = torch.full_like(b, sentinel)

    def solve(c=ctx, handle=S.op._h, **kw):
        opt = dict(method=mf.idrs_, precond=1, l_or_s=8, maxiter=2000, max_pass=4, check_every=32, converge_tol=S.tol, seed=1)
        opt.update(kw)
        oo = _lib.SolveOptions(**opt)
        return _lib.lib.mfem_solve_operator(c._h, handle, b.data_ptr(), x.data_ptr(), C.byref(oo), C.byref(st))

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
    other = mf.Context(0)
    try:
        y = torch.full_like(b, sentinel)
        assert solve(c=other) == INVALID  # an operator of another context
        assert b"another context" in _lib.lib.mfem_last_error()
        assert _lib.lib.mfem_brick_operator_apply(other._h, S.op._h, b.data_ptr(), y.data_ptr(), 1.0, 0.0) == INVALID
        assert _lib.lib.mfem_brick_operator_diagonal(other._h, S.op._h, y.data_ptr()) == INVALID
        assert _lib.lib.mfem_brick_operator_create_hex27(other._h, S.brick._h, C.byref(p), C.byref(h)) == INVALID
        torch.cuda.synchronize()
        assert bool((y == sentinel).all())
    finally:
        other.close()
    assert _lib.lib.mfem_brick_operator_apply(ctx._h, S.op._h, None, x.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_brick_operator_diagonal(ctx._h, S.op._h, None) == INVALID
    torch.cuda.synchronize()
    assert int(_lib.lib.mfem_debug_brick_operator_count()) == n0  # nothing launched
    assert bool((x == sentinel).all())                            # nothing written
    # ... and the handle is still usable
    assert solve() == 0 and st.converged == 1 and not bool((x == sentinel).any())
    res = float((b - mf.mul_(torch.empty_like(x), S.A, S.K, x)).norm()) / np.sqrt(S.n)
    assert res <= 2 * S.tol


# ---- 8. set_params and live coordinates --------------------------------------------------------------------------------------------------------------
def test_set_params_changes_the_product_and_coordinates_are_read_live(mf):
    import torch

    brick = mf.make_Brick(X, (3, 2, 4), 2, 5)
    A = brick.pattern(1)
    op = brick.thermal_operator_hex27(K_COND, H, TENV, 0x3F)
    x = _dev(np.random.default_rng(2).uniform(-1.0, 1.0, A.n))
    before = op.mul_(torch.empty_like(x), x)
    moved = _distort(np.stack([brick.coords_view(d).cpu().numpy() for d in range(3)], axis=1))  # move the coordinates under the operator
    _move(brick, moved)
    after_move = op.mul_(torch.empty_like(x), x)
    assert not torch.equal(before, after_move)
    op.set_params(2.0 * K_COND, H, TENV, _bits([0, 1]), fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)
    K = brick.assemble_thermal(A, 2.0 * K_COND, H, TENV, _bits([0, 1]), fixed_faces=_bits([4]), h_penalty=H_PEN, Tw=TW)
    want = mf.mul_(torch.empty_like(x), A, K, x)
    got = op.mul_(torch.empty_like(x), x)
    assert not torch.equal(got, after_move)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- 9. ThermalDomain(matrix_free="any") ---------------------------------------------------------------------------------------------------------------
def test_matrix_free_any_domain_reproduces_the_default_domain_and_holds_no_matrix(mf):
    n, tol = (4, 3, 5), 1e-12

    def run(brick, **kw):
        dom = mf.ThermalDomain(brick, K_COND, H, TENV, **kw)
        dom.s.fill_(SRC)
        dom.converge_tol = 1e-9
        dom.linear_solver = lambda gf: mf.iterative_Solve(gf.A, gf.K_total, gf.residue, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=4000, max_pass=3)[0]
        hist = dom.update_OneStep()
        assert len(hist) == 2 and hist[1] < 1e-9, hist
        return dom

    ref = run(mf.make_Brick(X, n, 2, 5))
    brick = mf.make_Brick(X, n, 2, 5)
    brick.pattern = None  # never called
    dom = run(brick, matrix_free="any")
    assert dom.matrix_free is True and dom.matrix_free_reason is None
    assert isinstance(dom.A, mf.Hex27BrickOperator) and dom.K_linear is None and dom.K_total is None and dom.A.nnz == 0 and not hasattr(dom.A, "rowptr")
    err = float((dom.x - ref.x).abs().max()) / float(ref.x.abs().max())
    # Both Newton updates solve K dx = r(0) (the same residual kernel on the same input) to a normalised residual of tol, one on the operator, one on
    # the assembled K; test 1 bounds the two products' difference by 1e-12 max|K x|.  So K (x_a - x_b), on the assembled K, is within 2 tol plus that.
    import torch

    Kx = mf.mul_(torch.empty_like(ref.x), ref.A, ref.K_linear, ref.x)
    Kd = mf.mul_(torch.empty_like(ref.x), ref.A, ref.K_linear, dom.x - ref.x)
    gap, bound = mf.normalized_norm(Kd), 2 * tol + 2e-12 * float(Kx.abs().max())
    print(f"|x_matrix_free - x_default| / |x| = {err:.2e}; |K (x_a - x_b)| / sqrt(n) = {gap:.2e} (bound {bound:.2e})")
    assert gap <= bound
    assert err <= 1e-9  # (and nothing gross hides in K's near-null space: the Robin faces make K definite)


def test_matrix_free_any_on_a_hex8_brick_is_matrix_free_true(mf):
    import torch

    doms = []
    for word in ("any", True):
        dom = mf.ThermalDomain(mf.make_Brick(X, (5, 4, 3), 1, 3), K_COND, H, TENV, matrix_free=word)
        assert dom.matrix_free is True and type(dom.A) is mf.BrickOperator and dom.K_linear is None
        dom.s.fill_(SRC)
        dom.update_OneStep()
        doms.append(dom)
    assert torch.equal(doms[0].x, doms[1].x)
