"""GPU: the matrix-free hex-27 ELASTICITY brick operator (mfem_brick_operator_create_elasticity_hex27, csrc/brick_operator_elasticity_hex27.hip)
against the oracle's K of the cantilever form on the Lagrange-2 lattice -- product, affine shortcut, column scaling, diagonal, reproducibility, the
fold, every admitted solver through mfem_solve_operator, the residual, the refusals, set_params and live coordinates, and
ElasticityDomain(matrix_free="any").  Laid out like tests/test_gpu_brick_operator_hex27.py, with its bounds (product 1e-11, diagonal 1e-12 of the largest
entry).  No assembled hex-27 elasticity matrix exists on the device: every reference is the oracle's K on the CPU, built once per case and shared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_gpu_thermal import _distort

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_MOD, NU = 1.0, 0.3
LAM, MU = E_MOD * NU / ((1 + NU) * (1 - 2 * NU)), E_MOD / (2 * (1 + NU))
TAU_ONE, TAU_REF = 1.0, 1000.0  # parity cases: tau = 1 (the penalty entries do not hide the elastic ones); the domain: tau = 1000
X = (3.0, 1.0, 2.0)
FACE_NAMES = ["z0", "y0", "x1", "y1", "x0", "z1"]  # oracle face id f == bit f of the operator's mask
ALL = [0, 1, 2, 3, 4, 5]
SIG6 = (0.01, -0.004, 0.006, 0.003, -0.002, 0.005)  # 11, 22, 33, 23, 13, 12


def _const(name):
    text = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_elasticity_hex27_decide.h")).read()
    return int(re.search(r"#define " + name + r"\s+(\d+)", text).group(1))


TE, LMIN = _const("E27_TE"), _const("E27_LMIN")
# one full tile plus one element in each tiled direction; along the sweep two segments plus one plane
FAMILY = (2 * LMIN + 1, TE + 1, TE + 1)

# n, itg, distorted, penalty faces, traction faces
CASES = [
    ((1, 1, 1), 5, False, [4], []),
    ((2, 1, 3), 1, True, [], []),
    (FAMILY, 3, True, [4], [2]),
    (FAMILY, 5, True, [4], [2]),
    (FAMILY, 7, True, [4], [2]),
    ((3, 4, 2), 5, True, ALL, []),
]
IDS = ["x".join(map(str, c[0])) + f"-itg{c[1]}" for c in CASES]


def _bits(faces):
    return sum(1 << f for f in faces)


def _sig33(s):
    return [[s[0], s[5], s[4]], [s[5], s[1], s[3]], [s[4], s[3], s[2]]]


def _oracle(x, n, itg, distorted, pen, tra, tau=TAU_ONE, lam=LAM, mu=MU, sig=SIG6, coords=None):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 2, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    if coords is not None:
        msh.coords[:] = coords
    elif distorted:
        msh.coords[:] = _distort(msh.coords)
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = []
    if pen:
        bnd.append((fac.select(np.isin(fac.element_eindex, pen)), problems.elasticity_penalty(3, tau)))
    if tra:
        bnd.append((fac.select(np.isin(fac.element_eindex, tra)), problems.elasticity_traction(3, _sig33(sig))))
    od = fem.FEMDomain(msh, disc, 3, problems.elasticity_domain(3, lam, mu), bnd)
    od.update_time()
    od.K_linear_func()
    return od


def _Ko(od):
    import scipy.sparse as sp

    return sp.csr_matrix((od.K_linear, od.pattern.colidx, od.pattern.rowptr), shape=(od.pattern.n,) * 2)


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


def _served(mf, itg):
    """the rule predicate of the decide header, through its Python restatement (test 8 holds the two together)"""
    return mf.brick_operator_elasticity_hex27_waves(itg // 2 + 1) > 0


def _built(mf, case):
    """brick, operator and the oracle's K of a case: computed once, shared, never changed"""
    key = (case[0], case[1])
    if key in _CACHE:
        return _CACHE[key]
    n, itg, distorted, pen, tra = case
    od = _oracle(X, n, itg, distorted, pen, tra)
    S = _Built()
    S.od, S.Ko = od, _Ko(od)
    S.brick = mf.make_Brick(X, n, 2, itg)
    if distorted:
        _move(S.brick, od.mesh.coords)
    S.op = S.brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, _bits(pen), _bits(tra), SIG6)
    S.n = S.Ko.shape[0]
    rng = np.random.default_rng(11)
    S.x = rng.uniform(-1.0, 1.0, S.n)
    S.y0 = rng.uniform(-1.0, 1.0, S.n)
    _CACHE[key] = S
    return S


def _case(mf, case):
    """the built case, or -- for a rule the predicate refuses -- the assertion of that refusal in its place (returns None)"""
    if _served(mf, case[1]):
        return _built(mf, case)
    brick = mf.make_Brick(X, case[0], 2, case[1])
    with pytest.raises(mf.BrickOperatorRefused, match="4-point Gauss rule"):
        brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, _bits(case[3]))
    assert "4-point Gauss rule" in mf.brick_operator_elasticity_hex27_refusal(brick)
    return None


# ---- 1. product ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_equals_the_oracle(mf, case):
    import torch

    S = _case(mf, case)
    if S is None:
        return
    assert isinstance(S.op, mf.Hex27ElasticityBrickOperator) and isinstance(S.op, mf.BrickOperator) and S.op.n == S.n == 3 * S.brick.ncp
    x = _dev(S.x)
    for alpha, beta in ((1.0, 0.0), (-0.7, 0.3)):
        y_in = torch.full_like(x, float("nan")) if beta == 0.0 else _dev(S.y0)  # beta == 0: y must not be read
        got = mf.mul_(y_in, S.op, None, x, alpha, beta).cpu().numpy()
        want = alpha * (S.Ko @ S.x) + beta * S.y0
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{case[0]} itg {case[1]} ({alpha}, {beta}): vs oracle {err:.2e} (widest row {np.diff(S.Ko.indptr).max()})")
        assert np.isfinite(got).all()
        assert err <= 1e-11, (alpha, beta)


# ---- 2. the affine shortcut -----------------------------------------------------------------------------------------------------------------------
def test_affine_shortcut_and_general_branch_agree_on_an_affine_brick(mf):
    """The undistorted family brick takes the constant-Jacobian shortcut in every element; mfem_debug_set("elasticity_hex27", 1) sends every
    element through the general branch.  The two agree to the sibling test's 1e-12, and the shortcut agrees with the oracle."""
    import torch
    from metafem_jl_amd import _lib

    pen = [4]
    od = _oracle(X, FAMILY, 5, False, pen, [])
    brick = mf.make_Brick(X, FAMILY, 2, 5)
    op = brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, _bits(pen))
    xh = np.random.default_rng(3).uniform(-1.0, 1.0, op.n)
    x = _dev(xh)
    fast = op.mul_(torch.full_like(x, float("nan")), x)
    try:
        _lib.check(_lib.lib.mfem_debug_set(b"elasticity_hex27", 1, 0))
        general = op.mul_(torch.full_like(x, float("nan")), x)
    finally:
        _lib.lib.mfem_debug_set(b"elasticity_hex27", 0, 0)
    want = _Ko(od) @ xh
    e_gen = float((fast - general).abs().max()) / float(general.abs().max())
    e_or = np.abs(fast.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"affine {FAMILY}: shortcut vs general branch {e_gen:.2e}, shortcut vs oracle {e_or:.2e}")
    assert e_gen <= 1e-12
    assert e_or <= 1e-11


# ---- 3. column scaling ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[3], CASES[4]], ids=[IDS[3], IDS[4]])
def test_product_with_a_column_scaling(mf, case):
    """The solvers on A D^-1 hand d = |diag K| to the product, which reads x_j / d_j: idrs!(8) with Pr_Jacobi! on b = K x0, the residual of its x
    recomputed on the CPU with the oracle's K."""
    S = _case(mf, case)
    if S is None:
        return
    bh = S.Ko @ S.x
    tol = 1e-8 * np.abs(bh).max()
    sol, st = mf.iterative_Solve(S.op, None, _dev(bh), tol, Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, s=8, maxiter=4000, max_pass=4)
    res = np.linalg.norm(bh - S.Ko @ sol.cpu().numpy()) / np.sqrt(S.n)
    print(f"{case[0]} itg {case[1]}: idrs!(8) + Pr_Jacobi!: {st.iterations} iterations, residual {res:.2e} (tol {tol:.2e})")
    assert st.converged == 1 and res <= 2 * tol


# ---- 4. diagonal --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_diagonal_equals_the_oracles(mf, case):
    """|diag K| against |diag Ko| under the guarded rule (an exactly zero K_ii keeps the preset 1: on the 1-point rule every node but the face
    centres has a zero gradient at the one Gauss point).  The shipped diagonal is the per-control-point form (not the signed sweep): only the
    absolute value exists."""
    S = _case(mf, case)
    if S is None:
        return
    d = S.op.diagonal().cpu().numpy()
    dk = S.Ko.diagonal()
    want = np.where(dk == 0.0, 1.0, np.abs(dk))
    assert case[1] == 1 or (dk != 0.0).all()
    err = np.abs(d - want).max() / np.abs(want).max()
    print(f"{case[0]} itg {case[1]}: |d - |diag Ko|| / max|d| = {err:.2e}")
    assert d.shape == (S.n,)
    assert err <= 1e-12


def test_zero_parameters_keep_the_preset(mf):
    op = mf.make_Brick(X, (3, 2, 4), 2, 5).elasticity_operator_hex27(0.0, 0.0, 0.0, 0x3F)
    d = op.diagonal(preset=7.5).cpu().numpy()
    assert d.shape == (3 * 7 * 5 * 9,) and (d == 7.5).all()


# ---- 5. reproducibility -----------------------------------------------------------------------------------------------------------------------------
def test_two_applications_and_two_solves_give_the_same_bits(mf):
    import torch

    S = _built(mf, CASES[3])
    x = _dev(S.x)
    a = S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    assert S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == a
    b = _dev(S.Ko @ S.x)
    xs = [mf.iterative_Solve(S.op, None, b, 1e-8 * float(b.abs().max()), Sv_func=mf.idrs_, s=8, seed=0x5EED, maxiter=2000,
                             max_pass=2)[0].cpu().numpy().tobytes() for _ in range(2)]
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


@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
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
        assert abs(partials[:npart].sum() - dot) <= 1e-13 * scale
        assert (partials[npart:] == 0.0).all()


def test_folded_product_equals_the_unfolded_one_bit_for_bit(mf):
    """A one-element-thick brick of 60 x 60 tiles: 3600 work items, more than the 3584 partial sums of the volume kernel.  With partial sums asked for
    a workgroup sweeps two items (LDS reused, one dot sum across them); without, one workgroup per item.  The same y, bit for bit."""
    import torch

    cap = 4096 - 512
    tiles = 60
    assert tiles * tiles > cap
    n = (1, TE * (tiles - 1) + 1, TE * (tiles - 1) + 1)
    brick = mf.make_Brick((0.1, 4.0, 4.0), n, 2, 5)
    op = brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, 0x3F)
    g = torch.Generator(device="cuda").manual_seed(8)
    x, w, y0 = (torch.rand(op.n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1 for _ in range(3))
    unfolded = op.mul_(y0.clone(), x, -0.7, 0.3)
    y = y0.clone()
    partials, npart = _apply_dot(op, x, y, -0.7, 0.3, w)
    assert npart <= 4096
    assert npart < tiles * tiles  # folded
    assert torch.equal(y, unfolded) and bool(torch.isfinite(y).all())
    dot, scale = float((w * y).sum()), float((w * y).abs().sum())
    assert abs(partials[:npart].sum() - dot) <= 1e-12 * scale


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


def _form(mf):
    """the (3, 4, 2) case (itg 5, distorted, penalty on all six faces: K is symmetric and definite): b = Ko x0"""
    S = _built(mf, CASES[5])
    if not hasattr(S, "b"):
        S.bh = S.Ko @ np.random.default_rng(4).uniform(-1.0, 1.0, S.n)
        S.b = _dev(S.bh)
        # test 1 bounds the product's error by 1e-11 max|K x|; the solve's tolerance stands 1e3 above that: the factor 2 below never decides
        S.tol = 1e-8 * np.abs(S.bh).max()
    return S


@pytest.mark.parametrize("precond", ["Identity", "Pr_Jacobi_"])
@pytest.mark.parametrize("solver", list(SOLVERS))
def test_every_solver_converges_with_the_products_of_its_formula(mf, solver, precond):
    from metafem_jl_amd import _lib

    S = _form(mf)
    sv, s = SOLVERS[solver]
    kw = dict(Sv_func=getattr(mf, sv), Pr_func=getattr(mf, precond), s=s, maxiter=MAXITER, max_pass=MAX_PASS)
    m0 = int(_lib.lib.mfem_debug_mesh_operator_count())
    x, st = mf.iterative_Solve(S.op, None, S.b, S.tol, **kw)
    res = np.linalg.norm(S.bh - S.Ko @ x.cpu().numpy()) / np.sqrt(S.n)  # the true residual, on the CPU with the oracle's K
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


def test_cached_cycle_replays_with_its_own_rule_while_an_assembly_changes_the_mutable_tables(mf):
    """Two identical fixed passes on the itg 5 operator, cycle graphs on: the second replays the first one's cached cycles.  In between an operator with
    the 2-point rule serves a product and a diagonal, and a hex-27 thermal assembly with a third rule re-uploads the assembly's mutable tables.  The
    same bits both times, and the CPU residual says the answer is right."""
    import torch

    S = _form(mf)
    kw = dict(Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, s=8, maxiter=40, max_pass=1, fixed_iterations=True)
    first, st1 = mf.iterative_Solve(S.op, None, S.b, 1e-300, **kw)
    other = mf.make_Brick(X, (2, 2, 2), 2, 3).elasticity_operator_hex27(LAM, MU, TAU_REF, 0x3F)
    v = torch.ones(other.n, dtype=torch.float64, device="cuda")
    other.mul_(torch.empty_like(v), v)
    other.diagonal()
    third = mf.make_Brick(X, (2, 2, 2), 2, 7)
    third.assemble_thermal(third.pattern(1), 0.6, 25.0, 293.15, 0x3F)  # (the mutable tables now hold the 4-point rule)
    second, st2 = mf.iterative_Solve(S.op, None, S.b, 1e-300, **kw)
    assert st1.spmv_count == st2.spmv_count
    assert second.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()
    res = np.linalg.norm(S.bh - S.Ko @ second.cpu().numpy()) / np.sqrt(S.n)
    assert abs(res - st2.final_res) <= 1e-6 * np.abs(S.bh).max(), (res, st2.final_res)


# ---- 7. residual ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tra", [[2], [2, 5]], ids=["traction-x1", "traction-x1-z1"])
def test_residual_equals_the_oracles(mf, tra):
    """op.residual(x*) = K x* + f against the oracle's K_nonlinear_func at a random x*, on the distorted (3, 4, 2) brick, penalty on x0"""
    n, itg, pen = (3, 4, 2), 5, [4]
    od = _oracle(X, n, itg, True, pen, tra)
    od.x_star[:] = 0.01 * np.random.default_rng(2).standard_normal(od.basicfield_size)
    od.K_nonlinear_func()
    brick = mf.make_Brick(X, n, 2, itg)
    _move(brick, od.mesh.coords)
    op = brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, _bits(pen), _bits(tra), SIG6)
    got = op.residual(_dev(od.x_star)).cpu().numpy()
    f = od.residue - _Ko(od) @ od.x_star
    err = np.abs(got - od.residue).max() / np.abs(od.residue).max()
    print(f"traction {tra}: |r - r_oracle| / max|r| = {err:.2e} (max|f| / max|r| = {np.abs(f).max() / np.abs(od.residue).max():.2e})")
    assert np.abs(f).max() > 1e-3 * np.abs(od.residue).max()  # (the load is seen)
    assert err <= 1e-11
    # without traction faces the residual is the product
    op.set_params(LAM, MU, TAU_ONE, _bits(pen))
    import torch

    assert torch.equal(op.residual(_dev(od.x_star)), op.mul_(torch.empty(op.n, dtype=torch.float64, device="cuda"), _dev(od.x_star)))


# ---- 8. refusals and kinds --------------------------------------------------------------------------------------------------------------------------
def test_refusals(mf):
    import torch
    from metafem_jl_amd import _lib

    INVALID, UNSUPPORTED = -1, -3
    S = _form(mf)
    ctx = S.brick.ctx
    p = _lib.ElasticityParams(LAM, MU, TAU_ONE, 0x3F, 0, (C.c_double * 6)(*([0.0] * 6)))
    h = C.c_uint64(1)
    n0 = int(_lib.lib.mfem_debug_brick_operator_count())
    # an order-1 brick, a slab
    b8 = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 1, 3)
    assert _lib.lib.mfem_brick_operator_create_elasticity_hex27(ctx._h, b8._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"mfem_brick_operator_create_elasticity" in _lib.lib.mfem_last_error() and b"hex-8" in _lib.lib.mfem_last_error()
    assert mf.brick_operator_elasticity_hex27_refusal(b8).encode() in _lib.lib.mfem_last_error()
    with pytest.raises(mf.BrickOperatorRefused):
        b8.elasticity_operator_hex27(LAM, MU)
    slab = mf.make_Brick((1.0, 1.0, 1.0), (3, 2, 2), 2, 5)
    slab.set_slab(2, 4)
    h.value = 1
    assert _lib.lib.mfem_brick_operator_create_elasticity_hex27(ctx._h, slab._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"slab" in _lib.lib.mfem_last_error() and mf.brick_operator_elasticity_hex27_refusal(slab).encode() in _lib.lib.mfem_last_error()
    # every rule: the forecast and the library agree
    for itg in range(1, 8):
        rb = mf.make_Brick((1.0, 1.0, 1.0), (1, 1, 1), 2, itg)
        h.value = 1
        rc = _lib.lib.mfem_brick_operator_create_elasticity_hex27(ctx._h, rb._h, C.byref(p), C.byref(h))
        why = mf.brick_operator_elasticity_hex27_refusal(rb)
        if why is None:
            assert rc == 0 and h.value != 0
            _lib.check(_lib.lib.mfem_brick_operator_destroy(h))
        else:
            assert rc == UNSUPPORTED and h.value == 0 and why.encode() in _lib.lib.mfem_last_error() and itg >= 6
        assert itg >= 6 or why is None  # the rules with 1 to 3 points are served
    h.value = 1
    assert _lib.lib.mfem_brick_operator_create_elasticity_hex27(ctx._h, None, C.byref(p), C.byref(h)) == INVALID and h.value == 0
    assert _lib.lib.mfem_brick_operator_create_elasticity_hex27(ctx._h, S.brick._h, None, C.byref(h)) == INVALID
    assert _lib.lib.mfem_brick_operator_create_elasticity_hex27(ctx._h, S.brick._h, C.byref(p), None) == INVALID
    # the existing name keeps refusing a hex-27 brick, with its present text
    assert _lib.lib.mfem_brick_operator_create_elasticity(ctx._h, S.brick._h, C.byref(p), C.byref(h)) == UNSUPPORTED and h.value == 0
    assert b"an order-2 (hex-27) brick: the matrix-free brick operator covers hex-8 bricks" in _lib.lib.mfem_last_error()
    with pytest.raises(mf.BrickOperatorRefused, match="hex-27"):
        S.brick.elasticity_operator(LAM, MU)
    # a slab set after the operator was created: apply, diagonal, the residual and the solve answer it
    late_brick = mf.make_Brick((1.0, 1.0, 1.0), (3, 2, 2), 2, 5)
    late = late_brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, 0x3F)
    late_brick.set_slab(2, 4)
    v = torch.full((late.n,), 123.25, dtype=torch.float64, device="cuda")
    o = _lib.SolveOptions(method=mf.cg_, precond=1, l_or_s=0, maxiter=10, max_pass=1, check_every=1, converge_tol=1e-8, seed=1)
    st = _lib.SolveStats()
    assert _lib.lib.mfem_brick_operator_apply(ctx._h, late._h, v.data_ptr(), v.data_ptr(), 1.0, 0.0) == UNSUPPORTED and b"slab" in _lib.lib.mfem_last_error()
    assert _lib.lib.mfem_brick_operator_diagonal(ctx._h, late._h, v.data_ptr()) == UNSUPPORTED
    assert _lib.lib.mfem_brick_operator_residual_elasticity(ctx._h, late._h, v.data_ptr(), v.data_ptr()) == UNSUPPORTED and b"slab" in _lib.lib.mfem_last_error()
    assert _lib.lib.mfem_solve_operator(ctx._h, late._h, v.data_ptr(), v.data_ptr(), C.byref(o), C.byref(st)) == UNSUPPORTED
    assert bool((v == 123.25).all())
    # the thermal set-params
    pt = _lib.ThermalParams(0.6, 25.0, 293.15, 0x3F, 0, 0.0, 0.0)
    x = _dev(S.x)
    before = S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    c1 = int(_lib.lib.mfem_debug_brick_operator_count())
    assert c1 == n0 + 1
    assert _lib.lib.mfem_brick_operator_set_params(S.op._h, C.byref(pt)) == INVALID
    assert S.op.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == before
    n0 += 2
    # the residual on the other three kinds
    sentinel = 123.25
    b8x = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 1, 3)
    b27 = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 2, 5)
    for other in (b8x.thermal_operator(0.6), b8x.elasticity_operator(LAM, MU, TAU_ONE, 0x3F), b27.thermal_operator_hex27(0.6)):
        r = torch.full((3 * 125,), sentinel, dtype=torch.float64, device="cuda")
        assert _lib.lib.mfem_brick_operator_residual_elasticity(ctx._h, other._h, r.data_ptr(), r.data_ptr()) == UNSUPPORTED
        assert b"hex-27 elasticity operator" in _lib.lib.mfem_last_error()
        torch.cuda.synchronize()
        assert bool((r == sentinel).all())
    # ... and on a mesh operator's handle
    from metafem_jl_amd import element, generic as G, mesh as pm, physics as P

    space = element.classical_space(3, "Lagrange", 1, 3, shape="CUBE")
    vert, conn = pm.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), "CUBE")
    msh = pm.mesh_Classical(vert, conn, space)
    md = G.GenericDomain(ctx, space, msh.coords, msh.cp_ids, 1, P.thermal_domain(3, 0.6), [], matrix_free=True)
    md.update_Time()
    md.K_linear_func()
    assert md.matrix_free and isinstance(md.A, mf.MeshOperator)
    r = torch.full((3 * 125,), sentinel, dtype=torch.float64, device="cuda")
    assert _lib.lib.mfem_brick_operator_residual_elasticity(ctx._h, md.A._h, r.data_ptr(), r.data_ptr()) == UNSUPPORTED
    assert b"hex-27 elasticity operator" in _lib.lib.mfem_last_error() and b"mesh operator" in _lib.lib.mfem_last_error()
    torch.cuda.synchronize()
    assert bool((r == sentinel).all())
    # all four multigrid creates and Pr_Multigrid_
    hm = C.c_uint64(1)
    for name in ("mfem_brick_multigrid_create", "mfem_brick_multigrid_create_nonsymmetric", "mfem_brick_multigrid_create_elasticity",
                 "mfem_brick_multigrid_create_hex27"):
        hm.value = 1
        assert getattr(_lib.lib, name)(ctx._h, S.op._h, None, C.byref(hm)) == UNSUPPORTED and hm.value == 0, name
        assert b"does not exist yet" in _lib.lib.mfem_last_error(), name
    with pytest.raises(mf.MultigridRefused, match="does not exist yet"):
        S.op.multigrid()
    xs = torch.full_like(S.b, sentinel)

    def solve(c=ctx, handle=S.op._h, **kw):
        opt = dict(method=mf.idrs_, precond=1, l_or_s=8, maxiter=2000, max_pass=4, check_every=32, converge_tol=S.tol, seed=1)
        opt.update(kw)
        oo = _lib.SolveOptions(**opt)
        return _lib.lib.mfem_solve_operator(c._h, handle, S.b.data_ptr(), xs.data_ptr(), C.byref(oo), C.byref(st))

    assert solve(method=mf.cg_, precond=mf.Pr_Multigrid_, l_or_s=0) == UNSUPPORTED
    assert b"does not exist yet" in _lib.lib.mfem_last_error()
    with pytest.raises(mf.MetaFEMError):
        mf.iterative_Solve(S.op, None, S.b, S.tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Multigrid_)
    assert solve(method=mf.lsqr_) == UNSUPPORTED
    assert solve(precond=mf.Pr_Jacobi_colnorm_) == UNSUPPORTED
    assert solve(left_precond=mf.Pl_Jacobi_) == UNSUPPORTED
    assert solve(scale_in_place=1) == INVALID
    other_ctx = mf.Context(0)
    try:
        assert solve(c=other_ctx) == INVALID and b"another context" in _lib.lib.mfem_last_error()
        assert _lib.lib.mfem_brick_operator_residual_elasticity(other_ctx._h, S.op._h, S.b.data_ptr(), xs.data_ptr()) == INVALID
    finally:
        other_ctx.close()
    assert _lib.lib.mfem_brick_operator_residual_elasticity(ctx._h, S.op._h, None, xs.data_ptr()) == INVALID
    torch.cuda.synchronize()
    assert int(_lib.lib.mfem_debug_brick_operator_count()) == n0  # nothing launched
    assert bool((xs == sentinel).all())                            # nothing written
    # ... and the handle is still usable
    assert solve() == 0 and st.converged == 1 and not bool((xs == sentinel).any())
    res = np.linalg.norm(S.bh - S.Ko @ xs.cpu().numpy()) / np.sqrt(S.n)
    assert res <= 2 * S.tol


# ---- 9. set_params and live coordinates --------------------------------------------------------------------------------------------------------------
def test_set_params_changes_the_product_and_coordinates_are_read_live(mf):
    import torch

    n, itg = (3, 2, 4), 5
    brick = mf.make_Brick(X, n, 2, itg)
    op = brick.elasticity_operator_hex27(LAM, MU, TAU_ONE, _bits([4]))
    xh = np.random.default_rng(2).uniform(-1.0, 1.0, op.n)
    x = _dev(xh)
    before = op.mul_(torch.empty_like(x), x)
    moved = _distort(np.stack([brick.coords_view(d).cpu().numpy() for d in range(3)], axis=1))  # move the coordinates under the operator
    _move(brick, moved)
    after_move = op.mul_(torch.empty_like(x), x).cpu().numpy()
    want = _Ko(_oracle(X, n, itg, False, [4], [], coords=moved)) @ xh
    assert not np.array_equal(before.cpu().numpy(), after_move)
    assert np.abs(after_move - want).max() <= 1e-11 * np.abs(want).max()
    op.set_params(2.0 * LAM, 0.5 * MU, 3.0, _bits([4, 3]))
    want = _Ko(_oracle(X, n, itg, False, [4, 3], [], tau=3.0, lam=2.0 * LAM, mu=0.5 * MU, coords=moved)) @ xh
    got = op.mul_(torch.empty_like(x), x).cpu().numpy()
    assert not np.array_equal(got, after_move)
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


# ---- 10. ElasticityDomain(matrix_free="any") -----------------------------------------------------------------------------------------------------------
def test_matrix_free_any_domain_solves_the_cantilever_and_holds_no_matrix(mf):
    """The unit cube of 4 x 2 x 2 order-2 elements held by the penalty on x0, sigma_11 = 0.01 pulled on x1: one Newton step with cg! + Pr_Jacobi! to
    1e-12, against -spsolve(Ko, f) of the oracle (the sibling domain test's argument and its bound, 1e-5 of max |x|)."""
    import scipy.sparse.linalg as spl

    x, n, itg = (1.0, 1.0, 1.0), (4, 2, 2), 5
    pen, tra = mf.FACE_BITS["x0"], mf.FACE_BITS["x1"]
    sig = (0.01, 0.0, 0.0, 0.0, 0.0, 0.0)
    od = _oracle(x, n, itg, False, [FACE_NAMES.index("x0")], [FACE_NAMES.index("x1")], tau=TAU_REF, sig=sig)
    od.x_star[:] = 0.0
    od.K_nonlinear_func()
    want = -spl.spsolve(_Ko(od).tocsc(), od.residue)
    brick = mf.make_Brick(x, n, 2, itg)
    brick.pattern = None  # never called
    dom = mf.ElasticityDomain(brick, LAM, MU, TAU_REF, pen, tra, sig, matrix_free="any")
    assert dom.matrix_free is True and dom.matrix_free_reason is None
    assert isinstance(dom.A, mf.Hex27ElasticityBrickOperator) and dom.A.n == 3 * brick.ncp and dom.K_linear is None and dom.K_total is None
    assert dom.A.nnz == 0 and not hasattr(dom.A, "rowptr")
    default_solver = dom.linear_solver
    dom.converge_tol = 1e-10
    stats = []

    def solver(gf):
        dx, st = mf.iterative_Solve(gf.A, gf.K_total, gf.residue, 1e-12, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=4000, max_pass=3)
        stats.append(st)
        return dx

    dom.linear_solver = solver
    hist = dom.update_OneStep()
    print(f"history {hist}, {stats[0].iterations} iterations")
    assert len(hist) == 2 and hist[1] < 1e-10 and stats[0].converged == 1
    got = dom.x.cpu().numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print(f"|x - x_oracle| / max|x| = {err:.2e} (max|x| = {scale:.3e})")
    assert scale > 1e-3
    assert err <= 1e-5
    # the default solver stands (idrs!(8)) and converges too
    dom2 = mf.ElasticityDomain(mf.make_Brick(x, n, 2, itg), LAM, MU, TAU_REF, pen, tra, sig, matrix_free="any", multigrid=True)
    assert dom2.multigrid is False and "does not exist yet" in dom2.multigrid_reason
    assert dom2.linear_solver.__code__ is default_solver.__code__
    dom2.converge_tol = 1e-8
    hist2 = dom2.update_OneStep()
    assert len(hist2) == 2 and hist2[-1] < 1e-8, hist2
    # matrix_free = True keeps falling back on a hex-27 brick; a slab falls back under "any"
    dom3 = mf.ElasticityDomain(mf.make_Brick(x, n, 2, itg), LAM, MU, TAU_REF, pen, matrix_free=True)
    assert dom3.matrix_free is False and "hex-27" in dom3.matrix_free_reason and isinstance(dom3.A, mf.FEM_SpMat_CSR)
    slab = mf.make_Brick(x, (3, 2, 2), 2, itg)
    slab.set_slab(2, 4)
    dom4 = mf.ElasticityDomain(slab, LAM, MU, TAU_REF, pen, matrix_free="any")
    assert dom4.matrix_free is False and "slab" in dom4.matrix_free_reason and isinstance(dom4.A, mf.FEM_SpMat_CSR)
    with pytest.raises(ValueError):
        mf.ElasticityDomain(brick, LAM, MU, TAU_REF, pen, matrix_free="all")


def test_matrix_free_any_on_a_hex8_brick_is_matrix_free_true(mf):
    import torch

    doms = []
    for word in ("any", True):
        dom = mf.ElasticityDomain(mf.make_Brick(X, (5, 4, 3), 1, 3), LAM, MU, TAU_REF, mf.FACE_BITS["x0"], mf.FACE_BITS["x1"], SIG6, matrix_free=word)
        assert dom.matrix_free is True and type(dom.A) is mf.ElasticityBrickOperator and dom.K_linear is None
        dom.update_OneStep()
        doms.append(dom)
    assert torch.equal(doms[0].x, doms[1].x)
