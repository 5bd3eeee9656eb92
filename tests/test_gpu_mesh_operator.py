"""The matrix-free mesh operator (mfem_mesh_operator_*, mfem_solve_operator, csrc/mesh_operator.hip; MeshOperator, GenericDomain(matrix_free=True))
against the assembled K of the default domain (CSR kernel) and the oracle's term-by-term K, on the curved, element-shuffled meshes and forms of
tests/test_gpu_mesh_residual.py (restated here, data only): product, diagonal, bitwise reproducibility, a collapsed element, every Krylov solver with
its product count, reductions across hundreds of workgroups with cycle graphs on and off, the refusals, and the matrix-free domain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (dim, itp_type, itp_order, itg_order, shape, cells)
FAMILIES = {
    "quad8": (2, "Serendipity", 2, 5, "CUBE", (6, 5)),
    "tet10": (3, "Serendipity", 2, 5, "SIMPLEX", (3, 2, 2)),
    "hex8": (3, "Lagrange", 1, 3, "CUBE", (3, 3, 2)),
    "hex20": (3, "Serendipity", 2, 5, "CUBE", (3, 3, 2)),
    "hex27": (3, "Lagrange", 2, 5, "CUBE", (3, 3, 2)),
}
DT = 0.1


def _warp(c):
    dim = c.shape[1]
    out = c.copy()
    for i in range(dim):
        j, k = (i + 1) % dim, (i + 2) % dim
        out[:, i] += 0.05 * np.sin(2.3 * c[:, j] + 1.1 * c[:, k] + 0.4 * i) + 0.04 * c[:, i] * c[:, j]
    return out


def _mesh(fam, block=4, seed=11, cells=None, oracle=True):
    """(space, mesh (warped: curved elements), boundary facets, oracle disc, oracle mesh on the same arrays)."""
    from metafem_jl_amd import element, mesh as pm
    from oracle import mesh as om, reference_element as re_

    dim, itp_type, order, itg, shape, n = FAMILIES[fam]
    n = cells or n
    space = element.classical_space(dim, itp_type, order, itg, shape=shape)
    vert, conn = (pm.make_Square((1.0, 0.8), n, shape) if dim == 2 else pm.make_Brick((1.0, 0.8, 0.9), n, shape))
    nel = conn.shape[1]
    nb = (nel + block - 1) // block
    perm = (np.random.default_rng(seed).permutation(nb)[:, None] * block + np.arange(block)[None, :]).ravel()
    msh = pm.mesh_Classical(vert, conn[:, perm[perm < nel]], space)
    fac = pm.get_BoundaryMesh(msh)
    msh.coords = _warp(msh.coords)
    if not oracle:
        return space, msh, fac, None, None
    disc = re_.initialize_classical_element(dim, shape, order, 1, itg, itp_type=itp_type)
    omesh = om.ClassicalMesh(dim, np.asarray(msh.coords), np.asarray(msh.cp_ids), np.asarray(msh.vert_conn), msh.n_vertices)
    return space, msh, fac, disc, omesh


def _case(name, dim, fac):
    """-> (n_fields, domain form, [(facets, form)], max_time_level, nodal externals)"""
    from metafem_jl_amd import physics as P

    c = fac.centroid
    x0, y1 = fac.select(np.abs(c[:, 0]) < 1e-9), fac.select(np.abs(c[:, 1] - 0.8) < 1e-9)
    rest = fac.select(np.abs(c[:, 0]) >= 1e-9)
    if name == "thermal":
        return 1, P.thermal_domain(dim, 0.6, alpha=0.7, Tenv=300.0), [(fac, P.thermal_convection(25.0, 293.15))], 0, ["s"]
    if name == "nitsche":
        return 1, P.thermal_domain(dim, 0.6), [(rest, P.thermal_convection(25.0, 293.15)), (x0, P.thermal_fixed(dim, 1000.0, 1173.15, 0.6))], 0, ["s"]
    if name == "transient":
        return 1, P.thermal_domain(dim, 0.6, C=4.0), [(fac, P.thermal_convection(25.0, 293.15))], 1, ["s"]
    sl = [f"sl{v}" for v in ((1, 2, 3) if dim == 2 else (1, 2, 3, 4, 5, 6))]
    if name == "elasticity":
        return dim, P.elasticity_domain(dim, 1.7, 0.6), [(x0, P.penalty(list(range(dim)), 37.0)), (y1, P.traction(dim, "sl", rows=[1]))], 0, sl
    if name == "wall":
        return dim, P.elasticity_domain(dim, 1.7, 0.6), [(x0, P.penalty(list(range(dim)), 37.0, wall_syms=[f"w{i}" for i in range(dim)])),
                                                         (y1, P.traction(dim, "sl"))], 0, sl + [f"w{i}" for i in range(dim)]
    if name == "dynamics":
        return dim, P.merge(P.elasticity_domain(dim, 1.7, 0.6), P.elasticity_inertia(dim, 7.8, c=0.3)), [(y1, P.traction(dim, "sl"))], 2, sl
    raise KeyError(name)


CASES = [("hex20", "thermal"), ("hex20", "elasticity"), ("hex20", "transient"), ("tet10", "thermal"), ("tet10", "wall"), ("hex8", "thermal"),
         ("hex8", "dynamics"), ("hex27", "thermal"), ("quad8", "nitsche"), ("quad8", "elasticity")]
IDS = [f"{a}-{b}" for a, b in CASES]
SYMMETRIC = {("hex20", "thermal"), ("hex20", "elasticity"), ("tet10", "wall")}
SOLVE_CASES = [("hex20", "thermal"), ("hex20", "elasticity"), ("tet10", "wall"), ("quad8", "nitsche")]

_BUILT = {}


class _Sys:
    pass


def _built(mf, fam, name):
    """The matrix-free domain, the default domain with K_linear assembled and the oracle's K of one case (dt = 0.1), built once and shared."""
    key = (fam, name)
    if key in _BUILT:
        return _BUILT[key]
    import torch
    from metafem_jl_amd import generic as G
    from oracle import fem, solvers

    space, msh, fac, disc, omesh = _mesh(fam)
    dim = FAMILIES[fam][0]
    nf, wf, bnd, mtl, ext = _case(name, dim, fac)
    S = _Sys()
    doms = []
    for matrix_free in (True, False):
        gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf, [(f.element_ID, f.element_eindex, w) for f, w in bnd],
                             max_time_level=mtl, matrix_free=matrix_free)
        gd.dt = DT
        gd.update_Time()
        gd.K_linear_func()
        doms.append(gd)
    S.md, S.gd = doms
    assert S.md.matrix_free and S.md.matrix_free_reason is None
    od = fem.FEMDomain(omesh, disc, nf, wf, list(bnd), max_time_level=mtl)
    for k in ext:  # (the oracle evaluates every external before the gradient terms; K does not depend on them)
        od.controlpoints[k] = np.zeros(msh.ncp)
    od.dt = DT
    od.update_time()
    od.K_linear_func()
    S.Ko = solvers.csr(od.pattern.rowptr, od.pattern.colidx, od.K_linear.copy(), od.pattern.n)
    S.n = S.gd.A.n
    S.Kg = solvers.csr(S.gd.A.rowptr.cpu().numpy(), S.gd.A.colidx.cpu().numpy(), S.gd.K_linear.cpu().numpy(), S.n)
    rng = np.random.default_rng(7)
    S.x = rng.uniform(-1.0, 1.0, S.n)
    S.b = rng.uniform(-1.0, 1.0, S.n)
    S.dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    _BUILT[key] = S
    return S


@pytest.mark.parametrize("fam,name", CASES, ids=IDS)
def test_product_equals_the_assembled_matrix_and_the_oracle(mf, fam, name):
    import torch

    S = _built(mf, fam, name)
    assert isinstance(S.md.A, mf.MeshOperator) and S.md.A.n == S.n
    x = S.dev(S.x)
    y_csr = mf.mul_(torch.empty_like(x), S.gd.A, S.gd.K_linear, x).cpu().numpy()
    y = mf.mul_(torch.empty_like(x), S.md.A, None, x).cpu().numpy()
    scale = np.abs(y_csr).max()
    assert scale > 0
    e_csr, e_or = np.abs(y - y_csr).max() / scale, np.abs(y - S.Ko @ S.x).max() / np.abs(S.Ko @ S.x).max()
    print(f"{fam}-{name}: |y - y_csr| / max|y| = {e_csr:.2e}, against the oracle {e_or:.2e}")
    assert e_csr <= 1e-12
    assert e_or <= 1e-11
    y0 = np.random.default_rng(8).uniform(-1.0, 1.0, S.n)
    for alpha, beta in ((-1.0, 1.0), (0.5, -2.0)):
        got = S.md.A.mul_(S.dev(y0), x, alpha, beta).cpu().numpy()
        want = mf.mul_(S.dev(y0), S.gd.A, S.gd.K_linear, x, alpha, beta).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (alpha, beta)
    nan = torch.full_like(x, float("nan"))
    got = S.md.A.mul_(nan, x, 1.0, 0.0).cpu().numpy()  # beta == 0 must not read y
    assert np.isfinite(got).all() and got.tobytes() == y.tobytes()


@pytest.mark.parametrize("fam,name", CASES, ids=IDS)
def test_diagonal_equals_the_assembled_diagonal(mf, fam, name):
    S = _built(mf, fam, name)
    d = S.md.A.diagonal().cpu().numpy()
    want = S.Kg.diagonal()
    err = np.abs(d - want).max() / np.abs(want).max()
    print(f"{fam}-{name}: |d - diag K| / max|diag| = {err:.2e}")
    assert err <= 1e-12


def test_control_point_without_elements_has_an_empty_row_and_keeps_the_preset(mf):
    """One extra control point that no element lists: y = beta y on its row, diag 0, and the Jacobi solve keeps d = 1 there and converges."""
    import torch
    from metafem_jl_amd import generic as G

    space, msh, fac, _, _ = _mesh("hex8", oracle=False)
    nf, wf, bnd, mtl, _ = _case("thermal", 3, fac)
    coords = np.vstack([msh.coords, [[3.0, 3.0, 3.0]]])
    md = G.GenericDomain(mf.default_context(), space, coords, msh.cp_ids, nf, wf, [(f.element_ID, f.element_eindex, w) for f, w in bnd],
                         matrix_free=True)
    assert md.matrix_free
    md.K_linear_func()
    n, last = md.A.n, md.A.n - 1
    assert n == msh.ncp + 1
    rng = np.random.default_rng(5)
    x = torch.tensor(rng.uniform(-1.0, 1.0, n), device="cuda")
    y0 = torch.tensor(rng.uniform(-1.0, 1.0, n), device="cuda")
    y = md.A.mul_(y0.clone(), x, 0.7, -3.0)
    assert float(y[last]) == -3.0 * float(y0[last])
    assert float(md.A.mul_(torch.full_like(x, float("nan")), x)[last]) == 0.0
    assert float(md.A.diagonal()[last]) == 0.0
    x[last] = 0.0
    b = md.A.mul_(torch.empty_like(x), x)
    for sv in (mf.idrs_, mf.cg_):
        sol, st = mf.iterative_Solve(md.A, None, b, 1e-10, Sv_func=sv, s=8, maxiter=2000, max_pass=4)
        assert st.converged == 1, (sv, st.final_res)
        r = b - md.A.mul_(torch.empty_like(x), sol)
        assert float(r.norm()) / np.sqrt(n) <= 2e-10
        assert float(sol[last]) == 0.0 and bool(torch.isfinite(sol).all())


def test_two_applications_and_two_solves_give_the_same_bits(mf):
    import torch

    S = _built(mf, "hex20", "elasticity")
    x = S.dev(S.x)
    a = S.md.A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    assert S.md.A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == a
    b = S.dev(S.b)
    xs = [mf.iterative_Solve(S.md.A, None, b, 1e-10, Sv_func=mf.idrs_, s=8, seed=0x5EED, maxiter=2000, max_pass=4)[0].cpu().numpy().tobytes()
          for _ in range(2)]
    assert xs[0] == xs[1]


def test_collapsed_element_gives_the_assembled_product(mf):
    """A hex-8 whose face x = 1 is pinched to an edge (two nodes listed twice): the adjacency holds both entries."""
    import torch
    from metafem_jl_amd import element, generic as G, physics as P

    space = element.classical_space(3, "Lagrange", 1, 3)
    coords = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0], [0, 0, 1], [0, 1, 1]], dtype=float)
    cp = np.array([[0, 1, 2, 3, 4, 1, 2, 5]]).T
    wf = P.thermal_domain(3, 0.6, alpha=0.7, Tenv=300.0)
    x = torch.linspace(-1.0, 2.0, 6, dtype=torch.float64, device="cuda")
    y = []
    for matrix_free in (True, False):
        gd = G.GenericDomain(mf.default_context(), space, coords, cp, 1, wf, [], matrix_free=matrix_free)
        gd.K_linear_func()
        y.append(mf.mul_(torch.empty_like(x), gd.A, gd.K_linear, x).cpu().numpy())
        assert gd.matrix_free == matrix_free
    assert np.abs(y[0] - y[1]).max() <= 1e-12 * np.abs(y[1]).max()


# name -> (Sv_func attribute, s)
SOLVERS = {"cg": ("cg_", 0), "idrs": ("idrs_", 8), "bicgstabl": ("bicgstabl_GS_", 2), "cgs2": ("cgs2_", 0), "gmres": ("gmres_", 0), "cgs": ("cgs_", 0),
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


# (cg! on the symmetric cases only: the Nitsche wall makes K nonsymmetric)
SOLVES = [(sv, fam, name) for sv in SOLVERS for fam, name in SOLVE_CASES if sv != "cg" or (fam, name) in SYMMETRIC]


@pytest.mark.parametrize("solver,fam,name", SOLVES, ids=[f"{s}-{a}-{b}" for s, a, b in SOLVES])
def test_every_solver_converges_with_the_products_of_its_formula(mf, solver, fam, name):
    S = _built(mf, fam, name)
    sv, s = SOLVERS[solver]
    x, st = mf.iterative_Solve(S.md.A, None, S.dev(S.b), 1e-10, Sv_func=getattr(mf, sv), Pr_func=mf.Pr_Jacobi_, s=s, maxiter=MAXITER, max_pass=MAX_PASS)
    res = np.linalg.norm(S.b - S.Ko @ x.cpu().numpy()) / np.sqrt(S.n)
    print(f"{solver} on {fam}-{name}: {st.iterations} iterations, {st.passes} passes, {st.spmv_count} products, residual {res:.2e}")
    assert st.converged == 1
    assert res <= 2e-10
    assert st.spmv_count == _expected_products(solver, st)


def test_solve_without_a_preconditioner(mf):
    S = _built(mf, "hex20", "thermal")
    x, st = mf.iterative_Solve(S.md.A, None, S.dev(S.b), 1e-10, Sv_func=mf.idrs_, Pr_func=mf.Identity, s=8, maxiter=MAXITER, max_pass=MAX_PASS)
    assert st.converged == 1
    assert np.linalg.norm(S.b - S.Ko @ x.cpu().numpy()) / np.sqrt(S.n) <= 2e-10
    assert st.spmv_count == _expected_products("idrs", st)


def test_reductions_across_many_workgroups_with_and_without_cycle_graphs(mf):
    """hex-20 16^3 (4 096 elements, 18 785 control points), elasticity with a penalty wall: the gather and its dot partials span hundreds of workgroups."""
    import torch
    from metafem_jl_amd import _lib, generic as G

    space, msh, fac, _, _ = _mesh("hex20", cells=(16, 16, 16), oracle=False)
    assert msh.cp_ids.shape[1] == 4096 and msh.ncp == 18785
    nf, wf, bnd, mtl, _ = _case("wall", 3, fac)
    doms = []
    for matrix_free in (True, False):
        gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf, [(f.element_ID, f.element_eindex, w) for f, w in bnd],
                             matrix_free=matrix_free)
        gd.K_linear_func()
        doms.append(gd)
    md, gd = doms
    assert md.matrix_free
    n = md.A.n
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.uniform(-1.0, 1.0, n), device="cuda")
    y_csr = mf.mul_(torch.empty_like(x), gd.A, gd.K_linear, x)
    y = md.A.mul_(torch.empty_like(x), x)
    assert float((y - y_csr).abs().max()) <= 1e-12 * float(y_csr.abs().max())
    b = torch.tensor(rng.uniform(-1.0, 1.0, n), device="cuda")
    try:
        for graphs in (1, 0):
            _lib.check(_lib.lib.mfem_debug_set_graphs(graphs, 0))
            for sv in (mf.idrs_, mf.cg_):
                sol, st = mf.iterative_Solve(md.A, None, b, 1e-9, Sv_func=sv, s=8, maxiter=MAXITER, max_pass=MAX_PASS)
                res = float((b - mf.mul_(torch.empty_like(x), gd.A, gd.K_linear, sol)).norm()) / np.sqrt(n)
                print(f"graphs {graphs}, solver {sv}: {st.iterations} iterations, residual {res:.2e}")
                assert st.converged == 1 and res <= 2e-9, (graphs, sv, res)
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)


def test_refusals(mf):
    import torch
    from metafem_jl_amd import _lib

    INVALID, UNSUPPORTED = -1, -3
    S = _built(mf, "hex8", "thermal")
    md = S.md
    ctx = md.ctx
    b = S.dev(S.b)
    sentinel = 123.25
    x = torch.full_like(b, sentinel)
    st = _lib.SolveStats()
    n0 = int(_lib.lib.mfem_debug_mesh_operator_count())

    def solve(handle=md.A._h, bp=None, xp=None, **kw):
        opt = dict(method=mf.idrs_, precond=1, l_or_s=8, maxiter=50, max_pass=1, check_every=32, converge_tol=1e-10, seed=1)
        opt.update(kw)
        o = _lib.SolveOptions(**opt)
        return _lib.lib.mfem_solve_operator(ctx._h, handle, b.data_ptr() if bp is None else bp, x.data_ptr() if xp is None else xp, C.byref(o),
                                            C.byref(st))

    assert solve(method=mf.lsqr_) == UNSUPPORTED
    assert solve(precond=mf.Pr_Jacobi_colnorm_) == UNSUPPORTED
    assert solve(left_precond=mf.Pl_Jacobi_) == UNSUPPORTED
    assert solve(scale_in_place=1) == INVALID
    assert solve(handle=0) == INVALID
    assert _lib.lib.mfem_solve_operator(ctx._h, md.A._h, None, x.data_ptr(), C.byref(_lib.SolveOptions(method=mf.idrs_, maxiter=5, max_pass=1)),
                                        C.byref(st)) == INVALID
    assert _lib.lib.mfem_solve_operator(ctx._h, md.A._h, b.data_ptr(), None, C.byref(_lib.SolveOptions(method=mf.idrs_, maxiter=5, max_pass=1)),
                                        C.byref(st)) == INVALID
    ops = _lib.CommHostOps(None, _lib.ALLREDUCE_CB(lambda *a: 1), _lib.EXCHANGE_CB(lambda *a: 1), 0, 0)
    h = C.c_void_p()
    _lib.check(_lib.lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(h)))
    try:
        _lib.check(_lib.lib.mfem_context_set_comm(ctx._h, h, md.A.n, 1, 1))
        assert solve() == INVALID
        assert b"one rank only" in _lib.lib.mfem_last_error()
    finally:
        _lib.lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        _lib.lib.mfem_comm_destroy(h)
    torch.cuda.synchronize()
    assert int(_lib.lib.mfem_debug_mesh_operator_count()) == n0  # nothing launched
    assert bool((x == sentinel).all())                           # nothing written
    assert solve() == 0 and not bool((x == sentinel).any())
    # apply / diagonal: null handles and arrays
    y = torch.empty_like(b)
    assert _lib.lib.mfem_mesh_operator_apply(ctx._h, 0, b.data_ptr(), y.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_mesh_operator_apply(None, md.A._h, b.data_ptr(), y.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_mesh_operator_apply(ctx._h, md.A._h, None, y.data_ptr(), 1.0, 0.0) == INVALID
    assert _lib.lib.mfem_mesh_operator_diagonal(ctx._h, md.A._h, None) == INVALID
    # the terms: a fresh operator on the same mesh with 9 fields
    T = lambda ds, bs, block, c, nrm=(0.0, 0.0, 0.0): _lib.OperatorTerm(ds, bs, block, 0, c, (C.c_double * 3)(*nrm))
    hnd = C.c_uint64()
    _lib.check(_lib.lib.mfem_mesh_operator_create(ctx._h, 3, md.itp, md.nel, md.ncp, 9, md.coords.data_ptr(), md.cp.data_ptr(), 1, C.byref(hnd)))
    try:
        def set_elements(terms, ref=md._ref.data_ptr()):
            arr = (_lib.OperatorTerm * max(len(terms), 1))(*terms)
            return _lib.lib.mfem_mesh_operator_set_elements(hnd, md.space.itg, ref, md._itgw.data_ptr(), md._adj_ptr.data_ptr(), md._adj.data_ptr(),
                                                            len(terms), arr)

        assert set_elements([T(0, 0, 0, 1.0)]) == 0
        assert set_elements([T(0, 0, 0, 1.0)], ref=None) == INVALID
        assert set_elements([T(0, 0, 0, 1.0, (0.0, 0.5, 0.0))]) == INVALID   # normals exist on facets only
        assert set_elements([T(0, 0, 81, 1.0)]) == INVALID                    # block out of range
        assert set_elements([T(0, 0, -1, 1.0)]) == INVALID
        assert set_elements([T(4, 0, 0, 1.0)]) == INVALID
        assert set_elements([T(0, 0, 0, 1.0)] * 49) == UNSUPPORTED
        assert set_elements([T(0, 0, f * 9 + f, 1.0) for f in range(9)]) == UNSUPPORTED  # 9 dual fields
        assert set_elements([T(0, 0, f * 9 + f, 1.0) for f in range(8)]) == 0
        arr = (_lib.OperatorTerm * 1)(T(0, 0, 0, 1.0))
        assert _lib.lib.mfem_mesh_operator_set_terms(hnd, 3, 1, arr) == INVALID  # no such part
        assert _lib.lib.mfem_mesh_operator_set_terms(0, 0, 1, arr) == INVALID
    finally:
        _lib.lib.mfem_mesh_operator_destroy(hnd)
    bad = C.c_uint64(1)
    assert _lib.lib.mfem_mesh_operator_create(ctx._h, 3, md.itp, md.nel, md.ncp, 1, None, md.cp.data_ptr(), 1, C.byref(bad)) == INVALID and bad.value == 0
    assert _lib.lib.mfem_mesh_operator_create(ctx._h, 3, md.itp, md.nel, md.ncp, 33, md.coords.data_ptr(), md.cp.data_ptr(), 1, C.byref(bad)) == UNSUPPORTED


def _stepped(mf, fam, name, steps, solver, extra=None, ctx=None):
    """update_OneStep on the matrix-free and the default domain with the same linear_solver lambda -> [(domain, histories)]"""
    import torch
    from metafem_jl_amd import generic as G

    space, msh, fac, _, _ = _mesh(fam, oracle=False)
    nf, wf, bnd, mtl, ext = _case(name, FAMILIES[fam][0], fac)
    if extra is not None:
        bnd = extra(fac)
    rng = np.random.default_rng(9)
    ev = {k: rng.uniform(0.5, 1.5, msh.ncp) * (1600.0 if k == "s" else 1.0) for k in ext}
    out = []
    for matrix_free in (True, False):
        gd = G.GenericDomain(ctx or mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf, [(f.element_ID, f.element_eindex, w) for f, w in bnd],
                             max_time_level=mtl, matrix_free=matrix_free)
        for k, v in ev.items():
            gd.controlpoints[k] = torch.tensor(v, device="cuda")
        gd.converge_tol = 1e-9
        # relative residual 1e-12: with condition numbers <= 1e4 the error of each x is below 1e-8 |x| in the worst case (cond * residual / |b|)
        gd.linear_solver = lambda g: mf.iterative_Solve(g.A, g.K_total, g.residue, 1e-12 * mf.normalized_norm(g.residue), Sv_func=solver, s=8,
                                                        maxiter=2000, max_pass=4)[0]
        hist = []
        for dt in steps:
            gd.dt = dt
            hist.append(list(gd.update_OneStep()))
        out.append((gd, hist))
    return out


@pytest.mark.parametrize("fam,name,steps,solver", [("hex20", "thermal", (1.0,), "cg_"), ("hex8", "dynamics", (0.1, 0.05), "idrs_")],
                         ids=["hex20-thermal-robin", "hex8-dynamics-two-steps"])
def test_matrix_free_domain_steps_like_the_default_one(mf, fam, name, steps, solver):
    (md, hm), (gd, hg) = _stepped(mf, fam, name, steps, getattr(mf, solver))
    assert md.matrix_free is True and gd.matrix_free is False
    assert isinstance(md.A, mf.MeshOperator) and md.K_linear is None and md.K_total is None and md.slots is None and md.table_bytes == 0
    xm, xg = md.x.cpu().numpy(), gd.x.cpu().numpy()
    assert np.abs(xg).max() > 0
    assert np.abs(xm - xg).max() <= 1e-8 * np.abs(xg).max()
    assert [len(h) for h in hm] == [len(h) for h in hg]
    assert hm[-1][-1] < 1e-9


def test_matrix_free_domain_holds_no_matrix(mf):
    """hex-20 8^3 thermal on a fresh context: the workspace is the solve's vectors plus the scratch, and construction plus one step allocate less
    than the values of the default domain's pattern alone."""
    import torch
    from metafem_jl_amd import _lib, generic as G, physics as P

    space, msh, fac, _, _ = _mesh("hex20", cells=(8, 8, 8), oracle=False)
    wf, bnd = P.thermal_domain(3, 0.6), [(fac.element_ID, fac.element_eindex, P.thermal_convection(25.0, 293.15))]
    ctx = mf.Context(0)
    try:
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        md = G.GenericDomain(ctx, space, msh.coords, msh.cp_ids, 1, wf, bnd, matrix_free=True)
        assert md.matrix_free
        md.controlpoints["s"] = torch.full((msh.ncp,), 1600.0, dtype=torch.float64, device="cuda")
        md.converge_tol = 1e-9
        stats = []

        def solver(g):
            x, st = mf.iterative_Solve(g.A, g.K_total, g.residue, 1e-11 * mf.normalized_norm(g.residue), Sv_func=mf.cg_, maxiter=2000, max_pass=4)
            stats.append(st)
            return x
        md.linear_solver = solver
        md.update_OneStep()
        torch.cuda.synchronize()
        rise = torch.cuda.memory_allocated() - m0
        assert stats and stats[0].converged == 1 and md.history[-1] < 1e-9
        itp, nel = msh.cp_ids.shape
        n = msh.ncp
        nv, nwork = (n + 31) // 32 * 32, 3  # cg!: r, p, Ap
        scratch = (nel + len(fac.element_ID)) * itp * 1
        ws = int(_lib.lib.mfem_debug_ws_bytes(ctx._h))
        print(f"workspace {ws} B, bound {8 * nv * (4 + nwork) + 8 * scratch + 4096} B")
        assert ws <= 8 * nv * (4 + nwork) + 8 * scratch + 4096
        A, _ = mf.assemble_SparseID(md.cp, n, n_fields=1, index_base=1, with_slots=False, ctx=ctx)
        print(f"rise {rise} B, 8 nnz = {8 * A.nnz} B")
        assert rise < 8 * A.nnz
        A.close()
        md.A.close()
    finally:
        ctx.close()


def test_nonlinear_gradient_falls_back_to_the_default_domain(mf):
    from metafem_jl_amd import physics as P

    extra = lambda fac: [(fac, P.thermal_convection(25.0, 293.15, em=0.8, sigma_b=5.67e-8))]
    (md, hm), (gd, hg) = _stepped(mf, "hex8", "thermal", (1.0,), mf.idrs_, extra=extra)
    assert md.matrix_free is False and "nonlinear" in md.matrix_free_reason
    assert md.K_linear is not None and not isinstance(md.A, mf.MeshOperator)
    assert len(hm[0]) == len(hg[0])
    assert np.abs(md.x.cpu().numpy() - gd.x.cpu().numpy()).max() <= 1e-8 * np.abs(gd.x.cpu().numpy()).max()
