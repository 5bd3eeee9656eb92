"""GPU parity of gmres! (05_GMRES.jl:48-100) through iterative_Solve! (02_Preconditioner.jl:32-76): against the numpy restatement
of tests/test_gmres_cpu.py under the unchanged oracle.solvers.iterative_solve, the direct solve, the reference's MGS order
(mfem_debug_set("gmres", 1, 0)), the solver layouts, and the reference's stress-concentration example that selects gmres!."""
import importlib.util
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _restated():
    spec = importlib.util.spec_from_file_location("_gmres_restated", os.path.join(HERE, "test_gmres_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.gmres


gmres_ref = _restated()


def _thermal_system(n=(7, 6, 5), distort=True):
    from oracle import fem, mesh as om, problems, reference_element as re_

    x = (1.0, 1.0, 1.0)
    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, 3)
    msh = om.lattice_mesh(x, n, disc)
    if distort:
        c = msh.coords
        msh.coords = c + 0.02 * np.stack([np.sin(3 * c[:, 1]), np.sin(2 * c[:, 2]), c[:, 0] * c[:, 1]], axis=1)
    fac = om.boundary_facets_structured(x, n, 3)
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, 0.6), [(fac, problems.thermal_convection(25.0, 293.15))])
    od.controlpoints["s"] = np.full(msh.ncp, 1600.0)
    od.update_time(); od.K_linear_func(); od.update_x_star(); od.K_nonlinear_func()
    return od.pattern.rowptr, od.pattern.colidx, od.K_total.copy(), od.residue.copy()


def _nonsymmetric_system():
    """quad-8 serendipity, Nitsche Dirichlet => nonsymmetric K."""
    from oracle import fem, mesh as om, problems, reference_element as re_

    L1, L2, nx, ny = 0.02, 0.01, 16, 8
    disc = re_.initialize_classical_element(2, "CUBE", 2, 1, 5, itp_type="Serendipity")
    vert, conn = om.make_square((L1, L2), (nx, ny))
    mesh = om.mesh_classical(vert, conn, disc)
    fac = om.boundary_facets(mesh)
    err = (L1 / nx) * 0.01
    lr = (np.abs(fac.centroid[:, 0]) < err) | (np.abs(fac.centroid[:, 0] - L1) < err)
    top = np.abs(fac.centroid[:, 1] - L2) < err
    dom = fem.FEMDomain(mesh, disc, 1, problems.thermal_domain(2, 3),
                        [(fac.select(lr), problems.thermal_fixed(2, 1000.0, 1173.15, 3)),
                         (fac.select(top), problems.thermal_convection(50, 323.15, 0.7, 5.669e-8))])
    dom.controlpoints["s"] = np.zeros(mesh.ncp)
    dom.update_time(); dom.K_linear_func(); dom.update_x_star(); dom.K_nonlinear_func()
    return dom.pattern.rowptr, dom.pattern.colidx, dom.K_total.copy(), dom.residue.copy()


def _gpu_solve(mf, sysm, **kw):
    import torch

    rowptr, col, K, b = sysm
    A = mf.FEM_SpMat_CSR(torch.tensor(rowptr, device="cuda"), torch.tensor(col, device="cuda"), b.size)
    Kt = torch.tensor(K, device="cuda")
    dx, st = mf.iterative_Solve(A, Kt, torch.tensor(b, device="cuda"), **kw)
    return dx.cpu().numpy(), st, Kt.cpu().numpy()


def _diag_system(n, v=3.0):
    rowptr = np.arange(n + 1, dtype=np.int32)
    col = np.arange(n, dtype=np.int32)
    return rowptr, col, np.full(n, v), np.ones(n)


@pytest.mark.parametrize("system", ["thermal", "nonsym"])
@pytest.mark.parametrize("s", [5, 20])
def test_gmres_matches_restatement_and_direct(mf, system, s):
    from oracle import solvers

    sysm = _thermal_system() if system == "thermal" else _nonsymmetric_system()
    rowptr, col, K, b = sysm
    ref = solvers.solver_lu_cpu(rowptr, col, K, b)
    tol = 1e-10 * solvers.normalized_norm(b)
    info = solvers.SolveInfo()
    xo = solvers.iterative_solve(rowptr, col, K, b, tol, Sv_func=gmres_ref, maxiter=2000, max_pass=6, s=s, info=info)
    x, st, K_after = _gpu_solve(mf, sysm, converge_tol=tol, Sv_func=mf.gmres_, maxiter=2000, max_pass=6, s=s, check_every=5)
    assert st.converged == 1 and st.final_res < tol
    assert np.array_equal(K_after, K)
    scale = np.abs(ref).max()
    assert np.abs(x - ref).max() <= 1e-8 * scale
    assert np.abs(x - xo).max() <= 1e-8 * scale
    assert st.passes == info.passes
    # CGS2 against the restatement's MGS order: the same iteration in exact arithmetic.  Over the ~250 cycles GMRES(5) needs on the nonsymmetric
    # system the round-off moves the cycle where the true residual crosses tol by a few cycles (measured: 1241 against 1286 iterations)
    assert abs(st.iterations - info.iters) <= (s if s >= 20 else 0.05 * info.iters), (st.iterations, info.iters)


def test_first_cycle_step_by_step(mf):
    """One cycle from x0 = 0: the reference's MGS order matches the restatement to round-off, the default CGS2 form matches it."""
    from metafem_jl_amd import _lib
    from oracle import solvers

    sysm = _nonsymmetric_system()
    rowptr, col, K, b = sysm
    for s in (5, 20):
        xo = solvers.iterative_solve(rowptr, col, K, b, 1e-300, Sv_func=gmres_ref, maxiter=s, max_pass=1, s=s)
        try:
            _lib.lib.mfem_debug_set_gmres(1)
            xl, st, _ = _gpu_solve(mf, sysm, converge_tol=1e-300, Sv_func=mf.gmres_, maxiter=s, max_pass=1, s=s)
        finally:
            _lib.lib.mfem_debug_set_gmres(0)
        assert st.iterations == s + 1
        assert np.abs(xl - xo).max() <= 1e-11 * np.abs(xo).max(), s
        xc, st, _ = _gpu_solve(mf, sysm, converge_tol=1e-300, Sv_func=mf.gmres_, maxiter=s, max_pass=1, s=s)
        assert np.abs(xc - xl).max() <= 1e-10 * np.abs(xl).max(), s


def test_exact_breakdown(mf):
    """A = 3 I, b = ones(16): Q1 = 0.25, Q1.Q1 = 1, H[1,1] = 3 and Q2 = 0 exactly.  The reference's slice H[1:1, 1:0] (05_GMRES.jl:73) would return b."""
    sysm = _diag_system(16)
    x, st, _ = _gpu_solve(mf, sysm, converge_tol=1e-12, Sv_func=mf.gmres_, Pr_func=mf.Identity, maxiter=2000, max_pass=1, s=20)
    assert st.converged == 1 and st.iterations == 2
    assert np.abs(x - 1.0 / 3.0).max() <= 1e-15 / 3.0
    # fewer unknowns than the restart length
    from oracle import solvers

    rng = np.random.default_rng(3)
    n = 8
    M = np.eye(n) * 4.0 + rng.random((n, n)) * 0.5
    rowptr = np.arange(0, n * n + 1, n, dtype=np.int32)
    col = np.tile(np.arange(n, dtype=np.int32), n)
    rhs = rng.random(n)
    x, st, _ = _gpu_solve(mf, (rowptr, col, M.ravel().copy(), rhs), converge_tol=1e-12, Sv_func=mf.gmres_, maxiter=2000, max_pass=4, s=20)
    assert np.all(np.isfinite(x)) and st.converged == 1
    assert np.abs(x - np.linalg.solve(M, rhs)).max() <= 1e-10 * np.abs(x).max()
    assert solvers.normalized_norm(M @ x - rhs) < 1e-12


def test_limits_and_accounting(mf):
    sysm = _thermal_system((5, 5, 5), distort=False)
    s, maxiter, passes = 20, 40, 3
    _, st, _ = _gpu_solve(mf, sysm, converge_tol=1e-300, Sv_func=mf.gmres_, maxiter=maxiter, max_pass=passes, s=s)
    assert st.passes == passes and st.iterations == passes * 41 and not st.converged
    # two cycles of s + 1 products per pass, the start-of-pass products of passes 2 and 3 (pass 1 starts from x0 = 0), the products between passes
    assert st.spmv_count == passes * 2 * (s + 1) + (passes - 1) + passes
    rowptr, col, K, b = sysm
    _, st, _ = _gpu_solve(mf, (rowptr, col, K, np.zeros_like(b)), converge_tol=1e-8, Sv_func=mf.gmres_, maxiter=100, max_pass=2, s=20)
    assert st.iterations == 0 and st.converged == 1
    with pytest.raises(mf.MetaFEMError):
        _gpu_solve(mf, sysm, converge_tol=1e-8, Sv_func=mf.gmres_, maxiter=100, max_pass=2, s=33)


@pytest.mark.parametrize("pl,pr", [("diag", "diag"), ("rownorm", "diag"), ("none", "colnorm")])
def test_preconditioners(mf, pl, pr):
    from oracle import solvers

    sysm = _nonsymmetric_system()
    rowptr, col, K, b = sysm
    tol = 1e-10 * solvers.normalized_norm(b)
    pl_o = {"diag": solvers.pl_jacobi, "rownorm": lambda A: solvers.pl_jacobi(A, normalized_by_row=True), "none": None}[pl]
    pr_o = {"diag": solvers.pr_jacobi, "colnorm": lambda A: solvers.pr_jacobi(A, normalized_by_column=True)}[pr]
    info = solvers.SolveInfo()
    xo = solvers.iterative_solve(rowptr, col, K, b, tol, Sv_func=gmres_ref, Pr_func=pr_o, Pl_func=pl_o, maxiter=2000, max_pass=6, s=20, info=info)
    pl_d = {"diag": mf.Pl_Jacobi_, "rownorm": mf.Pl_Jacobi_rownorm_, "none": mf.Identity}[pl]
    pr_d = {"diag": mf.Pr_Jacobi_, "colnorm": mf.Pr_Jacobi_colnorm_}[pr]
    x, st, K_after = _gpu_solve(mf, sysm, converge_tol=tol, Sv_func=mf.gmres_, Pr_func=pr_d, Pl_func=pl_d, maxiter=2000, max_pass=6, s=20)
    assert st.converged == 1 and np.array_equal(K_after, K)
    assert np.abs(x - xo).max() <= 1e-8 * np.abs(xo).max()
    # (with a left preconditioner a pass stops on the preconditioned residual: the true one can land on either side of tol -- one pass more or less)
    assert abs(st.passes - info.passes) <= 1


@pytest.fixture()
def small_layouts():
    from metafem_jl_amd import _lib

    _lib.lib.mfem_debug_set_layout_min_rows(0, 0)
    yield _lib
    _lib.lib.mfem_debug_set_layout_min_rows(262144, 1000000)
    _lib.lib.mfem_debug_set_lat8(1)
    _lib.lib.mfem_debug_set_ell(1)
    _lib.lib.mfem_debug_set_sell(1)
    _lib.lib.mfem_debug_set_graphs(1, 0)


def test_layouts_and_reproducibility(mf, small_layouts):
    """hex-8 brick on the solver layouts (symmetric lattice tiles for one and three fields) against the CSR kernel; bitwise repeatability on the
    CSR kernel; graph replay against direct launches."""
    _lib = small_layouts
    b = mf.make_Brick((1.0, 1.0, 1.0), (12, 9, 10), 1, 3)
    for fields in (1, 3):
        A = b.pattern(fields)
        if fields == 1:
            K = b.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F)
        else:
            K = b.assemble_elasticity(A, 0.5769230769230769, 0.38461538461538464, 1000.0, mf.FACE_BITS["x0"])
        rhs = mf.FEM_rand(A.n, 5, 0) - 0.5
        c0 = int(_lib.lib.mfem_debug_lat8_spmv_count())
        x_lay, st = mf.iterative_Solve(A, K, rhs, 1e-11, Sv_func=mf.gmres_, maxiter=6000, max_pass=6, s=20)
        assert st.converged and int(_lib.lib.mfem_debug_lat8_spmv_count()) > c0
        _lib.lib.mfem_debug_set_lat8(0)
        _lib.lib.mfem_debug_set_ell(0)
        _lib.lib.mfem_debug_set_sell(0)
        try:
            x_csr, st = mf.iterative_Solve(A, K, rhs, 1e-11, Sv_func=mf.gmres_, maxiter=6000, max_pass=6, s=20)
            assert st.converged
            x_csr2, _ = mf.iterative_Solve(A, K, rhs, 1e-11, Sv_func=mf.gmres_, maxiter=6000, max_pass=6, s=20)
            _lib.lib.mfem_debug_set_graphs(0, 0)
            x_nog, _ = mf.iterative_Solve(A, K, rhs, 1e-11, Sv_func=mf.gmres_, maxiter=6000, max_pass=6, s=20)
        finally:
            _lib.lib.mfem_debug_set_graphs(1, 0)
            _lib.lib.mfem_debug_set_lat8(1)
            _lib.lib.mfem_debug_set_ell(1)
            _lib.lib.mfem_debug_set_sell(1)
        x_lay, x_csr = x_lay.cpu().numpy(), x_csr.cpu().numpy()
        assert np.abs(x_lay - x_csr).max() <= 1e-10 * np.abs(x_csr).max(), fields
        assert np.array_equal(x_csr, x_csr2.cpu().numpy()), fields
        assert np.array_equal(x_csr, x_nog.cpu().numpy()), fields


def _wf(wf):
    from metafem_jl_amd import generic as G

    return G.WeakForm(inner_vars=list(wf.inner_vars), cp_ext_vars=list(wf.cp_ext_vars), normals=list(wf.normals),
                      residues=[G.ResTerm(r.dual_pos, r.dual_s, r.fn) for r in wf.residues],
                      linear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.linear_gradients],
                      nonlinear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.nonlinear_gradients])


@pytest.mark.parametrize("dim", [2, 3])
def test_stress_concentration_script_with_gmres(mf, dim):
    """2D_Script.jl:63 as written (and 3D_Script.jl:68's gmres! line): gmres!, maxiter 2000, max_pass 20, s = 20, converge_tol 1e-8."""
    import torch
    from metafem_jl_amd import element, generic as G, mesh as pm
    from oracle import problems, stress_concentration as scn
    from oracle.cantilever import traction_field

    z = np.load(os.path.join(GOLD, f"stress_concentration_{dim}d.npz"))
    space = element.classical_space(dim, "Serendipity", 2, 5)
    msh = pm.mesh_Classical(z["vert"], z["conn"].astype(np.int64), space)
    fac = pm.get_BoundaryMesh(msh)
    E, nu, L, err = 210e9, 0.3, 5.0, 0.05  # 2D_Script.jl:15,31-35
    lam, mu, tau = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu)), 10000 * E / L ** 2
    c = fac.centroid
    bnd = []
    for d in range(dim):
        f = fac.select(np.abs(c[:, d]) < err)
        bnd.append((f.element_ID, f.element_eindex, _wf(scn.penalty_component(d, tau))))
    f = fac.select(np.abs(c[:, 1] - L) < err)
    bnd.append((f.element_ID, f.element_eindex, _wf(traction_field(dim, "sl", rows=[1]))))
    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, dim, _wf(problems.elasticity_domain(dim, lam, mu)), bnd)
    for v in {2: (2, 3), 3: (2, 4, 6)}[dim]:
        gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device="cuda")
    gd.converge_tol = 1e-8
    stats = []

    def solver(g):
        dx, st = mf.iterative_Solve(g.A, g.K_total, g.residue, g.converge_tol, Sv_func=mf.gmres_, maxiter=2000, max_pass=20, s=20)
        stats.append(st)
        return dx

    gd.linear_solver = solver
    hist = gd.update_OneStep()
    assert len(stats) == 1 and stats[0].converged and stats[0].passes == 1, [(s.passes, s.iterations, s.final_res) for s in stats]
    assert hist[-1] < gd.converge_tol
    got = gd.x.cpu().numpy()
    d, idx = cKDTree(msh.coords).query(z["xyz"])
    assert d.max() < 1e-7 and msh.ncp == z["d1"].size
    n, scale = msh.ncp, np.abs(z["d2"]).max()
    for fld in range(dim):
        assert np.abs(got[fld * n:(fld + 1) * n][idx] - z[f"d{fld + 1}"]).max() < 1e-5 * scale
