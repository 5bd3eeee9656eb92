"""tfqmr! and lsqr! without a GPU: numpy restatements of the reference's solvers (src/solver/linear_solver/08_QMR.jl:3-74 and
06_LSQR.jl:10-70), statement for statement, as bodies of the unchanged oracle.solvers.iterative_solve; cgs! (07_CGS.jl:13-52) is
oracle.solvers_next.cgs.  They reach the direct solve on the small thermal system and on a nonsymmetric Nitsche system, lsqr! on a random
nonsymmetric sparse matrix too.  tests/test_gpu_krylov_next.py compares the device solvers with them iterate by iterate.

Every restatement takes an optional `products` list whose first entry counts the products with A and A' it runs (the header's
spmv_count formula of mfem_solve_stats); `beta_zero` collects the lsqr! iterations that took the beta == 0 branch."""
import os
import re

import numpy as np
import scipy.sparse as sp

from oracle import solvers
from oracle.solvers_next import cgs as cgs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _count(products, k=1):
    if products is not None:
        products[0] += k


def cgs(x, A, b, r, *, Pl=solvers.Identity(), tol, maxiter, products=None, **kw):
    """cgs! (oracle.solvers_next.cgs) with its products counted: the residual at the start, then A u and the true residual per iteration."""
    _count(products)
    it = cgs_oracle(x, A, b, r, Pl=Pl, tol=tol, maxiter=maxiter, **kw)
    _count(products, 2 * max(it - 1, 0))
    return it


def tfqmr(x, A, b, r, *, Pl=solvers.Identity(), tol, maxiter, checkiter=200, products=None, **_):
    """tfqmr! (08_QMR.jl:3-74)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _tfqmr(x, A, b, r, Pl=Pl, tol=tol, maxiter=maxiter, checkiter=checkiter, products=products)


def _tfqmr(x, A, b, r, *, Pl, tol, maxiter, checkiter, products):
    solvers.mul(r, A, x, -1.0)  # :4-7
    _count(products)
    r += b
    Pl(r)
    if solvers.normalized_norm(r) <= tol:
        return 0
    it = 1  # :9
    n = r.size
    alpha = beta = c = 1.0  # :12
    r0, r_cgs, p, q, u, v, d, tmp = (np.zeros(n) for _ in range(8))  # :13-20
    r0[:] = r  # :22-25
    r_cgs[:] = r
    p[:] = r
    u[:] = r
    solvers.mul(v, A, p)  # :26-27
    _count(products)
    Pl(v)
    # (scalars as numpy floats: a breakdown divides by zero into inf / nan as Julia's Float64 does, instead of raising)
    r_norm = r_norm_old = tau = np.float64(np.linalg.norm(r))  # :28
    rho = rhobar = np.float64(r @ r)  # :29
    theta = eta = np.float64(0.0)  # :30
    while True:
        alpha = rho / np.float64(v @ r0)  # :33
        q[:] = u - alpha * v  # :34
        v[:] = u + q  # :35
        solvers.mul(tmp, A, v)  # :36-37
        _count(products)
        Pl(tmp)
        r_cgs -= alpha * tmp  # :38
        r_norm_old = r_norm  # :40
        r_norm = np.float64(np.linalg.norm(r_cgs))  # :41
        d[:] = u + (theta ** 2 * eta / alpha) * d  # :43
        theta = r_norm_old / tau  # :44
        c = 1 / np.sqrt(1 + theta ** 2)  # :45
        tau *= theta * c  # :46
        eta = c ** 2 * alpha  # :47
        x += eta * d  # :48
        d[:] = q + (theta ** 2 * eta / alpha) * d  # :50
        theta = np.sqrt(r_norm * r_norm_old) / tau  # :51
        c = 1 / np.sqrt(1 + theta ** 2)  # :52
        tau *= theta * c  # :53
        eta = c ** 2 * alpha  # :54
        x += eta * d  # :55
        rhobar = rho  # :57
        rho = np.float64(r_cgs @ r0)  # :58
        beta = rho / rhobar  # :59
        u[:] = r_cgs + beta * q  # :60
        p[:] = u + beta * (q + beta * p)  # :61
        solvers.mul(v, A, p)  # :62-63
        _count(products)
        Pl(v)
        it += 1  # :65
        if it > maxiter:  # :66
            return it
        if it % checkiter == 0:  # :67-72
            solvers.mul(r, A, x, -1.0)
            _count(products)
            r += b
            Pl(r)
            if solvers.normalized_norm(r) <= tol:
                return it


def lsqr(x, A, b, r, *, Pl=solvers.Identity(), tol, maxiter, products=None, beta_zero=None, **_):
    """lsqr! (06_LSQR.jl:10-70); A' u is tmul!(tmp, A, u) = A.T @ u, on the Pr-scaled A the restart wrapper hands over."""
    solvers.mul(r, A, x, -1.0)  # :11-14
    _count(products)
    r += b
    Pl(r)
    if solvers.normalized_norm(r) <= tol:
        return 0
    it = 1  # :16
    u = r.copy()  # :18
    beta = float(np.linalg.norm(u))  # :19
    u /= beta  # :20
    v = A.T @ u  # :23 tmul!(v, A, u)
    _count(products)
    Pl(v)  # :24
    alpha = float(np.linalg.norm(v))  # :25
    if alpha != 0:  # :26-28
        v /= alpha
    w = v.copy()  # :30
    phibar = beta  # :31
    rhobar = alpha  # :32
    tmp = u.copy()  # :34
    while True:
        solvers.mul(tmp, A, v)  # :36
        _count(products)
        u[:] = Pl(tmp) - alpha * u  # :37
        beta = float(np.linalg.norm(u))  # :39
        if beta != 0:  # :40-49
            u /= beta
            tmp[:] = A.T @ u
            _count(products)
            v[:] = Pl(tmp) - beta * v
            alpha = float(np.linalg.norm(v))
            if alpha != 0:
                v /= alpha
        elif beta_zero is not None:
            beta_zero.append(it)
        rho = np.sqrt(abs(rhobar) ** 2 + abs(beta) ** 2)  # :51
        c = rhobar / rho  # :52
        s = beta / rho  # :53
        theta = s * alpha  # :54
        rhobar = -c * alpha  # :55
        phi = c * phibar  # :56
        phibar = s * phibar  # :57
        x += (phi / rho) * w  # :59
        w[:] = v - (theta / rho) * w  # :60
        it += 1  # :62
        solvers.mul(r, A, x, -1.0)  # :64-66
        _count(products)
        r += b
        Pl(r)
        if solvers.normalized_norm(r) <= tol or it > maxiter:  # :67
            return it


# -- systems ---------------------------------------------------------------------------------------------------------------------
def thermal_system(n=(7, 6, 5), distort=True):
    """hex-8 thermal brick with convection faces (symmetric K)."""
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


def nitsche_system(nx=16, ny=8):
    """quad-8 serendipity, temperature fixed by the Nitsche form on two faces: nonsymmetric K."""
    from oracle import fem, mesh as om, problems, reference_element as re_

    L1, L2 = 0.02, 0.01
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


def random_system(n=120, density=0.05, seed=7):
    """sprand-like nonsymmetric sparse matrix with a nonzero diagonal (rows in CSR order, columns sorted)."""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=density, random_state=rng, format="csr") + sp.eye(n) * 0.5
    A = A.tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), rng.standard_normal(n)


# -- tests -----------------------------------------------------------------------------------------------------------------------
def _solve(sysm, Sv_func, tol_rel, **kw):
    rowptr, col, K, b = sysm
    ref = solvers.solver_lu_cpu(rowptr, col, K, b)
    info = solvers.SolveInfo()
    tol = tol_rel * solvers.normalized_norm(b)
    x = solvers.iterative_solve(rowptr, col, K, b, tol, Sv_func=Sv_func, info=info, **kw)
    return x, ref, info, tol


def test_tfqmr_reaches_the_direct_solve_on_the_thermal_system():
    x, ref, info, tol = _solve(thermal_system(), tfqmr, 1e-10, maxiter=2000, max_pass=4, checkiter=10)
    assert info.res < tol
    assert np.abs(x - ref).max() <= 1e-8 * np.abs(ref).max()


def test_tfqmr_reaches_the_direct_solve_on_the_nitsche_system():
    x, ref, info, tol = _solve(nitsche_system(), tfqmr, 1e-10, maxiter=4000, max_pass=6, checkiter=20)
    assert info.res < tol
    assert np.abs(x - ref).max() <= 1e-7 * np.abs(ref).max()


def test_lsqr_reaches_the_direct_solve_on_the_thermal_system():
    x, ref, info, tol = _solve(thermal_system(), lsqr, 1e-10, maxiter=5000, max_pass=4)
    assert info.res < tol
    assert np.abs(x - ref).max() <= 1e-8 * np.abs(ref).max()


def test_lsqr_reaches_the_direct_solve_on_the_nitsche_system():
    x, ref, info, tol = _solve(nitsche_system(), lsqr, 1e-10, maxiter=20000, max_pass=6)
    assert info.res < tol
    assert np.abs(x - ref).max() <= 1e-7 * np.abs(ref).max()


def test_lsqr_reaches_the_direct_solve_on_a_random_nonsymmetric_matrix():
    x, ref, info, tol = _solve(random_system(), lsqr, 1e-10, maxiter=5000, max_pass=4, Pr_func=None)
    assert info.res < tol
    assert np.abs(x - ref).max() <= 1e-7 * np.abs(ref).max()


def test_cgs_reaches_the_direct_solve_on_the_thermal_system():
    x, ref, info, tol = _solve(thermal_system(), cgs, 1e-10, maxiter=2000, max_pass=4)
    assert info.res < tol
    assert np.abs(x - ref).max() <= 1e-8 * np.abs(ref).max()


def test_lsqr_takes_the_beta_zero_branch_on_a_scaled_identity():
    """A = 3 I, b = ones(16): u = b / 4, v = A' u / 3 = u; then A v - alpha u = 3/4 - 3 * 1/4 = 0 exactly -- beta == 0, the A' u of the
    branch is skipped and one step gives x = b / 3."""
    n = 16
    A = sp.csr_matrix(3.0 * np.eye(n))
    b = np.ones(n)
    x = np.zeros(n)
    products, beta_zero = [0], []
    it = lsqr(x, A, b, b.copy(), tol=1e-300, maxiter=1, products=products, beta_zero=beta_zero)
    assert it == 2
    assert beta_zero == [1]
    assert products[0] == 1 + 1 + 2  # the start residual, A' u, then A v and the true residual (no A' u)
    assert np.abs(x - b / 3).max() <= 1e-15


def test_header_and_julia_binding_define_the_solver_ids():
    src = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"MFEM_SOLVER_(\w+)\s*=\s*(\d+)", src)}
    assert ids["CGS"] == 5 and ids["TFQMR"] == 6 and ids["LSQR"] == 7
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    m = re.search(r"const SOLVER_ID = Dict\(([^)]*)\)", jl)
    jids = dict((k, int(v)) for k, v in re.findall(r":(\w+!?)\s*=>\s*(\d+)", m.group(1)))
    assert jids["cgs!"] == 5 and jids["tfqmr!"] == 6 and jids["lsqr!"] == 7
    assert "mfem_spmv_csr_t" in jl
