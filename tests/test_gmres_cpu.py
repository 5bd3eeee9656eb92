"""gmres! without a GPU: the solver id in the C header and the Julia binding, and a numpy restatement of the reference's
gmres! (src/solver/linear_solver/05_GMRES.jl:48-100, Hessenberg :7-37) that reproduces the committed result of
examples/linear_elasticity/stress_concentration/2D_Script.jl, which selects it.  tests/test_gpu_gmres.py compares the
device solver with this restatement."""
import math
import os
import re

import numpy as np
from scipy.spatial import cKDTree

from oracle import solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def givens_algorithm(f, g):
    """LinearAlgebra.givensAlgorithm (LAPACK dlartg): (c, s) with [c s; -s c] [f; g] = [r; 0]."""
    safmn2, safmx2 = 2.0 ** -511, 2.0 ** 511  # floatmin2(Float64) and its inverse
    if g == 0.0:
        return 1.0, 0.0
    if f == 0.0:
        return 0.0, 1.0
    f1, g1 = f, g
    scale = max(abs(f1), abs(g1))
    if scale >= safmx2:
        count = 0
        while True:
            count += 1
            f1, g1 = f1 * safmn2, g1 * safmn2
            scale = max(abs(f1), abs(g1))
            if scale < safmx2 or count >= 20:
                break
    elif scale <= safmn2:
        while True:
            f1, g1 = f1 * safmx2, g1 * safmx2
            scale = max(abs(f1), abs(g1))
            if scale > safmn2:
                break
    r = math.sqrt(f1 * f1 + g1 * g1)
    c, s = f1 / r, g1 / r
    if abs(f) > abs(g) and c < 0:
        c, s = -c, -s
    return c, s


def hessenberg(H, rhs):
    """Hessenberg(H, rhs) (05_GMRES.jl:7-37): least squares of the (w+1) x w Hessenberg H by Givens rotations, in place;
    the solution lands in rhs[:w]."""
    width = H.shape[1]
    for i in range(width):
        c, s = givens_algorithm(H[i, i], H[i + 1, i])
        H[i, i] = c * H[i, i] + s * H[i + 1, i]
        for j in range(i + 1, width):
            tmp = -s * H[i, j] + c * H[i + 1, j]
            H[i, j] = c * H[i, j] + s * H[i + 1, j]
            H[i + 1, j] = tmp
        tmp = -s * rhs[i] + c * rhs[i + 1]
        rhs[i] = c * rhs[i] + s * rhs[i + 1]
        rhs[i + 1] = tmp
    for j in range(width - 1, -1, -1):  # ldiv!(UpperTriangular(H[1:w, 1:w]), rhs[1:w]), column by column
        rhs[j] = rhs[j] / H[j, j]
        rhs[:j] -= H[:j, j] * rhs[j]


def gmres(x, A, b, r, *, Pl=solvers.Identity(), tol, maxiter, s=20, **_):
    """gmres! (05_GMRES.jl:48-100), restated operation by operation (modified Gram-Schmidt order).  Body of
    oracle.solvers.iterative_solve: returns the iteration count."""
    solvers.mul(r, A, x, -1.0)
    r += b
    Pl(r)
    if solvers.normalized_norm(r) <= tol:
        return 0
    it = 1
    n = b.size
    Q = [np.zeros(n) for _ in range(s + 1)]
    H = np.zeros((s + 1, s))
    y = np.zeros(s + 1)
    r_norm = np.linalg.norm(r)
    y[0] = r_norm
    while True:
        Q[0][:] = r / r_norm
        for i in range(1, s + 1):  # the reference's i = 2 .. s + 1
            solvers.mul(Q[i], A, Q[i - 1])
            Pl(Q[i])
            for j in range(i):
                H[j, i - 1] = np.dot(Q[j], Q[i])
                Q[i] -= H[j, i - 1] * Q[j]
            H[i, i - 1] = np.linalg.norm(Q[i])
            if H[i, i - 1] == 0:
                # 05_GMRES.jl:73 passes H[1:(i-1), 1:(i-2)], which drops the column just computed (right only if H[1,1] = 1); the
                # least-squares problem of all i - 1 computed columns is meant, and solved here
                hessenberg(H[:i + 1, :i].copy(), y)
                for j in range(i):
                    x += Q[j] * y[j]
                return it + i
            Q[i] /= H[i, i - 1]
        hessenberg(H, y)
        for i in range(s):
            x += Q[i] * y[i]
        it += s
        solvers.mul(r, A, x, -1.0)
        r += b
        Pl(r)
        if solvers.normalized_norm(r) <= tol or it > maxiter:
            return it
        y[:] = 0.0
        r_norm = np.linalg.norm(r)
        y[0] = r_norm


def test_header_defines_gmres_solver_id():
    src = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    m = re.search(r"MFEM_SOLVER_GMRES\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 4


def test_julia_binding_maps_gmres_to_the_header_id():
    src = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    m = re.search(r"const SOLVER_ID = Dict\(([^)]*)\)", src)
    assert m
    ids = dict((k, int(v)) for k, v in re.findall(r":(\w+!?)\s*=>\s*(\d+)", m.group(1)))
    assert ids["gmres!"] == 4


def test_exact_breakdown_solves_with_all_computed_columns():
    """A = 3 I, b = ones(16): Q1 = 0.25, H[1,1] = 3 and Q2 = 0 exactly -- the breakdown branch returns b / 3 after 2 iterations."""
    import scipy.sparse as sp

    n = 16
    A = sp.csr_matrix(3.0 * np.eye(n))
    b = np.ones(n)
    x = np.zeros(n)
    it = gmres(x, A, b, b.copy(), tol=1e-12, maxiter=100, s=20)
    assert it == 2
    assert np.abs(x - b / 3).max() <= 1e-15


def test_restated_gmres_reproduces_the_2d_stress_concentration_vtk():
    """2D_Script.jl:63 as written (gmres!, s = 20, maxiter 2000, max_pass 20, converge_tol 1e-8, right Jacobi): one Newton step."""
    from oracle import stress_concentration as scn

    z = np.load(os.path.join(GOLD, "stress_concentration_2d.npz"))
    dom = scn.build(z["vert"], z["conn"].astype(np.int64))
    infos = []

    def solve(d):
        info = solvers.SolveInfo()
        dx = solvers.iterative_solve(d.pattern.rowptr, d.pattern.colidx, d.K_total, d.residue, d.converge_tol, Sv_func=gmres,
                                     maxiter=2000, max_pass=20, s=20, info=info)
        infos.append(info)
        return dx

    dom.linear_solver = solve
    hist = dom.update_one_step()
    assert hist[-1] < dom.converge_tol
    assert len(infos) == 1 and infos[0].passes == 1 and infos[0].res < 1e-8
    d, idx = cKDTree(dom.mesh.coords).query(z["xyz"])
    assert d.max() < 1e-7
    n, scale = dom.mesh.ncp, np.abs(z["d2"]).max()
    for f in range(2):
        assert np.abs(dom.x[f * n:(f + 1) * n][idx] - z[f"d{f + 1}"]).max() < 1e-5 * scale
