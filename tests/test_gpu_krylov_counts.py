"""mfem_solve_stats.spmv_count is the number of products that ran, for every solver: the formula of include/metafem_mi355x.h from the
iteration and pass counts, (a) on converged multi-pass solves with the default check_every -- the cycles the host replays after the device has
stopped count nothing -- and (b) on fixed-iteration passes whose maxiter is no multiple of the cycle length.  (c) The cycles a fixed-iteration
pass launches as graphs (mfem_debug_graph_launch_count) stay where they were when the host counted the products: none were added."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# name -> (Sv_func attribute, s, cg_variant, debug knobs)
SOLVERS = {
    "cg1": ("cg_", 0, 1, {}),
    "cg2": ("cg_", 0, 2, {}),
    "cg4": ("cg_", 0, 4, {}),
    "bicgstabl_fused": ("bicgstabl_GS_", 2, 0, {}),
    "bicgstabl_literal": ("bicgstabl_GS_", 2, 0, {"bicgstabl": 1}),
    "idrs_fused": ("idrs_", 8, 0, {}),
    "idrs_literal": ("idrs_", 8, 0, {"idrs": 1}),
    "cgs2": ("cgs2_", 0, 0, {}),
    "gmres": ("gmres_", 20, 0, {}),
    "cgs": ("cgs_", 0, 0, {}),
    "tfqmr": ("tfqmr_", 0, 0, {}),
    "lsqr": ("lsqr_", 0, 0, {}),
}
CHECKITER = 5  # tfqmr!


@contextlib.contextmanager
def _knobs(knobs):
    from metafem_jl_amd import _lib

    try:
        for key, a in knobs.items():
            _lib.check(_lib.lib.mfem_debug_set(key.encode(), int(a), 0))
        yield
    finally:
        for key in knobs:
            _lib.lib.mfem_debug_set(key.encode(), 0, 0)


def _thermal_system(n):
    from oracle import fem, mesh as om, problems, reference_element as re_

    x = (1.0, 1.0, 1.0)
    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, 3)
    msh = om.lattice_mesh(x, n, disc)
    c = msh.coords
    msh.coords = c + 0.02 * np.stack([np.sin(3 * c[:, 1]), np.sin(2 * c[:, 2]), c[:, 0] * c[:, 1]], axis=1)
    fac = om.boundary_facets_structured(x, n, 3)
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, 0.6), [(fac, problems.thermal_convection(25.0, 293.15))])
    od.controlpoints["s"] = np.full(msh.ncp, 1600.0)
    od.update_time(); od.K_linear_func(); od.update_x_star(); od.K_nonlinear_func()
    return od.pattern.rowptr, od.pattern.colidx, od.K_total.copy(), od.residue.copy()


_SYSTEMS = {}


def _system(n):
    if n not in _SYSTEMS:
        _SYSTEMS[n] = _thermal_system(n)
    return _SYSTEMS[n]


def _solve(mf, sysm, name, **kw):
    import torch
    from metafem_jl_amd import _lib

    rowptr, col, K, b = sysm
    sv, s, cg_variant, knobs = SOLVERS[name]
    A = mf.FEM_SpMat_CSR(torch.tensor(rowptr, device="cuda"), torch.tensor(col, device="cuda"), b.size)
    with _knobs(knobs):
        g0 = int(_lib.lib.mfem_debug_graph_launch_count())
        _, st = mf.iterative_Solve(A, torch.tensor(K, device="cuda"), torch.tensor(b, device="cuda"), Sv_func=getattr(mf, sv), s=s,
                                   cg_variant=cg_variant, checkiter=CHECKITER, **kw)
        torch.cuda.synchronize()
        launches = int(_lib.lib.mfem_debug_graph_launch_count()) - g0
    return st, launches


def _cap(name, maxiter):
    """the iteration count a pass returns when maxiter ends it"""
    _, s, _, _ = SOLVERS[name]
    if name in ("cg1", "cg2", "cg4") or name.startswith("idrs"):
        return maxiter
    if name.startswith("bicgstabl"):
        return 1 + s * -(-(maxiter - 1) // s)
    if name == "gmres":
        return 1 + s * -(-maxiter // s)
    return maxiter + 1  # cgs2, cgs, tfqmr, lsqr: iter > maxiter ends the pass


def _pass_products(name, it, maxiter, fixed):
    """products of one pass that returned `it` iterations, start-of-pass residual and the wrapper's residual not included"""
    _, s, _, _ = SOLVERS[name]
    if name == "cg2":
        return 1 + it  # the initial A u runs also when the start has converged
    if it == 0:
        return 0
    if name in ("cg1", "cg4") or name.startswith("idrs"):
        return it
    if name.startswith("bicgstabl") or name in ("cgs2", "cgs"):
        return 2 * (it - 1)
    if name == "gmres":
        assert (it - 1) % s == 0, it  # (no exact breakdown here: every cycle ends with its true residual)
        return (it - 1) + (it - 1) // s
    if name == "tfqmr":
        checks = 0 if fixed else sum(1 for j in range(2, it + 1) if j % CHECKITER == 0 and j <= maxiter)
        return 1 + 2 * (it - 1) + checks
    if name == "lsqr":
        return 1 + 3 * (it - 1)
    raise AssertionError(name)


def _formula(name, its, maxiter, fixed):
    return sum((1 if p > 0 else 0) + _pass_products(name, it, maxiter, fixed) + 1 for p, it in enumerate(its))


# (a): the system and maxiter -- small enough that the first pass does not converge (gmres!(20): a larger system; every pass is one cycle)
CONVERGED = {"bicgstabl_fused": ((7, 6, 5), 10), "bicgstabl_literal": ((7, 6, 5), 10), "gmres": ((12, 12, 12), 12)}


@pytest.mark.parametrize("name", list(SOLVERS))
def test_converged_multi_pass_counts_the_products_that_ran(mf, name):
    """(a) maxiter caps every pass but the last, which converges between two of the host's flag reads"""
    n, maxiter = CONVERGED.get(name, ((7, 6, 5), 12))
    sysm = _system(n)
    b = sysm[3]
    tol = 1e-9 * float(np.sqrt(np.mean(b * b)))
    st, _ = _solve(mf, sysm, name, converge_tol=tol, maxiter=maxiter, max_pass=400)
    assert st.converged == 1 and st.passes >= 2, (name, st.passes, st.iterations)
    cap = _cap(name, maxiter)
    last = st.iterations - (st.passes - 1) * cap
    assert 1 <= last <= cap, (name, st.iterations, st.passes, cap)
    its = [cap] * (st.passes - 1) + [last]
    assert st.spmv_count == _formula(name, its, maxiter, False), (name, st.spmv_count, its)


# maxiter of the fixed passes: no multiple of the cycle (idrs!(8): 9 steps, bicgstabl_GS!(2): 2, gmres!(20): 20; cg!: an odd one ends on a
# direct launch after its captured pairs) -> the graph launches the parent build made for them
FIXED = {
    "cg1": (31, 15), "cg2": (31, 31), "cg4": (31, 15),
    "bicgstabl_fused": (31, 14), "bicgstabl_literal": (31, 15),  # (the fused form's first sweep is launched directly)
    "idrs_fused": (200, 23), "idrs_literal": (200, 23),
    "cgs2": (31, 31), "gmres": (30, 2), "cgs": (31, 31), "tfqmr": (31, 31), "lsqr": (31, 31),
}


@pytest.mark.parametrize("name", list(SOLVERS))
def test_fixed_pass_counts_and_launches(mf, name):
    """(b) spmv_count of a fixed-iteration pass is exact; (c) it launches as many captured cycles as before"""
    maxiter, launches_before = FIXED[name]
    st, launches = _solve(mf, _system((12, 12, 12)), name, converge_tol=1e-300, maxiter=maxiter, max_pass=1, fixed_iterations=True)
    cap = _cap(name, maxiter)
    assert st.passes == 1 and st.iterations == cap, (name, st.iterations, cap)
    assert st.spmv_count == _formula(name, [cap], maxiter, True), (name, st.spmv_count)
    assert launches == launches_before, (name, launches)
