"""GPU parity of cgs!, tfqmr! and lsqr! (07_CGS.jl:13-52, 08_QMR.jl:3-74, 06_LSQR.jl:10-70) through iterative_Solve! and of tmul!
(04_GPU_Utils.jl:132, mfem_spmv_csr_t).  The device solvers are compared iterate by iterate with the numpy restatements of
tests/test_krylov_next_cpu.py under the unchanged oracle.solvers.iterative_solve (converge_tol = 1e-300, one pass of k iterations):
delta_x to 1e-10 relative, the iteration count exactly, and spmv_count against the formula of include/metafem_mi355x.h.  For one pass
from x0 = 0 that formula equals the restatement's product count: the device skips the first residual product (r = b) and adds the
wrapper's true residual after the pass."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
# max |x - x_restated| / max |x_restated|: the bar of tests/test_gpu_krylov_scale.py -- or, where the system itself is more sensitive than that,
# 10 x the spread of the restatement's own iterate when K is perturbed by one ulp (_spread).  The Nitsche matrices are: measured on the host,
# a 1-ulp perturbation moves cgs!'s 17th iterate on the quad-8 Nitsche system with right Jacobi by 9e-8 (tfqmr! 1.8e-9, lsqr! 1.0e-10), and
# cgs! with Jacobi-colnorm and left Jacobi by 8.7e-10 after three steps; no implementation can agree better than that.
TOL_X = 1e-10


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("_krylov_next_restated", "test_krylov_next_cpu.py")
REF = {"cgs": cpu.cgs, "tfqmr": cpu.tfqmr, "lsqr": cpu.lsqr}
_SYS = {}


def _system(name):
    if name not in _SYS:
        _SYS[name] = {"thermal": cpu.thermal_system, "nitsche": cpu.nitsche_system, "random": cpu.random_system}[name]()
    return _SYS[name]


def _sv(mf, solver):
    return {"cgs": mf.cgs_, "tfqmr": mf.tfqmr_, "lsqr": mf.lsqr_}[solver]


def _pattern(mf, rowptr, col, n, index_base=0, rowptr64=False, ctx=None):
    import torch

    rp = torch.tensor(np.asarray(rowptr) + index_base, dtype=torch.int64 if rowptr64 else torch.int32, device="cuda")
    ci = torch.tensor(np.asarray(col) + index_base, dtype=torch.int32, device="cuda")
    return mf.FEM_SpMat_CSR(rp, ci, n, index_base=index_base, ctx=ctx)


PR = {"identity": (0, None), "diag": (1, "diag"), "colnorm": (2, "colnorm")}
PL = {"none": (0, None), "diag": (1, "diag"), "rownorm": (2, "rownorm")}


def _oracle_pr(kind):
    from oracle import solvers

    return {None: None, "diag": solvers.pr_jacobi, "colnorm": lambda A: solvers.pr_jacobi(A, True)}[kind]


def _oracle_pl(kind):
    from oracle import solvers

    return {None: None, "diag": solvers.pl_jacobi, "rownorm": lambda A: solvers.pl_jacobi(A, True)}[kind]


def _restated(sysm, solver, k, pr="diag", pl="none", **kw):
    from oracle import solvers

    rowptr, col, K, b = sysm
    products, info = [0], solvers.SolveInfo()
    x = solvers.iterative_solve(rowptr, col, K, b, 1e-300, Sv_func=REF[solver], Pr_func=_oracle_pr(PR[pr][1]), Pl_func=_oracle_pl(PL[pl][1]),
                                maxiter=k, max_pass=1, info=info, products=products, **kw)
    return x, info.iters, products[0]


def _device(mf, A, K, b, solver, k, pr="diag", pl="none", **kw):
    import torch

    dx, st = mf.iterative_Solve(A, torch.as_tensor(K, device="cuda"), torch.as_tensor(b, device="cuda"), 1e-300, Sv_func=_sv(mf, solver),
                                Pr_func=PR[pr][0], Pl_func=PL[pl][0], maxiter=k, max_pass=1, **kw)
    return dx.cpu().numpy(), st


def _spread(sysm, solver, k, pr, pl, xo, **kw):
    """max relative change of the restatement's iterate when every entry of K is perturbed by about one ulp (two draws)."""
    rowptr, col, K, b = sysm
    rng = np.random.default_rng(0x5EED)
    worst = 0.0
    for _ in range(2):
        Kp = K * (1.0 + 1.1e-16 * rng.standard_normal(K.size))
        xp, _, _ = _restated((rowptr, col, Kp, b), solver, k, pr, pl, **kw)
        worst = max(worst, np.abs(xp - xo).max() / np.abs(xo).max())
    return worst


def _compare(mf, sysm, solver, k, A=None, pr="diag", pl="none", extra_products=0, **kw):
    rowptr, col, K, b = sysm
    A = A if A is not None else _pattern(mf, rowptr, col, b.size)
    xo, it, products = _restated(sysm, solver, k, pr, pl, **kw)
    x, st = _device(mf, A, K, b, solver, k, pr, pl, **kw)
    err = np.abs(x - xo).max() / np.abs(xo).max()
    if err > TOL_X:
        spread = _spread(sysm, solver, k, pr, pl, xo, **kw)
        assert err <= 10 * spread, (solver, k, pr, pl, err, spread)
    assert st.iterations == it and st.passes == 1
    assert st.spmv_count == products + extra_products, (st.spmv_count, products, extra_products)
    return x, st


@pytest.mark.parametrize("k", [1, 2, 3, 17])
@pytest.mark.parametrize("solver", ["cgs", "tfqmr", "lsqr"])
@pytest.mark.parametrize("system", ["thermal", "nitsche"])
def test_iterates_match_restatement(mf, system, solver, k):
    _compare(mf, _system(system), solver, k, checkiter=5)


@pytest.mark.parametrize("k,checkiter", [(199, 200), (200, 200), (201, 200), (4, 5), (5, 5), (6, 5), (17, 5), (10, 1)])
def test_tfqmr_checkiter(mf, k, checkiter):
    """iter % checkiter == 0 computes the true residual; iter > maxiter ends the pass without one (08_QMR.jl:65-72).  Identity right
    preconditioner on the 12 x 10 x 8 thermal brick: slow enough that 201 steps stay far above round-off."""
    sysm = _system("thermal_big") if "thermal_big" in _SYS else _SYS.setdefault("thermal_big", cpu.thermal_system((12, 10, 8)))
    _compare(mf, sysm, "tfqmr", k, pr="identity", checkiter=checkiter)


@pytest.mark.parametrize("pl", ["none", "diag", "rownorm"])
@pytest.mark.parametrize("pr", ["identity", "diag", "colnorm"])
@pytest.mark.parametrize("solver", ["cgs", "tfqmr", "lsqr"])
def test_preconditioner_grid(mf, solver, pr, pl):
    """Right Identity / Jacobi-diag / Jacobi-colnorm x left none / diag / rownorm on the nonsymmetric Nitsche matrix.  lsqr!'s A' is
    P A_r' (row i scaled by p_i c_i), not (P A_r)': this grid fails if the transposed values are scaled by p_j."""
    _compare(mf, _system("nitsche"), solver, 17, pr=pr, pl=pl, checkiter=5)


@pytest.fixture()
def knobs():
    from metafem_jl_amd import _lib

    defaults = {"layout_min_rows": (262144, 1000000), "ell": (1, 0), "sell": (1, 0), "lat8": (1, 0), "lat27": (1, 0), "remainder": (1, 0),
                "graphs": (1, 4000000)}
    used = []

    def set_(**kw):
        for key, ab in kw.items():
            a, b = ab if isinstance(ab, tuple) else (ab, 0)
            _lib.check(_lib.lib.mfem_debug_set(key.encode(), int(a), int(b)))
            used.append(key)

    yield set_
    for key in used:
        _lib.lib.mfem_debug_set(key.encode(), *defaults[key])


def _layout_mode(mf, A):
    from metafem_jl_amd import _lib

    mode, slots, pad, reg = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib.mfem_csr_solver_layout(A.ctx._h, A._h, C.byref(mode), C.byref(slots), C.byref(pad), C.byref(reg)))
    return mode.value


def _brick_system(mf, nitsche=False, dims=(10, 9, 8)):
    b = mf.make_Brick((1.0, 0.7, 1.3), dims, 1, 3)
    A = b.pattern(1)
    x0 = mf.FACE_BITS["x0"]
    if nitsche:
        K = b.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F & ~x0, fixed_faces=x0, h_penalty=1000.0, Tw=1173.15)
    else:
        K = b.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F)
    rhs = (mf.FEM_rand(A.n, 11, 0) - 0.5).cpu().numpy()
    sysm = (A.rowptr.cpu().numpy().astype(np.int64), A.colidx.cpu().numpy(), K.cpu().numpy(), rhs)
    return b, A, sysm


@pytest.mark.parametrize("layout", ["mode2", "mode5", "mode5_remainder", "mode3_caller_base1", "mode0_rowptr64"])
@pytest.mark.parametrize("solver", ["cgs", "tfqmr", "lsqr"])
def test_solver_layouts(mf, knobs, layout, solver):
    """The forward products on the solver layouts (forced with the knobs of tests/test_gpu_krylov_scale.py), the transposed one on the
    CSR kernel: mode 2 (diagonal-slotted copy, the fused right scaling), mode 5 (symmetric lattice tiles: the right scaling applied to
    x), the tiles with the skew remainder of a Nitsche brick, mode 3 on a caller-supplied CSR with index_base = 1, and the CSR kernel on
    a 64-bit rowptr handle."""
    from metafem_jl_amd import _lib

    knobs(layout_min_rows=(0, 0))
    keep = None
    if layout in ("mode2", "mode5", "mode5_remainder"):
        if layout == "mode2":  # (the slot-major copy wants <= 10 % padding: rows of 27 entries dominate from about 32 elements per edge)
            knobs(lat8=0)
        keep, A, sysm = _brick_system(mf, nitsche=layout == "mode5_remainder", dims=(40, 40, 40) if layout == "mode2" else (10, 9, 8))
    elif layout == "mode3_caller_base1":
        knobs(ell=0)
        sysm = _system("nitsche")
        A = _pattern(mf, sysm[0], sysm[1], sysm[3].size, index_base=1)
    else:
        knobs(layout_min_rows=(262144, 1000000))
        sysm = _system("nitsche")
        A = _pattern(mf, sysm[0], sysm[1], sysm[3].size, rowptr64=True)
    c8, cr = int(_lib.lib.mfem_debug_lat8_spmv_count()), int(_lib.lib.mfem_debug_rem_spmv_count())
    for k in (3, 17):  # (the tiles' solve recomputes the residual it reports from the caller's CSR values: one product more, krylov.hip)
        _compare(mf, sysm, solver, k, A=A, checkiter=5, extra_products=1 if layout.startswith("mode5") else 0)
    mode = _layout_mode(mf, A)
    used8, usedr = int(_lib.lib.mfem_debug_lat8_spmv_count()) > c8, int(_lib.lib.mfem_debug_rem_spmv_count()) > cr
    if layout == "mode2":
        assert mode == 2 and not used8
    elif layout.startswith("mode5"):
        assert used8
        assert usedr == (layout == "mode5_remainder")
    elif layout == "mode3_caller_base1":
        assert mode == 3
    else:
        assert mode == 0
    del keep


@pytest.mark.parametrize("solver", ["cgs", "tfqmr", "lsqr"])
def test_graphs_bitwise_and_repeatable(mf, knobs, solver):
    """Graph replay equals direct launches bit for bit; two identical solves are identical (the CSR kernel and the transposed gather
    have a fixed summation order)."""
    sysm = _system("nitsche")
    rowptr, col, K, b = sysm
    A = _pattern(mf, rowptr, col, b.size)
    kw = dict(pl="diag", checkiter=5)
    x1, s1 = _device(mf, A, K, b, solver, 40, **kw)
    x2, s2 = _device(mf, A, K, b, solver, 40, **kw)
    knobs(graphs=(1, 1))
    x3, s3 = _device(mf, A, K, b, solver, 40, **kw)
    assert np.array_equal(x1, x2) and np.array_equal(x1, x3)
    assert s1.iterations == s2.iterations == s3.iterations and s1.spmv_count == s2.spmv_count == s3.spmv_count


def test_lsqr_beta_zero_branch_on_device(mf):
    """A = 3 I, b = ones(16): the first step's u is exactly 0, beta == 0 skips A' u on the device (no host round trip)."""
    import torch

    n = 16
    A = _pattern(mf, np.arange(n + 1), np.arange(n), n)
    dx, st = mf.iterative_Solve(A, torch.full((n,), 3.0, dtype=torch.float64, device="cuda"), torch.ones(n, dtype=torch.float64, device="cuda"),
                                1e-300, Sv_func=mf.lsqr_, Pr_func=mf.Identity, maxiter=1, max_pass=1)
    assert st.iterations == 2
    assert st.spmv_count == 1 + 2 + 1  # A' u ; A v and the true residual (no A' u) ; the wrapper's residual
    assert np.abs(dx.cpu().numpy() - 1.0 / 3.0).max() <= 1e-15


# -- tmul! -----------------------------------------------------------------------------------------------------------------------------
def _tmul_check(mf, A, vals_h, M, ncols, repeat=True):
    import torch

    rng = np.random.default_rng(3)
    xh, y0 = rng.standard_normal(A.n), rng.standard_normal(ncols)
    vals, x = torch.tensor(vals_h, device="cuda"), torch.tensor(xh, device="cuda")
    ref = M.T @ xh
    y = torch.zeros(ncols, dtype=torch.float64, device="cuda")
    mf.tmul_(y, A, vals, x)
    got = y.cpu().numpy()
    scale = np.maximum(np.abs(M).T @ np.abs(xh), np.finfo(float).tiny)
    assert (np.abs(got - ref) / scale).max() <= 1e-14
    yb = torch.tensor(y0, device="cuda")
    mf.tmul_(yb, A, vals, x, 2.0, -0.5)
    assert np.abs(yb.cpu().numpy() - (2.0 * ref - 0.5 * y0)).max() <= 1e-14 * (2.0 * scale + 0.5 * np.abs(y0)).max()
    if repeat:
        y2 = torch.zeros(ncols, dtype=torch.float64, device="cuda")
        for _ in range(3):
            mf.tmul_(y2, A, vals, x)
            assert np.array_equal(y2.cpu().numpy(), got)
    return got


def _tplan(A):
    from metafem_jl_amd import _lib

    b, ms = C.c_int64(), C.c_double()
    on = _lib.lib.mfem_debug_csr_tplan(A._h, C.byref(b), C.byref(ms))
    return on, b.value


def test_tmul_fem_pattern_and_replan(mf):
    rowptr, col, K, b = _system("nitsche")
    A = _pattern(mf, rowptr, col, b.size)
    assert _tplan(A) == (0, 0)  # nothing planned before the first product
    M = sp.csr_matrix((K, col, rowptr), shape=(b.size, b.size))
    got = _tmul_check(mf, A, K, M, b.size)
    on, nbytes = _tplan(A)
    assert on == 1 and nbytes == 8 * (b.size + 1) + 8 * K.size
    A.replan()
    assert _tplan(A) == (0, 0)
    assert np.array_equal(_tmul_check(mf, A, K, M, b.size, repeat=False), got)
    assert _tplan(A)[0] == 1


@pytest.mark.parametrize("base,rowptr64", [(0, False), (1, False), (0, True), (1, True)])
def test_tmul_random_nonsymmetric_unsorted(mf, base, rowptr64):
    """Structurally nonsymmetric pattern, columns of every row shuffled, empty rows and columns."""
    rng = np.random.default_rng(11)
    n = 997
    M = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    M = sp.csr_matrix(M.multiply(sp.csr_matrix((rng.random(n) > 0.05).astype(float)[:, None])))  # some empty rows
    rowptr, col, vals = M.indptr.copy(), M.indices.copy(), M.data.copy()
    for r in range(n):
        sl = slice(rowptr[r], rowptr[r + 1])
        p = rng.permutation(rowptr[r + 1] - rowptr[r])
        col[sl], vals[sl] = col[sl][p], vals[sl][p]
    assert (M != M.T).nnz > 0
    A = _pattern(mf, rowptr, col, n, index_base=base, rowptr64=rowptr64)
    _tmul_check(mf, A, vals, sp.csr_matrix((vals, col, rowptr), shape=(n, n)), n)


def test_tmul_slab_pattern_with_ghost_columns(mf):
    """A slab of a brick: ncols = owned + ghost entries > n, y = A' x has ncols entries."""
    brick = mf.make_Brick((2.0, 1.0, 1.5), (11, 6, 5))
    brick.set_slab(3, 8)
    A = brick.pattern(1)
    ncols = A.ncols
    assert ncols > A.n
    K = brick.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F).cpu().numpy()
    rp, ci = A.rowptr.cpu().numpy().astype(np.int64), A.colidx.cpu().numpy()
    _tmul_check(mf, A, K, sp.csr_matrix((K, ci, rp), shape=(A.n, ncols)), ncols)


# -- the reference's examples ----------------------------------------------------------------------------------------------------------
def _cavity_system(mf):
    import torch

    import test_gpu_generic as tg
    from oracle import cavity, solvers

    od = cavity.build_cavity(40, Cb=8.0)
    gd = tg._gpu_domain(mf, od, "Serendipity", 2, 5)
    n = od.mesh.ncp
    od.controlpoints["u1"], od.controlpoints["u2"] = np.zeros(n), np.zeros(n)
    cavity.set_step_parameters(od, 0.1)
    for key in ("uw1", "uw2", "taum", "tauc"):
        gd.controlpoints[key] = torch.tensor(od.controlpoints[key], device="cuda")
    gd.K_linear_func(); gd.x_star.zero_(); gd.K_nonlinear_func()
    sysm = (gd.A.rowptr.cpu().numpy(), gd.A.colidx.cpu().numpy(), gd.K_total.cpu().numpy(), gd.residue.cpu().numpy())
    return gd, sysm, solvers.solver_lu_cpu(*sysm)


class _NonFinite(Exception):
    pass


def _restated_converges(sysm, solver, tol, **kw):
    """Does the restatement converge under these limits?  A pass that leaves x non-finite ends the question: normalized_norm(r) <= tol
    can never hold again (the reference carries the NaN through every later pass)."""
    from oracle import solvers

    def body(x, *a, **k):
        try:
            it = REF[solver](x, *a, **k)
        except ZeroDivisionError:  # (a Python float division by zero: Julia's Float64 gives inf / nan there)
            raise _NonFinite
        if not np.all(np.isfinite(x)):
            raise _NonFinite
        return it

    info = solvers.SolveInfo()
    try:
        solvers.iterative_solve(*sysm, tol, Sv_func=body, info=info, **kw)
    except _NonFinite:
        return False
    return info.res < tol


@pytest.mark.parametrize("solver", ["cgs", "tfqmr"])
def test_cavity_step(mf, solver):
    """The lid-driven cavity step of tools/cavity_solvers.py under 2D_Script.jl's limits (maxiter 10000, max_pass 20).  Converged, it is
    the LU answer: the velocities, and the pressure up to the constant the walls leave free.  Neither solver converges within the first
    pass, on the device or in the restatement; what the later passes do is decided by round-off (seen on one MI355X: both converged in the
    second pass right at the tolerance, 8.9e-9 and 1.8e-9, in one process, and ran into a breakdown, nan, in another -- so does the
    restatement, depending on the assembly's last bits), so only the first pass is compared when the script's solve fails."""
    import sys

    sys.path.insert(0, HERE)
    gd, sysm, ref = _cavity_system(mf)
    tol = 1e-8
    dx, st = mf.iterative_Solve(gd.A, gd.K_total, gd.residue, tol, Sv_func=_sv(mf, solver), maxiter=10000, max_pass=20)
    print(f"cavity {solver}: converged {st.converged}, {st.passes} passes, {st.iterations} iterations, final_res {st.final_res:.3e}")
    if not st.converged:
        _, st1 = mf.iterative_Solve(gd.A, gd.K_total, gd.residue, tol, Sv_func=_sv(mf, solver), maxiter=10000, max_pass=1)
        assert not st1.converged and st1.iterations == 10001
        assert not _restated_converges(sysm, solver, tol, maxiter=10000, max_pass=1), solver
        return
    x, n = dx.cpu().numpy(), sysm[3].size // 3
    uref = ref[n:]
    assert np.abs(x[n:] - uref).max() <= 1e-5 * np.abs(uref).max()
    p, pref = x[:n] - x[:n].mean(), ref[:n] - ref[:n].mean()
    assert np.abs(p - pref).max() <= 1e-5 * np.abs(pref).max()


def _stress_domain(mf, dim):
    import torch

    gg = _load("_gmres_gpu", "test_gpu_gmres.py")
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
        bnd.append((f.element_ID, f.element_eindex, gg._wf(scn.penalty_component(d, tau))))
    f = fac.select(np.abs(c[:, 1] - L) < err)
    bnd.append((f.element_ID, f.element_eindex, gg._wf(traction_field(dim, "sl", rows=[1]))))
    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, dim, gg._wf(problems.elasticity_domain(dim, lam, mu)), bnd)
    for v in {2: (2, 3), 3: (2, 4, 6)}[dim]:
        gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device="cuda")
    gd.converge_tol = 1e-8
    return gd, msh, z


@pytest.mark.parametrize("solver", ["tfqmr", "lsqr"])
def test_stress_concentration_2d(mf, solver):
    """2D_Script.jl with its gmres! line swapped for tfqmr! / lsqr! (maxiter 2000, max_pass 20, converge_tol 1e-8): the committed result."""
    gd, msh, z = _stress_domain(mf, 2)
    stats, systems = [], []

    def solve(g):
        systems.append((g.A.rowptr.cpu().numpy(), g.A.colidx.cpu().numpy(), g.K_total.cpu().numpy(), g.residue.cpu().numpy()))
        dx, st = mf.iterative_Solve(g.A, g.K_total, g.residue, g.converge_tol, Sv_func=_sv(mf, solver), maxiter=2000, max_pass=20)
        stats.append(st)
        return dx

    gd.linear_solver = solve
    hist = gd.update_OneStep()
    print(f"stress 2D {solver}: " + "; ".join(f"converged {s.converged}, {s.passes} passes, {s.iterations} iterations, final_res {s.final_res:.3e}"
                                              for s in stats))
    if not all(s.converged for s in stats):  # not under the script's limits: neither does the restatement
        assert not stats[0].converged and not _restated_converges(systems[0], solver, gd.converge_tol, maxiter=2000, max_pass=20)
        return
    assert hist[-1] < gd.converge_tol
    got = gd.x.cpu().numpy()
    d, idx = cKDTree(msh.coords).query(z["xyz"])
    assert d.max() < 1e-7
    n, scale = msh.ncp, np.abs(z["d2"]).max()
    for fld in range(2):
        assert np.abs(got[fld * n:(fld + 1) * n][idx] - z[f"d{fld + 1}"]).max() < 1e-5 * scale


# -- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(mf):
    """A communicator attached: cgs!, tfqmr! and lsqr! return MFEM_ERR_INVALID before any collective.  Method 8 is unknown."""
    import torch
    from metafem_jl_amd import _lib

    rowptr, col, K, b = _system("thermal")
    ctx = mf.Context(0)
    A = _pattern(mf, rowptr, col, b.size, ctx=ctx)
    Kt, bt, x = (torch.tensor(v, device="cuda") for v in (K, b, np.zeros(b.size)))
    st = _lib.SolveStats()

    def solve(method):
        o = _lib.SolveOptions(method=method, precond=1, l_or_s=0, maxiter=10, max_pass=1, check_every=32, converge_tol=1e-8, seed=1)
        return _lib.lib.mfem_solve(ctx._h, A._h, Kt.data_ptr(), bt.data_ptr(), x.data_ptr(), C.byref(o), C.byref(st))

    assert solve(8) == -1
    for m in (mf.cgs_, mf.tfqmr_, mf.lsqr_):
        assert solve(m) == 0
    ops = _lib.CommHostOps(None, _lib.ALLREDUCE_CB(lambda *a: 1), _lib.EXCHANGE_CB(lambda *a: 1), 0, 0)
    h = C.c_void_p()
    _lib.check(_lib.lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(h)))
    try:
        _lib.check(_lib.lib.mfem_context_set_comm(ctx._h, h, b.size, 1, 1))
        for m in (mf.cgs_, mf.tfqmr_, mf.lsqr_):
            assert solve(m) == -1
            assert b"one rank only" in _lib.lib.mfem_last_error()
    finally:
        _lib.lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        _lib.lib.mfem_comm_destroy(h)
