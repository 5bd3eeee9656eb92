"""Variable terms of the matrix-free mesh operator (mfem_mesh_operator_set_variable_terms, MeshOperator.set_variable_terms,
GenericDomain(matrix_free="any")): nonlinear and variable-coefficient weak forms without a matrix, against the assembled K_total of the default
domain (CSR kernel) and the oracle's term-by-term K_total, on the curved, element-shuffled meshes of tests/test_gpu_mesh_operator.py (restated here,
data only; 18 elements and 4 waves per workgroup leave a tail wave without an item; itg = 9, 27 and the simplex rule wrap the lane <-> (dual word, q)
mapping unevenly).  Product, diagonal, in-place coefficient update, removal of the variable terms, bitwise reproducibility with cycle graphs on and
off, Newton runs, memory, refusals, and the opt-in boundary.
Measured on one MI355X: product against the CSR kernel on K_total 1.9e-16 .. 4.5e-16 (bound 1e-12), against the oracle 1.9e-16 .. 4.6e-15 (bound 1e-11),
diagonal 2.7e-16 .. 5.9e-16 (bound 1e-12); min det F 0.979 (hex-20) / 0.976 (tet-10); memory rise 19.1 kB against 72.6 kB per element."""
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
INVALID, UNSUPPORTED = -1, -3


def _wf(wf):
    from metafem_jl_amd import generic as G

    return G.WeakForm(inner_vars=list(wf.inner_vars), cp_ext_vars=list(wf.cp_ext_vars), normals=list(wf.normals),
                      residues=[G.ResTerm(r.dual_pos, r.dual_s, r.fn) for r in wf.residues],
                      linear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.linear_gradients],
                      nonlinear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.nonlinear_gradients])


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


def _smooth(coords, nf):
    """u_i = 0.05 sin(2.3 x_j + 1.1 x_k + 0.4 i): a displacement whose det F stays well above 0."""
    dim = coords.shape[1]
    return np.concatenate([0.05 * np.sin(2.3 * coords[:, (i + 1) % dim] + 1.1 * coords[:, (i + 2) % dim] + 0.4 * i) for i in range(nf)])


def _conductivity_form():
    """Thermal conduction whose conductivity is the nodal external kx: -Bilinear(T{;i}, kx T{;i}) + Bilinear(T, s + 0.7 (300 - T)) -- linear gradients
    with a variable coefficient beside a constant one on the same part."""
    from metafem_jl_amd import generic as G

    wf = G.WeakForm(inner_vars=[("T", 0, 0, 0)], cp_ext_vars=[("kx", "kx", 0), ("s", "s", 0)])
    for d in range(3):
        wf.inner_vars.append((f"T_{d}", 0, 1 + d, 0))
        wf.residues.append(G.ResTerm(0, 1 + d, lambda env, d=d: -env["kx"] * env[f"T_{d}"]))
        wf.linear_gradients.append(G.GradTerm(0, 1 + d, 0, 1 + d, lambda env: -env["kx"]))
    wf.residues.append(G.ResTerm(0, 0, lambda env: env["s"] + 0.7 * (300.0 - env["T"])))
    wf.linear_gradients.append(G.GradTerm(0, 0, 0, 0, lambda env: -0.7))
    return wf


def _case(name, msh, fac, rng):
    """-> (n_fields, domain form, [(facets, form)], max_time_level, nodal externals {symbol: array}, x_star)"""
    from metafem_jl_amd import physics as P
    from oracle import hyperelastic as he, problems

    dim, ncp = msh.coords.shape[1], msh.ncp
    c = fac.centroid
    x0, y1 = fac.select(np.abs(c[:, 0]) < 1e-9), fac.select(np.abs(c[:, 1] - 0.8) < 1e-9)
    U = lambda lo, hi: rng.uniform(lo, hi, ncp)
    if name == "neo_hookean":  # 81 variable terms on the elements; a constant penalty wall; traction facets (no gradient: no part)
        sl = {f"sl{v}": U(-0.05, 0.05) for v in (1, 2, 3, 4, 5, 6)}
        return (3, _wf(he.domain_weakform(dict(mu=1.0, lam=1.5), "neo_hookean")), [(x0, P.penalty([0, 1, 2], 37.0)), (y1, P.traction(3, "sl"))], 0, sl,
                _smooth(msh.coords, 3))
    if name == "cavity":  # p, u1, u2: nonsymmetric, externals inside nonlinear expressions, Nitsche walls
        wd, wfix, wtop = problems.cavity_weakforms(1.0, 1.0, 100.0)
        rest = fac.select(np.abs(c[:, 1] - 0.8) >= 1e-9)
        ext = {"taum": U(0.005, 0.015), "tauc": U(0.005, 0.015), "uw1": U(0.5, 1.5), "uw2": U(-0.1, 0.1)}
        return 3, _wf(wd), [(rest, _wf(wfix)), (y1, _wf(wtop))], 0, ext, 0.05 * rng.uniform(-1.0, 1.0, 3 * ncp)
    if name == "cavity_newton":
        # The closed cavity fixes p up to a constant, and on the warped mesh the lid's velocity has a net flux through the curved top edge: the steady
        # system is singular AND inconsistent (measured on the oracle: sigma_min / sigma_2 = 1e-12, Newton with LU stalls at 1e-2).  A pressure mass
        # term eps Bilinear(p, p), of the sign of the PSPG block, makes the problem well-posed (cond 1e4; the oracle's Newton with LU and with
        # cgs2! reaches 4e-16 in three iterations) and adds a constant term beside the 32 variable ones of the element part.
        from metafem_jl_amd import generic as G

        dx, u_top, eps = 1.0 / 6, 1.0, 1.0
        wd, wfix, wtop = problems.cavity_weakforms(1.0, 1.0, 8.0 / dx)
        wd = _wf(wd)
        wd.inner_vars.append(("p_reg", 0, 0, 0))
        wd.residues.append(G.ResTerm(0, 0, lambda env: eps * env["p_reg"]))
        wd.linear_gradients.append(G.GradTerm(0, 0, 0, 0, lambda env: eps))
        rest = fac.select(np.abs(c[:, 1] - 0.8) >= 1e-9)
        taum = (4 / (0.2 * dx / u_top) ** 2 + 9 * 16 * 2 * dx ** (-4)) ** (-0.5)  # (2D_Script.jl:122-127 at rest, nu = 1)
        ext = {"taum": np.full(ncp, taum), "tauc": np.full(ncp, 1.0 / (taum * 2 / dx ** 2)), "uw1": np.full(ncp, u_top), "uw2": np.zeros(ncp)}
        return 3, wd, [(rest, _wf(wfix)), (y1, _wf(wtop))], 0, ext, np.zeros(3 * ncp)
    if name == "radiation":  # constant terms on the elements, one variable term on the facets only (beside the constant -h)
        return (1, P.thermal_domain(dim, 0.6, alpha=0.7, Tenv=300.0), [(fac, P.thermal_convection(25.0, 293.15, em=0.8, sigma_b=5.67e-8))], 0,
                {"s": U(800.0, 2400.0)}, 300.0 + 50.0 * rng.uniform(-1.0, 1.0, ncp))
    if name == "conductivity":  # a variable LINEAR gradient
        return 1, _conductivity_form(), [(fac, P.thermal_convection(25.0, 293.15))], 0, {"s": U(800.0, 2400.0), "kx": U(0.4, 0.9)}, U(250.0, 350.0)
    if name == "transient_radiation":  # max_time_level = 1: K_params in the coefficients
        xs = np.concatenate([300.0 + 50.0 * rng.uniform(-1.0, 1.0, ncp), rng.uniform(-1.0, 1.0, ncp)])
        return (1, P.thermal_domain(dim, 0.6, C=4.0), [(fac, P.thermal_convection(25.0, 293.15, em=0.8, sigma_b=5.67e-8))], 1, {"s": U(800.0, 2400.0)},
                xs)
    raise KeyError(name)


CASES = [("hex20", "neo_hookean"), ("tet10", "neo_hookean"), ("quad8", "cavity"), ("hex8", "radiation"), ("hex27", "conductivity"),
         ("hex8", "transient_radiation")]
IDS = [f"{a}-{b}" for a, b in CASES]
_BUILT = {}


class _Sys:
    pass


def _domain(mf, space, msh, nf, wf, bnd, mtl, ext, ctx=None, **kw):
    import torch
    from metafem_jl_amd import generic as G

    gd = G.GenericDomain(ctx or mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf, [(f.element_ID, f.element_eindex, w) for f, w in bnd],
                         max_time_level=mtl, **kw)
    for k, v in ext.items():
        gd.controlpoints[k] = torch.tensor(v, device="cuda")
    return gd


def _min_det_F(od, xs):
    """min over all Gauss points of det(1 + grad u), the words evaluated by the oracle on the CPU."""
    from oracle import operators as ops

    ids = np.arange(od.mesh.nel)
    F = np.empty((3, 3) + od.elgeo.integral_weights.shape)
    for i in range(3):
        for j in range(3):
            F[i, j] = ops.var_basic(od.elgeo.integral_vals, 1 + j, i * od.mesh.ncp, od.mesh.cp_ids, xs, ids, ids) + (1.0 if i == j else 0.0)
    return float(np.linalg.det(np.moveaxis(F, (0, 1), (-2, -1))).min())


def _built(mf, fam, name):
    """The matrix_free="any" domain, the default domain and the oracle of one case at one state (dt = 0.1), K_linear_func and K_nonlinear_func run on
    all three; built once and shared."""
    key = (fam, name)
    if key in _BUILT:
        return _BUILT[key]
    import torch
    from oracle import fem, solvers

    space, msh, fac, disc, omesh = _mesh(fam)
    nf, wf, bnd, mtl, ext, xs = _case(name, msh, fac, np.random.default_rng(3))
    S = _Sys()
    S.xs = xs
    od = fem.FEMDomain(omesh, disc, nf, wf, list(bnd), max_time_level=mtl)
    if name == "neo_hookean":  # before anything else: the state is admissible
        dmin = _min_det_F(od, xs)
        print(f"{fam}-{name}: min det F = {dmin:.3f}")
        assert dmin > 0.5
    for k, v in ext.items():
        od.controlpoints[k] = v
    od.dt = DT
    od.update_time()
    od.K_linear_func()
    od.x_star[:] = xs
    od.K_nonlinear_func()
    doms = []
    for kw in (dict(matrix_free="any"), dict()):
        gd = _domain(mf, space, msh, nf, wf, bnd, mtl, ext, **kw)
        gd.dt = DT
        gd.update_Time()
        gd.x_star.copy_(torch.tensor(xs))
        gd.K_linear_func()
        gd.K_nonlinear_func()
        doms.append(gd)
    S.md, S.gd = doms
    assert S.md.matrix_free is True and S.md.matrix_free_reason is None, S.md.matrix_free_reason
    assert isinstance(S.md.A, mf.MeshOperator) and S.md.K_linear is None and S.md.K_total is None and S.md.slots is None and S.md.table_bytes == 0
    S.n = S.gd.A.n
    S.Ko = solvers.csr(od.pattern.rowptr, od.pattern.colidx, od.K_total.copy(), od.pattern.n)
    S.Kg = solvers.csr(S.gd.A.rowptr.cpu().numpy(), S.gd.A.colidx.cpu().numpy(), S.gd.K_total.cpu().numpy(), S.n)
    S.ro = od.residue.copy()
    rng = np.random.default_rng(7)
    S.x = rng.uniform(-1.0, 1.0, S.n)
    S.b = rng.uniform(-1.0, 1.0, S.n)
    S.dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    S.case = (space, msh, fac, nf, wf, bnd, mtl, ext)
    _BUILT[key] = S
    return S


# ---- 1. product and diagonal ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,name", CASES, ids=IDS)
def test_product_equals_the_assembled_K_total_and_the_oracle(mf, fam, name):
    import torch

    S = _built(mf, fam, name)
    nvar = [0 if b is None else b.shape[0] for b in S.md._var_buf]
    if name == "neo_hookean":
        assert nvar[0] == 81 and sum(nvar[1:]) == 0
    if name in ("radiation", "transient_radiation"):
        assert nvar == [0, 1]
    if name == "conductivity":
        assert nvar == [3, 0]
    if name == "cavity":  # (4 variable linear + 28 nonlinear gradients on the elements; the walls' gradients are constant plus normal-linear)
        assert nvar == [32, 0, 0]
    res = S.md.residue.cpu().numpy()
    assert np.abs(res - S.gd.residue.cpu().numpy()).max() <= 1e-12 * np.abs(res).max()
    assert np.abs(res - S.ro).max() <= 1e-11 * np.abs(S.ro).max()
    x = S.dev(S.x)
    y_csr = mf.mul_(torch.empty_like(x), S.gd.A, S.gd.K_total, x).cpu().numpy()
    y = mf.mul_(torch.empty_like(x), S.md.A, None, x).cpu().numpy()
    scale = np.abs(y_csr).max()
    assert scale > 0
    yo = S.Ko @ S.x
    e_csr, e_or = np.abs(y - y_csr).max() / scale, np.abs(y - yo).max() / np.abs(yo).max()
    print(f"{fam}-{name}: |y - y_csr| / max|y| = {e_csr:.2e}, against the oracle {e_or:.2e}")
    assert e_csr <= 1e-12
    assert e_or <= 1e-11
    y0 = np.random.default_rng(8).uniform(-1.0, 1.0, S.n)
    for alpha, beta in ((-1.0, 1.0), (0.5, -2.0)):
        got = S.md.A.mul_(S.dev(y0), x, alpha, beta).cpu().numpy()
        want = mf.mul_(S.dev(y0), S.gd.A, S.gd.K_total, x, alpha, beta).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (alpha, beta)
    nan = torch.full_like(x, float("nan"))
    got = S.md.A.mul_(nan, x, 1.0, 0.0).cpu().numpy()  # beta == 0 must not read y
    assert np.isfinite(got).all() and got.tobytes() == y.tobytes()


@pytest.mark.parametrize("fam,name", CASES, ids=IDS)
def test_diagonal_equals_the_diagonal_of_K_total(mf, fam, name):
    S = _built(mf, fam, name)
    d = S.md.A.diagonal().cpu().numpy()
    want = S.Kg.diagonal()
    err = np.abs(d - want).max() / np.abs(want).max()
    print(f"{fam}-{name}: |d - diag K_total| / max|diag| = {err:.2e}")
    assert err <= 1e-12


# ---- 2. in-place update, removal ------------------------------------------------------------------------------------------------------------------
def test_rewritten_coefficients_change_the_product_without_a_set_call(mf):
    import torch

    S = _built(mf, "hex8", "radiation")
    space, msh, fac, nf, wf, bnd, mtl, ext = S.case
    xs2 = 320.0 + 60.0 * np.random.default_rng(21).uniform(-1.0, 1.0, msh.ncp)
    doms = []
    for kw in (dict(matrix_free="any"), dict()):
        gd = _domain(mf, space, msh, nf, wf, bnd, mtl, ext, **kw)
        gd.dt = DT
        gd.update_Time()
        gd.x_star.copy_(torch.tensor(S.xs))
        gd.K_linear_func()
        gd.K_nonlinear_func()
        doms.append(gd)
    md, gd = doms
    x = S.dev(S.x)
    y1 = md.A.mul_(torch.empty_like(x), x).cpu().numpy()
    ptrs = [None if b is None else b.data_ptr() for b in md._var_buf]

    def refuse(*a, **k):
        raise AssertionError("set_variable_terms called again")
    md.A.set_variable_terms = refuse
    try:
        for d in (md, gd):
            d.x_star.copy_(torch.tensor(xs2))
            d.K_nonlinear_func()
    finally:
        del md.A.set_variable_terms
    assert [None if b is None else b.data_ptr() for b in md._var_buf] == ptrs
    y2 = md.A.mul_(torch.empty_like(x), x).cpu().numpy()
    want = mf.mul_(torch.empty_like(x), gd.A, gd.K_total, x).cpu().numpy()
    assert np.abs(y2 - y1).max() > 1e-6 * np.abs(y1).max()  # (the coefficients did change the operator)
    assert np.abs(y2 - want).max() <= 1e-12 * np.abs(want).max()
    # by hand: twice the coefficient array -> the constant part + twice the variable part
    part = md._op_part[1]
    md.A.set_variable_terms(part, [], None)
    y_const = md.A.mul_(torch.empty_like(x), x).cpu().numpy()
    t = md._op_parts[1].variable[0]
    assert md.A.set_variable_terms(part, [(t.dual_s, t.base_s, 0)], md._var_buf[1]) == 0
    assert md.A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == y2.tobytes()
    md._var_buf[1].mul_(2.0)
    y3 = md.A.mul_(torch.empty_like(x), x).cpu().numpy()
    assert np.abs(y3 - (y_const + 2.0 * (y2 - y_const))).max() <= 1e-12 * np.abs(y3).max()


def test_without_variable_terms_the_part_is_the_constant_operator_bit_for_bit(mf):
    import torch
    from metafem_jl_amd import physics as P

    S = _built(mf, "hex8", "radiation")
    space, msh, fac, nf, wf, bnd, mtl, ext = S.case
    md = _domain(mf, space, msh, nf, wf, bnd, mtl, ext, matrix_free="any")
    cd = _domain(mf, space, msh, nf, wf, [(fac, P.thermal_convection(25.0, 293.15))], mtl, ext, matrix_free=True)  # the same constant terms
    assert md.matrix_free is True and cd.matrix_free is True
    for d in (md, cd):
        d.x_star.copy_(torch.tensor(S.xs))
        d.K_linear_func()
        d.K_nonlinear_func()
    x = S.dev(S.x)
    y_c = cd.A.mul_(torch.empty_like(x), x).cpu().numpy()
    y_v = md.A.mul_(torch.empty_like(x), x).cpu().numpy()
    assert y_v.tobytes() != y_c.tobytes()
    assert md.A.set_variable_terms(md._op_part[1], [], None) == 0
    assert md.A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == y_c.tobytes()
    assert md.A.diagonal().cpu().numpy().tobytes() == cd.A.diagonal().cpu().numpy().tobytes()


# ---- 3. reproducibility, cycle graphs ---------------------------------------------------------------------------------------------------------------
def test_two_applications_and_two_solves_give_the_same_bits_with_graphs_on_and_off(mf):
    import torch
    from metafem_jl_amd import _lib

    S = _built(mf, "hex20", "neo_hookean")
    A = S.md.A
    x = S.dev(S.x)
    a = A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    assert A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == a
    assert A.diagonal().cpu().numpy().tobytes() == A.diagonal().cpu().numpy().tobytes()
    b = S.dev(S.b)

    def solve():
        sol, st = mf.iterative_Solve(A, None, b, 1e-10, Sv_func=mf.idrs_, s=8, seed=0x5EED, maxiter=2000, max_pass=4)
        return sol.cpu().numpy().tobytes(), st.iterations, st.converged

    buf = S.md._var_buf[0]
    other = buf.clone()
    terms = [(t.dual_s, t.base_s, t.dual_pos * 3 + t.base_pos) for t in S.md._op_parts[0].variable]
    try:
        on = [solve() for _ in range(2)]
        assert on[0] == on[1] and on[0][2] == 1
        # a captured cycle must not outlive its coefficient array: the same values in another array, then other values in it
        assert A.set_variable_terms(0, terms, other) == 0
        assert solve() == on[0]
        other.mul_(1.5)
        scaled_on = solve()
        assert scaled_on[0] != on[0][0]
        _lib.check(_lib.lib.mfem_debug_set_graphs(0, 0))
        assert solve() == scaled_on
        assert A.set_variable_terms(0, terms, buf) == 0
        off = solve()
        assert off == on[0]  # the same iterates with cycle graphs off
    finally:
        _lib.lib.mfem_debug_set_graphs(1, 0)
        A.set_variable_terms(0, terms, buf)


# ---- 4. Newton --------------------------------------------------------------------------------------------------------------------------------------
def _newton(mf, fam, name, solver, s, loads):
    """update_OneStep on the "any" and the default domain with the same linear_solver lambda -> [(domain, histories)]"""
    import torch

    space, msh, fac, _, _ = _mesh(fam, oracle=False)
    nf, wf, bnd, mtl, ext, _ = _case("cavity_newton" if name == "cavity" else name, msh, fac, np.random.default_rng(9))
    out = []
    for kw in (dict(matrix_free="any"), dict()):
        gd = _domain(mf, space, msh, nf, wf, bnd, mtl, ext, **kw)
        gd.converge_tol = 1e-9
        # relative residual 1e-12: with condition numbers <= 1e4 the error of each x is below 1e-8 |x| in the worst case (cond * residual / |b|)
        gd.linear_solver = lambda g: mf.iterative_Solve(g.A, g.K_total, g.residue, 1e-12 * mf.normalized_norm(g.residue), Sv_func=solver, s=s,
                                                        maxiter=4000, max_pass=8)[0]
        hist = []
        for load in loads:
            if name == "neo_hookean":  # sigma_22 on the face y = 0.8, the other components free
                for v in (1, 2, 3, 4, 5, 6):
                    gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), load if v == 2 else 0.0, dtype=torch.float64, device="cuda")
            hist.append(list(gd.update_OneStep(max_iter=12)))
        out.append((gd, hist))
    return out


@pytest.mark.parametrize("fam,name,solver,s,loads", [("hex20", "neo_hookean", "bicgstabl_GS_", 4, (0.05, 0.10, 0.15)), ("quad8", "cavity", "cgs2_", 0, (1,)),
                                                     ("hex8", "radiation", "idrs_", 8, (1,))],
                         ids=["hex20-neo_hookean-three-loads", "quad8-cavity", "hex8-radiation"])
def test_newton_on_the_operator_steps_like_the_default_domain(mf, fam, name, solver, s, loads):
    (md, hm), (gd, hg) = _newton(mf, fam, name, getattr(mf, solver), s, loads)
    assert md.matrix_free is True and gd.matrix_free is False
    assert isinstance(md.A, mf.MeshOperator)
    assert md.K_linear is None and md.K_total is None and md.slots is None and md.table_bytes == 0
    print(f"{fam}-{name}: histories {hm} / {hg}")
    assert [len(h) for h in hm] == [len(h) for h in hg]
    assert hm[-1][-1] < md.converge_tol and hg[-1][-1] < gd.converge_tol
    xm, xg = md.x.cpu().numpy(), gd.x.cpu().numpy()
    assert np.abs(xg).max() > 0
    err = np.abs(xm - xg).max() / np.abs(xg).max()
    print(f"{fam}-{name}: |x - x_default| / max|x| = {err:.2e}")
    assert err <= 1e-8


# ---- 5. memory --------------------------------------------------------------------------------------------------------------------------------------
def test_any_domain_holds_less_than_half_of_the_default_domain(mf):
    """hex-20 6^3 Neo-Hookean on fresh contexts: construction and one Newton step.  The default path holds >= 60 kB per element (two value arrays,
    columns, sparse_IDs_by_el, tables, the layout copy), the matrix-free one about 20 kB (coefficients, nine words, vectors)."""
    import torch

    space, msh, fac, _, _ = _mesh("hex20", cells=(6, 6, 6), oracle=False)
    nf, wf, bnd, mtl, ext, _ = _case("neo_hookean", msh, fac, np.random.default_rng(9))
    rise = []
    for kw in (dict(matrix_free="any"), dict()):
        ctx = mf.Context(0)
        try:
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            gd = _domain(mf, space, msh, nf, wf, bnd, mtl, {}, ctx=ctx, **kw)
            for v in (1, 2, 3, 4, 5, 6):
                gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 0.05 if v == 2 else 0.0, dtype=torch.float64, device="cuda")
            gd.converge_tol = 1e-9
            gd.linear_solver = lambda g: mf.iterative_Solve(g.A, g.K_total, g.residue, 1e-10 * mf.normalized_norm(g.residue), Sv_func=mf.bicgstabl_GS_,
                                                            s=4, maxiter=4000, max_pass=8)[0]
            hist = gd.update_OneStep(max_iter=0)
            torch.cuda.synchronize()
            rise.append(torch.cuda.memory_allocated() - m0)
            assert len(hist) == 2 and np.isfinite(hist).all()  # (one Newton step was taken: residual, solve, residual)
            assert gd.matrix_free is bool(kw)
            gd.A.close()
            del gd
        finally:
            ctx.close()
    print(f"rise of memory_allocated: matrix_free='any' {rise[0]} B, default {rise[1]} B, per element {rise[0] / 216:.0f} / {rise[1] / 216:.0f} B")
    assert rise[0] < 0.5 * rise[1]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(mf):
    import torch
    from metafem_jl_amd import _lib

    S = _built(mf, "hex8", "radiation")
    md = S.md
    ctx, h = md.ctx, md.A._h
    part = md._op_part[1]
    buf = md._var_buf[1]
    K = lambda ds, bs, block: _lib.KvalTerm(ds, bs, block, 0)
    x = S.dev(S.x)
    y_before = md.A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes()
    torch.cuda.synchronize()
    n0 = int(_lib.lib.mfem_debug_mesh_operator_count())

    def set_var(terms, vals=buf.data_ptr(), p=part, handle=h):
        arr = (_lib.KvalTerm * max(len(terms), 1))(*terms)
        return _lib.lib.mfem_mesh_operator_set_variable_terms(handle, p, len(terms), arr, vals)

    big = torch.zeros(129 * buf[0].numel(), dtype=torch.float64, device="cuda")
    assert set_var([K(0, 0, 0)] * 129, vals=big.data_ptr()) == UNSUPPORTED  # 129 variable terms
    assert set_var([K(0, 0, 0)] * 128, vals=big.data_ptr()) == UNSUPPORTED  # 128 + the constant -h: 129 entries
    assert b"128" in _lib.lib.mfem_last_error()
    assert set_var([K(0, 0, 0)], vals=None) == INVALID
    assert set_var([K(0, 0, 1)]) == INVALID   # block out of range (one field)
    assert set_var([K(0, 0, -1)]) == INVALID
    assert set_var([K(4, 0, 0)]) == INVALID   # words: 0 .. dim
    assert set_var([K(0, -1, 0)]) == INVALID
    assert set_var([K(0, 0, 0)], p=7) == INVALID   # no such part
    assert set_var([K(0, 0, 0)], p=-1) == INVALID
    assert set_var([K(0, 0, 0)], handle=0) == INVALID
    assert _lib.lib.mfem_mesh_operator_set_variable_terms(h, part, 1, None, buf.data_ptr()) == INVALID
    # the solve gate is what it was
    b = S.dev(S.b)
    sentinel = 123.25
    xo = torch.full_like(b, sentinel)
    st = _lib.SolveStats()

    def solve(**kw):
        opt = dict(method=mf.idrs_, precond=1, l_or_s=8, maxiter=50, max_pass=1, check_every=32, converge_tol=1e-10, seed=1)
        opt.update(kw)
        o = _lib.SolveOptions(**opt)
        return _lib.lib.mfem_solve_operator(ctx._h, h, b.data_ptr(), xo.data_ptr(), C.byref(o), C.byref(st))

    assert solve(method=mf.lsqr_) == UNSUPPORTED
    assert solve(left_precond=mf.Pl_Jacobi_) == UNSUPPORTED
    ops = _lib.CommHostOps(None, _lib.ALLREDUCE_CB(lambda *a: 1), _lib.EXCHANGE_CB(lambda *a: 1), 0, 0)
    hc = C.c_void_p()
    _lib.check(_lib.lib.mfem_comm_create_host(ctx._h, 0, 1, C.byref(ops), C.byref(hc)))
    try:
        _lib.check(_lib.lib.mfem_context_set_comm(ctx._h, hc, md.A.n, 1, 1))
        assert solve() == INVALID
        assert b"one rank only" in _lib.lib.mfem_last_error()
    finally:
        _lib.lib.mfem_context_set_comm(ctx._h, None, 0, 0, 0)
        _lib.lib.mfem_comm_destroy(hc)
    torch.cuda.synchronize()
    assert int(_lib.lib.mfem_debug_mesh_operator_count()) == n0  # nothing launched
    assert bool((xo == sentinel).all())                           # nothing written
    assert md.A.mul_(torch.empty_like(x), x).cpu().numpy().tobytes() == y_before  # a refused call leaves the part as it was
    assert solve() == 0 and not bool((xo == sentinel).any())
    # a part that has not been set takes no variable terms
    op = mf.MeshOperator(ctx, 3, md.itp, md.nel, md.ncp, 1, md.coords, md.cp, 1)
    try:
        assert set_var([K(0, 0, 0)], p=0, handle=op._h) == INVALID
    finally:
        op.close()


# ---- 7. the opt-in boundary ---------------------------------------------------------------------------------------------------------------------------
def test_matrix_free_true_still_falls_back_on_the_radiation_form(mf):
    S = _built(mf, "hex8", "radiation")
    space, msh, fac, nf, wf, bnd, mtl, ext = S.case
    gd = _domain(mf, space, msh, nf, wf, bnd, mtl, ext, matrix_free=True)
    assert gd.matrix_free is False and "nonlinear" in gd.matrix_free_reason
    assert gd.K_linear is not None and not isinstance(gd.A, mf.MeshOperator)
    assert getattr(gd, "matrix_free_any") is False
