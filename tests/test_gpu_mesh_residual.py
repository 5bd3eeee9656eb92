"""The fused mesh residual (mfem_mesh_residual_elements / _facets, csrc/residual_mesh.hip; GenericDomain(fused_residual=True)) against the operator
path (mfem_op_var_batch + mfem_op_res_batch on the stored geometry tables) and the oracle's term-by-term residual (oracle/fem.py), on curved meshes of
every family the examples use, with facets (convection, Nitsche wall, penalty, traction), time levels 1 and 2, a collapsed element, the refusals of
the C entry points, a nonlinear form that keeps the operator path for its other terms, and a full-size hex-20 mesh without any table."""
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


def _warp(c):
    dim = c.shape[1]
    out = c.copy()
    for i in range(dim):
        j, k = (i + 1) % dim, (i + 2) % dim
        out[:, i] += 0.05 * np.sin(2.3 * c[:, j] + 1.1 * c[:, k] + 0.4 * i) + 0.04 * c[:, i] * c[:, j]
    return out


def _mesh(fam, block=4, seed=11):
    """(space, mesh (warped: curved elements), boundary facets, oracle disc, oracle mesh on the same arrays)."""
    from metafem_jl_amd import element, mesh as pm
    from oracle import mesh as om, reference_element as re_

    dim, itp_type, order, itg, shape, n = FAMILIES[fam]
    space = element.classical_space(dim, itp_type, order, itg, shape=shape)
    vert, conn = (pm.make_Square((1.0, 0.8), n, shape) if dim == 2 else pm.make_Brick((1.0, 0.8, 0.9), n, shape))
    nel = conn.shape[1]
    nb = (nel + block - 1) // block
    perm = (np.random.default_rng(seed).permutation(nb)[:, None] * block + np.arange(block)[None, :]).ravel()
    msh = pm.mesh_Classical(vert, conn[:, perm[perm < nel]], space)
    fac = pm.get_BoundaryMesh(msh)
    msh.coords = _warp(msh.coords)
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


def _domains(mf, fam, name, seed=3):
    """Fused and operator-path domains (and the oracle's) at one random x_star and random externals; residuals computed."""
    import torch
    from metafem_jl_amd import generic as G
    from oracle import fem

    space, msh, fac, disc, omesh = _mesh(fam)
    dim = FAMILIES[fam][0]
    nf, wf, bnd, mtl, ext = _case(name, dim, fac)
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-1.0, 1.0, (mtl + 1) * nf * msh.ncp)
    ev = {k: rng.uniform(-1.0, 1.0, msh.ncp) for k in ext}
    out = []
    for fused in (True, False):
        gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf, [(f.element_ID, f.element_eindex, w) for f, w in bnd],
                             max_time_level=mtl, fused_residual=fused)
        for k, v in ev.items():
            gd.controlpoints[k] = torch.tensor(v, device="cuda")
        gd.x_star.copy_(torch.tensor(xs))
        gd.K_nonlinear_func()
        out.append(gd)
    od = fem.FEMDomain(omesh, disc, nf, wf, list(bnd), max_time_level=mtl)
    for k, v in ev.items():
        od.controlpoints[k] = v
    od.update_time()
    od.x_star[:] = xs
    od.K_nonlinear_func()
    return out[0], out[1], od


CASES = [("hex20", "thermal"), ("hex20", "elasticity"), ("tet10", "thermal"), ("tet10", "wall"), ("hex8", "thermal"), ("hex27", "thermal"),
         ("quad8", "nitsche"), ("hex20", "transient"), ("hex8", "dynamics"), ("quad8", "wall")]


@pytest.mark.parametrize("fam,name", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_fused_residual_equals_the_operator_path_and_the_oracle(mf, fam, name):
    from metafem_jl_amd import _lib

    n0 = int(_lib.lib.mfem_debug_mesh_residual_count())
    fd, gd, od = _domains(mf, fam, name)
    launches = 1 + len(fd.groups) - 1
    assert int(_lib.lib.mfem_debug_mesh_residual_count()) - n0 == launches  # every group took the fused launch
    assert fd.table_bytes == 0 and gd.table_bytes > 0
    rf, rg = fd.residue.cpu().numpy(), gd.residue.cpu().numpy()
    scale = np.abs(rg).max()
    assert scale > 0
    assert np.abs(rf - rg).max() <= 1e-12 * scale
    assert np.abs(rf - od.residue).max() <= 1e-11 * np.abs(od.residue).max()


def test_two_evaluations_give_the_same_bits(mf):
    fd, _, _ = _domains(mf, "hex20", "elasticity")
    a = fd.residue.clone()
    fd.K_nonlinear_func()
    assert fd.residue.cpu().numpy().tobytes() == a.cpu().numpy().tobytes()


def test_normals_on_the_fly_equal_the_boundary_tables(mf):
    """A facet term c * n_j alone: the fused residual integrates the on-the-fly normal exactly as the operator path its stored one."""
    import torch
    from metafem_jl_amd import generic as G

    space, msh, fac, _, _ = _mesh("hex20")
    for j in range(3):
        wf = G.WeakForm(normals=[(f"n{j}", j)], residues=[G.ResTerm(0, 0, lambda env, j=j: 2.5 * env[f"n{j}"])])
        r = []
        for fused in (True, False):
            gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, 1, G.WeakForm(), [(fac.element_ID, fac.element_eindex, wf)],
                                 fused_residual=fused)
            gd.K_nonlinear_func()
            r.append(gd.residue.cpu().numpy())
        assert np.abs(r[0] - r[1]).max() <= 1e-13 * np.abs(r[1]).max()


def test_table_free_domain_solves_like_the_default_one(mf):
    import torch
    from metafem_jl_amd import generic as G, physics as P

    space, msh, fac, _, _ = _mesh("hex20")
    wf, bnd = P.thermal_domain(3, 0.6), [(fac.element_ID, fac.element_eindex, P.thermal_convection(25.0, 293.15))]
    itg, itp, nel = space.itg, msh.cp_ids.shape[0], msh.cp_ids.shape[1]
    table = itg * itp * 4 * nel * 8
    fd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, 1, wf, bnd, fused_residual=True)
    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, 1, wf, bnd)
    xs = []
    for d in (fd, gd):
        d.controlpoints["s"] = torch.full((msh.ncp,), 1600.0, dtype=torch.float64, device="cuda")
        d.converge_tol = 1e-9
        d.linear_solver = lambda g: mf.iterative_Solve(g.A, g.K_total, g.residue, 1e-13, Sv_func=mf.cg_, maxiter=2000, max_pass=4)[0]
        if d is fd:  # what evaluating K and the residual adds to the fused domain
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            d.K_linear_func()
            d.K_nonlinear_func()
            torch.cuda.synchronize()
            rise = torch.cuda.memory_allocated() - m0
        d.update_OneStep()
        xs.append(d.x.cpu().numpy())
    assert fd.table_bytes == 0 and gd.table_bytes >= table
    assert rise < table
    assert np.abs(xs[0] - xs[1]).max() <= 1e-10 * np.abs(xs[1]).max()
    assert fd.history[-1] < 1e-9


def test_collapsed_element_gives_the_operator_residual(mf):
    """A hex-8 whose face x = 1 is pinched to an edge (two nodes listed twice): the adjacency holds both entries."""
    import torch
    from metafem_jl_amd import element, generic as G, physics as P

    space = element.classical_space(3, "Lagrange", 1, 3)
    # nodes (1, 0, z) and (1, 1, z) of the face x = 1 meet at z = 0.5: the element lists control points 1 and 2 twice
    coords = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0], [0, 0, 1], [0, 1, 1]], dtype=float)
    cp = np.array([[0, 1, 2, 3, 4, 1, 2, 5]]).T
    wf = P.thermal_domain(3, 0.6, alpha=0.7, Tenv=300.0)
    r = []
    for fused in (True, False):
        gd = G.GenericDomain(mf.default_context(), space, coords, cp, 1, wf, [], fused_residual=fused)
        gd.controlpoints["s"] = torch.arange(6, dtype=torch.float64, device="cuda")
        gd.x_star.copy_(torch.linspace(-1.0, 2.0, 6, dtype=torch.float64))
        gd.K_nonlinear_func()
        r.append(gd.residue.cpu().numpy())
    assert np.abs(r[0] - r[1]).max() <= 1e-12 * np.abs(r[1]).max()


def test_nonlinear_form_keeps_its_other_terms_on_the_operator_path(mf):
    """The cavity (SUPG / PSPG, Nitsche walls): affine residual terms fused, the rest and the nonlinear gradients through the operators -- the same
    Newton histories as the default path."""
    import torch
    from oracle import cavity
    from metafem_jl_amd import element, generic as G

    od = cavity.build_cavity(8, Cb=128.0)

    def conv(wf):
        return G.WeakForm(inner_vars=list(wf.inner_vars), cp_ext_vars=list(wf.cp_ext_vars), normals=list(wf.normals),
                          residues=[G.ResTerm(r.dual_pos, r.dual_s, r.fn) for r in wf.residues],
                          linear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.linear_gradients],
                          nonlinear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.nonlinear_gradients])

    space = element.classical_space(2, "Serendipity", 2, 5)
    hist = []
    for fused in (True, False):
        gd = G.GenericDomain(mf.default_context(), space, od.mesh.coords, od.mesh.cp_ids, od.n_fields, conv(od.domain_wf),
                             [(f.element_ID, f.element_eindex, conv(w)) for f, w in od.boundaries], max_time_level=od.max_time_level,
                             dissipative=od.time.gamma_params[0] == 1.0, fused_residual=fused)
        gd.converge_tol = 1e-8
        gd.linear_solver = lambda g: mf.iterative_Solve(g.A, g.K_total, g.residue, 1e-10 * mf.normalized_norm(g.residue), Sv_func=mf.idrs_,
                                                        maxiter=4000, max_pass=20, s=8)[0]
        h = []
        od.x[:] = 0.0
        od.dessemble_x(cavity.INNER_INFOS)
        for step in (1, 2):
            cavity.set_step_parameters(od, 0.05 * step)
            for k in ("uw1", "uw2", "taum", "tauc"):
                gd.controlpoints[k] = torch.tensor(od.controlpoints[k], device="cuda")
            gd.dt = od.dt
            h += gd.update_OneStep(max_iter=6)
        hist.append(h)
        if fused:
            descs = [d for i, (wf, g) in enumerate(gd._parts()) for d in gd._affine_terms(i, wf)]
            assert any(d is not None for d in descs) and any(d is None for d in descs)
            assert gd.table_bytes > 0  # (the other terms read the tables)
    assert len(hist[0]) == len(hist[1])
    assert np.allclose(hist[0], hist[1], rtol=1e-8)


def _raw_call(mf, fd, symbols, terms, **over):
    from metafem_jl_amd import _lib

    a = dict(ctx=fd.ctx._h, dim=fd.dim, itg=fd.space.itg, itp=fd.itp, nel=fd.nel, ncp=fd.ncp, ref=fd._ref.data_ptr(), w=fd._itgw.data_ptr(),
             coords=fd.coords.data_ptr(), cp=fd.cp.data_ptr(), base=1, ptr=fd._adj_ptr.data_ptr(), adj=fd._adj.data_ptr(), res=fd.residue.data_ptr())
    a.update(over)
    arr_s = (_lib.ResSymbol * max(len(symbols), 1))(*symbols)
    arr_t = (_lib.AffineTerm * max(len(terms), 1))(*terms)
    return _lib.lib.mfem_mesh_residual_elements(a["ctx"], a["dim"], a["itg"], a["itp"], a["nel"], a["ncp"], a["ref"], a["w"], a["coords"], a["cp"],
                                                a["base"], len(symbols), arr_s if symbols else None, len(terms), arr_t if terms else None,
                                                a["ptr"], a["adj"], a["res"])


def test_refusals(mf):
    import torch
    from metafem_jl_amd import _lib

    fd, gd, _ = _domains(mf, "hex8", "thermal")
    x = fd.x_star.data_ptr()
    sym = lambda word=0: _lib.ResSymbol(word, 0, 0, x)

    def term(n_pairs=1, sym_ids=(0,), normals=(-1,), dual_sd=0):
        t = _lib.AffineTerm()
        t.dual_pos, t.dual_sd, t.n_pairs, t.c0 = 0, dual_sd, n_pairs, 1.0
        for p in range(min(n_pairs, 8)):
            t.sym[p], t.normal[p], t.coef[p] = sym_ids[p % len(sym_ids)], normals[p % len(normals)], 1.0
        return t

    assert _raw_call(mf, fd, [sym()], [term()]) == 0
    INVALID, UNSUPPORTED = -1, -3
    assert _raw_call(mf, fd, [sym()], [term()], ctx=None) == INVALID
    assert _raw_call(mf, fd, [sym()], [term()], coords=None) == INVALID
    assert _raw_call(mf, fd, [sym()], [term()], ptr=None) == INVALID
    assert _raw_call(mf, fd, [sym()], [term()], dim=4) == INVALID
    assert _raw_call(mf, fd, [sym()], [term()], base=2) == INVALID
    assert _raw_call(mf, fd, [sym()], []) == INVALID
    assert _raw_call(mf, fd, [sym(word=4)], [term()]) == INVALID
    assert _raw_call(mf, fd, [_lib.ResSymbol(0, 0, 0, None)], [term()]) == INVALID
    assert _raw_call(mf, fd, [sym()], [term(sym_ids=(1,))]) == INVALID
    assert _raw_call(mf, fd, [sym()], [term(normals=(0,))]) == INVALID  # (normals exist on facets only)
    assert _raw_call(mf, fd, [sym()], [term(dual_sd=5)]) == INVALID
    assert _raw_call(mf, fd, [sym()] * 17, [term()]) == UNSUPPORTED
    assert _raw_call(mf, fd, [sym()], [term()] * 49) == UNSUPPORTED
    assert _raw_call(mf, fd, [sym()], [term(n_pairs=9)]) == UNSUPPORTED
    # the host falls back when the caps are exceeded: 17 distinct symbols on one dual word -> the operator path, the same residual
    from metafem_jl_amd import generic as G

    space, msh, _, _, _ = _mesh("hex8")
    wf = G.WeakForm(inner_vars=[(f"T{i}", 0, i % 4, 0) for i in range(4)], cp_ext_vars=[(f"e{i}", f"e{i}", i % 4) for i in range(13)])
    wf.residues.append(G.ResTerm(0, 0, lambda env: sum((1.0 + 0.1 * i) * env[f"T{i}"] for i in range(4)) +
                                 sum((0.5 - 0.05 * i) * env[f"e{i}"] for i in range(13))))
    r = []
    for fused in (True, False):
        d = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, 1, wf, [], fused_residual=fused)
        for i in range(13):
            d.controlpoints[f"e{i}"] = torch.linspace(-1.0, 1.0 + i, msh.ncp, dtype=torch.float64, device="cuda")
        d.x_star.copy_(torch.linspace(0.5, -2.0, msh.ncp, dtype=torch.float64, device="cuda"))
        d.K_nonlinear_func()
        r.append(d.residue.cpu().numpy())
    assert np.abs(r[0] - r[1]).max() <= 1e-12 * np.abs(r[1]).max()


def test_full_size_hex20_thermal_without_tables(mf):
    """The hex-20 thermal leg's mesh at 64^3 (262 144 elements): fused residual = operator residual, and no table on the fused domain."""
    import torch
    import bench
    import bench_legs as L
    from metafem_jl_amd import generic as G, physics as P

    Bn = L.Bench(bench.parse_args([]))
    space, msh, fac = Bn.unstructured_mesh(64)
    wf, bnd = P.thermal_domain(3, L.K_COND), [(fac.element_ID, fac.element_eindex, P.thermal_convection(L.H, L.TENV))]
    xs = torch.tensor(np.random.default_rng(5).uniform(250.0, 350.0, msh.ncp), device="cuda")
    r = []
    for fused in (True, False):
        d = G.GenericDomain(Bn.ctx, space, msh.coords, msh.cp_ids, 1, wf, bnd, fused_residual=fused)
        d.controlpoints["s"] = torch.full((msh.ncp,), L.SRC, dtype=torch.float64, device="cuda")
        d.x_star.copy_(xs)
        d.K_nonlinear_func()
        r.append(d.residue.cpu().numpy())
        if fused:
            assert d.table_bytes == 0
        else:
            assert d.table_bytes > 0
        del d
        torch.cuda.empty_cache()
    assert np.abs(r[0] - r[1]).max() <= 1e-12 * np.abs(r[1]).max()
