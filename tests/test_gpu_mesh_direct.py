"""The direct row assembly (GenericDomain(direct_rows=True) -> mfem_mesh_assemble_elements_direct, csrc/mesh_direct.hip) against the oracle on
every element family, form and field count of tests/test_gpu_mesh_oracle.py (whose meshes, forms and bound are copied here), against the two-pass
row-owner form, bit for bit against itself under three batch budgets, on a mesh with more batches than resident waves, without the element-matrix
scratch, and its refusals.

Meshes: make_Square / make_Brick (CUBE, SIMPLEX) -> element order shuffled in blocks (owners differ from element order) -> mesh_Classical -> every
control point moved by a smooth non-affine map (the Jacobian varies over every element).  The tet-10 mesh is also the high-valence case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (dim, itp_type, itp_order, itg_order, shape, cells)  -- tests/test_gpu_mesh_oracle.py
FAMILIES = {
    "tri3": (2, "Lagrange", 1, 3, "SIMPLEX", (5, 4)),
    "tri6": (2, "Lagrange", 2, 5, "SIMPLEX", (5, 4)),
    "quad4": (2, "Lagrange", 1, 3, "CUBE", (6, 5)),
    "quad8": (2, "Serendipity", 2, 5, "CUBE", (6, 5)),
    "quad9": (2, "Lagrange", 2, 5, "CUBE", (6, 5)),
    "quad16": (2, "Lagrange", 3, 7, "CUBE", (5, 4)),
    "tet4": (3, "Lagrange", 1, 3, "SIMPLEX", (3, 2, 2)),
    "tet10": (3, "Serendipity", 2, 5, "SIMPLEX", (3, 2, 2)),
    "tet10_24": (3, "Serendipity", 2, 6, "SIMPLEX", (3, 2, 2)),
    "hex8": (3, "Lagrange", 1, 3, "CUBE", (3, 3, 2)),
    "hex20": (3, "Serendipity", 2, 5, "CUBE", (3, 3, 2)),
    "hex20_64": (3, "Serendipity", 2, 7, "CUBE", (3, 2, 2)),
    "hex27": (3, "Lagrange", 2, 5, "CUBE", (3, 3, 2)),
    "hex27_64": (3, "Lagrange", 2, 7, "CUBE", (3, 2, 2)),
}
FORMS = ("values", "grads-diag", "grads", "mixed")
TOL = 1e-12  # |K - K_oracle| <= TOL max |K_oracle|: the project's bound for this comparison
K_CASES = ([(fam, form, (i + j) % 3 + 1) for i, fam in enumerate(FAMILIES) for j, form in enumerate(FORMS)]
           + [("hex8", "mixed", 4), ("tet10", "mixed", 4), ("quad8", "mixed", 4), ("hex20", "grads", 4)])
PHYSICS = ("thermal", "elasticity")
# What the direct form refuses here (MFEM_ERR_UNSUPPORTED -> the two-pass chain): hex-27 with 64 Gauss points and gradient words.  Its reference
# table is 64 * 27 * 4 = 6912 doubles, its physical table with 3 (4) slots 5184 (6912) more, w det / J^-1 / X 721: beyond the 12288 doubles
# (96 KB) of a workgroup before a single row is staged.  Values only (1728 doubles of table) fits.  Every other family fits with the rows of its
# largest control point (hex-20 with 64 points, four slots, three fields: 5120 + 144 + 5820 + 729 doubles).
REFUSED = {("hex27_64", f) for f in ("grads-diag", "grads", "mixed", "thermal", "elasticity")}

_cache = {}


def _warp(c):
    dim = c.shape[1]
    out = c.copy()
    for i in range(dim):
        j, k = (i + 1) % dim, (i + 2) % dim
        out[:, i] += 0.05 * np.sin(2.3 * c[:, j] + 1.1 * c[:, k] + 0.4 * i) + 0.04 * c[:, i] * c[:, j]
    return out


def _mesh(fam, cells=None, block=4, seed=11, oracle=True):
    """(product space, product mesh (warped), boundary facets, oracle disc, oracle mesh on the product's arrays)."""
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


def _form(kind, dim, nf, seed):
    """Seeded constant-coefficient term lists, every block (fd, fb) coupled; coefficients +-[0.5, 1.5], distinct."""
    from metafem_jl_amd.generic import GradTerm, WeakForm

    rng = np.random.default_rng(seed)
    words = {"values": [(0, 0)],
             "grads-diag": [(d, d) for d in range(1, dim + 1)],
             "grads": [(d, e) for d in range(1, dim + 1) for e in range(1, dim + 1)],
             "mixed": [(d, e) for d in range(dim + 1) for e in range(dim + 1)]}[kind]
    wf = WeakForm()
    terms = [(fd, ds, fb, bs) for fd in range(nf) for fb in range(nf) for ds, bs in words]
    coefs = rng.uniform(0.5, 1.5, len(terms)) * rng.choice([-1.0, 1.0], len(terms))
    for (fd, ds, fb, bs), c in zip(terms, coefs):
        wf.linear_gradients.append(GradTerm(fd, ds, fb, bs, lambda env, c=float(c): c))
    return wf


def _oracle_K(omesh, disc, nf, wf, bnd=()):
    from oracle import fem

    od = fem.FEMDomain(omesh, disc, nf, wf, list(bnd))
    for _, sym, _ in [v for w in [wf] + [b[1] for b in bnd] for v in w.cp_ext_vars]:
        od.controlpoints[sym] = np.zeros(omesh.ncp)
    od.update_time()
    od.K_linear_func()
    return od.K_linear


def _physics(name, dim, fac):
    import bench_legs as L
    from metafem_jl_amd import physics

    if name == "thermal":
        return 1, physics.thermal_domain(dim, L.K_COND, alpha=0.7, Tenv=300.0), [(fac, physics.thermal_convection(L.H, L.TENV))]
    c = fac.centroid
    return dim, physics.elasticity_domain(dim, 1.7, 0.6), [(fac.select(np.abs(c[:, 0]) < 1e-9), physics.penalty(list(range(dim)), 37.0)),
                                                            (fac.select(np.abs(c[:, 1] - 0.8) < 1e-9), physics.traction(dim, "sl", rows=[1]))]


def _reference(fam, form, nf):
    """(space, mesh, form, oracle K) of a seeded case, computed once."""
    key = (fam, form, nf)
    if key not in _cache:
        space, msh, _, disc, omesh = _mesh(fam)
        wf = _form(form, space.dim, nf, seed=1000 * nf + 100 * FORMS.index(form) + list(FAMILIES).index(fam))
        Ko = _oracle_K(omesh, disc, nf, wf)
        Ko.setflags(write=False)
        _cache[key] = (space, msh, wf, Ko)
    return _cache[key]


def _domain(mf, space, msh, nf, wf, bnd=(), ctx=None, **opts):
    import torch

    from metafem_jl_amd import generic as G

    gd = G.GenericDomain(ctx or mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf,
                         [(f.element_ID, f.element_eindex, w) for f, w in bnd], **opts)
    for _, sym, _ in [v for w in [wf] + [b[1] for b in bnd] for v in w.cp_ext_vars]:
        gd.controlpoints[sym] = torch.zeros(msh.ncp, dtype=torch.float64, device="cuda")
    gd.update_Time()
    return gd


def _assemble(mf, space, msh, nf, wf, bnd=(), ctx=None, **opts):
    """(domain, K_linear as a fresh device tensor, rise of mfem_debug_mesh_direct_count)."""
    from metafem_jl_amd import _lib

    gd = _domain(mf, space, msh, nf, wf, bnd, ctx, **opts)
    n0 = int(_lib.lib.mfem_debug_mesh_direct_count())
    gd.K_linear_func()
    return gd, gd.K_linear.clone(), int(_lib.lib.mfem_debug_mesh_direct_count()) - n0


def _element_assemblies(wf):
    """Calls the element group of a domain makes: its constant-coefficient terms in chunks of MAX_BATCH_TERMS."""
    from metafem_jl_amd import _lib
    from metafem_jl_amd.generic import constant_coefficient

    n = sum(constant_coefficient(t.fn) is not None for t in wf.linear_gradients)
    return -(-n // _lib.MAX_BATCH_TERMS)


@pytest.fixture
def budget():
    """Set mfem_debug_set("mesh_direct_budget", bytes); the default comes back whatever happens."""
    from metafem_jl_amd import _lib

    try:
        yield lambda nbytes: _lib.check(_lib.lib.mfem_debug_set_mesh_direct_budget(int(nbytes)))
    finally:
        _lib.lib.mfem_debug_set_mesh_direct_budget(0)


def _rel(K, Kref):
    return float(np.abs(K - Kref).max() / np.abs(Kref).max())


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,form,nf", K_CASES, ids=[f"{a}-{b}-{c}f" for a, b, c in K_CASES])
def test_direct_K_against_the_oracle(mf, fam, form, nf):
    space, msh, wf, Ko = _reference(fam, form, nf)
    gd, K, rise = _assemble(mf, space, msh, nf, wf, direct_rows=True)
    K = K.cpu().numpy()
    assert K.shape == Ko.shape and np.abs(K).max() > 0
    err = _rel(K, Ko)
    print(f"{fam} {form} {nf} fields: |K - K_oracle| / |K_oracle| = {err:.3e}, direct calls {rise}, stats {gd.direct_stats()}")
    assert err <= TOL, f"{fam} {form} {nf} fields: {err:.3e}"
    if (fam, form) in REFUSED:
        assert rise == 0 and gd.direct_rows is False  # the two-pass chain took over
    else:
        assert rise == _element_assemblies(wf) and gd.direct_rows is True


@pytest.mark.parametrize("phys", PHYSICS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_direct_physics_forms_against_the_oracle(mf, fam, phys):
    """thermal_domain (value and gradient words) + convection on every facet; elasticity_domain + penalty and traction facets: the element group
    takes the direct form, the facet groups are unchanged."""
    space, msh, fac, disc, omesh = _mesh(fam)
    nf, wf, bnd = _physics(phys, space.dim, fac)
    Ko = _oracle_K(omesh, disc, nf, wf, bnd)
    gd, K, rise = _assemble(mf, space, msh, nf, wf, bnd, direct_rows=True)
    K = K.cpu().numpy()
    assert np.abs(K).max() > 0
    err = _rel(K, Ko)
    print(f"{fam} {phys}: {err:.3e}, direct calls {rise}")
    assert err <= TOL, f"{fam} {phys}: {err:.3e}"
    assert rise == (0 if (fam, phys) in REFUSED else _element_assemblies(wf))


def test_tet10_is_the_high_valence_case():
    """The tet-10 mesh of the cases above has a vertex with 32 adjacency entries: many element runs per batch, rows far longer than an element."""
    _, msh, _, _, _ = _mesh("tet10", oracle=False)
    assert np.bincount(np.asarray(msh.cp_ids).ravel()).max() == 32


# ---- 2. reproducible, and independent of the batching -------------------------------------------------------------------------------------------
REPRO = [("hex20", "grads", 3), ("tet10", "mixed", 3)]


@pytest.mark.parametrize("fam,form,nf", REPRO, ids=[f"{a}-{b}-{c}f" for a, b, c in REPRO])
def test_same_bits_twice_and_under_every_budget(mf, budget, fam, form, nf):
    import torch

    from metafem_jl_amd import _lib

    space, msh, wf, Ko = _reference(fam, form, nf)
    gd, K0, rise = _assemble(mf, space, msh, nf, wf, direct_rows=True)
    assert rise == _element_assemblies(wf)
    gd.K_linear_func()
    assert torch.equal(gd.K_linear, K0), "two direct assemblies differ"
    st0 = gd.direct_stats()
    assert st0["tasks"] == msh.nel * space.itp and st0["budget_doubles"] == 2048
    # the smallest budget that holds the largest control point: one owner's control points go to two or more batches
    budget(8 * st0["max_control_point_doubles"])
    gmin, Kmin, _ = _assemble(mf, space, msh, nf, wf, direct_rows=True)
    smin = gmin.direct_stats()
    assert smin["budget_doubles"] == st0["max_control_point_doubles"] and smin["split_owners"] >= 1, smin
    assert smin["max_batch_doubles"] <= smin["budget_doubles"] and smin["batches"] > st0["batches"]
    # a budget at the LDS cap (the library keeps what fits beside the element's tables): two or more owner elements in one batch
    budget(96 * 1024)
    gmax, Kmax, _ = _assemble(mf, space, msh, nf, wf, direct_rows=True)
    smax = gmax.direct_stats()
    assert smax["budget_doubles"] > 2048 and smax["max_batch_owners"] >= 2 and smax["batches"] < st0["batches"], smax
    assert smax["lds_bytes"] <= 96 * 1024 and smax["waves_per_workgroup"] == 1
    print(st0, smin, smax, sep="\n")
    assert torch.equal(Kmin, K0), "the smallest budget changes bits"
    assert torch.equal(Kmax, K0), "the largest budget changes bits"
    # one below the smallest: refused when the plan is made, the two-pass form serves
    budget(8 * st0["max_control_point_doubles"] - 8)
    n0 = int(_lib.lib.mfem_debug_mesh_rows_count())
    gref, Kref, rise = _assemble(mf, space, msh, nf, wf, direct_rows=True)
    assert rise == 0 and gref.direct_rows is False and int(_lib.lib.mfem_debug_mesh_rows_count()) > n0
    assert _rel(K0.cpu().numpy(), Kref.cpu().numpy()) <= TOL


# ---- 3. against the two-pass form -----------------------------------------------------------------------------------------------------------------
TWO_PASS = REPRO + [("quad8", "mixed", 2), ("hex8", "values", 1)]


@pytest.mark.parametrize("fam,form,nf", TWO_PASS, ids=[f"{a}-{b}-{c}f" for a, b, c in TWO_PASS])
def test_direct_against_the_two_pass_form(mf, fam, form, nf):
    import torch

    from metafem_jl_amd import _lib
    from metafem_jl_amd.generic import constant_coefficient

    space, msh, wf, _ = _reference(fam, form, nf)
    n0 = int(_lib.lib.mfem_debug_mesh_rows_count())
    _, K2, rise2 = _assemble(mf, space, msh, nf, wf)
    assert rise2 == 0 and int(_lib.lib.mfem_debug_mesh_rows_count()) - n0 == _element_assemblies(wf)
    gd, K, rise = _assemble(mf, space, msh, nf, wf, direct_rows=True)
    assert rise == _element_assemblies(wf)
    scale = float(K2.abs().max())
    assert float((K - K2).abs().max()) <= TOL * scale
    # the set form on a NaN-filled K: every row is written
    gd.K_linear.fill_(float("nan"))
    gd.K_linear_func()
    assert not bool(torch.isnan(gd.K_linear).any())
    assert torch.equal(gd.K_linear, K)
    # the add form on a prefilled K: prefill + K
    pre = torch.linspace(-1.0, 1.0, K.numel(), dtype=torch.float64, device="cuda") * scale
    Kadd = pre.clone()
    gd._K_fresh = False
    n1 = int(_lib.lib.mfem_debug_mesh_direct_count())
    gd._assemble_const(gd.groups[0], [(t, constant_coefficient(t.fn)) for t in wf.linear_gradients], Kadd)
    assert int(_lib.lib.mfem_debug_mesh_direct_count()) - n1 == _element_assemblies(wf)
    assert float((Kadd - (pre + K)).abs().max()) <= TOL * scale
    assert float((Kadd - pre).abs().max()) > 0.5 * scale


# ---- 4. more batches than resident waves ----------------------------------------------------------------------------------------------------------
def test_persistent_loop_on_more_batches_than_waves(mf, budget):
    """hex-8, three fields, 16^3 elements at the smallest budget (9 * 27 doubles: a batch per interior control point): the waves walk several
    batches each."""
    space, msh, _, _, _ = _mesh("hex8", cells=(16, 16, 16), oracle=False)
    wf = _form("grads", 3, 3, seed=77)
    _, K2, _ = _assemble(mf, space, msh, 3, wf)
    budget(8 * 9 * 27)
    gd, K, rise = _assemble(mf, space, msh, 3, wf, direct_rows=True)
    st = gd.direct_stats()
    print(st)
    assert rise == _element_assemblies(wf) == 2
    assert st["max_control_point_doubles"] == 9 * 27 == st["budget_doubles"]
    assert st["waves_per_trip"] > 0 and st["batches"] > st["waves_per_trip"], st
    assert float((K - K2).abs().max()) <= TOL * float(K2.abs().max())


# ---- 5. no scratch ----------------------------------------------------------------------------------------------------------------------------------
def test_no_element_matrix_scratch(mf):
    """On a fresh context whose first device work is the direct assembly the workspace stays below the 8 nel itp^2 nb bytes the two-pass form
    reserves -- which a second fresh context then does reserve."""
    import torch

    from metafem_jl_amd import _lib

    space, msh, wf, Ko = _reference("hex20", "grads", 3)
    # 81 terms sorted by block go in chunks of 48 and 33: the blocks of a chunk are the scratch the two-pass form reserves for it
    key = lambda t: t.dual_pos * 3 + t.base_pos
    order = sorted(wf.linear_gradients, key=key)
    blocks = [len({key(t) for t in order[c0:c0 + _lib.MAX_BATCH_TERMS]}) for c0 in range(0, len(order), _lib.MAX_BATCH_TERMS)]
    assert blocks == [6, 4]
    scratch = [8 * msh.nel * space.itp ** 2 * nb for nb in blocks]
    for direct in (True, False):
        ctx = mf.Context(torch.cuda.current_device())
        try:
            assert int(_lib.lib.mfem_debug_ws_bytes(ctx._h)) == 0
            gd, K, rise = _assemble(mf, space, msh, 3, wf, ctx=ctx, direct_rows=direct)
            ws = int(_lib.lib.mfem_debug_ws_bytes(ctx._h))
            assert _rel(K.cpu().numpy(), Ko) <= TOL
            if direct:
                assert rise == 2 and ws < min(scratch), (ws, scratch)
            else:
                assert rise == 0 and ws >= max(scratch), (ws, scratch)
            del gd
        finally:
            ctx.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def _plan_create(gd, nf, ranks):
    from metafem_jl_amd import _lib

    h = C.c_uint64()
    rc = _lib.lib.mfem_mesh_direct_plan_create(gd.ctx._h, gd.itp, gd.nel, gd.ncp, nf, gd.A._h, gd._adj_ptr.data_ptr(), gd._adj.data_ptr(),
                                               gd.cp.data_ptr(), 1, ranks.data_ptr(), C.byref(h))
    return rc, h


def _refused(rc, n0, word):
    from metafem_jl_amd import _lib

    msg = _lib.lib.mfem_last_error().decode()
    assert rc == -3, (rc, msg)
    assert word in msg and "mfem_mesh_assemble_elements_rows" in msg, msg
    assert int(_lib.lib.mfem_debug_mesh_direct_count()) == n0  # nothing launched


def test_refusals(mf, budget):
    import torch

    from metafem_jl_amd import _lib, generic as G

    lib = _lib.lib
    n0 = int(lib.mfem_debug_mesh_direct_count())
    # (1) five fields: the plan and the assembly
    space, msh, _, _, _ = _mesh("quad4", oracle=False)
    wf5 = _form("values", 2, 5, 3)
    g5 = _domain(mf, space, msh, 5, wf5)
    ranks = torch.zeros(g5.nel * g5.itp * g5.itp, dtype=torch.int16, device="cuda")
    rc, h = _plan_create(g5, 5, ranks)
    _refused(rc, n0, "5 fields")
    assert not h.value
    arr = (_lib.ConstTerm * 1)(_lib.ConstTerm(0, 0, 0, 0, 1.0))
    K = torch.zeros(g5.A.nnz, dtype=torch.float64, device="cuda")
    rc = lib.mfem_mesh_assemble_elements_direct(g5.ctx._h, 2, space.itg, g5.itp, g5.nel, g5.ncp, g5._ref.data_ptr(), g5._itgw.data_ptr(),
                                                g5.coords.data_ptr(), g5.cp.data_ptr(), 1, 1, arr, 5, g5.A._h, 0, K.data_ptr(), 1)
    _refused(rc, n0, "5 fields")
    assert float(K.abs().max()) == 0.0
    g5.direct_rows = True
    g5.K_linear_func()  # (row ranks refuse five fields first: the scatter form)
    assert g5.direct_rows is False and int(lib.mfem_debug_mesh_direct_count()) == n0
    # (2) one control point beyond the budget
    space, msh, wf, Ko = _reference("hex20", "grads", 3)
    gd = _domain(mf, space, msh, 3, wf)
    rk = gd._row_ranks()
    budget(8 * 9 * 81 - 8)  # (an interior vertex of the 3 x 3 x 2 mesh couples 81 control points)
    rc, h = _plan_create(gd, 3, rk)
    _refused(rc, n0, "budget")
    assert not h.value
    budget(0)
    # (3) an element that lists a control point twice
    cp2 = np.asarray(msh.cp_ids).copy()
    cp2[1, 0] = cp2[0, 0]
    gc = G.GenericDomain(mf.default_context(), space, msh.coords, cp2, 3, wf, [])
    rc, h = _plan_create(gc, 3, torch.zeros(gc.nel * gc.itp * gc.itp, dtype=torch.int16, device="cuda"))
    _refused(rc, n0, "twice")
    assert not h.value
    # (4) a wave block over the LDS cap: hex-27 with 64 Gauss points and every table slot
    space, msh, _, _, _ = _mesh("hex27_64", oracle=False)
    wf = _form("mixed", 3, 1, seed=9)
    gb = _domain(mf, space, msh, 1, wf)
    rc, h = _plan_create(gb, 1, gb._row_ranks())
    assert rc == 0 and h.value
    try:
        terms = sorted(wf.linear_gradients, key=lambda t: t.dual_pos + t.base_pos)
        arr = (_lib.ConstTerm * len(terms))(*[_lib.ConstTerm(t.dual_s, t.base_s, 0, 0, t.fn(None)) for t in terms])
        K = torch.zeros(gb.A.nnz, dtype=torch.float64, device="cuda")
        rc = lib.mfem_mesh_assemble_elements_direct(gb.ctx._h, 3, space.itg, gb.itp, gb.nel, gb.ncp, gb._ref.data_ptr(), gb._itgw.data_ptr(),
                                                    gb.coords.data_ptr(), gb.cp.data_ptr(), 1, len(terms), arr, 1, gb.A._h, h, K.data_ptr(), 1)
        _refused(rc, n0, "LDS")
        assert float(K.abs().max()) == 0.0
    finally:
        _lib.check(lib.mfem_mesh_direct_plan_destroy(h))


def test_collapsed_element_falls_back_to_the_oracles_K(mf):
    """2 x 1 quads, the second collapsed to a triangle (tests/test_gpu_round3_abi.py): the row ranks report the control point listed twice, the
    scatter form serves, K is the oracle's."""
    from metafem_jl_amd import _lib, element
    from oracle import mesh as om, reference_element as re_

    space = element.classical_space(2, "Lagrange", 1, 3)
    coords = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 0.5]])
    cp = np.array([[0, 1, 2, 3], [1, 4, 3, 4]]).T

    class M:
        pass
    msh = M()
    msh.coords, msh.cp_ids, msh.ncp = coords, cp, 5
    wf = _form("mixed", 2, 2, seed=5)
    disc = re_.initialize_classical_element(2, "CUBE", 1, 1, 3, itp_type="Lagrange")
    Ko = _oracle_K(om.ClassicalMesh(2, coords, cp, cp, 5), disc, 2, wf)
    n0 = int(_lib.lib.mfem_debug_mesh_direct_count())
    gd, K, rise = _assemble(mf, space, msh, 2, wf, direct_rows=True)
    assert rise == 0 and gd.direct_rows is False and gd.row_owner is False and int(_lib.lib.mfem_debug_mesh_direct_count()) == n0
    assert _rel(K.cpu().numpy(), Ko) <= TOL
