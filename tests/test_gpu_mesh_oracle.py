"""The unstructured element kernels against the oracle on every element family, field count and kernel variant.

  * K_linear_func through the fused mesh assembly (k_mesh_assemble, csrc/assemble_mesh.hip) -- tri-3/6, quad-4/8/9/16, tet-4/10, hex-8/20/27 with
    seeded constant-coefficient forms (values only, gradients paired with themselves, all gradient pairs, values and gradients mixed) on 1..5 fields
    and the physics forms, under every output form and switch -- against oracle.fem.FEMDomain.K_linear on the same mesh arrays.
  * The residual of K_nonlinear_func through the wave forms of the batched operators (k_op_var_batch_wave / k_op_res_batch_wave, csrc/ops.hip) on
    tet-10, hex-20 and hex-27 against the oracle's term-by-term residual, forced on small meshes and by the production trigger (256+ elements).
  * Which variants of k_mesh_assemble the module launched (mfem_debug_mesh_variants): the last test requires every reachable one.

Meshes: make_Square / make_Brick (CUBE, SIMPLEX) -> element order shuffled in blocks -> mesh_Classical -> every control point moved by a smooth
non-affine map (curved elements; the Jacobian varies over every element but the linear simplices, and stays positive)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (dim, itp_type, itp_order, itg_order, shape, cells)
FAMILIES = {
    "tri3": (2, "Lagrange", 1, 3, "SIMPLEX", (5, 4)),
    "tri6": (2, "Lagrange", 2, 5, "SIMPLEX", (5, 4)),
    "quad4": (2, "Lagrange", 1, 3, "CUBE", (6, 5)),
    "quad8": (2, "Serendipity", 2, 5, "CUBE", (6, 5)),
    "quad9": (2, "Lagrange", 2, 5, "CUBE", (6, 5)),
    "quad16": (2, "Lagrange", 3, 7, "CUBE", (5, 4)),  # the 2-D element of 16 nodes: staged by default, the four-node pair loop with staging off
    "tet4": (3, "Lagrange", 1, 3, "SIMPLEX", (3, 2, 2)),
    "tet10": (3, "Serendipity", 2, 5, "SIMPLEX", (3, 2, 2)),  # tet10_elasticity_64's element and rule (itg 14)
    "tet10_24": (3, "Serendipity", 2, 6, "SIMPLEX", (3, 2, 2)),  # the cylinder script's rule (itg 24)
    "hex8": (3, "Lagrange", 1, 3, "CUBE", (3, 3, 2)),
    "hex20": (3, "Serendipity", 2, 5, "CUBE", (3, 3, 2)),  # staged, the Jacobian sum split over two lane groups (2 * 27 <= 64)
    "hex20_64": (3, "Serendipity", 2, 7, "CUBE", (3, 2, 2)),  # staged, one lane group per Gauss point
    "hex27": (3, "Lagrange", 2, 5, "CUBE", (3, 3, 2)),  # staged tails: odd itp, no 16-byte pair stores
    "hex27_64": (3, "Lagrange", 2, 7, "CUBE", (3, 2, 2)),  # values + gradients: the staged table does not fit its LDS cap
}
FORMS = ("values", "grads-diag", "grads", "mixed")
PATHS = ("default", "scatter", "colours", "stage_all", "stage_off", "term_list", "colours_term_list")
TOL = 1e-12  # |K - K_oracle| <= TOL max |K_oracle|, as tests/test_gpu_u20.py
K_CASES = ([(fam, form, f) for i, fam in enumerate(FAMILIES) for j, form in enumerate(FORMS) for f in [(i + j) % 3 + 1]]
           + [("hex8", "mixed", 4), ("tet10", "mixed", 4), ("quad8", "mixed", 4), ("hex20", "grads", 4),  # 16 blocks; 3-D mixed: 256 terms in 48-term chunks
              # 25 blocks: more runs than the term matrix holds -- the term list walked by the colour and atomic forms, every dimension and mode
              ("tri3", "values", 5), ("quad4", "grads", 5), ("quad8", "mixed", 5), ("tet4", "values", 5), ("hex8", "grads", 5), ("tet10", "mixed", 5),
              ("hex27", "grads-diag", 5)])
PHYSICS = ("thermal", "elasticity")
PHYSICS_PATHS = ("default", "scatter", "colours")

_seen = {"variants": 0, "ran": set()}  # variant bits launched, fused-K cases assembled
_oracle_cache = {}


def _warp(c):
    """Smooth, non-affine, gradient well below 1: every control point moves, elements curve, Jacobians stay positive."""
    dim = c.shape[1]
    out = c.copy()
    for i in range(dim):
        j, k = (i + 1) % dim, (i + 2) % dim
        out[:, i] += 0.05 * np.sin(2.3 * c[:, j] + 1.1 * c[:, k] + 0.4 * i) + 0.04 * c[:, i] * c[:, j]
    return out


def _mesh(fam, cells=None, block=4, seed=11):
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
    fac = pm.get_BoundaryMesh(msh)  # (centroids of the unwarped mesh: the facets of the faces x = 0, y = 0.8 are selected by them)
    msh.coords = _warp(msh.coords)
    disc = re_.initialize_classical_element(dim, shape, order, 1, itg, itp_type=itp_type)
    omesh = om.ClassicalMesh(dim, np.asarray(msh.coords), np.asarray(msh.cp_ids), np.asarray(msh.vert_conn), msh.n_vertices)
    return space, msh, fac, disc, omesh


def _check_geometry(od, fam):
    dim, _, order, _, shape, _ = FAMILIES[fam]
    g = od.elgeo
    assert (g.dets > 0).all(), "a Jacobian is not positive"
    if not (shape == "SIMPLEX" and order == 1):  # (linear simplices are affine whatever the map)
        J = g.jacobian  # [i, X, q, e]
        spread = np.abs(J - J.mean(axis=2, keepdims=True)).max(axis=(0, 1, 2))
        assert (spread > 1e-4).all(), "an element is affine"


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


def _regrade(wf, edit):
    """A copy of wf with its terms rewritten by edit(i, (fd, ds, fb, bs, c)) -> (fd, ds, fb, bs, c)."""
    from metafem_jl_amd.generic import GradTerm, WeakForm

    out = WeakForm()
    for i, t in enumerate(wf.linear_gradients):
        fd, ds, fb, bs, c = edit(i, (t.dual_pos, t.dual_s, t.base_pos, t.base_s, t.fn(None)))
        out.linear_gradients.append(GradTerm(fd, ds, fb, bs, lambda env, c=c: c))
    return out


def _oracle_K(omesh, disc, nf, wf, bnd=()):
    from oracle import fem

    od = fem.FEMDomain(omesh, disc, nf, wf, list(bnd))
    for _, sym, _ in [v for w in [wf] + [b[1] for b in bnd] for v in w.cp_ext_vars]:
        od.controlpoints[sym] = np.zeros(omesh.ncp)
    od.update_time()
    od.K_linear_func()
    return od


def _physics(name, dim, fac):
    """Domain form + boundary groups [(facets, form)]: thermal with a reaction term and convection on every facet; elasticity with lam != mu, a
    penalty wall on the (slanted) face x = 0 and a traction on y = 0.8."""
    import bench_legs as L
    from metafem_jl_amd import physics

    if name == "thermal":
        return 1, physics.thermal_domain(dim, L.K_COND, alpha=0.7, Tenv=300.0), [(fac, physics.thermal_convection(L.H, L.TENV))]
    c = fac.centroid
    return dim, physics.elasticity_domain(dim, 1.7, 0.6), [(fac.select(np.abs(c[:, 0]) < 1e-9), physics.penalty(list(range(dim)), 37.0)),
                                                            (fac.select(np.abs(c[:, 1] - 0.8) < 1e-9), physics.traction(dim, "sl", rows=[1]))]


@pytest.fixture
def path():
    """Set the switches of one assembly path; restore the defaults whatever happens."""
    from metafem_jl_amd import _lib

    def reset():
        _lib.lib.mfem_debug_set_mesh_stage_min_itp(16)
        _lib.lib.mfem_debug_set_mesh_term_matrix(1)

    def set_(name):
        reset()
        if name == "stage_all":
            _lib.lib.mfem_debug_set_mesh_stage_min_itp(1)  # every family staged, 3- and 4-node tails included
        elif name == "stage_off":
            _lib.lib.mfem_debug_set_mesh_stage_min_itp(1000)
        elif name in ("term_list", "colours_term_list"):
            _lib.lib.mfem_debug_set_mesh_term_matrix(0)  # (more than 16 runs in a launch take the term list too: 25 blocks of one or two terms)
        colours = name.startswith("colours")
        return dict(row_owner=name != "scatter" and not colours, element_colours="auto" if colours else None)

    try:
        yield set_
    finally:
        reset()


def _gpu_K(mf, space, msh, nf, wf, bnd, opts, twice=False):
    import torch

    from metafem_jl_amd import _lib, generic as G

    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf,
                         [(f.element_ID, f.element_eindex, w) for f, w in bnd], **opts)
    for _, sym, _ in [v for w in [wf] + [b[1] for b in bnd] for v in w.cp_ext_vars]:
        gd.controlpoints[sym] = torch.zeros(msh.ncp, dtype=torch.float64, device="cuda")
    _lib.lib.mfem_debug_mesh_variants(1)
    rows0 = int(_lib.lib.mfem_debug_mesh_rows_count())
    try:
        gd.update_Time()
        gd.K_linear_func()
        K = gd.K_linear.cpu().numpy()
        rows_ran = int(_lib.lib.mfem_debug_mesh_rows_count()) > rows0
        K2 = None
        if twice:
            gd.K_linear_func()
            K2 = gd.K_linear.cpu().numpy()
    finally:
        _seen["variants"] |= int(_lib.lib.mfem_debug_mesh_variants(1))
    return K, K2, rows_ran


def _degenerate_check(omesh, disc, nf, wf, Ko):
    """The form is not degenerate: one coefficient off by 1e-6 relative, the words of one block transposed, or a pair of off-diagonal blocks each
    replaced by the other's transpose, each moves the oracle's K by more than 100 x the tolerance."""
    rng = np.random.default_rng(7)
    scale = np.abs(Ko).max()
    nterm = len(wf.linear_gradients)
    i0 = int(rng.integers(nterm))
    edits = [lambda i, t: t[:4] + (t[4] * (1 + 1e-6) if i == i0 else t[4],)]
    blk = [(t.dual_pos, t.base_pos) for t in wf.linear_gradients if t.dual_s != t.base_s]
    if blk:
        b0 = blk[int(rng.integers(len(blk)))]
        edits.append(lambda i, t: (t[0], t[3], t[2], t[1], t[4]) if (t[0], t[2]) == b0 else t)
    if nf > 1:
        fd, fb = 0, 1 + int(rng.integers(nf - 1))
        edits.append(lambda i, t: (t[2], t[3], t[0], t[1], t[4]) if (t[0], t[2]) in ((fd, fb), (fb, fd)) else t)  # (blocks fd fb and fb fd swapped)
    for e in edits:
        Kp = _oracle_K(omesh, disc, nf, _regrade(wf, e)).K_linear
        assert np.abs(Kp - Ko).max() > 100 * TOL * scale


def _reference(fam, form, nf):
    key = (fam, form, nf)
    if key not in _oracle_cache:
        space, msh, fac, disc, omesh = _mesh(fam)
        wf = _form(form, space.dim, nf, seed=1000 * nf + 100 * FORMS.index(form) + list(FAMILIES).index(fam))
        od = _oracle_K(omesh, disc, nf, wf)
        _check_geometry(od, fam)
        Ko = od.K_linear
        _degenerate_check(omesh, disc, nf, wf, Ko)
        _oracle_cache[key] = (space, msh, wf, Ko)
    return _oracle_cache[key]


@pytest.mark.parametrize("pname", PATHS)
@pytest.mark.parametrize("fam,form,nf", K_CASES, ids=[f"{a}-{b}-{c}f" for a, b, c in K_CASES])
def test_fused_K_against_the_oracle(mf, path, fam, form, nf, pname):
    space, msh, wf, Ko = _reference(fam, form, nf)
    opts = path(pname)
    K, K2, rows_ran = _gpu_K(mf, space, msh, nf, wf, [], opts, twice=True)
    _seen["ran"].add(("K", fam, form, nf, pname))
    assert K.shape == Ko.shape
    assert np.abs(K).max() > 0
    err = np.abs(K - Ko).max() / np.abs(Ko).max()
    assert err <= TOL, f"{fam} {form} {nf} fields, {pname}: |K - K_oracle| / |K_oracle| = {err:.3e}"
    assert rows_ran == (opts["row_owner"] and nf <= 4)  # 5+ fields: the row-owner form declines, the scatter form takes over
    if rows_ran:
        assert np.array_equal(K, K2), "two row-owner assemblies differ"
    else:
        assert np.abs(K2 - Ko).max() <= TOL * np.abs(Ko).max()


@pytest.mark.parametrize("pname", PHYSICS_PATHS)
@pytest.mark.parametrize("phys", PHYSICS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_physics_forms_against_the_oracle(mf, path, fam, phys, pname):
    """thermal_domain (alpha: value and gradient words, every term on its own word) + convection on every facet; elasticity_domain with lam != mu +
    penalty and traction on facets of two faces -- the facet kernel on edges, triangles and quadrilaterals."""
    from oracle import mesh as om

    space, msh, fac, disc, omesh = _mesh(fam)
    ofac = om.boundary_facets(omesh)
    assert np.array_equal(ofac.element_ID, fac.element_ID) and np.array_equal(ofac.element_eindex, fac.element_eindex)
    nf, wf, bnd = _physics(phys, space.dim, fac)
    assert all(len(f) > 0 for f, _ in bnd)
    od = _oracle_K(omesh, disc, nf, wf, bnd)
    Ko = od.K_linear
    K, _, _ = _gpu_K(mf, space, msh, nf, wf, bnd, path(pname))
    _seen["ran"].add(("P", fam, phys, pname))
    assert np.abs(K).max() > 0
    err = np.abs(K - Ko).max() / np.abs(Ko).max()
    assert err <= TOL, f"{fam} {phys} {pname}: {err:.3e}"


def test_five_fields_take_the_scatter_form(mf):
    """Row ranks and the row-owner assembly decline 5+ fields with MFEM_ERR_UNSUPPORTED (the scatter form's cue), not MFEM_ERR_INVALID."""
    import torch

    from metafem_jl_amd import _lib, generic as G

    space, msh, _, _, _ = _mesh("quad4")
    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, 5, _form("values", 2, 5, 3), [])
    ranks = torch.empty(gd.nel * gd.itp * gd.itp, dtype=torch.int16, device="cuda")
    rc = _lib.lib.mfem_mesh_row_ranks(gd.ctx._h, gd.itp, gd.nel, gd.ncp, 5, gd.A._h, gd._adj_ptr.data_ptr(), gd._adj.data_ptr(), gd.cp.data_ptr(), 1,
                                      ranks.data_ptr())
    assert rc == -3
    gd.K_linear_func()
    assert gd.row_owner is False


# ---- wave forms of the batched operators ----------------------------------------------------------------------------------------------------------------
BIG_CELLS = {"tet10": (4, 4, 4), "tet10_24": (4, 4, 4), "hex20": (7, 7, 6), "hex27": (7, 7, 6)}  # 320 / 320 / 294 / 294 elements


def _res_form(dim, nf, n_res, extra_var, words, seed):
    """inner variables: words lo..hi of every field (+ word hi of field 0 once more when extra_var); residues: n_res seeded linear combinations of
    all of them and a control-point external g, on seeded (field, word) duals within lo..hi (the first two on hi and lo: the slab range of both
    kernels is lo..hi); a values-only linear gradient per block (the pattern)."""
    from metafem_jl_amd.generic import GradTerm, ResTerm, WeakForm

    lo, hi = words
    rng = np.random.default_rng(seed)
    wf = WeakForm()
    for f in range(nf):
        for s in range(lo, hi + 1):
            wf.inner_vars.append((f"u{f}_{s}", f, s, 0))
    if extra_var:
        wf.inner_vars.append(("u0_x", 0, hi, 0))
    wf.cp_ext_vars.append(("g", "g", 0))
    names = [v[0] for v in wf.inner_vars] + ["g"]
    for r in range(n_res):
        c = rng.uniform(0.5, 1.5, len(names)) * rng.choice([-1.0, 1.0], len(names))
        ds = hi if r == 0 else lo if r == 1 else int(rng.integers(lo, hi + 1))
        wf.residues.append(ResTerm(int(rng.integers(nf)), ds, lambda env, c=c: sum(float(ci) * env[n] for ci, n in zip(c, names))))
    for fd in range(nf):
        for fb in range(nf):
            wf.linear_gradients.append(GradTerm(fd, 0, fb, 0, lambda env: 1.0))
    return wf


def _wave_blocks(fam, wf):
    """{kernel: (LDS doubles per wave before rounding, whether mfem_op_*_batch takes the wave form)} for the residual call and the inner-variable
    call of wf -- the host arithmetic and gate of ops.hip (mfem_op_res_batch / mfem_op_var_batch: U.n itg itp + n_terms itg | itp, rounded up to
    even, four waves in 80 KB, at most 64 terms; 10 to 64 nodes (res) / up to 64 Gauss points (var))."""
    from metafem_jl_amd import element

    dim, itp_type, order, itg, shape, _ = FAMILIES[fam]
    sp = element.classical_space(dim, itp_type, order, itg, shape=shape)
    out = {}
    for kernel, words, per_term, fits in (("res", [r.dual_s for r in wf.residues], sp.itg, sp.itp <= 64),
                                          ("var", [v[2] for v in wf.inner_vars], sp.itp, sp.itg <= 64)):
        raw = (max(words) - min(words) + 1) * sp.itg * sp.itp + len(words) * per_term
        out[kernel] = (raw, sp.itp >= 10 and fits and len(words) <= 64 and 8 * ((raw + 1) & ~1) * 4 <= 80 * 1024)
    return out


# (family, fields, residues, extra inner variable, words): hex-27 (itg = itp = 27) takes the wave forms with a slab range of three words at most --
# four words are 2916 + 27 n doubles per wave, over the 80 KB of four waves
WAVE_CASES = ([(fam, nf, n_res, extra, (0, 3)) for fam in ("tet10", "tet10_24", "hex20")
               for nf, n_res, extra in ((1, 3, False), (1, 4, True), (3, 5, True), (3, 6, False))]
              + [("hex27", 1, 3, False, (0, 2)), ("hex27", 1, 4, True, (1, 3)), ("hex27", 3, 5, True, (1, 3)), ("hex27", 3, 6, False, (0, 2))])
BIG_CELLS = {"tet10": (4, 4, 4), "tet10_24": (4, 4, 4), "hex20": (7, 7, 6), "hex27": (7, 7, 6)}  # 320 / 320 / 294 / 294 elements


def _wave_seed(nf, n_res):
    return 31 * nf + n_res


def test_wave_cases_have_odd_and_even_lds_blocks():
    """Every case below takes the wave form in both kernels, and between them the cases give each kernel an odd per-wave block (before rounding:
    the blocks that are not 16-byte aligned without it) and an even one."""
    blocks = {c: _wave_blocks(c[0], _res_form(FAMILIES[c[0]][0], c[1], c[2], c[3], c[4], _wave_seed(c[1], c[2]))) for c in WAVE_CASES}
    assert all(ok for b in blocks.values() for _, ok in b.values()), blocks
    for kernel in ("res", "var"):
        assert {b[kernel][0] & 1 for b in blocks.values()} == {0, 1}, (kernel, blocks)


@pytest.mark.parametrize("trigger", ["forced", "default"])
@pytest.mark.parametrize("coloured", [False, True], ids=["atomic", "coloured"])
@pytest.mark.parametrize("fam,nf,n_res,extra,words", WAVE_CASES,
                         ids=[f"{a}-{b}f-{c}res{'-x' if d else ''}-w{e[0]}{e[1]}" for a, b, c, d, e in WAVE_CASES])
def test_wave_form_residual_against_the_oracle(mf, fam, nf, n_res, extra, words, coloured, trigger):
    """R of K_nonlinear_func at a seeded x* against the oracle's term-by-term residual.  forced: mfem_debug_set("op_wave_forms", 2) on a small mesh;
    default: the switches untouched on a mesh of 256+ elements (the production trigger).  Both calls of the inner variables / external and the
    residual call must take the wave forms (mfem_debug_op_wave_count)."""
    import torch

    from metafem_jl_amd import _lib, generic as G
    from oracle import fem

    space, msh, _, disc, omesh = _mesh(fam, cells=None if trigger == "forced" else BIG_CELLS[fam], block=8)
    if trigger == "default":
        assert msh.nel >= 256 and space.itp >= 10  # (ops.hip: g_op_wave_min_itp 10, 256 items)
    wf = _res_form(space.dim, nf, n_res, extra, words, _wave_seed(nf, n_res))
    od = fem.FEMDomain(omesh, disc, nf, wf, [])
    _check_geometry(od, fam)
    rng = np.random.default_rng(5 + nf)
    xs = rng.standard_normal(nf * msh.ncp)
    g = 1.0 + msh.coords[:, 0] * msh.coords[:, 1]
    od.controlpoints["g"] = g
    od.update_time()
    od.K_linear_func()
    od.x_star[:xs.size] = xs
    od.K_nonlinear_func()
    try:
        if trigger == "forced":
            _lib.lib.mfem_debug_set_op_wave_forms(2)
        gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, nf, wf, [], element_colours="auto" if coloured else None)
        gd.controlpoints["g"] = torch.tensor(g, device="cuda")
        gd.update_Time()
        gd.K_linear_func()
        gd.x_star[:xs.size] = torch.tensor(xs, device="cuda")
        var0, res0 = int(_lib.lib.mfem_debug_op_wave_count(0)), int(_lib.lib.mfem_debug_op_wave_count(1))
        gd.K_nonlinear_func()
        got = gd.residue.cpu().numpy()
        ran = int(_lib.lib.mfem_debug_op_wave_count(0)) - var0, int(_lib.lib.mfem_debug_op_wave_count(1)) - res0
    finally:
        _lib.lib.mfem_debug_set_op_wave_forms(1)
    assert ran == (2, 1), f"wave-form calls (var, res) = {ran}: expected the inner variables, the external and the residual"
    assert np.abs(od.residue).max() > 0
    err = np.abs(got - od.residue).max() / np.abs(od.residue).max()
    assert err <= 1e-11, f"{fam} {nf} fields {n_res} residues: {err:.3e}"


# ---- variant coverage (last: the union over the module) ----------------------------------------------------------------------------------------------
KINDS = ("colour-tm", "colour-list", "atomic-tm", "atomic-list", "rows-tm", "rows-list", "rows-4", "staged", "staged-diag")  # mfem_debug_mesh_variants
MODES = ("mixed", "grads", "values")  # ma_launch's mode 0 / 1 / 2
# every (dim, mode, kind) ma_launch can reach, in 2-D and 3-D (the 2-D four-node pair loop needs quad-16): all but the staged non-diagonal form of a
# values-only form (its one word pairs with itself)
EXPECTED = {(dim, mode, kind) for dim in (2, 3) for mode in MODES for kind in KINDS} - {(2, "values", "staged"), (3, "values", "staged")}


def _decode(mask):
    out = set()
    for bit in range(64):
        if mask >> bit & 1:
            grp, kind = divmod(bit, len(KINDS))
            assert grp < 6, f"unknown variant bit {bit}"
            out.add((2 + grp // 3, MODES[grp % 3], KINDS[kind]))
    return out


def test_every_mesh_assembly_variant_ran(mf, path):
    """The union of the variants over the fused-K cases.  A case this session did not assemble (deselected, or failed before its assembly) is
    assembled here, without the oracle: the check does not depend on which tests ran or in what order."""
    for fam, form, nf in K_CASES:
        for pname in PATHS:
            if ("K", fam, form, nf, pname) not in _seen["ran"]:
                space, msh, wf, _ = _reference(fam, form, nf)
                _gpu_K(mf, space, msh, nf, wf, [], path(pname))
    for fam in FAMILIES:
        for phys in PHYSICS:
            for pname in PHYSICS_PATHS:
                if ("P", fam, phys, pname) not in _seen["ran"]:
                    space, msh, fac, _, _ = _mesh(fam)
                    nf, wf, bnd = _physics(phys, space.dim, fac)
                    _gpu_K(mf, space, msh, nf, wf, bnd, path(pname))
    got = _decode(_seen["variants"])
    assert got == EXPECTED, (sorted(EXPECTED - got), sorted(got - EXPECTED))
