"""GPU parity of the hex-27 (Lagrange-2) thermal kernels with the oracle on every face, at every quadrature rule, at the sizes where
their tiles end, on mixed meshes at the ends of the element list, on slabs and away from the origin.

tests/test_gpu_hex27.py, the five order-2 rows of tests/test_gpu_nitsche.py and tests/test_gpu_slab.py compare a handful of configurations
with the oracle.  Here, laid out like tests/test_gpu_thermal_edges.py: each face alone as the Robin and as the fixed (Nitsche) face, at
h_penalty = 1000 and at h_penalty = 1 (where the k n_i T_;i term is not hidden below a tolerance scaled by the penalty entries), opposite
pairs and corners (part A); itg_order 0 to 7, i.e. 1 to 4 Gauss points per direction (part B); bricks whose element, row and lattice counts
end on, one short of and one past a tile of every kernel, and the two lattices on either side of D27_TAB (part C); meshes with 1, 8, 9, 64
and 65 distorted elements under the forced per-element choice (part D); slabs of a distorted brick with both boundary terms against the rows
of the whole brick, bit for bit (part E); a brick translated by (1024, -333, 77.7) (part F).  The oracle's own order-2 face numbering,
normal and boundary forms are pinned without the product in tests/test_oracle_hex27_faces.py.

Matrix paths per case, by the "hex27" knob word and what h27_path (csrc/hex27_decide.h) makes of it: 0 the default (direct on all-affine
meshes, rows from G_q on distorted meshes with three Gauss points per direction, two-pass otherwise); 1 << 9 the two-pass ring (no count is
taken); (1 << 9) | 1 | (1 << 16) the ring with one element plane per chunk; (1 << 11) | (100 << 24) the per-element choice forced (distorted
meshes only); 2 FP64 atomics; 3 colour scatter.  Which path ran is asserted through the three counters.  Residual paths: 0 (affine shortcut
where the element is affine) and 1 << 8 (general branch everywhere).  Tolerances are the project's for hex-27: K to 1e-12 max|K_oracle|, R to
1e-11 max|R_oracle|, every path against the two-pass path to 2e-13 max|K|, R knob 0 against R knob 1 << 8 to 1e-12 max|R|; a second call
gives the same bits on every path but the atomics; without a fixed face K is symmetric to 1e-13 max|K|, with one it is not (beyond 1e-6
max|K|) and the asymmetric rows lie within two lattice points of the fixed faces.  Every comparison prints its figure (relative to its
tolerance) before it asserts.

Part E, bitwise on a distorted brick: every path builds a row from the Ke (or G_q) of the elements around it in an order that depends on
the row's place in its element neighbourhood only -- the gather and the row owners walk a row's elements in lattice order, the ring only
changes which launch has written them -- so where a slab starts changes which workgroup computes a row, not the order of its sum.  The
face kernels add to a row in the order (direction, side, colour, face element), and the Nitsche kernel after them, which a slab does not
change.

Which case closes which gap: the one-sided face launches of every direction and side, and the residual form of the face kernel on each
of them: part A, each face alone; the slab branch of an x face with one side only: part E, fixed x1 (Robin x0|z0); a tangential extent of
one element (three of the four colour classes empty) without all faces: part C, fixed x0|y1 on (1, 1, 1), (1, 1, 3) and (257, 1, 1); one
Gauss point per direction and the general residual branch with faces away from three: part B; a fixed face alone, at h_penalty = 1, under
every matrix path and on slabs: parts A and E.  No case exceeded a tolerance: neither a kernel nor a tolerance had to change.

Largest printed figure per part, as a fraction of its tolerance (MI355X; the figures print with three decimals):
  A  K 0.003 (no fixed face), 0.003 (fixed, h_penalty = 1000), 0.002 (fixed, h_penalty = 1); paths against two-pass 0.005; K - K^T 0.002;
     R 0.003 (s = None, Robin y1), R shortcut against general below 0.0005
  B  K 0.016 (itg = 2, distorted), paths against two-pass 0.002, R 0.002, R shortcut against general below 0.0005
  C  K 0.132 (n = (257, 1, 1), distorted, fixed x0|y1), paths against two-pass 0.005, K - K^T 0.005, R 0.012, R shortcut against general 0.029
     (n = (257, 1, 1), uniform); the two D27_TAB bricks: direct against two-pass 0.010 of 1e-13, against the oracle 0.237
  D  K 0.017 (one distorted element), forced choice against two-pass 0.001
  E  whole brick against the oracle K 0.003, R below 0.0005; the slabs are bitwise
  F  K 0.258, R 0.060 of max(tolerance, 4 d_ref); R shortcut against general 0.048

Part F (n = (3, 2, 1), x = (3, 1, 2), translation (1024, -333, 77.7); relative to max|K_oracle| and max|R_oracle| on the untranslated brick):
  d_ref (the oracle translated against the oracle untranslated): distorted K 4.7e-13, R 3.8e-13; sheared K 5.5e-13, R 5.8e-13
  every matrix path against the oracle on the translated coordinates: distorted 4.8e-13 = 1.03 d_ref, sheared 5.6e-13 = 1.02 d_ref;
  both residual paths: distorted 3.8e-13 = 1.01 d_ref, sheared 6.0e-13 = 1.03 d_ref
"""
import numpy as np
import pytest

from test_gpu_elasticity_edges import FACE_NAMES, FACE_NORMAL, SHEAR, _bits, _close, _ids
from test_gpu_thermal import _distort

gpu = pytest.mark.gpu

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
TW = 1173.15
HP_REF, HP_ONE = 1000.0, 1.0
X = (3.0, 1.0, 2.0)
K_TOL, R_TOL = 1e-12, 1e-11   # against the oracle
PATH_TOL = 2e-13              # a matrix path against the two-pass path
RR_TOL = 1e-12                # the residual's affine shortcut against its general branch
SYM_TOL = 1e-13
ALL = "|".join(FACE_NAMES)
TWO_PASS, RING_1, CHOICE, ATOMICS, COLOUR = 1 << 9, (1 << 9) | 1 | (1 << 16), (1 << 11) | (100 << 24), 2, 3
K_PATHS = (("default", 0), ("two-pass", TWO_PASS), ("ring of 1 plane", RING_1), ("forced choice", CHOICE), ("atomics", ATOMICS), ("colour scatter", COLOUR))
R_PATHS = (("R shortcut", 0), ("R general", 1 << 8))


class _Knob:
    """mfem_debug_set_hex27(v) for the block, 0 afterwards."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_hex27(self.v)

    def __exit__(self, *exc):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_hex27(0)
        return False


def _counts():
    """(direct, per-element choice, rows from G_q) assemblies so far."""
    from metafem_jl_amd import _lib

    lib = _lib.lib
    return np.array([lib.mfem_debug_hex27_direct_count(), lib.mfem_debug_hex27_mixed_count(), lib.mfem_debug_hex27_rows_count()])


def _expected_counts(knob, general, ng):
    """What one assembly adds to _counts(): on an all-affine mesh (general False) or on a mesh whose elements are all distorted."""
    if knob == 0:
        return (1, 0, 0) if not general else ((0, 0, 1) if ng == 3 else (0, 0, 0))
    if knob == CHOICE:
        assert general
        return (0, 1, 0)
    return (0, 0, 0)


def _fields(ncp, seed=1):
    """x_star = 300 + 20 randn and a non-constant source."""
    rng = np.random.default_rng(seed)
    return 300.0 + 20.0 * rng.standard_normal(ncp), SRC * (1.0 + 0.1 * rng.standard_normal(ncp))


_ORACLE = {}


def _oracle(x, n, robin="", fixed="", hp=HP_REF, itg=5, shape="distorted", coords=None, src=True, h=H):
    """The oracle's K_linear and residue at _fields() on the order-2 brick for Robin faces `robin` and fixed faces `fixed`; computed once per
    configuration and shared (nobody writes to it).  `coords` (with `shape` as its name) overrides the named shapes."""
    from oracle import fem, mesh as om, problems, reference_element as re_

    key = (x, n, robin, fixed, hp, itg, shape, src, h)
    if key in _ORACLE:
        return _ORACLE[key]
    disc = re_.initialize_classical_element(3, "CUBE", 2, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    if coords is not None:
        msh.coords[:] = coords
    elif shape == "distorted":
        msh.coords[:] = _distort(msh.coords)
    elif shape == "sheared":
        msh.coords[:] = msh.coords @ SHEAR.T + np.array([0.3, -0.2, 0.1])
    else:
        assert shape == "uniform"
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = []
    if robin:
        bnd.append((fac.select(np.isin(fac.element_eindex, _ids(robin))), problems.thermal_convection(h, TENV)))
    if fixed:
        bnd.append((fac.select(np.isin(fac.element_eindex, _ids(fixed))), problems.thermal_fixed(3, hp, TW, K_COND)))
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, K_COND), bnd)
    xs, s = _fields(msh.ncp)
    od.controlpoints["s"] = s if src else np.zeros(msh.ncp)
    od.update_time()
    od.K_linear_func()
    od.x_star[:] = xs
    od.K_nonlinear_func()
    _ORACLE[key] = od
    return od


def _brick(mf, x, n, itg, coords=None):
    import torch

    brick = mf.make_Brick(x, n, 2, itg)
    if coords is not None:
        for d in range(3):
            brick.coords_view(d).copy_(torch.tensor(np.ascontiguousarray(coords[:, d]), device="cuda"))
    return brick


def _csr(K, A):
    import scipy.sparse as sp

    return sp.csr_matrix((K, A.colidx.cpu().numpy(), A.rowptr.cpu().numpy()), shape=(A.n, A.n))


def _asymmetry(K, A):
    D = _csr(K, A)
    D = (D - D.T).tocoo()
    return D.row[D.data != 0.0], (np.abs(D.data).max() if D.nnz else 0.0)


def _near(n, names):
    """Control points on, or within two lattice points (one element) of, one of the named faces."""
    idx = np.indices([2 * v + 1 for v in n]).reshape(3, -1)
    near = np.zeros(idx.shape[1], dtype=bool)
    for f in names.split("|"):
        nd, sign = FACE_NORMAL[f]
        near |= (idx[nd] >= 2 * n[nd] - 2) if sign > 0 else (idx[nd] <= 2)
    return near


def _check_symmetry(A, K, n, fixed, label):
    """No fixed face: K symmetric to 1e-13 max|K|.  A fixed face makes K nonsymmetric, in the rows of the nodes on that face and of their
    element neighbours only."""
    rows, amax = _asymmetry(K, A)
    kmax = np.abs(K).max()
    if not fixed:
        print(f"SYMMETRY {label}: {amax / (SYM_TOL * kmax):.3f} of tol (max|K - K^T| {amax:.3e}, max|K| {kmax:.3e})")
        assert amax <= SYM_TOL * kmax, label
        return
    big = np.zeros(A.n, dtype=bool)
    D = _csr(K, A)
    D = (D - D.T).tocoo()
    big[D.row[np.abs(D.data) > SYM_TOL * kmax]] = True
    print(f"ASYMMETRY {label}: max {amax:.3e} ({amax / kmax:.2e} of max|K|), {int(big.sum())} rows beyond round-off")
    assert amax > 1e-6 * kmax, label
    assert np.all(_near(n, fixed)[big]), label


def _all_paths(mf, brick, od, n, robin, fixed, hp, label, itg=5, general=True, src=True, h=H, k_tol=K_TOL, r_tol=R_TOL, path_tol=PATH_TOL,
               rr_tol=RR_TOL):
    """K from every matrix path and R from both residual paths, each against the oracle and each called twice (same bits, but for the
    atomics); which path ran; every matrix path against the two-pass path; the two residual paths against each other; the symmetry of K.
    `general`: every element of the mesh is distorted (else: every element is affine).  Returns the arrays by (letter, knob)."""
    import torch

    A = brick.pattern(1)
    assert np.array_equal(A.rowptr.cpu().numpy(), od.pattern.rowptr) and np.array_equal(A.colidx.cpu().numpy(), od.pattern.colidx)
    ng = (itg + 2) // 2
    rb, fb = _bits(mf, robin), _bits(mf, fixed)
    kw = dict(fixed_faces=fb, h_penalty=hp, Tw=TW)
    xs_np, s_np = _fields(brick.ncp)
    xs = torch.tensor(xs_np, device="cuda")
    s = torch.tensor(s_np, device="cuda") if src else None
    out = {}
    for name, knob in K_PATHS:
        if knob == CHOICE and not general:
            continue
        with _Knob(knob):
            before = _counts()
            got = brick.assemble_thermal(A, K_COND, h, TENV, rb, **kw).cpu().numpy()
            again = brick.assemble_thermal(A, K_COND, h, TENV, rb, **kw).cpu().numpy()
            moved = _counts() - before
        assert tuple(moved) == tuple(2 * v for v in _expected_counts(knob, general, ng)), f"{label} {name}: another path ran: {moved}"
        _close(f"{label} K {name}", got, od.K_linear, k_tol)
        if knob == ATOMICS:
            _close(f"{label} K {name} again", again, od.K_linear, k_tol)
        else:
            assert np.array_equal(got, again), f"{label} K {name}: a second call gives other bits"
        _check_symmetry(A, got, n, fixed, f"{label} K {name}")
        out["K", knob] = got
    for name, knob in K_PATHS:
        if ("K", knob) in out and knob != TWO_PASS:
            _close(f"{label} K {name} vs two-pass", out["K", knob], out["K", TWO_PASS], path_tol)
    for name, knob in R_PATHS:
        with _Knob(knob):
            got = brick.residual_thermal(xs, K_COND, h, TENV, rb, s=s, **kw).cpu().numpy()
            again = brick.residual_thermal(xs, K_COND, h, TENV, rb, s=s, **kw).cpu().numpy()
        _close(f"{label} {name}", got, od.residue, r_tol)
        assert np.array_equal(got, again), f"{label} {name}: a second call gives other bits"
        out["R", knob] = got
    _close(f"{label} R shortcut vs general", out["R", 0], out["R", 1 << 8], rr_tol)
    return out


# ---- A. every face, both boundary terms, every path --------------------------------------------------------------------------------
N_A = (3, 2, 1)  # every direction sees tangential extents of 1, 2 and 3 elements: colour counts 1/0, 1/1 and 2/1 in h27_face_schedule


def REST_OF(fixed):
    return "|".join(f for f in FACE_NAMES if f not in fixed.split("|"))


CASES_A = ([(f, "", HP_REF) for f in FACE_NAMES]                                      # 1. each face alone as the Robin face: every one-sided launch
           + [("", f, hp) for f in FACE_NAMES for hp in (HP_REF, HP_ONE)]             # 2. each face alone as the fixed face
           + [("x0|x1", "", HP_REF), ("y0|y1", "", HP_REF), ("z0|z1", "", HP_REF)]    # 3. opposite pairs: the side = -1 launch
           + [("x1|y0|z1", "x0", HP_ONE), (REST_OF("x0|y1|z0"), "x0|y1|z0", HP_ONE)]  # 4. both corners
           + [("", ALL, HP_ONE)])                                                     # 5. all six fixed


@gpu
@pytest.mark.parametrize("robin,fixed,hp", CASES_A, ids=[f"robin[{r}]-fixed[{f}]-hp{int(p)}" for r, f, p in CASES_A])
def test_faces_against_the_oracle(mf, robin, fixed, hp):
    """Every case: K on every matrix path, R on both residual paths, and R once more without a source vector (s = None)."""
    od = _oracle(X, N_A, robin, fixed, hp)
    brick = _brick(mf, X, N_A, 5, od.mesh.coords)
    label = f"A robin[{robin}] fixed[{fixed}] hp={hp:g}"
    _all_paths(mf, brick, od, N_A, robin, fixed, hp, label)
    import torch

    o0 = _oracle(X, N_A, robin, fixed, hp, src=False)
    xs = torch.tensor(_fields(brick.ncp)[0], device="cuda")
    kw = dict(fixed_faces=_bits(mf, fixed), h_penalty=hp, Tw=TW)
    R = {}
    for name, knob in R_PATHS:
        with _Knob(knob):
            R[knob] = brick.residual_thermal(xs, K_COND, H, TENV, _bits(mf, robin), s=None, **kw).cpu().numpy()
        _close(f"{label} s=None {name}", R[knob], o0.residue, R_TOL)
    _close(f"{label} s=None R shortcut vs general", R[0], R[1 << 8], RR_TOL)


@gpu
@pytest.mark.parametrize("shape", ["distorted", "uniform"])
@pytest.mark.parametrize("what", ["robin_bits_h_zero", "h_without_bits"])
def test_a_disabled_robin_term_is_no_term(mf, what, shape):
    """Bits without a coefficient and a coefficient without bits launch no face kernel (h27_face_schedule returns no launch): the oracle
    without the term, and bitwise the product's own no-face result."""
    od = _oracle(X, N_A, shape=shape)
    brick = _brick(mf, X, N_A, 5, od.mesh.coords)
    general = shape == "distorted"
    plain = _all_paths(mf, brick, od, N_A, "", "", 0.0, f"A6 {what} {shape} plain", general=general, h=0.0)
    h, robin = {"robin_bits_h_zero": (0.0, ALL), "h_without_bits": (H, "")}[what]
    got = _all_paths(mf, brick, od, N_A, robin, "", 0.0, f"A6 {what} {shape}", general=general, h=h)
    for key in plain:
        if key != ("K", ATOMICS):
            assert np.array_equal(got[key], plain[key]), (what, key)


# ---- B. every quadrature rule ----------------------------------------------------------------------------------------------------
N_B, FIXED_B = (2, 1, 2), "x0"
ROBIN_B = REST_OF(FIXED_B)
_PRODUCT_B = {}


def _rule(mf, itg, shape):
    """Part B's arrays of one (order, shape), computed (and compared with the oracle) once."""
    if (itg, shape) not in _PRODUCT_B:
        od = _oracle(X, N_B, ROBIN_B, FIXED_B, HP_ONE, itg=itg, shape=shape)
        assert od.elgeo.integral_weights.shape[0] == ((itg + 2) // 2) ** 3
        brick = _brick(mf, X, N_B, itg, od.mesh.coords)
        _PRODUCT_B[itg, shape] = _all_paths(mf, brick, od, N_B, ROBIN_B, FIXED_B, HP_ONE, f"B itg={itg} {shape}", itg=itg, general=shape == "distorted")
    return _PRODUCT_B[itg, shape]


@gpu
@pytest.mark.parametrize("shape", ["distorted", "uniform"])
@pytest.mark.parametrize("itg", range(8))
def test_quadrature_rules_against_the_oracle(mf, itg, shape):
    """ng = (itg + 2) // 2 = 1, 1, 2, 2, 3, 3, 4, 4 Gauss points per direction.  ng = 1: three of the four Gauss points of the only MFMA
    k-group are padding.  The rows counter moves at ng = 3 on the distorted brick only (asserted by _all_paths through _expected_counts)."""
    _rule(mf, itg, shape)


@gpu
@pytest.mark.parametrize("shape", ["distorted", "uniform"])
@pytest.mark.parametrize("itg", [0, 2, 4, 6])
def test_the_two_orders_of_one_rule_give_the_same_bits(mf, itg, shape):
    a, b = _rule(mf, itg, shape), _rule(mf, itg + 1, shape)
    assert a.keys() == b.keys()
    for key in a:
        if key != ("K", ATOMICS):
            assert np.array_equal(a[key], b[key]), (itg, shape, key)


# ---- C. where tiles end ------------------------------------------------------------------------------------------------------------
CASES_C = [(1, 1, 1), (1, 1, 3), (2, 2, 4), (2, 3, 5), (3, 3, 1), (13, 2, 2), (4, 4, 4), (13, 5, 1), (9, 7, 1), (8, 8, 4), (17, 5, 3), (257, 1, 1)]
FIXED_C = "x0|y1"
ROBIN_C = REST_OF(FIXED_C)
N_TAB = [(505, 3, 2), (506, 3, 2)]
# the tile constants, with the line they come from
H27_WAVES = 8          # csrc/hex27_decide.h: #define H27_WAVES 8 (waves = elements per workgroup and launch of k_hex27)
G27_NODES = 32         # csrc/hex27_decide.h: #define G27_NODES 32 (control points per workgroup of k_hex27_gather_lds)
D27_NODES, D27_TRIP = 64, 8  # csrc/hex27_decide.h: #define D27_NODES (8 * D27_WAVES), D27_WAVES 8: 8 rows per trip of the block's 8 waves
GQ_WAVE, GQ_BLOCK = 64, 256  # csrc/hex27_rows.hip: e_wave = (int64_t)blockIdx.x * 256 + wv * 64 (k_hex27_gq_lane)
G0_BLOCK = 256         # csrc/hex27_direct.hip: k_hex27_affine_g0, __launch_bounds__(MFEM_BLOCK), one element per thread
R27_TILE = 4           # csrc/hex27_decide.h: h27_rows_grid, tiles of 4 x 4 x 4 control points
FACE_BLOCK, FACE_NODES = 256, 9  # csrc/hex27_decide.h: #define H27_FACE_BLOCK 256 (= MFEM_BLOCK); nthreads = n1 * n2 * 9 * (side < 0 ? 2 : 1)
D27_TAB = 1024         # csrc/hex27_direct.hip: #define D27_TAB 1024


def _face_schedule(robin, n):
    """h27_face_schedule of csrc/hex27_decide.h, transcribed: (nd, side, colour, face elements, threads) per launch; robin by face names."""
    out = []
    for nd, (lo, hi) in enumerate((("x0", "x1"), ("y0", "y1"), ("z0", "z1"))):
        lo, hi = lo in robin.split("|"), hi in robin.split("|")
        t1, t2 = (nd + 1) % 3, (nd + 2) % 3
        for side in ((-1,) if lo and hi else (0,) * lo + (1,) * hi):
            for colour in range(4):
                n1, n2 = (n[t1] - (colour & 1) + 1) >> 1, (n[t2] - (colour >> 1) + 1) >> 1
                if n1 > 0 and n2 > 0:
                    out.append((nd, side, colour, n1 * n2, n1 * n2 * FACE_NODES * (2 if side < 0 else 1)))
    return out


def _colour_counts(n):
    return [((n[0] - (c & 1) + 1) >> 1) * ((n[1] - ((c >> 1) & 1) + 1) >> 1) * ((n[2] - (c >> 2) + 1) >> 1) for c in range(8)]


def test_part_c_covers_the_tile_ends():
    """(CPU arithmetic.)  The sizes of part C meet every kernel's tile at its end, one short of it where the odd lattice counts allow, and
    one past it."""
    nel = {int(np.prod(n)) for n in CASES_C}
    rows = {int(np.prod([2 * v + 1 for v in n])) for n in CASES_C}
    assert all(r % 2 == 1 for r in rows)  # (a row count is a product of odd numbers: no row tile ends on its last row)
    # k_hex27_gq_lane: 64 elements per wave, 256 per block; k_hex27_affine_g0: 256 per block
    assert {GQ_WAVE - 1, GQ_WAVE, GQ_WAVE + 1, GQ_BLOCK - 1, GQ_BLOCK, GQ_BLOCK + 1} <= nel and GQ_BLOCK == G0_BLOCK
    # k_hex27: a wave per element, 8 per workgroup, over one colour (colour scatter, residual), all elements (atomics, two-pass) or one element
    # plane (the ring of one plane)
    walks = set()
    for n in CASES_C:
        walks |= set(_colour_counts(n)) | {int(np.prod(n)), n[1] * n[2]}
    assert {1, H27_WAVES - 1, H27_WAVES, H27_WAVES + 1} <= walks
    assert any(0 in _colour_counts(n) for n in CASES_C)  # a colour without an element: no launch
    # k_hex27_gather_lds: 32 rows per workgroup; k_hex27_direct: 64 rows per block, 8 per trip -- one short of and one past a tile
    assert {G27_NODES - 1, 1} <= {r % G27_NODES for r in rows} and any(r < G27_NODES for r in rows)
    assert {D27_NODES - 1, 1} <= {r % D27_NODES for r in rows} and any(r < D27_NODES for r in rows)
    assert {D27_TRIP - 1, 1} <= {r % D27_TRIP for r in rows}
    assert 63 in rows and 225 in rows and 385 in rows  # 2 * 32 - 1 = 64 - 1, 7 * 32 + 1, 6 * 64 + 1
    # k_hex27_rows_gq: 4 x 4 x 4 control points per tile: 3, 5, 7 and 9 lattice points in every direction
    for d in range(3):
        assert {R27_TILE - 1, R27_TILE + 1, 2 * R27_TILE - 1, 2 * R27_TILE + 1} <= {2 * n[d] + 1 for n in CASES_C}, d
    # k_hex27_faces: 256 threads at 9 per face element: one block and several; a launch whose last face element just fits the first block and one
    # whose first block ends inside a face element's threads (252 and 270 of a two-sided launch); one-sided launches on every side
    launches = [L for n in CASES_C for robin in (ALL, ROBIN_C) for L in _face_schedule(robin, n)]
    threads = {L[4] for L in launches}
    assert any(FACE_BLOCK - 2 * FACE_NODES < t <= FACE_BLOCK for t in threads) and any(FACE_BLOCK < t <= FACE_BLOCK + 2 * FACE_NODES for t in threads)
    assert min(threads) == FACE_NODES and max(threads) > 4 * FACE_BLOCK
    assert {(0, 1), (1, 0), (2, -1)} <= {(L[0], L[1]) for L in launches}
    assert {(nd, side) for f in FACE_NAMES for (nd, side, *_r) in _face_schedule(f, N_A)} == {(nd, side) for nd in range(3) for side in (0, 1)}
    for nd in range(3):  # part A: tangential extents 1, 2, 3: colour classes 1/0 (three of four empty), 1/1, 2/1
        assert sorted(N_A[t] for t in range(3) if t != nd) in ([1, 2], [1, 3], [2, 3])
    assert len(_face_schedule("x0", N_A)) == 2 and len(_face_schedule("z1", N_A)) == 4 and len(_face_schedule("y0", N_A)) == 2
    # D27_TAB: the sum of the three lattice counts on either side of it (a sum of three odd numbers is odd)
    assert [sum(2 * v + 1 for v in n) for n in N_TAB] == [D27_TAB - 1, D27_TAB + 1]


@gpu
@pytest.mark.parametrize("faces", ["robin_all", "fixed_x0y1"])
@pytest.mark.parametrize("shape", ["distorted", "uniform"])
@pytest.mark.parametrize("n", CASES_C, ids=["x".join(map(str, n)) for n in CASES_C])
def test_tile_ends_against_the_oracle(mf, n, shape, faces):
    robin, fixed = (ALL, "") if faces == "robin_all" else (ROBIN_C, FIXED_C)
    od = _oracle(X, n, robin, fixed, HP_ONE, shape=shape)
    brick = _brick(mf, X, n, 5, od.mesh.coords)
    _all_paths(mf, brick, od, n, robin, fixed, HP_ONE, f"C n={n} {shape} {faces}", general=shape == "distorted")


@gpu
@pytest.mark.parametrize("n", N_TAB, ids=["x".join(map(str, n)) for n in N_TAB])
def test_row_box_tables_on_either_side_of_the_lds_table(mf, n):
    """1023 and 1025 lattice coordinates: k_hex27_direct keeps the row-box tables in LDS up to D27_TAB = 1024 and reads them from memory
    beyond.  The direct path against the two-pass path to 1e-13 and against the oracle."""
    import torch

    x = (0.05 * n[0], 0.3, 0.2)
    od = _oracle(x, n, ALL, "", HP_ONE, shape="uniform")
    brick = _brick(mf, x, n, 5, od.mesh.coords)
    A = brick.pattern(1)
    before = _counts()
    Kd = brick.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    assert tuple(_counts() - before) == (1, 0, 0)
    with _Knob(TWO_PASS):
        Kt = brick.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    assert tuple(_counts() - before) == (1, 0, 0)
    assert bool(torch.isfinite(Kd).all()) and bool(torch.isfinite(Kt).all())
    Kd, Kt = Kd.cpu().numpy(), Kt.cpu().numpy()
    label = f"C n={n} (lattice coordinates {sum(2 * v + 1 for v in n)})"
    _close(f"{label} K direct vs two-pass", Kd, Kt, 1e-13)
    _close(f"{label} K direct", Kd, od.K_linear, K_TOL)
    _close(f"{label} K two-pass", Kt, od.K_linear, K_TOL)


# ---- D. mixed meshes at the ends of the element list ------------------------------------------------------------------------------
N_D, FIXED_D = (5, 4, 13), "x0"
ROBIN_D = REST_OF(FIXED_D)


def _centre_nodes(n):
    """Lattice ids of the elements' centre nodes (odd, odd, odd): a node of ONE element -- moving it makes exactly that element non-affine."""
    m = [2 * v + 1 for v in n]
    I, J, K = np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing="ij")
    return (((2 * I + 1) * m[1] + (2 * J + 1)) * m[2] + (2 * K + 1)).ravel()


@gpu
@pytest.mark.parametrize("count", [1, 8, 9, 64, 65])
def test_mixed_meshes_at_the_element_list_ends(mf, count):
    """260 elements, exactly `count` of them distorted: k_hex27<true, true> in list mode walks a list of one element, of a full workgroup of 8
    waves, of one more, and of one and two lanes' worth of 64 stored elements; the row owners of k_hex27_direct stream them in."""
    assert int(np.prod(N_D)) == 260
    cn = _centre_nodes(N_D)
    rng = np.random.default_rng(count)
    pick = rng.choice(cn, size=count, replace=False)
    coords = np.indices([2 * v + 1 for v in N_D]).reshape(3, -1).T * (np.array(X) / np.array(N_D) / 2)
    coords[pick] += 0.03 * rng.standard_normal((count, 3)) * np.array(X) / np.array(N_D)
    od = _oracle(X, N_D, ROBIN_D, FIXED_D, HP_ONE, shape=f"centres{count}", coords=coords)
    brick = _brick(mf, X, N_D, 5, coords)
    A = brick.pattern(1)
    rb, fb = _bits(mf, ROBIN_D), _bits(mf, FIXED_D)
    kw = dict(fixed_faces=fb, h_penalty=HP_ONE, Tw=TW)
    label = f"D {count} distorted elements"
    K = {}
    for knob, expect in ((CHOICE, (0, 2, 0)), (TWO_PASS, (0, 0, 0))):
        with _Knob(knob):
            before = _counts()
            K[knob] = brick.assemble_thermal(A, K_COND, H, TENV, rb, **kw).cpu().numpy()
            again = brick.assemble_thermal(A, K_COND, H, TENV, rb, **kw).cpu().numpy()
            assert tuple(_counts() - before) == expect, f"{label}: another path ran"
        assert np.array_equal(K[knob], again), f"{label} knob {knob}: a second call gives other bits"
        _close(f"{label} K knob {knob}", K[knob], od.K_linear, K_TOL)
    _close(f"{label} K forced choice vs two-pass", K[CHOICE], K[TWO_PASS], PATH_TOL)
    _check_symmetry(A, K[CHOICE], N_D, FIXED_D, label)


# ---- E. slabs with both boundary terms ---------------------------------------------------------------------------------------------
N_E = (6, 2, 3)  # m0 = 13 control-point planes
ROBIN_E = "x0|x1|z0"  # both slab end planes and a face every slab cuts
SLABS_E = [(0, 4), (4, 8), (8, 13), (4, 6)]
NO_ROWS = 1 << 11
PATHS_E = [("rows", 0, (0, 0, 1)), ("two_pass", NO_ROWS, (0, 0, 0)), ("ring_1_plane", NO_ROWS | 1 | (1 << 16), (0, 0, 0)), ("forced_choice", CHOICE, (0, 1, 0))]


@gpu
@pytest.mark.parametrize("knob", [ATOMICS, COLOUR])
def test_atomics_and_colour_scatter_refuse_a_slab(mf, knob):
    sb = mf.make_Brick(X, N_E, 2, 5)
    sb.set_slab(4, 8)
    A = sb.pattern(1)
    with _Knob(knob):
        with pytest.raises(Exception):
            sb.assemble_thermal(A, K_COND, H, TENV, _bits(mf, ROBIN_E))


@gpu
@pytest.mark.parametrize("fixed", ["y1", "x1"])
@pytest.mark.parametrize("name,knob,expect", PATHS_E, ids=[p[0] for p in PATHS_E])
def test_distorted_slab_rows_equal_global_rows(mf, name, knob, expect, fixed):
    """The whole brick against the oracle, then every slab against the rows of the whole brick, bit for bit (why that holds: the module
    docstring): stored coordinate planes [lo - 2, hi + 2), x and s with their ghost planes where parallel.slab_local_index puts them.
    fixed = x1: the last slab's end plane carries the Nitsche term, taken out of the Robin set."""
    import torch
    from metafem_jl_amd import parallel as par

    robin = "|".join(f for f in ROBIN_E.split("|") if f != fixed)
    od = _oracle(X, N_E, robin, fixed, HP_ONE)
    m0, m1, m2 = [2 * v + 1 for v in N_E]
    pl = m1 * m2
    gb = _brick(mf, X, N_E, 5, od.mesh.coords)
    gA = gb.pattern(1)
    grp = gA.rowptr.cpu().numpy()
    rb, fb = _bits(mf, robin), _bits(mf, fixed)
    kw = dict(fixed_faces=fb, h_penalty=HP_ONE, Tw=TW)
    gx, gs = _fields(gb.ncp)
    label = f"E {name} fixed[{fixed}]"
    with _Knob(knob):
        before = _counts()
        gK = gb.assemble_thermal(gA, K_COND, H, TENV, rb, **kw).cpu().numpy()
        assert tuple(_counts() - before) == expect, f"{label}: another path ran"
    gR = {}
    for rname, rknob in R_PATHS:
        with _Knob(rknob):
            gR[rknob] = gb.residual_thermal(torch.tensor(gx, device="cuda"), K_COND, H, TENV, rb, s=torch.tensor(gs, device="cuda"), **kw).cpu().numpy()
        _close(f"{label} {rname}", gR[rknob], od.residue, R_TOL)
    _close(f"{label} K", gK, od.K_linear, K_TOL)
    jj, kk = [a.ravel() for a in np.meshgrid(np.arange(m1), np.arange(m2), indexing="ij")]
    for lo, hi in SLABS_E:
        sb = mf.make_Brick(X, N_E, 2, 5)
        sb.set_slab(lo, hi)
        clo, chi = max(lo - 2, 0), min(hi + 2, m0)
        for d in range(3):
            view = sb.coords_view(d)
            assert view.numel() == (chi - clo) * pl
            view.copy_(torch.tensor(np.ascontiguousarray(od.mesh.coords[clo * pl:chi * pl, d]), device="cuda"))
        sA = sb.pattern(1)
        n_owned = (hi - lo) * pl
        r0, r1 = lo * pl, hi * pl
        assert sA.n == n_owned and np.array_equal(sA.rowptr.cpu().numpy(), grp[r0:r1 + 1] - grp[r0])
        nloc = par.local_vector_length(lo, hi, m1, m2, 1, order=2)
        xl, sl = np.zeros(nloc), np.zeros(nloc)
        for i in range(clo, chi):
            li = par.slab_local_index(np.full(jj.size, i), jj, kk, 0, lo, hi, m1, m2, 1, order=2)
            xl[li] = gx[i * pl + jj * m2 + kk]
            sl[li] = gs[i * pl + jj * m2 + kk]
        with _Knob(knob):
            before = _counts()
            sK = sb.assemble_thermal(sA, K_COND, H, TENV, rb, **kw).cpu().numpy()
            assert tuple(_counts() - before) == expect, f"{label} slab ({lo}, {hi}): another path ran"
        assert np.array_equal(sK, gK[grp[r0]:grp[r1]]), f"{label} slab ({lo}, {hi}): K rows differ by {np.abs(sK - gK[grp[r0]:grp[r1]]).max():.3e}"
        for rname, rknob in R_PATHS:
            with _Knob(rknob):
                sR = sb.residual_thermal(torch.tensor(xl, device="cuda"), K_COND, H, TENV, rb, s=torch.tensor(sl, device="cuda"), **kw).cpu().numpy()
            assert np.array_equal(sR, gR[rknob][r0:r1]), f"{label} slab ({lo}, {hi}) {rname}: R rows differ by {np.abs(sR - gR[rknob][r0:r1]).max():.3e}"


# ---- F. a brick away from the origin -----------------------------------------------------------------------------------------------
T_F = np.array([1024.0, -333.0, 77.7])
ROBIN_F, FIXED_F = "x1|y0|z1", "x0"


@gpu
@pytest.mark.parametrize("shape", ["distorted", "sheared"])
def test_translated_brick(mf, shape):
    """The part-A brick moved by (1024, -333, 77.7): K and R are mathematically those of the brick at the origin.  The product and the oracle
    get the same (rounded) translated coordinates.  The yardstick d_ref is the oracle on the translated coordinates against itself on the
    untranslated ones: the float64 noise of a Jacobian made of differences of coordinates of that magnitude (one ulp of 1024 over a
    half-element of 0.5 is 4.5e-13 per entry of J).  Every comparison within max(project tolerance, 4 d_ref); the kernel's own error sets no
    bound.  The sheared brick stays all-affine to the kernels' test (16 ulp of the coordinates' magnitude): the direct path, asserted."""
    od = _oracle(X, N_A, ROBIN_F, FIXED_F, HP_ONE, shape=shape)
    ot = _oracle(X, N_A, ROBIN_F, FIXED_F, HP_ONE, shape=f"{shape}+T", coords=od.mesh.coords + T_F)
    kscale, rscale = np.abs(od.K_linear).max(), np.abs(od.residue).max()
    d_ref_k = np.abs(ot.K_linear - od.K_linear).max() / kscale
    d_ref_r = np.abs(ot.residue - od.residue).max() / rscale
    print(f"F {shape}: d_ref K {d_ref_k:.3e}, R {d_ref_r:.3e}")
    # (the yardstick is the noise it is taken for: below 100 ulp of 1024 over the half-element)
    assert 0 < d_ref_k < 5e-11 and 0 < d_ref_r < 5e-11
    brick = _brick(mf, X, N_A, 5, ot.mesh.coords)
    out = _all_paths(mf, brick, ot, N_A, ROBIN_F, FIXED_F, HP_ONE, f"F {shape}", general=shape == "distorted", k_tol=max(K_TOL, 4 * d_ref_k),
                     r_tol=max(R_TOL, 4 * d_ref_r), path_tol=max(PATH_TOL, 4 * d_ref_k), rr_tol=max(RR_TOL, 4 * d_ref_r))
    for (letter, knob), got in out.items():
        ref, scale, d_ref = (ot.K_linear, kscale, d_ref_k) if letter == "K" else (ot.residue, rscale, d_ref_r)
        print(f"F {shape} {letter} knob {knob}: {np.abs(got - ref).max() / scale:.3e} ({np.abs(got - ref).max() / scale / d_ref:.2f} d_ref)")
