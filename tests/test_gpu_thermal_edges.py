"""GPU parity of the fused hex-8 thermal kernels with the oracle on every face, at every quadrature rule, at the lattice sizes where
their tiles and plane segments end, on slabs and away from the origin.

tests/test_gpu_thermal.py and tests/test_gpu_nitsche.py compare a dozen configurations with the oracle; the brick operator is tested against
the K these kernels assemble.  Here, laid out like tests/test_gpu_elasticity_edges.py: each face alone as the Robin and as the fixed (Nitsche)
face, at h_penalty = 1000 and at h_penalty = 1 (where the k n_i T_;i term and the volume entries are not hidden below a tolerance scaled by the
penalty entries), edges and corners (part A); itg_order 1 to 7 (part B); bricks whose point counts end on, one past and two past a tile of
every kernel (part C); plane segments of 8, 16 and 32 planes on the general and on the affine path, sweep against tiles, at sizes the oracle
does not reach (part D); slabs of a distorted brick against the rows of the whole brick, bit for bit (part E); a brick translated by 1024
(part F).  The oracle's own face numbering, normal sign and boundary forms are pinned without the product in
tests/test_oracle_thermal_faces.py.

Kernels per case, by the "hex8_thermal" knob word: K from the matrix sweep with the staged write-out (0), with the per-thread write-out (2)
and from the 4 x 4 x 8 tiles (1); R from the residual sweep + the boundary kernel (0) and from the tiles (1).  The sweeps exist for the 2- and
3-point rules; at the other rules knob 0 and knob 1 must give the same bits (both are the tile kernels).  Tolerances are the project's:
K to 2e-13 max|K_oracle| and R to 1e-12 max|R_oracle| without a fixed face, 1e-12 and 1e-11 with one; without fixed faces K is bitwise
symmetric; a second call gives the same bits.  Every comparison prints its figure (relative to its tolerance) before it asserts.

Largest printed figure per part, as a fraction of its tolerance (MI355X; the figures print with three decimals):
  A  K 0.004 (no fixed face), 0.001 (fixed, h_penalty = 1000), 0.001 (fixed, h_penalty = 1);  R 0.001 / below 0.0005 / below 0.0005
  B  K 0.001, R below 0.0005
  C  K 0.010 (Robin on all faces, n = (16, 1, 30)), 0.002 (fixed x0|y1);  R 0.002 / below 0.0005
  D  K sweep against tiles 0.480 (L = 32, sheared), R 0.223 (L = 8, sheared); |R(x) - R(0) - K x| 1.5e-13 against a bound of 5e-9
  E  whole brick against the oracle K 0.001, R below 0.0005; the slabs are bitwise
  F  K 0.236, R 0.183 of max(tolerance, 4 d_ref); the shortcut inside the gate 7.4 d_ref of the 64 allowed: see below
No h_penalty = 1 case needed a bound from the oracle's own noise: all are within the project's tolerances, by two orders of magnitude.

Part E, bitwise on a distorted brick: a row's value is (what the four elements below its plane gave) + (what the four above give), each
summed over the elements in a fixed order, in every kernel; where a sweep segment or a tile starts changes which workgroup computes the two
halves, not the order of the sum.  The face kernels add to a row in the order (direction, side, face element), which a slab does not change.

Part F (n = (8, 16, 4), x = (1, 2, 0.5), translation 1024; relative to max|K_oracle| on the untranslated brick):
  d_ref (the oracle translated against the oracle untranslated): a = -12: K 6.1e-13, R 4.6e-13; a = -40: K 7.3e-13, R 5.3e-13
  a = -12: K knob 0 8.3e-16, knob 4 8.3e-16 (the sweeps take differences of the dyadic coordinates first: the translation is invisible to
           them), knob 1 (tiles, table-form Jacobian) 5.7e-13 = 0.94 d_ref; R knob 0 5.0e-16, knob 1 3.4e-13
  a = -40: K knob 0 (the shortcut taken: the distortion lies inside the gate) 5.4e-12 = 7.4 d_ref, knob 4 8.3e-16, knob 1 6.5e-13 = 0.90 d_ref;
           R knob 0 4.3e-12 = 8.0 d_ref, knob 4 8.7e-16, knob 1 3.9e-13
"""
import os
import re

import numpy as np
import pytest

from test_gpu_elasticity_edges import FACE_NAMES, FACE_NORMAL, SHEAR, _bits, _close, _ids
from test_gpu_thermal import _distort

pytestmark = pytest.mark.gpu

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
TW = 1173.15
HP_REF, HP_ONE = 1000.0, 1.0
X = (3.0, 1.0, 2.0)
K_TOL, R_TOL = 2e-13, 1e-12              # no fixed face
K_TOL_FIXED, R_TOL_FIXED = 1e-12, 1e-11  # with a fixed face
ALL = "|".join(FACE_NAMES)
K_KERNELS = (("K sweep staged", 0), ("K sweep per-thread", 2), ("K tiles", 1))
R_KERNELS = (("R sweep", 0), ("R tiles", 1))


class _Knob:
    """mfem_debug_set_hex8_thermal(v) for the block, 0 afterwards."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_hex8_thermal(self.v)

    def __exit__(self, *exc):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_hex8_thermal(0)
        return False


def _lattice(x, n):
    """Control points of the uniform brick, the last direction fastest (the oracle's lattice_mesh and the product's numbering)."""
    return np.indices([v + 1 for v in n]).reshape(3, -1).T * (np.array(x) / np.array(n))


def _fields(ncp, seed=1):
    """x_star = 300 + 20 randn and a non-constant source."""
    rng = np.random.default_rng(seed)
    return 300.0 + 20.0 * rng.standard_normal(ncp), SRC * (1.0 + 0.1 * rng.standard_normal(ncp))


_ORACLE = {}


def _oracle(x, n, robin="", fixed="", hp=HP_REF, itg=3, shape="distorted", coords=None, src=True, h=H):
    """The oracle's K_linear and residue at _fields() for Robin faces `robin` and fixed faces `fixed`; computed once per configuration and
    shared (nobody writes to it).  `coords` (with `shape` as its name) overrides the named shapes."""
    from oracle import fem, mesh as om, problems, reference_element as re_

    key = (x, n, robin, fixed, hp, itg, shape, src, h)
    if key in _ORACLE:
        return _ORACLE[key]
    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
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

    brick = mf.make_Brick(x, n, 1, itg)
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


def _all_kernels(mf, brick, od, robin, fixed, hp, label, itg=3, src=True, h=H, k_tol=None, r_tol=None):
    """K from the three matrix kernels and R from the two residual kernels, each against the oracle and each called twice (same bits).
    Rules without a sweep: every knob gives the same bits.  No fixed face: K bitwise symmetric.  Returns the arrays by (letter, knob)."""
    import torch

    A = brick.pattern(1)
    assert np.array_equal(A.rowptr.cpu().numpy(), od.pattern.rowptr) and np.array_equal(A.colidx.cpu().numpy(), od.pattern.colidx)
    k_tol = k_tol or (K_TOL_FIXED if fixed else K_TOL)
    r_tol = r_tol or (R_TOL_FIXED if fixed else R_TOL)
    rb, fb = _bits(mf, robin), _bits(mf, fixed)
    kw = dict(fixed_faces=fb, h_penalty=hp, Tw=TW)
    xs_np, s_np = _fields(brick.ncp)
    xs = torch.tensor(xs_np, device="cuda")
    s = torch.tensor(s_np, device="cuda") if src else None
    out = {}
    for name, knob in K_KERNELS:
        with _Knob(knob):
            got = brick.assemble_thermal(A, K_COND, h, TENV, rb, **kw).cpu().numpy()
            again = brick.assemble_thermal(A, K_COND, h, TENV, rb, **kw).cpu().numpy()
        _close(f"{label} {name}", got, od.K_linear, k_tol)
        assert np.array_equal(got, again), f"{label} {name}: a second call gives other bits"
        if not fixed:
            assert _asymmetry(got, A)[1] == 0.0, f"{label} {name}: K is not bitwise symmetric"
        out["K", knob] = got
    for name, knob in R_KERNELS:
        with _Knob(knob):
            got = brick.residual_thermal(xs, K_COND, h, TENV, rb, s=s, **kw).cpu().numpy()
            again = brick.residual_thermal(xs, K_COND, h, TENV, rb, s=s, **kw).cpu().numpy()
        _close(f"{label} {name}", got, od.residue, r_tol)
        assert np.array_equal(got, again), f"{label} {name}: a second call gives other bits"
        out["R", knob] = got
    assert np.array_equal(out["K", 0], out["K", 2]), f"{label}: the write-out touches the values"
    if (itg + 2) // 2 not in (2, 3):  # no sweep for this rule: the dispatch must send every knob to the tiles
        assert np.array_equal(out["K", 0], out["K", 1]) and np.array_equal(out["R", 0], out["R", 1]), f"{label}: knob 0 and knob 1 differ without a sweep"
    else:
        assert not np.array_equal(out["K", 0], out["K", 1]) and not np.array_equal(out["R", 0], out["R", 1]), f"{label}: the knob selects no other kernel"
    return out


def _near(n, names):
    """Control points on or adjacent to one of the named faces."""
    idx = np.indices([v + 1 for v in n]).reshape(3, -1)
    near = np.zeros(idx.shape[1], dtype=bool)
    for f in names.split("|"):
        nd, sign = FACE_NORMAL[f]
        near |= (idx[nd] >= n[nd] - 1) if sign > 0 else (idx[nd] <= 1)
    return near


def _check_asymmetry(brick, K, n, fixed, label):
    """A fixed face makes K nonsymmetric, in the rows of the nodes on that face and of their element neighbours only."""
    A = brick.pattern(1)
    rows, amax = _asymmetry(K, A)
    print(f"ASYMMETRY {label}: max {amax:.3e} ({amax / np.abs(K).max():.2e} of max|K|), {np.unique(rows).size} rows")
    assert amax > 1e-6 * np.abs(K).max(), label
    assert np.all(_near(n, fixed)[rows]), label


# ---- A. every face, both boundary terms, every kernel ----------------------------------------------------------------------------
N_A = (3, 4, 2)
CASES_A = ([(f, "", HP_REF) for f in FACE_NAMES]                                      # 1. each face alone as the Robin face
           + [("", f, hp) for f in FACE_NAMES for hp in (HP_REF, HP_ONE)]             # 2. each face alone as the fixed face
           + [("y0|x1", "y0|x1", hp) for hp in (HP_REF, HP_ONE)]                      # 3. a low face and a high face carrying both terms
           + [("y0", "x0", HP_ONE), ("z1", "x1", HP_ONE)]                             # 4. adjacent faces with one term each: a shared edge
           + [("x0|z0", "y0", HP_ONE), ("y1", "x1|z1", HP_ONE)]                       # 5. three faces meeting in a corner, the terms mixed
           + [("", ALL, HP_ONE), (ALL, "", HP_REF)])                                  # 6. all six


@pytest.mark.parametrize("robin,fixed,hp", CASES_A, ids=[f"robin[{r}]-fixed[{f}]-hp{int(p)}" for r, f, p in CASES_A])
def test_faces_against_the_oracle(mf, robin, fixed, hp):
    od = _oracle(X, N_A, robin, fixed, hp)
    brick = _brick(mf, X, N_A, 3, od.mesh.coords)
    out = _all_kernels(mf, brick, od, robin, fixed, hp, f"A robin[{robin}] fixed[{fixed}] hp={hp:g}")
    if fixed:
        for _, knob in K_KERNELS:
            _check_asymmetry(brick, out["K", knob], N_A, fixed, f"A fixed[{fixed}] hp={hp:g} knob {knob}")


@pytest.mark.parametrize("what", ["robin_bits_h_zero", "h_without_bits"])
def test_a_disabled_robin_term_is_no_term(mf, what):
    """Bits without a coefficient and a coefficient without bits launch no boundary kernel: the oracle without the term, and bitwise the
    product's own no-face result."""
    od = _oracle(X, N_A)
    brick = _brick(mf, X, N_A, 3, od.mesh.coords)
    plain = _all_kernels(mf, brick, od, "", "", 0.0, f"A7 {what} plain", h=0.0)
    h, robin = {"robin_bits_h_zero": (0.0, ALL), "h_without_bits": (H, "")}[what]
    got = _all_kernels(mf, brick, od, robin, "", 0.0, f"A7 {what}", h=h)
    for key in plain:
        assert np.array_equal(got[key], plain[key]), (what, key)


@pytest.mark.parametrize("robin,fixed", [("", ""), ("x1|y0|z1", "x0")])
def test_residual_without_a_source_vector(mf, robin, fixed):
    od = _oracle(X, N_A, robin, fixed, HP_ONE, src=False)
    brick = _brick(mf, X, N_A, 3, od.mesh.coords)
    _all_kernels(mf, brick, od, robin, fixed, HP_ONE, f"A8 s=None robin[{robin}] fixed[{fixed}]", src=False)


# ---- B. every quadrature rule ----------------------------------------------------------------------------------------------------
N_B, ROBIN_B, FIXED_B = (5, 3, 6), "y0|z1", "x0"


@pytest.mark.parametrize("itg", [1, 2, 3, 4, 5, 6, 7])
def test_quadrature_rules_against_the_oracle(mf, itg):
    """ng = (itg + 2) / 2 = 1, 2, 2, 3, 3, 4, 4 Gauss points per direction (the oracle builds the even orders too: asserted)."""
    od = _oracle(X, N_B, ROBIN_B, FIXED_B, HP_ONE, itg=itg)
    assert od.elgeo.integral_weights.shape[0] == ((itg + 2) // 2) ** 3
    brick = _brick(mf, X, N_B, itg, od.mesh.coords)
    _all_kernels(mf, brick, od, ROBIN_B, FIXED_B, HP_ONE, f"B itg={itg}", itg=itg)


# ---- C. where tiles and segments end ---------------------------------------------------------------------------------------------
# point counts m = n + 1: j of the matrix sweep (7-wide tiles) 7, 8, 14, 15; k of the matrix sweep and both directions of the residual sweep
# (15-wide) 15, 16, 17, 30, 31; the tile kernels (4 x 4 x 8) 4, 5, 8, 9; owned planes (segments of 4) 4, 5, 8, 9; one element thick: 2
CASES_C = [(1, 6, 14), (3, 7, 15), (4, 13, 16), (8, 8, 16), (7, 14, 30), (16, 1, 30), (3, 14, 1), (5, 15, 29)]
FIXED_C = "x0|y1"
ROBIN_C = "|".join(f for f in FACE_NAMES if f not in FIXED_C.split("|"))


def test_part_c_covers_the_tile_and_segment_ends():
    m = np.array(CASES_C) + 1
    assert {7, 8, 14, 15} <= set(m[:, 1])                        # j of the matrix sweep
    assert {15, 16, 17, 30, 31} <= set(m[:, 2])                  # k of either sweep
    assert {15, 16} <= set(m[:, 1])                              # j of the residual sweep
    assert {4, 5, 8, 9} <= set(m[:, 0])                          # owned planes: tiles of 4, segments of 4
    assert {8, 9} <= set(m[:, 1])                                # j of the tile kernels (4-wide); k (8-wide): 15, 16, 17 above
    assert all(2 in set(m[:, d]) for d in range(3))              # one element thick


@pytest.mark.parametrize("faces", ["robin_all", "fixed_x0y1"])
@pytest.mark.parametrize("itg", [3, 5])
@pytest.mark.parametrize("n", CASES_C, ids=["x".join(map(str, n)) for n in CASES_C])
def test_lattice_edges_against_the_oracle(mf, n, itg, faces):
    robin, fixed = (ALL, "") if faces == "robin_all" else (ROBIN_C, FIXED_C)
    od = _oracle(X, n, robin, fixed, HP_ONE, itg=itg)
    brick = _brick(mf, X, n, itg, od.mesh.coords)
    _all_kernels(mf, brick, od, robin, fixed, HP_ONE, f"C n={n} itg={itg} {faces}", itg=itg)


# ---- D. segments of 8, 16 and 32 planes --------------------------------------------------------------------------------------------
def _decide_constants():
    """SW_E, MS_EJ, MS_EK, SW_FILL, MS_FILL as csrc/hex8_decide.h defines them today."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metafem.jl_amd", "csrc", "hex8_decide.h")
    with open(path) as fh:
        text = fh.read()
    return {k: int(re.search(rf"^#define {k} (\d+)\s", text, re.M).group(1)) for k in ("SW_E", "MS_EJ", "MS_EK", "SW_FILL", "MS_FILL")}


def _sweep_segments(m1, m2, planes, nj, nk, fill):
    """h8_sweep_segments of csrc/hex8_decide.h, transcribed: L = 32, halved down to 4 while the grid stays below `fill` workgroups."""
    ntj, ntk = -(-m1 // nj), -(-m2 // nk)
    L = 32
    while L > 4 and ntj * ntk * (-(-planes // L)) < fill:
        L //= 2
    return L, ntj * ntk * (-(-planes // L))


def _segments_of(n):
    c = _decide_constants()
    m = [v + 1 for v in n]
    res = _sweep_segments(m[1], m[2], m[0], c["SW_E"] - 1, c["SW_E"] - 1, c["SW_FILL"])
    mat = _sweep_segments(m[1], m[2], m[0], c["MS_EJ"] - 1, c["MS_EK"] - 1, c["MS_FILL"])
    return res, mat


@pytest.mark.parametrize("n,L", [((8, 465, 465), 8), ((16, 465, 465), 16), ((32, 465, 465), 32), ((9, 33, 17), 4), ((5, 15, 29), 4)])
def test_transcribed_segment_lengths(n, L):
    """(CPU arithmetic.)  The part D shapes run with the segment lengths they are there for, both sweeps, a full segment followed by a
    one-plane tail; the part C and tests/test_gpu_thermal.py shapes with L = 4."""
    (Lr, gr), (Lm, gm) = _segments_of(n)
    assert (Lr, Lm) == (L, L), (n, Lr, Lm, gr, gm)
    if L > 4:
        assert n[0] + 1 == L + 1 and gr >= 2048 and gm >= 4096 and (n[1] + 1) % 15 == 1 and (n[2] + 1) % 15 == 1


_BIG = {}


def _big_brick(mf, n, itg):
    """The brick, its pattern and its uniform coordinates, built once per (n, itg)."""
    if (n, itg) not in _BIG:
        brick = mf.make_Brick(X, n, 1, itg)
        _BIG[n, itg] = (brick, brick.pattern(1), [brick.coords_view(d).clone() for d in range(3)])
    return _BIG[n, itg]


def _close_dev(label, got, ref, tol):
    """_close on device tensors."""
    import torch

    scale = float(ref.abs().max())
    diff = float((got - ref).abs().max())
    print(f"PARITY {label}: {diff / (tol * scale) if scale > 0 else float(diff > 0):.3f} of tol (diff {diff:.3e}, scale {scale:.3e})")
    assert scale > 0 and bool(torch.isfinite(got).all()), label
    assert diff <= tol * scale, label


ROBIN_D, FIXED_D = "x1|y0|y1|z0|z1", "x0"


@pytest.mark.parametrize("n,itg,shape", [((8, 465, 465), 3, "distorted"), ((8, 465, 465), 3, "sheared"), ((16, 465, 465), 3, "distorted"),
                                         ((16, 465, 465), 3, "sheared"), ((32, 465, 465), 3, "distorted"), ((32, 465, 465), 3, "sheared"),
                                         ((32, 465, 465), 5, "distorted")],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_long_segments_sweep_against_tiles(mf, n, itg, shape):
    """1.95 M, 3.7 M and 7.2 M rows: the sweeps run segments of L = n[0] planes followed by a one-plane tail, (j, k) tiles cut one point past a
    tile edge.  The independent implementation at these sizes is the tile kernels (parts A to C pin them against the oracle): K and R to
    2e-13, as test_sweep_kernels_equal_tile_kernels_and_keep_K_bitwise_symmetric; R(x) - R(0) = K x without source and ambient terms to
    27 entries per row x 1e-12 max|K| max|x|; a second call gives the same bits.  Which path ran: the shortcut switched off (knob 4) changes
    the bits on the sheared brick and none on the distorted one.  All on the device."""
    import torch

    (Lr, _), (Lm, _) = _segments_of(n)
    assert Lr == Lm == n[0] > 4
    brick, A, c0 = _big_brick(mf, n, itg)
    if shape == "distorted":
        c = [c0[0] + 0.03 * torch.sin(3 * c0[1]) * torch.cos(2 * c0[2]), c0[1] + 0.02 * torch.sin(2 * c0[0] + c0[2]), c0[2] + 0.025 * c0[0] * c0[1]]
    else:
        S = SHEAR
        c = [S[d][0] * c0[0] + S[d][1] * c0[1] + S[d][2] * c0[2] + off for d, off in enumerate((0.3, -0.2, 0.1))]
    for d in range(3):
        brick.coords_view(d).copy_(c[d])
    rb, fb = _bits(mf, ROBIN_D), _bits(mf, FIXED_D)
    kw = dict(fixed_faces=fb, h_penalty=HP_ONE, Tw=TW)
    g = torch.Generator(device="cuda").manual_seed(5)
    xs = 300.0 + 20.0 * torch.randn(A.n, dtype=torch.float64, device="cuda", generator=g)
    s = SRC * (1.0 + 0.1 * torch.randn(A.n, dtype=torch.float64, device="cuda", generator=g))
    label = f"D n={n} itg={itg} {shape}"
    K, R = {}, {}
    for knob in (1, 4, 0):
        with _Knob(knob):
            K[knob] = brick.assemble_thermal(A, K_COND, H, TENV, rb, **kw)
            R[knob] = brick.residual_thermal(xs, K_COND, H, TENV, rb, s=s, **kw)
            if knob == 0:
                assert torch.equal(K[0], brick.assemble_thermal(A, K_COND, H, TENV, rb, **kw)), f"{label}: a second call gives other K bits"
                assert torch.equal(R[0], brick.residual_thermal(xs, K_COND, H, TENV, rb, s=s, **kw)), f"{label}: a second call gives other R bits"
    _close_dev(f"{label} K sweep vs tiles", K[0], K[1], 2e-13)
    _close_dev(f"{label} R sweep vs tiles", R[0], R[1], 2e-13)
    _close_dev(f"{label} K general sweep vs tiles", K[4], K[1], 2e-13)
    _close_dev(f"{label} R general sweep vs tiles", R[4], R[1], 2e-13)
    assert torch.equal(K[0], K[4]) == (shape == "distorted") and torch.equal(R[0], R[4]) == (shape == "distorted"), f"{label}: another path ran"
    del K[1], K[4], R
    # R(x) - R(0) = K x: Tenv = Tw = 0 and no source, so nothing constant is subtracted from itself
    kw0 = dict(fixed_faces=fb, h_penalty=HP_ONE, Tw=0.0)
    Rx = brick.residual_thermal(xs, K_COND, H, 0.0, rb, **kw0)
    R0 = brick.residual_thermal(torch.zeros_like(xs), K_COND, H, 0.0, rb, **kw0)
    Kx = torch.zeros_like(xs)
    mf.mul_(Kx, A, K[0], xs)
    kmax, xmax = float(K[0].abs().max()), float(xs.abs().max())
    bound = 27 * (1e-12 * kmax) * xmax
    defect = float((Rx - R0 - Kx).abs().max())
    print(f"PARITY {label} |R(x) - R(0) - K x|: {defect / bound:.3f} of bound (defect {defect:.3e}, max|K| {kmax:.3e}, max|x| {xmax:.3e}, max|R| {float(Rx.abs().max()):.3e})")
    assert kmax > 0 and float(Rx.abs().max()) > 0 and bool(torch.isfinite(Rx).all()) and float(R0.abs().max()) == 0.0
    assert defect <= bound, label


# ---- E. slabs ----------------------------------------------------------------------------------------------------------------------
N_E = (9, 8, 16)  # m = (10, 9, 17): two matrix-sweep tiles in j, two tiles of either sweep in k
ROBIN_E = "x0|x1|z0"  # both slab end planes and a face every slab cuts
SLABS_E = [(0, 4), (4, 9), (9, 10), (3, 4)]


@pytest.mark.parametrize("fixed", ["y1", "x1"])
@pytest.mark.parametrize("itg,knob", [(3, 0), (3, 1), (5, 0), (5, 1), (1, 0)], ids=["itg3-sweep", "itg3-tiles", "itg5-sweep", "itg5-tiles", "itg1-tiles"])
def test_distorted_slab_rows_equal_global_rows(mf, itg, knob, fixed):
    """The whole brick against the oracle, then every slab against the rows of the whole brick, bit for bit (why that holds: the module
    docstring): stored coordinate planes [lo - 1, hi + 1), x and s with their ghost planes behind the owned entries."""
    import torch
    from metafem_jl_amd import parallel as par

    od = _oracle(X, N_E, ROBIN_E, fixed, HP_ONE, itg=itg)
    m0, m1, m2 = [v + 1 for v in N_E]
    pl = m1 * m2
    gb = _brick(mf, X, N_E, itg, od.mesh.coords)
    gA = gb.pattern(1)
    grp = gA.rowptr.cpu().numpy()
    rb, fb = _bits(mf, ROBIN_E), _bits(mf, fixed)
    kw = dict(fixed_faces=fb, h_penalty=HP_ONE, Tw=TW)
    gx, gs = _fields(gb.ncp)
    label = f"E itg={itg} knob {knob} fixed[{fixed}]"
    with _Knob(knob):
        gK = gb.assemble_thermal(gA, K_COND, H, TENV, rb, **kw).cpu().numpy()
        gR = gb.residual_thermal(torch.tensor(gx, device="cuda"), K_COND, H, TENV, rb, s=torch.tensor(gs, device="cuda"), **kw).cpu().numpy()
    _close(f"{label} K", gK, od.K_linear, K_TOL_FIXED)
    _close(f"{label} R", gR, od.residue, R_TOL_FIXED)
    for lo, hi in SLABS_E:
        sb = mf.make_Brick(X, N_E, 1, itg)
        sb.set_slab(lo, hi)
        clo, chi = max(lo - 1, 0), min(hi + 1, m0)
        for d in range(3):
            view = sb.coords_view(d)
            assert view.numel() == (chi - clo) * pl
            view.copy_(torch.tensor(np.ascontiguousarray(od.mesh.coords[clo * pl:chi * pl, d]), device="cuda"))
        sA = sb.pattern(1)
        n_owned = (hi - lo) * pl
        r0, r1 = lo * pl, hi * pl
        assert sA.n == n_owned and np.array_equal(sA.rowptr.cpu().numpy(), grp[r0:r1 + 1] - grp[r0])
        nloc = par.local_vector_length(lo, hi, m1, m2, 1)
        xl, sl = np.zeros(nloc), np.zeros(nloc)
        for loc, glob in ((xl, gx), (sl, gs)):
            loc[:n_owned] = glob[r0:r1]
            if lo > 0:
                loc[n_owned:n_owned + pl] = glob[r0 - pl:r0]
            if hi < m0:
                loc[n_owned + pl:n_owned + 2 * pl] = glob[r1:r1 + pl]
        with _Knob(knob):
            sK = sb.assemble_thermal(sA, K_COND, H, TENV, rb, **kw).cpu().numpy()
            sR = sb.residual_thermal(torch.tensor(xl, device="cuda"), K_COND, H, TENV, rb, s=torch.tensor(sl, device="cuda"), **kw).cpu().numpy()
        assert np.array_equal(sK, gK[grp[r0]:grp[r1]]), f"{label} slab ({lo}, {hi}): K rows differ by {np.abs(sK - gK[grp[r0]:grp[r1]]).max():.3e}"
        assert np.array_equal(sR, gR[r0:r1]), f"{label} slab ({lo}, {hi}): R rows differ by {np.abs(sR - gR[r0:r1]).max():.3e}"


# ---- F. a brick away from the origin -----------------------------------------------------------------------------------------------
N_F, X_F, T_F = (8, 16, 4), (1.0, 2.0, 0.5), 1024.0  # every lattice coordinate is dyadic


@pytest.mark.parametrize("a", [-12, -40])
def test_translated_brick(mf, a):
    """Nodes moved by random multiples of 2^a / 4 (up to 2^a) and the brick translated by 1024 in all three coordinates, exactly: K and R are
    mathematically those of the untranslated brick, which the oracle supplies.  The yardstick d_ref is the oracle on the translated
    coordinates against itself on the untranslated ones: the float64 noise of a table-form Jacobian at that offset.
    a = -12: the distortion (2e-3 of an edge) is far above the affine gate 3.6e-15 (|x0| + edges) = 3.7e-12: every kernel within
    max(tolerance, 4 d_ref); a gate that swallowed it would be off by 1e-3.  a = -40: the distortion (9e-13) is inside the gate: the kernels
    without the shortcut (knobs 4 and 1) within max(tolerance, 4 d_ref), the shortcut (knob 0) within 64 d_ref -- the gate admits 16 ulp of |x|
    on four mixed coefficients where the oracle's noise is about one ulp of |x| over h."""
    import torch

    base = _lattice(X_F, N_F)
    c = base + np.random.default_rng(11).integers(-4, 5, size=base.shape) * (2.0 ** a / 4)
    assert np.array_equal((c + T_F) - T_F, c) and not np.array_equal(c, base)
    od = _oracle(X_F, N_F, shape=f"dyadic{a}", coords=c)
    ot = _oracle(X_F, N_F, shape=f"dyadic{a}+T", coords=c + T_F)
    kscale, rscale = np.abs(od.K_linear).max(), np.abs(od.residue).max()
    d_ref_k = np.abs(ot.K_linear - od.K_linear).max() / kscale
    d_ref_r = np.abs(ot.residue - od.residue).max() / rscale
    print(f"F a={a}: d_ref K {d_ref_k:.3e}, R {d_ref_r:.3e}")
    # (the yardstick is the noise it is taken for: one ulp of 1024 over h = 0.125 is 1.8e-12 per direction, three directions; 7e-13 measured)
    assert 0 < d_ref_k < 5.5e-12 and 0 < d_ref_r < 5.5e-12
    brick = _brick(mf, X_F, N_F, 3, c + T_F)
    A = brick.pattern(1)
    xs_np, s_np = _fields(brick.ncp)
    xs, s = torch.tensor(xs_np, device="cuda"), torch.tensor(s_np, device="cuda")
    for knob in (0, 1, 4):
        with _Knob(knob):
            K = brick.assemble_thermal(A, K_COND, 0.0, TENV, 0).cpu().numpy()
            K2 = brick.assemble_thermal(A, K_COND, 0.0, TENV, 0).cpu().numpy()
            R = brick.residual_thermal(xs, K_COND, 0.0, TENV, 0, s=s).cpu().numpy()
            R2 = brick.residual_thermal(xs, K_COND, 0.0, TENV, 0, s=s).cpu().numpy()
        assert np.array_equal(K, K2) and np.array_equal(R, R2), knob
        shortcut = a == -40 and knob == 0
        ktol = 64 * d_ref_k if shortcut else max(K_TOL, 4 * d_ref_k)
        rtol = 64 * d_ref_r if shortcut else max(R_TOL, 4 * d_ref_r)
        print(f"F a={a} knob {knob}: K {np.abs(K - od.K_linear).max() / kscale:.3e} ({np.abs(K - od.K_linear).max() / kscale / d_ref_k:.2f} d_ref), "
              f"R {np.abs(R - od.residue).max() / rscale:.3e} ({np.abs(R - od.residue).max() / rscale / d_ref_r:.2f} d_ref)")
        _close(f"F a={a} knob {knob} K", K, od.K_linear, ktol)
        _close(f"F a={a} knob {knob} R", R, od.residue, rtol)
