"""GPU parity of the fused hex-8 elasticity kernels with the oracle on every face, at every quadrature rule and at the lattice
sizes where their tiles end.

tests/test_gpu_elasticity.py compares one boundary configuration (penalty on x0, sigma_22 on y1) with the oracle.  Here: the full
traction tensor and both boundary terms on each of the six faces and on edges and corners (part A), the 1- to 4-point Gauss rules
(part B), bricks one element thick, lines of 31 / 32 / 33 control points and residual tiles cut at 15 / 16 / 17 (part C), and the
identity R(x) - R(0) = K x at a size the oracle does not reach (part D).  The oracle's own face numbering and normal sign are pinned
without the product in tests/test_oracle_elasticity_faces.py.

Tolerances are those of test_elasticity_pattern_matrix_residual: K to 2e-13 max|K_oracle|, R to 1e-12 max|R_oracle|, and a second
call gives the same bits.  Every comparison prints its figure (relative to its tolerance) before it asserts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_MOD, NU = 1.0, 0.3
LAM, MU = E_MOD * NU / ((1 + NU) * (1 - 2 * NU)), E_MOD / (2 * (1 + NU))
TAU_REF = 1000.0 * E_MOD  # the reference script's penalty
TAU_ONE = 1.0             # elastic entries are not hidden below a tolerance scaled by the penalty entries (tau h^2 ~ 300 x an elastic entry at tau = 1000)
K_TOL, R_TOL = 2e-13, 1e-12
X = (3.0, 1.0, 2.0)
SIG = [[0.7, -0.4, 0.25], [-0.4, 1.0, 0.55], [0.25, 0.55, -0.3]]
SIG6 = (0.7, 1.0, -0.3, 0.55, 0.25, -0.4)  # (11, 22, 33, 23, 13, 12)
FACE_NAMES = ["z0", "y0", "x1", "y1", "x0", "z1"]  # oracle face id f == bit f of the product's mask
FACE_NORMAL = {"z0": (2, -1.0), "y0": (1, -1.0), "x1": (0, 1.0), "y1": (1, 1.0), "x0": (0, -1.0), "z1": (2, 1.0)}
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])


def _ids(names):
    return [FACE_NAMES.index(s) for s in names.split("|")] if names else []


def _bits(mf, names):
    b = 0
    for s in (names.split("|") if names else []):
        b |= mf.FACE_BITS[s]
    return b


def _distort(c, x):
    return c + 0.03 * np.stack([np.sin(2 * c[:, 1]), np.cos(2 * c[:, 2]) - 1, c[:, 0] * c[:, 1] / x[0]], axis=1)


def _oracle(x, n, pen="", tra="", sig=SIG, tau=TAU_REF, itg=3, shape="distorted", seed=2):
    """The oracle's K_linear and residue at x_star = 0.01 randn for penalty faces `pen` and traction faces `tra`."""
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    if shape == "distorted":
        msh.coords = _distort(msh.coords, x)
    elif shape == "sheared":
        msh.coords = msh.coords @ SHEAR.T + np.array([0.3, -0.2, 0.1])
    else:
        assert shape == "uniform"
    fac = om.boundary_facets_structured(x, n, 3)
    bnd = []
    if pen:
        bnd.append((fac.select(np.isin(fac.element_eindex, _ids(pen))), problems.elasticity_penalty(3, tau)))
    if tra:
        bnd.append((fac.select(np.isin(fac.element_eindex, _ids(tra))), problems.elasticity_traction(3, sig)))
    od = fem.FEMDomain(msh, disc, 3, problems.elasticity_domain(3, LAM, MU), bnd)
    od.update_time()
    od.K_linear_func()
    od.x_star[:] = 0.01 * np.random.default_rng(seed).standard_normal(od.basicfield_size)
    od.K_nonlinear_func()
    return od


def _brick(mf, x, n, itg, coords=None):
    import torch

    brick = mf.make_Brick(x, n, 1, itg)
    if coords is not None:
        for d in range(3):
            brick.coords_view(d).copy_(torch.tensor(np.ascontiguousarray(coords[:, d]), device="cuda"))
    return brick


class _Knob:
    """mfem_debug_set_elasticity(v) for the block, 0 afterwards."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_elasticity(self.v)

    def __exit__(self, *exc):
        from metafem_jl_amd import _lib

        _lib.lib.mfem_debug_set_elasticity(0)
        return False


def _close(label, got, ref, tol):
    """max|got - ref| <= tol max|ref|; prints the figure as a fraction of the tolerance first."""
    scale = np.abs(ref).max()
    diff = np.abs(got - ref).max()
    print(f"PARITY {label}: {diff / (tol * scale) if scale > 0 else float(diff > 0):.3f} of tol (diff {diff:.3e}, scale {scale:.3e})")
    assert scale > 0 and np.all(np.isfinite(got)), label
    assert diff <= tol * scale, label


def _four_kernels(mf, brick, od, tau, pen, tra, sig6, label, kernels="KkRr"):
    """K from the default (K) and the row-owner (k) kernel, R from the sweep form + face kernel (R) and the per-point kernel (r), each
    against the oracle and each called twice (same bits).  Returns the arrays by kernel letter."""
    import torch

    A = brick.pattern(3)
    assert np.array_equal(A.rowptr.cpu().numpy(), od.pattern.rowptr) and np.array_equal(A.colidx.cpu().numpy(), od.pattern.colidx)
    xs = torch.tensor(od.x_star, device="cuda")
    out = {}
    for kern, knob in (("K", 0), ("k", 1), ("R", 0), ("r", 2)):
        if kern not in kernels:
            continue
        with _Knob(knob):
            if kern in "Kk":
                got = brick.assemble_elasticity(A, LAM, MU, tau, pen).cpu().numpy()
                again = brick.assemble_elasticity(A, LAM, MU, tau, pen).cpu().numpy()
            else:
                got = brick.residual_elasticity(xs, LAM, MU, tau, pen, tra, sig6).cpu().numpy()
                again = brick.residual_elasticity(xs, LAM, MU, tau, pen, tra, sig6).cpu().numpy()
        if kern in "Kk":
            _close(f"{label} {kern}", got, od.K_linear, K_TOL)
        else:
            _close(f"{label} {kern}", got, od.residue, R_TOL)
        assert np.array_equal(got, again), f"{label} {kern}: a second call gives other bits"
        out[kern] = got
    return out


# ---- A. every face, both boundary terms, all four kernels ------------------------------------------------------------------------
N_A = (3, 4, 2)
CASES_A = ([(f, "", t) for f in FACE_NAMES for t in (TAU_REF, TAU_ONE)]          # 1. each face alone as the penalty face
           + [("", f, t) for f in FACE_NAMES for t in (TAU_REF, TAU_ONE)]        # 2. each face alone as the traction face
           + [("z0", "z0", TAU_REF), ("x1", "x1", TAU_REF)]                      # 3. one face carrying both terms: a low face, a high face
           + [("|".join(FACE_NAMES), "", TAU_REF), ("", "|".join(FACE_NAMES), TAU_REF)]  # 4. all six
           + [("x0|y0|z0", "x1|y1|z1", t) for t in (TAU_REF, TAU_ONE)])          # 5. corner and edge nodes collect two and three faces


@pytest.mark.parametrize("pen,tra,tau", CASES_A, ids=[f"pen[{p}]-tra[{t}]-tau{int(u)}" for p, t, u in CASES_A])
def test_faces_against_the_oracle(mf, pen, tra, tau):
    od = _oracle(X, N_A, pen, tra, tau=tau)
    brick = _brick(mf, X, N_A, 3, od.mesh.coords)
    _four_kernels(mf, brick, od, tau, _bits(mf, pen), _bits(mf, tra), SIG6, f"A pen[{pen}] tra[{tra}] tau={tau:g}")


@pytest.mark.parametrize("what", ["penalty_bits_tau_zero", "tau_without_bits", "traction_bits_sigma_zero"])
def test_a_disabled_term_is_no_term(mf, what):
    """Bits without a strength and a strength without bits: the oracle without that term, and bitwise the product's own no-face result."""
    import torch

    od = _oracle(X, N_A)  # no boundary term at all
    brick = _brick(mf, X, N_A, 3, od.mesh.coords)
    allf = mf.ALL_FACES
    tau, pen, tra, sig6 = {"penalty_bits_tau_zero": (0.0, allf, 0, SIG6), "tau_without_bits": (TAU_REF, 0, 0, SIG6),
                           "traction_bits_sigma_zero": (0.0, 0, allf, (0.0,) * 6)}[what]
    got = _four_kernels(mf, brick, od, tau, pen, tra, sig6, f"A6 {what}")
    A = brick.pattern(3)
    xs = torch.tensor(od.x_star, device="cuda")
    for kern, knob in (("K", 0), ("k", 1), ("R", 0), ("r", 2)):
        with _Knob(knob):
            if kern in "Kk":
                plain = brick.assemble_elasticity(A, LAM, MU, 0.0, 0).cpu().numpy()
            else:
                plain = brick.residual_elasticity(xs, LAM, MU, 0.0, 0, 0, (0.0,) * 6).cpu().numpy()
        assert np.array_equal(got[kern], plain), (what, kern)


@pytest.mark.parametrize("face", FACE_NAMES)
def test_closed_forms_on_the_undistorted_brick(mf, face):
    """No oracle: the net traction on a face is sigma.n.area and vanishes exactly off the face; the penalty entries sum to -3 tau area.
    The oracle meets these to 9e-16 of the expected value (tests/test_oracle_elasticity_faces.py); the bound is a round 100 x that."""
    import torch

    tol = 1e-13
    nd, sign = FACE_NORMAL[face]
    area = X[(nd + 1) % 3] * X[(nd + 2) % 3]
    brick = mf.make_Brick(X, N_A, 1, 3)
    A = brick.pattern(3)
    ncp = A.n // 3
    bit = mf.FACE_BITS[face]
    m = [v + 1 for v in N_A]
    on = (np.indices(m)[nd].ravel() == (N_A[nd] if sign > 0 else 0))
    zero = torch.zeros(A.n, dtype=torch.float64, device="cuda")
    expect = np.array(SIG)[:, nd] * sign * area
    for knob in (0, 2):
        with _Knob(knob):
            R = brick.residual_elasticity(zero, LAM, MU, 0.0, 0, bit, SIG6).cpu().numpy().reshape(3, ncp)
        got = R.sum(axis=1)
        print(f"CLOSED {face} knob {knob}: net traction defect {np.abs(got / expect - 1).max():.2e}")
        assert np.all(np.abs(got - expect) <= tol * np.abs(expect)), (face, knob, got, expect)
        assert np.all(R[:, ~on] == 0.0) and np.all(R[:, on] != 0.0), (face, knob)
    for knob in (0, 1):
        with _Knob(knob):
            K0 = brick.assemble_elasticity(A, LAM, MU, 0.0, 0).cpu().numpy()
            for tau in (TAU_REF, TAU_ONE):
                dK = brick.assemble_elasticity(A, LAM, MU, tau, bit).cpu().numpy() - K0
                print(f"CLOSED {face} knob {knob} tau {tau:g}: penalty sum defect {abs(dK.sum() / (-3 * tau * area) - 1):.2e}")
                assert abs(dK.sum() + 3.0 * tau * area) <= tol * 3.0 * tau * area, (face, knob, tau)


# ---- B. every quadrature rule ----------------------------------------------------------------------------------------------------
N_B, PEN_B, TRA_B = (3, 3, 2), "x0|z1", "y1|x0"


@pytest.mark.parametrize("itg", [1, 2, 3, 4, 5, 6, 7])
def test_quadrature_rules_against_the_oracle(mf, itg):
    """ng = (itg + 2) / 2 = 1, 2, 2, 3, 3, 4, 4 Gauss points per direction: both matrix kernels and the residual on a distorted mesh; on the
    uniform and on a sheared mesh (both affine) the matrix kernels with the reference-integral shortcut of that rule and without it (bit 5)."""
    pen, tra = _bits(mf, PEN_B), _bits(mf, TRA_B)
    od = _oracle(X, N_B, PEN_B, TRA_B, itg=itg)
    assert od.elgeo.integral_weights.shape[0] == ((itg + 2) // 2) ** 3
    brick = _brick(mf, X, N_B, itg, od.mesh.coords)
    # the sweep form exists for the 2-point rule only: at every other rule the default residual IS the per-point kernel
    _four_kernels(mf, brick, od, TAU_REF, pen, tra, SIG6, f"B itg={itg} distorted")
    for shape in ("uniform", "sheared"):
        oa = _oracle(X, N_B, PEN_B, TRA_B, itg=itg, shape=shape)
        ba = _brick(mf, X, N_B, itg, oa.mesh.coords)
        A = ba.pattern(3)
        Ks = {}
        for knob in (0, 1 << 5, 1):
            with _Knob(knob):
                Ks[knob] = ba.assemble_elasticity(A, LAM, MU, TAU_REF, pen).cpu().numpy()
            _close(f"B itg={itg} {shape} K knob {knob}", Ks[knob], oa.K_linear, K_TOL)


def test_quadrature_orders_share_their_rule(mf):
    """itg 2 and 3, 4 and 5, 6 and 7 run the same Gauss rule: the same bits from every kernel.  itg 1 (one point) differs from itg 3."""
    import torch

    pen, tra = _bits(mf, PEN_B), _bits(mf, TRA_B)
    m = [v + 1 for v in N_B]
    g = np.indices(m).reshape(3, -1).T * (np.array(X) / np.array(N_B))
    coords = _distort(g, X)
    xs = torch.tensor(0.01 * np.random.default_rng(2).standard_normal(3 * g.shape[0]), device="cuda")
    out = {}
    for itg in range(1, 8):
        brick = _brick(mf, X, N_B, itg, coords)
        A = brick.pattern(3)
        for kern, knob in (("K", 0), ("k", 1), ("R", 0), ("r", 2)):
            with _Knob(knob):
                if kern in "Kk":
                    out[itg, kern] = brick.assemble_elasticity(A, LAM, MU, TAU_REF, pen).cpu().numpy()
                else:
                    out[itg, kern] = brick.residual_elasticity(xs, LAM, MU, TAU_REF, pen, tra, SIG6).cpu().numpy()
    for kern in "KkRr":
        for a, b in ((2, 3), (4, 5), (6, 7)):
            assert np.array_equal(out[a, kern], out[b, kern]), (kern, a, b)
        for a, b in ((1, 3), (3, 5), (5, 7)):
            assert not np.array_equal(out[a, kern], out[b, kern]), (kern, a, b)


# ---- C. lattice edges ------------------------------------------------------------------------------------------------------------
PEN_C, TRA_C = "x0|y1", "z1|y0"
# The residual sweep cuts the planes into segments of L = 4 at every size here (h8_residual_sweep: L halves from 32 while the grid stays below
# 2048 workgroups, down to 4), so 10 planes are segments of 4, 4, 2 and 5 planes are segments of 4 and 1.
CASES_C = [(1, 1, 1), (2, 1, 1), (1, 1, 40), (1, 40, 1), (40, 1, 1),  # one element thick: a block of 32 control points spans many lines and planes
           (2, 1, 30), (2, 1, 31), (2, 1, 32),                        # lines of 31, 32, 33 control points: a block is a line, one short, one over
           (5, 14, 15), (5, 15, 16), (9, 16, 30),                     # residual tiles (15 x 15 control points) cut at 15, 16, 17; 10 planes = 4 + 4 + 2
           (4, 16, 3)]                                                # 5 planes = 4 + 1: a last segment of exactly one plane


@pytest.mark.parametrize("n", CASES_C, ids=["x".join(map(str, n)) for n in CASES_C])
def test_lattice_edges_against_the_oracle(mf, n):
    od = _oracle(X, n, PEN_C, TRA_C)
    brick = _brick(mf, X, n, 3, od.mesh.coords)
    _four_kernels(mf, brick, od, TAU_REF, _bits(mf, PEN_C), _bits(mf, TRA_C), SIG6, f"C n={n}", kernels="KkR")


# ---- D. K and R agree with each other --------------------------------------------------------------------------------------------
def test_residual_is_affine_with_the_matrix_as_its_slope(mf):
    """The problem is linear: R(x) - R(0) = K x, face terms included, on 20 x 33 x 47 distorted elements (12 residual tiles x 6 plane segments,
    1 071 matrix blocks).  Bound: each of the at most 81 entries of a row off by the K tolerance, each of the two residuals by the R tolerance."""
    import scipy.sparse as sp
    import torch

    n = (20, 33, 47)
    pen, tra = _bits(mf, "x1|y0|z1"), _bits(mf, "x0|z0")
    g = np.indices([v + 1 for v in n]).reshape(3, -1).T * (np.array(X) / np.array(n))
    brick = _brick(mf, X, n, 3, _distort(g, X))
    A = brick.pattern(3)
    ncp = A.n // 3
    K = brick.assemble_elasticity(A, LAM, MU, TAU_REF, pen).cpu().numpy()
    Kcsr = sp.csr_matrix((K, A.colidx.cpu().numpy(), A.rowptr.cpu().numpy()), shape=(A.n, A.n))
    assert np.diff(Kcsr.indptr).max() <= 81
    x = 0.01 * np.random.default_rng(2).standard_normal(A.n)
    Rx = brick.residual_elasticity(torch.tensor(x, device="cuda"), LAM, MU, TAU_REF, pen, tra, SIG6).cpu().numpy()
    R0 = brick.residual_elasticity(torch.zeros(A.n, dtype=torch.float64, device="cuda"), LAM, MU, TAU_REF, pen, tra, SIG6).cpu().numpy()
    bound = 81 * (K_TOL * np.abs(K).max()) * np.abs(x).max() + 2 * (R_TOL * np.abs(Rx).max())
    defect = np.abs(Rx - R0 - Kcsr @ x).max()
    print(f"PARITY D |R(x) - R(0) - K x|: {defect / bound:.3f} of bound (defect {defect:.3e}, max|K| {np.abs(K).max():.3e}, max|R| {np.abs(Rx).max():.3e})")
    assert np.abs(K).max() > 0 and np.abs(Rx).max() > 0
    assert defect <= bound
    i, _, k = np.indices([v + 1 for v in n]).reshape(3, -1)
    loaded = (i == 0) | (k == 0)  # traction on x0 | z0
    R0 = R0.reshape(3, ncp)
    assert np.all(R0[:, ~loaded] == 0.0) and np.all(R0[:, loaded] != 0.0)
