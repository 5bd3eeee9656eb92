"""The oracle's face conventions for the two thermal boundary forms, pinned by closed forms on an undistorted brick (CPU only).

tests/test_gpu_thermal_edges.py compares the product's Robin and fixed (Nitsche) faces with the oracle face by face; these checks
make that comparison non-circular: the oracle's local face id f (= bit f of the product's face mask), the sign of its normal and
both boundary forms are tested here against h.area and k.n.grad T.area, which need neither code."""
import numpy as np
import pytest

K_COND, H, TENV = 0.6, 25.0, 293.15
X, N = (3.0, 1.0, 2.0), (3, 4, 2)  # all extents and all counts differ: an axis mix-up cannot cancel
# oracle face id f -> (name, normal dimension, outward sign); the names in the order of the product's FACE_BITS
FACES = [("z0", 2, -1.0), ("y0", 1, -1.0), ("x1", 0, 1.0), ("y1", 1, 1.0), ("x0", 0, -1.0), ("z1", 2, 1.0)]
GRAD = 7.0  # dT/dx_nd of the linear temperature field
# the oracle's defect against the closed forms is 4.2e-16 of the expected value at the most (measured); a round bound about 200 x that
CLOSED_FORM_TOL = 1e-13


def _domain(robin=(), fixed=(), h_penalty=0.0, Tw=0.0, x_star=None, itg=3):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, itg)
    msh = om.lattice_mesh(X, N, disc)
    fac = om.boundary_facets_structured(X, N, 3)
    bnd = []
    if robin:
        bnd.append((fac.select(np.isin(fac.element_eindex, robin)), problems.thermal_convection(H, TENV)))
    if fixed:
        bnd.append((fac.select(np.isin(fac.element_eindex, fixed)), problems.thermal_fixed(3, h_penalty, Tw, K_COND)))
    od = fem.FEMDomain(msh, disc, 1, problems.thermal_domain(3, K_COND), bnd)
    od.controlpoints["s"] = np.zeros(msh.ncp)
    od.update_time()
    od.K_linear_func()
    if x_star is not None:
        od.x_star[:] = x_star(msh.coords)
    od.K_nonlinear_func()
    return od


def _lumped_area(nd, sign):
    """The integral of each node's shape function over the face with normal dimension nd: the face element's area / 4 per adjacent face
    element; zero off the face.  Lattice numbering: the last dimension fastest."""
    m = [v + 1 for v in N]
    t1, t2 = (nd + 1) % 3, (nd + 2) % 3
    idx = np.indices(m)
    on = idx[nd] == (N[nd] if sign > 0 else 0)
    cnt = [np.where((idx[t] == 0) | (idx[t] == N[t]), 1.0, 2.0) for t in (t1, t2)]
    a_el = (X[t1] / N[t1]) * (X[t2] / N[t2])
    return (np.where(on, cnt[0] * cnt[1] * a_el / 4.0, 0.0)).ravel(), on.ravel()


def _row_sums(od, K):
    rp = od.pattern.rowptr
    return np.add.reduceat(K, rp[:-1])


@pytest.mark.parametrize("f", range(6))
def test_robin_matrix_times_ones_is_minus_h_lumped_area(f):
    name, nd, sign = FACES[f]
    K0 = _domain().K_linear
    od = _domain(robin=(f,))
    lumped, on = _lumped_area(nd, sign)
    assert abs(lumped.sum() - X[(nd + 1) % 3] * X[(nd + 2) % 3]) <= 1e-14 * lumped.sum()
    got = _row_sums(od, od.K_linear - K0)  # (the volume form annihilates constants only to round-off: its rows are taken out)
    expect = -H * lumped
    scale = np.abs(expect).max()
    print(f"{name}: K_robin 1 defect {np.abs(got - expect).max() / scale:.2e} of max|h area|")
    assert np.all(np.abs(got - expect) <= CLOSED_FORM_TOL * scale), name
    assert np.all(np.abs(got[on]) > 0.1 * H * lumped[on].min()), name
    # and the whole matrix annihilates constants off the face to round-off
    full = _row_sums(od, od.K_linear)
    assert np.all(np.abs(full[~on]) <= CLOSED_FORM_TOL * np.abs(od.K_linear).max() * 27), name


@pytest.mark.parametrize("f", range(6))
def test_fixed_face_flux_term_has_the_outward_normal(f):
    """T = GRAD x_nd: grad T = GRAD e_nd everywhere, so k n.grad T = sign k GRAD on the face with that normal, and the term's residual is
    sign k GRAD times the lumped area at the face's nodes, zero elsewhere.  h_penalty = 0 leaves that term alone."""
    name, nd, sign = FACES[f]
    lin = lambda c: GRAD * c[:, nd] + 1.0
    R0 = _domain(x_star=lin).residue
    od = _domain(fixed=(f,), h_penalty=0.0, x_star=lin)
    lumped, on = _lumped_area(nd, sign)
    got = od.residue - R0
    expect = sign * K_COND * GRAD * lumped
    scale = np.abs(expect).max()
    print(f"{name}: flux residual defect {np.abs(got - expect).max() / scale:.2e} of max|k GRAD area|")
    assert np.all(np.abs(got - expect) <= CLOSED_FORM_TOL * scale), name
    assert np.all(np.sign(got[on]) == sign), name
    # the matrix of that term: rows of face nodes only, and K 1 = 0 (a constant has no flux)
    dK = od.K_linear - _domain().K_linear
    rp = od.pattern.rowptr
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    touched = np.abs(dK) > CLOSED_FORM_TOL * K_COND
    assert touched.sum() > 0 and np.all(on[rows[touched]]), name
    assert np.all(np.abs(_row_sums(od, dK)) <= CLOSED_FORM_TOL * np.abs(dK).max() * 27), name


@pytest.mark.parametrize("itg", [1, 2, 3, 4, 5, 6, 7])
def test_the_oracle_builds_every_rule_on_the_first_order_cube(itg):
    """Even orders included: (itg + 2) / 2 Gauss points per direction, weights that sum to the element's volume, and the same matrix from
    the two orders that share a rule (tests/test_gpu_thermal_edges.py part B relies on the oracle at every itg_order)."""
    od = _domain(robin=(2,), itg=itg)
    w = od.elgeo.integral_weights
    assert w.shape == (((itg + 2) // 2) ** 3, np.prod(N))
    vol = np.prod(X) / np.prod(N)
    assert np.all(np.abs(w.sum(axis=0) - vol) <= 1e-14 * vol)
    if itg % 2 == 0:
        assert np.array_equal(od.K_linear, _domain(robin=(2,), itg=itg + 1).K_linear)


@pytest.mark.parametrize("hp", [1.0, 1000.0])
@pytest.mark.parametrize("f", range(6))
def test_fixed_face_penalty_term(f, hp):
    """T = TW + 2 everywhere: the flux term vanishes and the penalty residual is h_penalty (Tw - T) = -2 h_penalty times the lumped area."""
    name, nd, sign = FACES[f]
    tw = 1173.15
    const = lambda c: np.full(c.shape[0], tw + 2.0)
    R0 = _domain(x_star=const).residue
    od = _domain(fixed=(f,), h_penalty=hp, Tw=tw, x_star=const)
    lumped, on = _lumped_area(nd, sign)
    got = od.residue - R0
    expect = -2.0 * hp * lumped
    scale = np.abs(expect).max()
    # (the flux term of a constant is zero to round-off of k T / h: 1e3 / 0.25 * 1e-16, against a penalty residual of 2 hp area)
    print(f"{name} hp={hp}: penalty residual defect {np.abs(got - expect).max() / scale:.2e}")
    assert np.all(np.abs(got - expect) <= 1e-11 * scale), name
