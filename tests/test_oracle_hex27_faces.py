"""The oracle's face conventions on order-2 (hex-27) facets, pinned by closed forms on a sheared brick and by a quadrature written out
here on a curved one (CPU only); the order-2 twin of tests/test_oracle_thermal_faces.py.

tests/test_gpu_hex27_edges.py compares the product's hex-27 Robin and fixed (Nitsche) faces with the oracle face by face.  These checks
make that comparison non-circular: the oracle's local face id f (= bit f of the product's face mask), the sign and the direction of its
normal and both boundary forms are tested against h.area and k.n.grad T.area per node.  The brick is the image of the lattice under
c -> S c + b with the full, nonsymmetric S of the GPU tests' sheared shape: no face normal is a coordinate axis, the three face
pairs have three different areas per element, and the Lagrange-2 basis still reproduces constants and linear fields exactly, so the
closed forms hold to round-off: a face element's area is |cof(S) e_nd| times the lattice area, its normal sign cof(S) e_nd normalised,
and the integral of the 1-D Lagrange-2 shape functions over an element is 1/6, 4/6, 1/6 of its length."""
import numpy as np
import pytest

K_COND, H, TENV = 0.6, 25.0, 293.15
X, N = (3.0, 1.0, 2.0), (3, 2, 1)  # all extents and all counts differ: an axis mix-up cannot cancel
M = tuple(2 * v + 1 for v in N)
# oracle face id f -> (name, normal dimension, outward sign); the names in the order of the product's FACE_BITS
FACES = [("z0", 2, -1.0), ("y0", 1, -1.0), ("x1", 0, 1.0), ("y1", 1, 1.0), ("x0", 0, -1.0), ("z1", 2, 1.0)]
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])
OFFSET = np.array([0.3, -0.2, 0.1])
COF = np.linalg.det(SHEAR) * np.linalg.inv(SHEAR).T  # cof(S) e_nd = (S t1) x (S t2) for the cyclic (nd, t1, t2)
GRAD = np.array([7.0, -3.0, 5.0])  # grad T of the linear temperature field
# the oracle's defect against the closed forms is 7.0e-15 of the expected value at the most (measured); a round bound above that
CLOSED_FORM_TOL = 1e-13


def _distort(c):
    """The curved shape of the GPU tests (tests/test_gpu_thermal.py)."""
    out = c.copy()
    out[:, 0] += 0.03 * np.sin(3 * c[:, 1]) * np.cos(2 * c[:, 2])
    out[:, 1] += 0.02 * np.sin(2 * c[:, 0] + c[:, 2])
    out[:, 2] += 0.025 * c[:, 0] * c[:, 1]
    return out


def _domain(robin=(), fixed=(), h_penalty=0.0, Tw=0.0, x_star=None, itg=5, shape="sheared", x=X, n=N):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 2, 1, itg)
    msh = om.lattice_mesh(x, n, disc)
    if shape == "sheared":
        msh.coords[:] = msh.coords @ SHEAR.T + OFFSET
    elif shape == "curved":
        msh.coords[:] = _distort(msh.coords)
    else:
        assert shape == "uniform"
    fac = om.boundary_facets_structured(x, n, 3)
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


def _lumped_1d(t):
    """The integrals of the 1-D Lagrange-2 lattice functions of direction t, in element lengths: 1/6 at the two ends, 2/6 at the other
    element boundaries (even lattice points), 4/6 at the mid-points (odd)."""
    i = np.arange(M[t])
    return np.where(i % 2 == 1, 4.0, np.where((i == 0) | (i == M[t] - 1), 1.0, 2.0)) / 6.0


def _lumped_area(nd, sign):
    """The integral of each node's shape function over the sheared face with normal dimension nd; zero off the face.  Lattice numbering: the
    last dimension fastest."""
    t1, t2 = (nd + 1) % 3, (nd + 2) % 3
    idx = np.indices(M)
    on = idx[nd] == (M[nd] - 1 if sign > 0 else 0)
    a_el = np.linalg.norm(COF[:, nd]) * (X[t1] / N[t1]) * (X[t2] / N[t2])
    lump = _lumped_1d(t1)[idx[t1]] * _lumped_1d(t2)[idx[t2]] * a_el
    return np.where(on, lump, 0.0).ravel(), on.ravel()


def _normal(nd, sign):
    return sign * COF[:, nd] / np.linalg.norm(COF[:, nd])


def _row_sums(od, K):
    return np.add.reduceat(K, od.pattern.rowptr[:-1])


def test_the_lattice_numbering_and_the_lumped_areas_are_what_the_closed_forms_assume():
    od = _domain(shape="uniform")
    assert od.mesh.ncp == np.prod(M)
    assert np.array_equal(od.mesh.coords, np.indices(M).reshape(3, -1).T * (np.array(X) / np.array(N) / 2))
    for _, nd, sign in FACES:
        lumped, _ = _lumped_area(nd, sign)
        t1, t2 = (nd + 1) % 3, (nd + 2) % 3
        total = np.linalg.norm(COF[:, nd]) * X[t1] * X[t2]
        assert abs(lumped.sum() - total) <= 1e-14 * total
        # (the normal is the cross product of the face's mapped tangents, outward)
        assert np.allclose(COF[:, nd], np.cross(SHEAR[:, t1], SHEAR[:, t2]), rtol=1e-14, atol=1e-15)
        assert sign * _normal(nd, sign) @ SHEAR[:, nd] > 0


@pytest.mark.parametrize("f", range(6))
def test_robin_matrix_times_ones_is_minus_h_lumped_area(f):
    name, nd, sign = FACES[f]
    K0 = _domain().K_linear
    od = _domain(robin=(f,))
    lumped, on = _lumped_area(nd, sign)
    got = _row_sums(od, od.K_linear - K0)  # (the volume form annihilates constants only to round-off: its rows are taken out)
    expect = -H * lumped
    scale = np.abs(expect).max()
    print(f"{name}: K_robin 1 defect {np.abs(got - expect).max() / scale:.2e} of max|h area|")
    assert np.all(np.abs(got - expect) <= CLOSED_FORM_TOL * scale), name
    assert np.all(np.abs(got[on]) > 0.1 * H * lumped[on].min()), name
    # and the whole matrix annihilates constants off the face to round-off
    full = _row_sums(od, od.K_linear)
    assert np.all(np.abs(full[~on]) <= CLOSED_FORM_TOL * np.abs(od.K_linear).max() * 125), name


@pytest.mark.parametrize("f", range(6))
def test_fixed_face_flux_term_has_the_outward_normal(f):
    """T = GRAD . x + 1 is reproduced exactly on the sheared brick: k n.grad T = k n.GRAD on the face, with n the unit normal of the sheared
    face (no coordinate axis), and the term's residual is that times the lumped area at the face's nodes, zero elsewhere.  h_penalty = 0
    leaves that term alone."""
    name, nd, sign = FACES[f]
    lin = lambda c: c @ GRAD + 1.0
    R0 = _domain(x_star=lin).residue
    od = _domain(fixed=(f,), h_penalty=0.0, x_star=lin)
    lumped, on = _lumped_area(nd, sign)
    got = od.residue - R0
    flux = K_COND * (_normal(nd, sign) @ GRAD)
    expect = flux * lumped
    scale = np.abs(expect).max()
    print(f"{name}: flux residual defect {np.abs(got - expect).max() / scale:.2e} of max|k n.GRAD area| (k n.GRAD = {flux:.3f})")
    assert abs(flux) > 0.5  # (no face on which the field has no flux)
    # (the residual without the face is -k (grad N, grad T) = O(k |GRAD| h) per node with round-off 1e-16 of the volume terms it sums)
    assert np.all(np.abs(got - expect) <= CLOSED_FORM_TOL * max(scale, np.abs(R0).max())), name
    assert np.all(np.sign(got[on]) == np.sign(flux)), name
    # the same field against the opposite normal would change the sign: the opposite face sees -flux
    opp = _normal(nd, -sign) @ GRAD
    assert np.sign(opp) == -np.sign(flux)
    # the matrix of that term: rows of face nodes only, and K 1 = 0 (a constant has no flux)
    dK = od.K_linear - _domain().K_linear
    rp = od.pattern.rowptr
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    touched = np.abs(dK) > CLOSED_FORM_TOL * K_COND
    assert touched.sum() > 0 and np.all(on[rows[touched]]), name
    assert np.all(np.abs(_row_sums(od, dK)) <= CLOSED_FORM_TOL * np.abs(dK).max() * 125), name


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
    assert np.all(got[~on] == 0.0) or np.abs(got[~on]).max() <= 1e-11 * scale, name


def _gauss(ng):
    p, w = np.polynomial.legendre.leggauss(ng)
    return p / 2 + 0.5, w / 2


def _lag2(x):
    return (np.array([2 * (x - 0.5) * (x - 1), -4 * x * (x - 1), 2 * x * (x - 0.5)]), np.array([4 * x - 3, -8 * x + 4, 4 * x - 1]))


@pytest.mark.parametrize("f", range(6))
def test_robin_row_sums_on_the_curved_brick_against_a_quadrature_written_out_here(f):
    """The curved faces of the GPU tests' distorted shape have no closed form; the lumped area per node is integrated here, face element
    by face element, with the same 3 x 3 Gauss rule on the nine face nodes (plain numpy, no oracle code)."""
    name, nd, sign = FACES[f]
    od = _domain(robin=(f,), shape="curved")
    K0 = _domain(shape="curved").K_linear
    c = od.mesh.coords.reshape(*M, 3)
    t1, t2 = (nd + 1) % 3, (nd + 2) % 3
    gp, gw = _gauss(3)
    lumped = np.zeros(M)
    for e1 in range(N[t1]):
        for e2 in range(N[t2]):
            sl = [None, None, None]
            sl[nd] = M[nd] - 1 if sign > 0 else 0
            sl[t1], sl[t2] = slice(2 * e1, 2 * e1 + 3), slice(2 * e2, 2 * e2 + 3)
            Xf = c[tuple(sl)]  # [3][3][xyz], the axes in the order of (t1, t2) as they appear in (0, 1, 2)
            if t1 > t2:
                Xf = Xf.transpose(1, 0, 2)
            loc = np.zeros((3, 3))
            for q1 in range(3):
                for q2 in range(3):
                    (L1, D1), (L2, D2) = _lag2(gp[q1]), _lag2(gp[q2])
                    ta = np.einsum("a,b,abi->i", D1, L2, Xf)
                    tb = np.einsum("a,b,abi->i", L1, D2, Xf)
                    loc += gw[q1] * gw[q2] * np.linalg.norm(np.cross(ta, tb)) * np.outer(L1, L2)
            if t1 > t2:
                loc = loc.T
            lumped[tuple(sl)] += loc
    got = _row_sums(od, od.K_linear - K0)
    expect = -H * lumped.ravel()
    scale = np.abs(expect).max()
    print(f"{name}: curved K_robin 1 defect {np.abs(got - expect).max() / scale:.2e} of max|h area|")
    assert np.all(np.abs(got - expect) <= CLOSED_FORM_TOL * scale), name


@pytest.mark.parametrize("itg", range(8))
def test_the_oracle_builds_every_rule_on_the_order_two_cube(itg):
    """All eight orders: (itg + 2) // 2 Gauss points per direction and weights that sum to the element's volume."""
    od = _domain(robin=(2,), itg=itg, shape="uniform")
    w = od.elgeo.integral_weights
    assert w.shape == (((itg + 2) // 2) ** 3, np.prod(N))
    vol = np.prod(X) / np.prod(N)
    assert np.all(np.abs(w.sum(axis=0) - vol) <= 1e-14 * vol)


@pytest.mark.parametrize("shape", ["uniform", "curved"])
@pytest.mark.parametrize("itg", [0, 2, 4, 6])
def test_the_two_orders_of_one_rule_give_the_same_bits(itg, shape):
    """itg and itg + 1 share a rule: the same K_linear and the same residual, bit for bit, with both boundary terms present
    (tests/test_gpu_hex27_edges.py part B compares the product with the oracle at every order, and the product's two orders with each
    other)."""
    rest, x0 = (0, 1, 2, 3, 5), (4,)
    field = lambda c: 300.0 + 20.0 * np.sin(c @ np.array([1.0, 2.0, 3.0]))
    kw = dict(robin=rest, fixed=x0, h_penalty=1.0, Tw=1173.15, x_star=field, shape=shape, n=(2, 1, 2))
    a, b = _domain(itg=itg, **kw), _domain(itg=itg + 1, **kw)
    assert np.abs(a.K_linear).max() > 0
    assert np.array_equal(a.K_linear, b.K_linear)
    assert np.array_equal(a.residue, b.residue)
