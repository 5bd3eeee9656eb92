"""The oracle's face conventions for the elasticity boundary terms, pinned by closed forms on an undistorted brick (CPU only).

tests/test_gpu_elasticity_edges.py compares the product's traction and penalty terms with the oracle face by face; these checks
make that comparison non-circular: the oracle's local face id f (= bit f of the product's face mask), the sign of its normal and
the use of the full traction tensor are tested here against sigma.n.area and tau.area, which need neither code."""
import numpy as np
import pytest

E_MOD, NU = 1.0, 0.3
LAM, MU = E_MOD * NU / ((1 + NU) * (1 - 2 * NU)), E_MOD / (2 * (1 + NU))
X, N = (3.0, 1.0, 2.0), (3, 4, 2)  # all extents and all counts differ: an axis mix-up cannot cancel
SIG = np.array([[0.7, -0.4, 0.25], [-0.4, 1.0, 0.55], [0.25, 0.55, -0.3]])  # six distinct non-zero components
# oracle face id f -> (name, normal dimension, outward sign); the names in the order of the product's FACE_BITS
FACES = [("z0", 2, -1.0), ("y0", 1, -1.0), ("x1", 0, 1.0), ("y1", 1, 1.0), ("x0", 0, -1.0), ("z1", 2, 1.0)]
# the oracle's defect against the closed forms is 9e-16 of the expected value (measured); a round bound about 100 x that
CLOSED_FORM_TOL = 1e-13


def _domain(pen=(), tra=(), tau=1.0):
    from oracle import fem, mesh as om, problems, reference_element as re_

    disc = re_.initialize_classical_element(3, "CUBE", 1, 1, 3)
    msh = om.lattice_mesh(X, N, disc)
    fac = om.boundary_facets_structured(X, N, 3)
    bnd = []
    if pen:
        bnd.append((fac.select(np.isin(fac.element_eindex, pen)), problems.elasticity_penalty(3, tau)))
    if tra:
        bnd.append((fac.select(np.isin(fac.element_eindex, tra)), problems.elasticity_traction(3, SIG.tolist())))
    od = fem.FEMDomain(msh, disc, 3, problems.elasticity_domain(3, LAM, MU), bnd)
    od.update_time()
    od.K_linear_func()
    od.K_nonlinear_func()  # x_star = 0
    return od


def _area(nd):
    return X[(nd + 1) % 3] * X[(nd + 2) % 3]


def _on_face(coords, nd, sign):
    return np.isclose(coords[:, nd], X[nd] if sign > 0 else 0.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("f", range(6))
def test_facet_selection_is_the_named_face(f):
    from oracle import mesh as om

    name, nd, sign = FACES[f]
    fac = om.boundary_facets_structured(X, N, 3)
    sel = fac.select(fac.element_eindex == f)
    assert len(sel) == N[(nd + 1) % 3] * N[(nd + 2) % 3], name
    assert np.all(sel.centroid[:, nd] == (X[nd] if sign > 0 else 0.0)), name


@pytest.mark.parametrize("f", range(6))
def test_net_traction_is_sigma_n_area_and_zero_off_the_face(f):
    name, nd, sign = FACES[f]
    od = _domain(tra=(f,))
    R = od.residue.reshape(3, -1)
    nrm = np.zeros(3)
    nrm[nd] = sign
    expect = SIG @ nrm * _area(nd)
    assert np.all(expect != 0.0)
    got = R.sum(axis=1)
    print(f"{name}: net traction {got}, expected {expect}, defect {np.abs(got / expect - 1).max():.2e}")
    assert np.all(np.abs(got - expect) <= CLOSED_FORM_TOL * np.abs(expect)), name
    on = _on_face(od.mesh.coords, nd, sign)
    # (off the face the oracle's facet shape functions vanish to round-off, not exactly: 3.5e-18 measured on x1)
    assert np.all(np.abs(R[:, ~on]) <= CLOSED_FORM_TOL * np.abs(expect).min()), name
    assert np.all(np.abs(R[:, on]) > 1e-3 * np.abs(expect).min() / on.sum()), name


@pytest.mark.parametrize("tau", [1.0, 1000.0 * E_MOD])
@pytest.mark.parametrize("f", range(6))
def test_penalty_matrix_sums_to_minus_three_tau_area(f, tau):
    name, nd, sign = FACES[f]
    K0 = _domain().K_linear
    od = _domain(pen=(f,), tau=tau)
    dK = od.K_linear - K0
    expect = -3.0 * tau * _area(nd)
    print(f"{name} tau={tau}: sum {dK.sum()!r}, expected {expect!r}, defect {abs(dK.sum() / expect - 1):.2e}")
    assert abs(dK.sum() - expect) <= CLOSED_FORM_TOL * abs(expect), name
    # the penalty couples only nodes of the face, and only a field with itself
    rp, ci = od.pattern.rowptr, od.pattern.colidx
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    ncp = od.mesh.ncp
    on = _on_face(od.mesh.coords, nd, sign)
    touched = np.abs(dK) > CLOSED_FORM_TOL * abs(expect)  # (as above: zero to round-off elsewhere)
    assert touched.sum() > 0
    assert np.all(on[rows[touched] % ncp]) and np.all(on[ci[touched] % ncp]), name
    assert np.all(rows[touched] // ncp == ci[touched] // ncp), name
