"""The guarded diagonal rule of oracle.solvers (guard_zero=True): a stored diagonal equal to +-0.0 keeps d = 1, as the product's kernels do
(csrc/jacobi.hip); the default stays the reference's |K_ii|."""
import numpy as np
import scipy.sparse as sp

from oracle import solvers


def _matrix(seed, n=60):
    """Random rows with a stored nonzero diagonal of either sign; returns the CSR matrix (sorted columns)."""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=0.1, random_state=seed, format="lil")
    M.setdiag(np.where(rng.random(n) < 0.5, -1.0, 1.0) * (1.0 + rng.random(n)))
    M = M.tocsr()
    M.sort_indices()
    return M


def _diag_slots(M):
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    on = np.flatnonzero(rows == M.indices)
    return dict(zip(rows[on].tolist(), on.tolist()))


def test_guard_changes_nothing_without_stored_zeros():
    M = _matrix(1)
    assert np.array_equal(solvers.jacobi_by_diagonal(M), solvers.jacobi_by_diagonal(M, guard_zero=True))
    assert np.array_equal(solvers.jacobi_by_diagonal(M), np.abs(M.diagonal()))
    for f in (solvers.pr_jacobi, solvers.pl_jacobi):
        A0, A1 = M.copy(), M.copy()
        assert np.array_equal(f(A0).jac_vec, f(A1, guard_zero=True).jac_vec)
        assert np.array_equal(A0.data, A1.data)
    b = np.random.default_rng(2).standard_normal(M.shape[0])
    S = (M + M.T).tocsr()
    S.sort_indices()
    x0 = solvers.solve_cg_jacobi(S.indptr, S.indices, S.data, b, 1e-300, 3)
    x1 = solvers.solve_cg_jacobi(S.indptr, S.indices, S.data, b, 1e-300, 3, guard_zero=True)
    assert np.array_equal(x0, x1)


def test_guard_differs_exactly_on_the_stored_zeros_and_missing_rows_give_one():
    M = _matrix(3)
    n = M.shape[0]
    slot = _diag_slots(M)
    zero_p, zero_m, missing = [4, 17, 33], [9, 50], [0, 21, 59]
    M.data[[slot[r] for r in zero_p]] = 0.0
    M.data[[slot[r] for r in zero_m]] = -0.0
    keep = np.ones(M.nnz, dtype=bool)
    keep[[slot[r] for r in missing]] = False
    rows = np.repeat(np.arange(n), np.diff(M.indptr))
    # (built from the arrays: scipy's constructors keep explicitly stored zeros this way)
    A = sp.csr_matrix((M.data[keep], M.indices[keep], np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])), shape=(n, n))
    assert A.nnz == M.nnz - len(missing)
    d0, d1 = solvers.jacobi_by_diagonal(A), solvers.jacobi_by_diagonal(A, guard_zero=True)
    zeros = sorted(zero_p + zero_m)
    assert np.flatnonzero(d0 != d1).tolist() == zeros
    assert np.all(d0[zeros] == 0.0) and np.all(d1[zeros] == 1.0)
    assert np.all(d0[missing] == 1.0) and np.all(d1[missing] == 1.0)
    others = np.setdiff1d(np.arange(n), zeros + missing)
    assert np.array_equal(d1[others], np.abs(A.diagonal()[others])) and np.all(d1[others] > 0.0)
    # the wrappers hand the keyword on
    assert np.array_equal(solvers.pr_jacobi(A.copy(), guard_zero=True).jac_vec, d1)
    assert np.array_equal(solvers.pl_jacobi(A.copy(), guard_zero=True).jac_vec, d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(solvers.pr_jacobi(A.copy()).jac_vec, d0)
    A1 = A.copy()
    solvers.pr_jacobi(A1, guard_zero=True)
    assert np.array_equal(A1.data, A.data / d1[A.indices]) and np.all(np.isfinite(A1.data))
