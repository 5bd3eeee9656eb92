"""The Jacobi kernels of csrc/jacobi.hip against host references, at their edges.

The guarded diagonal rule -- a row without a stored diagonal keeps its preset, and so does a row whose stored diagonal is exactly +-0.0 -- lives in
k_jacobi_rows mode 0 and in k_jacobi_diag_table (through the uint16 table k_diag_offsets builds); the expected value is oracle.solvers.jacobi_by_diagonal
with guard_zero=True, bit for bit.  The norms are compared with longdouble sums: |got - ref| <= (len + 2) eps ref holds for a float64 sum of len
non-negative terms in ANY order (each of the len - 1 additions and the len squarings adds at most eps / 2 relative, the square root halves the sum's
relative error and rounds once more), so it covers the atomics of the column kernel and the lane order of the row kernel.  Every matrix comes from a fixed
seed; the references are built with numpy and scipy, never with the library.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LENS = (0, 1, 7, 8, 9, 16, 17, 27, 81)   # the 8-lane group in its first, second and later trips
POS = ("first", "last", "eighth")
KINDS = ("missing", "+0", "-0", "negative", "positive")
BLOCK = 256                              # csrc/common.h MFEM_BLOCK; every launch here is capped at 16 workgroups per CU (mfem_grid_for)


# -- host side ------------------------------------------------------------------------------------------------------------------------------------------
def _grid_matrix(n, seed=5):
    """(rowptr, col, vals, kinds) base 0: row r takes the (length, diagonal position, diagonal kind) combination (r + 28) mod 135 (row 0: one stored
    +0.0, so that n = 1 is not an empty matrix), the length cut to what n columns allow.  Rows with r % 3 == 0 list their off-diagonal columns in random order; a diagonal put first / last / at position 8 leaves the row
    unsorted anyway."""
    rng = np.random.default_rng(seed)
    rowptr, cols, vals, kinds = [0], [], [], []
    for r in range(n):
        c = (r + 28) % (len(LENS) * len(POS) * len(KINDS))
        ln, pos, kind = LENS[c % 9], POS[(c // 9) % 3], KINDS[c // 27]
        ln = min(ln, n - 1 if kind == "missing" else n)
        if ln == 0:
            kind = "missing"
        others = np.setdiff1d(np.arange(n), [r])
        pick = np.sort(rng.choice(others, size=ln if kind == "missing" else ln - 1, replace=False))
        if r % 3 == 0:
            pick = rng.permutation(pick)
        v = rng.standard_normal(pick.size)
        v[v == 0.0] = 1.0
        if kind != "missing":
            at = {"first": 0, "last": ln - 1, "eighth": min(8, ln - 1)}[pos]
            dv = {"+0": 0.0, "-0": -0.0, "negative": -(1.0 + rng.random()), "positive": 1.0 + rng.random()}[kind]
            pick = np.insert(pick, at, r)
            v = np.insert(v, at, dv)
        cols.append(pick)
        vals.append(v)
        kinds.append(kind)
        rowptr.append(rowptr[-1] + pick.size)
    cat = (lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t))
    return np.array(rowptr, dtype=np.int64), cat(cols, np.int32), cat(vals, np.float64), kinds


def _guarded(rowptr, col, vals, n):
    from oracle import solvers

    return solvers.jacobi_by_diagonal(sp.csr_matrix((vals, col, rowptr), shape=(n, n)), guard_zero=True)


def _norms(index, vals, m):
    """(longdouble 2-norms, entry counts) of the entries grouped by `index` (rows or columns), m groups."""
    s = np.zeros(m, dtype=np.longdouble)
    v = vals.astype(np.longdouble)
    np.add.at(s, index, v * v)
    return np.sqrt(s), np.bincount(index, minlength=m)


def _assert_norm(got, ref, cnt):
    got = got.astype(np.longdouble)
    assert np.all(got[cnt == 0] == 0.0)
    excess = np.abs(got - ref) - (cnt + 2) * np.longdouble(EPS) * ref
    worst = int(np.argmax(excess))
    assert excess[worst] <= 0, (worst, float(got[worst]), float(ref[worst]), int(cnt[worst]))


def _rows_of(rowptr):
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def _handle(mf, rowptr, col, n, rp="int64", base=0):
    import torch

    rp_t = torch.tensor((rowptr + base).astype(rp), device="cuda")
    c_t = torch.tensor((col + base).astype(np.int32), device="cuda") if col.size else torch.zeros(0, dtype=torch.int32, device="cuda")
    return mf.FEM_SpMat_CSR(rp_t, c_t, n, index_base=base)


def _check_all(mf, rowptr, col, vals, n, rp, base, preset=True):
    """The four kernels on one matrix against the host references."""
    import torch
    from metafem_jl_amd import _lib

    A = _handle(mf, rowptr, col, n, rp, base)
    v = torch.tensor(vals, device="cuda")
    d_ref = _guarded(rowptr, col, vals, n)
    d1 = mf.jacobi_by_diagonal(A, v).cpu().numpy()
    d2 = mf.jacobi_by_diagonal(A, v).cpu().numpy()   # (the first call built the table, the second reads it)
    assert np.array_equal(d1, d_ref) and np.array_equal(d2, d_ref)
    rows = _rows_of(rowptr)
    if preset:  # "keeps its preset", not "writes 1"
        d7 = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib.mfem_jacobi_by_diagonal(A.ctx._h, A._h, C.c_void_p(v.data_ptr()), C.c_void_p(d7.data_ptr())))
        on = (rows == col) & (vals != 0.0)
        want = np.full(n, 7.0)
        want[rows[on]] = np.abs(vals[on])
        assert np.array_equal(d7.cpu().numpy(), want)
        assert np.count_nonzero(want == 7.0) == n - np.count_nonzero(on)
    _assert_norm(mf.jacobi_by_row(A, v).cpu().numpy(), *_norms(rows, vals, n))
    _assert_norm(mf.jacobi2_by_column(A, v).cpu().numpy(), *_norms(col, vals, n))
    mf.mat_div_jacobi_(A, v, torch.tensor(d_ref, device="cuda"))
    assert np.array_equal(v.cpu().numpy(), vals / d_ref[col])
    return A


# -- the row content grid -------------------------------------------------------------------------------------------------------------------------------
_GRID = {}


def _grid(n):
    if n not in _GRID:
        _GRID[n] = _grid_matrix(n)
    return _GRID[n]


def test_the_grid_matrix_holds_every_combination():
    rowptr, col, vals, kinds = _grid(300)
    rows = _rows_of(rowptr)
    lens = np.diff(rowptr)
    assert set(lens.tolist()) >= set(LENS)
    seen = set()
    for r in range(300):
        seg = col[rowptr[r]:rowptr[r + 1]]
        at = np.flatnonzero(seg == r)
        assert at.size == (0 if kinds[r] == "missing" else 1)
        if at.size:
            dv = vals[rowptr[r] + at[0]]
            kind = "+0" if dv == 0 and not np.signbit(dv) else "-0" if dv == 0 else "negative" if dv < 0 else "positive"
            assert kind == kinds[r]
            seen.add((int(lens[r]), "first" if at[0] == 0 else "last" if at[0] == lens[r] - 1 else int(at[0]), kind))
        else:
            seen.add((int(lens[r]), None, "missing"))
    for ln in LENS[1:]:
        assert (ln, None, "missing") in seen
        for kind in KINDS[1:]:
            assert (ln, "first", kind) in seen and ((ln, "last", kind) in seen or ln == 1)
            assert ln <= 9 or (ln, 8, kind) in seen   # (position 8 is the last one of a 9-entry row and does not exist in shorter ones)
    assert any(np.any(np.diff(col[rowptr[r]:rowptr[r + 1]]) < 0) for r in range(300))
    assert np.count_nonzero(rows == col) > 0


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("rp", ["int32", "int64"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 300])
def test_row_content_grid(mf, n, rp, base):
    """One workgroup holds 32 row groups of 8 lanes: n = 31, 32, 33 sit around that edge; n = 300 holds every (length, position, kind) twice."""
    rowptr, col, vals, _ = _grid(n)
    _check_all(mf, rowptr, col, vals, n, rp, base)


# -- the uint16 offset table ----------------------------------------------------------------------------------------------------------------------------
def _long_row_matrix(case):
    """n = 70 000, tridiagonal short rows (every 7th without its diagonal, every 11th with a stored zero), row 65 530 replaced by a long one."""
    n, big = 70000, 65530
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(n), 3)
    cols = rows + np.tile([-1, 0, 1], n)
    keep = (cols >= 0) & (cols < n) & ~((cols == rows) & (rows % 7 == 0)) & (rows != big)
    rows, cols = rows[keep], cols[keep]
    vals = rng.standard_normal(rows.size)
    vals[(cols == rows) & (rows % 11 == 0)] = 0.0
    if case == "table":            # 65 534 entries, the diagonal at offset 65 530: max_row_nnz < 0xFFFF
        long_cols = np.arange(65534)
    elif case == "row-scan":       # 65 535 entries: max_row_nnz == 0xFFFF, the gate sends every row to k_jacobi_rows
        long_cols = np.arange(65535)
    else:                          # 65 534 entries, the diagonal last: offset 65 533, the largest the table can hold beside its sentinel
        long_cols = np.concatenate([np.setdiff1d(np.arange(65534), [big]), [big]])
    at = int(np.searchsorted(rows, big))
    rows = np.concatenate([rows[:at], np.full(long_cols.size, big), rows[at:]])
    cols = np.concatenate([cols[:at], long_cols, cols[at:]])
    vals = np.concatenate([vals[:at], rng.standard_normal(long_cols.size), vals[at:]])
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return n, big, rowptr, cols.astype(np.int32), vals


@pytest.mark.parametrize("case", ["table", "row-scan", "diagonal-last"])
def test_uint16_offset_table(mf, case):
    import torch

    n, big, rowptr, col, vals = _long_row_matrix(case)
    ln = int(rowptr[big + 1] - rowptr[big])
    assert ln == (65535 if case == "row-scan" else 65534) and ln == np.diff(rowptr).max()
    off = int(np.flatnonzero(col[rowptr[big]:rowptr[big + 1]] == big)[0])
    assert off == (65533 if case == "diagonal-last" else 65530)
    A = _handle(mf, rowptr, col, n, "int32", 0)
    v = torch.tensor(vals, device="cuda")
    d_ref = _guarded(rowptr, col, vals, n)
    assert d_ref[big] == abs(vals[rowptr[big] + off]) and np.count_nonzero(d_ref == 1.0) >= n // 7
    first = mf.jacobi_by_diagonal(A, v).cpu().numpy()    # builds the table (or scans the rows)
    second = mf.jacobi_by_diagonal(A, v).cpu().numpy()
    assert np.array_equal(first, second)
    assert np.array_equal(first, d_ref)
    _assert_norm(mf.jacobi_by_row(A, v).cpu().numpy(), *_norms(_rows_of(rowptr), vals, n))   # a 65 534-term row sum under the bound


# -- grid-stride second trips ---------------------------------------------------------------------------------------------------------------------------
def test_second_grid_stride_trips(mf):
    """Every launch is capped at 16 workgroups of 256 threads per CU (mfem_grid_for): 512 CUs rows for the 8-lane kernels, 4096 CUs rows for the table
    kernel, 4096 CUs nonzeros for the column kernel, 8192 CUs nonzeros (two per thread) for mat_div_jacobi.  A tridiagonal matrix of 4096 CUs + 37 rows
    exceeds all four."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap_threads = 16 * cus * BLOCK
    n = cap_threads + 37
    rng = np.random.default_rng(13)
    rows = np.repeat(np.arange(n), 3)
    cols = rows + np.tile([-1, 0, 1], n)
    keep = (cols >= 0) & (cols < n) & ~((cols == rows) & ((rows % 1000 == 0) | (rows == n - 5)))   # (+ one in the table kernel's second trip)
    rows, cols = rows[keep], cols[keep]
    vals = rng.standard_normal(rows.size)
    vals[(cols == rows) & ((rows % 1001 == 0) | (rows == n - 3))] = 0.0
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    assert n > cap_threads // 8 and n > cap_threads and rows.size > cap_threads and rows.size > 2 * cap_threads
    d_ref = _guarded(rowptr, cols, vals, n)
    assert np.count_nonzero(d_ref[cap_threads:] == 1.0) >= 2 and d_ref[n - 1] == abs(vals[-1])   # (edge rows live in the second trip)
    _check_all(mf, rowptr, cols.astype(np.int32), vals, n, "int64", 0)


# -- mat_div_jacobi: alignment and parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ["aligned", "vals+8B", "colidx+4B"])
@pytest.mark.parametrize("nnz", [1, 2, 513, 514])
def test_mat_div_jacobi_alignment_and_parity(mf, nnz, shift):
    """The 16-byte path needs vals 16-byte and colidx 8-byte aligned and writes an odd tail from thread 0; a view one element in forces the scalar path."""
    import torch

    n = 64
    rng = np.random.default_rng(100 + nnz)
    flat = np.sort(rng.choice(n * n, size=nnz, replace=False))
    rows, col = flat // n, (flat % n).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    vals = rng.standard_normal(nnz)
    d = 0.5 + rng.random(n)
    vbuf = torch.zeros(nnz + 3, dtype=torch.float64, device="cuda")
    cbuf = torch.zeros(nnz + 3, dtype=torch.int32, device="cuda")
    v0 = 1 if shift == "vals+8B" else 2
    v = vbuf[v0:v0 + nnz]
    c = cbuf[1:1 + nnz] if shift == "colidx+4B" else cbuf[2:2 + nnz]
    assert v.data_ptr() % 16 == (8 if shift == "vals+8B" else 0) and c.data_ptr() % 8 == (4 if shift == "colidx+4B" else 0)
    v.copy_(torch.tensor(vals))
    c.copy_(torch.tensor(col))
    A = mf.FEM_SpMat_CSR(torch.tensor(rowptr, device="cuda"), c, n)
    mf.mat_div_jacobi_(A, v, torch.tensor(d, device="cuda"))
    assert np.array_equal(v.cpu().numpy(), vals / d[col])
    guard = vbuf.cpu().numpy()
    assert np.all(guard[:v0] == 0.0) and np.all(guard[v0 + nnz:] == 0.0)   # nothing written outside the view


# -- column norms on a slab pattern ---------------------------------------------------------------------------------------------------------------------
def test_column_norms_fill_the_ghost_columns_without_a_communicator(mf):
    """A slab pattern addresses ghost columns behind the owned ones (ncols > n).  With no communicator nothing exchanges them: all ncols entries are
    the column 2-norms of the local rectangular matrix."""
    b = mf.make_Brick((1.0, 1.0, 1.0), (12, 5, 6))
    b.set_slab(4, 9)
    A = b.pattern(1)
    n, ncols = A.n, A.ncols
    assert ncols > n
    K = mf.FEM_rand(A.nnz, 21, 0) - 0.5
    col = A.colidx.cpu().numpy().astype(np.int64) - A.index_base
    assert col.max() == ncols - 1 and np.count_nonzero(col >= n) > 0
    ref, cnt = _norms(col, K.cpu().numpy(), ncols)
    assert np.all(cnt[n:] > 0)
    _assert_norm(mf.jacobi2_by_column(A, K).cpu().numpy(), ref, cnt)
