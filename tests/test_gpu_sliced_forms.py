"""The two forms of the sliced solver layout (mode 3) -- the row-sorted SELL-128 of csrc/spmv_sell.hip and the node-blocked form of
csrc/spmv_bsell.hip -- on real meshes and on small adversarial node graphs, against the CSR arrays multiplied on the host in numpy.longdouble.

A node graph P1 on ncp nodes is expanded to the field-major F-field pattern kron(ones(F, F), P1): row f * ncp + i lists j + g * ncp for g < F, j in
list(i).  Every entry gets an independent random value in [-0.5, 0.5), so a misplaced value cannot cancel.  Every case lifts the size limits
(layout_min_rows = (0, 0)), makes a fresh pattern handle after setting its knobs and asserts the form it was written for: mode 3, the field count of the
node-blocked form (0: row-sorted), and the node-blocked product counter.

Bounds (derived, not measured): per row |y_i - ref_i| <= (len_i + 4) 2^-52 (|alpha| sum_j |a_ij x_j| + |beta y0_i|) -- any summation order, with or
without FMA, plus the roundings of alpha, beta and the final sum --; the fused x . y against the longdouble sum over the DEVICE's y:
(n + 2) 2^-52 sum |x_i y_i|.  The solves take TOL_X and TOL_RES of tests/test_gpu_krylov_scale.py.

Systems (maxL: the longest node list; copy: what bsell_copy(maxL, F, knobs) binds through by default -- "t" k_bsell_fill_t, the LDS transpose, up to
BSELL_T_MAXL = 127 coupled nodes, "q" k_bsell_fill, the lane quads, beyond; every accepted system runs again with the quads forced, bsell = 3, and on
the row-sorted form, bsell = 0).  y, dot: the largest error / bound seen on one MI355X over all formats, knobs and products of the system.

  system       ncp      maxL  F           copy  y      dot     why
  pikachu      23 703   130   2, 3, 4     q     0.043  2.0e-7  the tet-10 numbering of tests/golden/pikachu_tet10.npz: real valences (130, 105, 100, 100, 95, ...)
  hub(H)       200, 193 H     2, 3, 4     t, q  0.114  2.3e-4  ring i - 1, i, i + 1 + a hub: H = 126, 127 take the transpose, 128, 129 the quads; Kb = H leaves a
                                                                tail for every unroll; 193 = 3 * 64 + 1: a one-node last block
  ring         64 .. 129 3    4, 4, 2, 2  t     0.090  4.3e-4  the smallest accepted sizes (n = 256) and one node more ("ell" = 0: uniform rows)
  below        63 .. 127 3    4, 3, 2, 3  -     0.139  5.9e-4  n < 256: the node-blocked form must NOT be taken
  empties      200      40    3           t     0.085  1.7e-4  hub(40) with the lists of nodes 3, 64, 65, 199 emptied
  singles      200      40    3           t     0.076  8.3e-5  hub(40) with the lists of nodes 5, 64, 65, 130, 199 cut down to the node itself
  shuffled     200      129   3           q     0.069  3.1e-5  hub(129), every node list permuted (the same permutation in all F rows and segments)
  near_miss_a  200      40    3           -     0.068  1.5e-6  hub(40); in row (f = 2, i = 100) two columns of segment g = 1 swapped: must fall back
  near_miss_b  200      40    3           -     0.109  2.6e-6  hub(40); one entry removed from row (1, 150): must fall back
  quad8_2d     367      21    2, 3        t     0.048  6.2e-5  make_Square (12 x 9), serendipity order 2, elements shuffled
  hex27_u      693      125   3           t     0.020  1.8e-5  make_Brick (5 x 4 x 3), Lagrange order 2, elements shuffled: just under the transpose's limit
  trips        65 601   129   2           q     0.160  8.1e-8  hub(129) on 64 * 4 * cus + 65 nodes: with wg_per_cu = 1 a wave sweeps two blocks (both forms)

pikachu is handed over as the library builds it (assemble_SparseID: 64-bit row pointers, base 0) and as a caller's CSR with 32-bit row pointers and
base 1; quad8_2d and hex27_u as built and in the three caller formats; every other system but trips in the three caller formats (int64 base 0,
int32 base 1, int64 base 1).

The window sort (bits 8-13 of the "sell" knob) at 2^7 rows makes every 128-row block its own window: on hub(129) and on pikachu every block that
holds a long row pads to it, sell_padding_ok refuses the row-sorted plan (restated here: row_sorted_accepted) and the pattern stays on the CSR
kernel, mode 0 -- the case asserts exactly that, and the window sort is seen serving on quad8_2d (both windows) and on the two systems at 2^10.
The XCD walk needs a grid that is a multiple of eight: neither sweep system has one (2 and 139 workgroups), trips with wg_per_cu = 1 has.

Solves, err = max |x - x_oracle| / max |x_oracle| against TOL_X = 1e-10, all on the node-blocked form:
  pikachu F = 3  idrs(4) 1.4e-12, bicgstabl(2) 6.5e-14, cg 3.9e-16;  pikachu F = 2  idrs(4) 1.6e-14
  hub(127) on 193 nodes  idrs(4)  F = 2 7.3e-14, F = 4 5.4e-14;  hub(128)  F = 2 7.9e-14, F = 4 1.7e-13, F = 4 with Pl_Jacobi_ 1.7e-13
"""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
EPS = 2.0 ** -52
BSELL_B, BSELL_T_MAXL = 64, 127  # csrc/sell_decide.h


@functools.lru_cache(maxsize=None)
def _scale():
    """tests/test_gpu_krylov_scale.py, for _knobs, System, _oracle, _k, _maxiter, DEFAULT_KNOBS, TOL_X, TOL_RES (loaded the way that file loads
    test_gmres_cpu.py)."""
    spec = importlib.util.spec_from_file_location("_krylov_scale_helpers", os.path.join(HERE, "test_gpu_krylov_scale.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# -- node graphs (numpy only) -------------------------------------------------------------------------------------------------------------------------
def _graph(ncp, i, j):
    """(ptr, idx) of the node lists, sorted, from coupled pairs (i, j)."""
    import scipy.sparse as sp

    M = sp.csr_matrix((np.ones(len(i)), (np.asarray(i), np.asarray(j))), shape=(ncp, ncp))
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int64)


def ring(ncp):
    a = np.arange(ncp)
    return _graph(ncp, np.concatenate([a, a, a]), np.concatenate([(a - 1) % ncp, a, (a + 1) % ncp]))


def hub(ncp, H):
    """ring i - 1, i, i + 1; nodes < H also list node 7; node 7 lists 0 .. H - 1 (H entries: its own ring neighbours are among them)."""
    a, h = np.arange(ncp), np.arange(H)
    return _graph(ncp, np.concatenate([a, a, a, h, np.full(H, 7)]), np.concatenate([(a - 1) % ncp, a, (a + 1) % ncp, np.full(H, 7), h]))


def emptied(ptr, idx, nodes):
    keep = np.ones(idx.size, dtype=bool)
    for i in nodes:
        keep[ptr[i]:ptr[i + 1]] = False
    lens = np.diff(ptr)
    lens[list(nodes)] = 0
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx[keep]


def only_self(ptr, idx, nodes):
    """the lists of `nodes` cut down to one entry: the node itself"""
    keep = np.ones(idx.size, dtype=bool)
    for i in nodes:
        keep[ptr[i]:ptr[i + 1]] = idx[ptr[i]:ptr[i + 1]] == i
    lens = np.diff(ptr)
    lens[list(nodes)] = 1
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx[keep]


def shuffled(ptr, idx, seed):
    rng = np.random.default_rng(seed)
    out = idx.copy()
    for i in range(ptr.size - 1):
        out[ptr[i]:ptr[i + 1]] = rng.permutation(idx[ptr[i]:ptr[i + 1]])
    return ptr, out


def mesh_graph(cp_ids, ncp):
    """nodes coupled through an element of the connectivity cp_ids [itp, nel]"""
    import scipy.sparse as sp

    itp, nel = cp_ids.shape
    E = sp.csr_matrix((np.ones(itp * nel), (np.repeat(np.arange(nel), itp), cp_ids.T.ravel())), shape=(nel, ncp))
    P = (E.T @ E).tocsr()
    P.sort_indices()
    return P.indptr.astype(np.int64), P.indices.astype(np.int64)


def expand(ptr, idx, ncp, F):
    """(rowptr, col), 0-based, of the field-major F-field pattern: row f * ncp + i lists idx[list(i)] + g * ncp for g < F, list order kept."""
    lens = np.diff(ptr)
    node = np.repeat(np.arange(ncp), lens)
    t = np.arange(idx.size) - ptr[node]
    E = np.empty(F * idx.size, dtype=np.int64)
    for g in range(F):
        E[F * ptr[node] + g * lens[node] + t] = idx + g * ncp
    rowptr = np.concatenate([[0], np.cumsum(np.tile(F * lens, F))]).astype(np.int64)
    return rowptr, np.tile(E, F)


def node_blocked_plan(ptr, ncp, F):
    """The plan of the node-blocked form restated: nodes stably sorted by decreasing list length, blocks of 64, every block as long as its first
    node.  (node slots x 64 over all blocks, blocks)"""
    lens = np.diff(ptr)
    order = np.argsort(-lens, kind="stable")
    first = lens[order[::BSELL_B]]
    return int(BSELL_B * first.sum()), int(first.size)


def gates(n, nnz, max_row, F, slots):
    """bsell_may_try (no ghosts, no lattice hint), bsell_enough_nodes, bsell_padding_ok of csrc/sell_decide.h"""
    return n >= BSELL_B * 4 and n // F >= BSELL_B and slots * F * F <= 1.15 * nnz + 128.0 * max_row * F


def row_sorted_accepted(rowptr, window_log2=0):
    """The plan of the row-sorted form restated -- rows stably sorted by decreasing length within windows of 2^w rows (one window: w = 0), blocks of
    128, every block as long as its longest row -- and sell_padding_ok of csrc/sell_decide.h (no ghost columns, no lattice regions)."""
    lens = np.diff(rowptr)
    n, mx = lens.size, int(lens.max())
    win = np.arange(n) >> window_log2 if window_log2 > 0 else np.zeros(n, dtype=np.int64)
    order = np.argsort(win * (mx + 1) + (mx - lens), kind="stable")
    padded = np.zeros(-(-n // 128) * 128, dtype=np.int64)
    padded[:n] = lens[order]
    total = 128 * int(padded.reshape(-1, 128).max(axis=1).sum())
    return total <= 1.15 * lens.sum() + 128.0 * mx


class Graph:
    """A system of the table: the node graph, its F-field pattern and what the case expects of the layout."""

    def __init__(self, name, ptr, idx, ncp, F, accepted=True, ell_off=False, cp_ids=None, edit=None):
        self.name, self.ptr, self.idx, self.ncp, self.F, self.accepted, self.ell_off, self.cp_ids = name, ptr, idx, ncp, F, accepted, ell_off, cp_ids
        self.id = f"{name}-F{F}"
        self.rowptr, self.col = expand(ptr, idx, ncp, F)
        if edit is not None:
            self.rowptr, self.col = edit(self.rowptr, self.col)
        self.n, self.nnz = F * ncp, int(self.col.size)
        self.maxL = int(np.diff(ptr).max())
        self.slots, self.nblk = node_blocked_plan(ptr, ncp, F)
        self.rng = np.random.default_rng(sum(map(ord, self.id)) * 7919)

    @functools.cached_property
    def host(self):
        """values, x, y0 and the longdouble reference: P = A x and mag = |A| |x| per row (one reduceat each; rows without entries give 0)"""
        K = self.rng.random(self.nnz) - 0.5
        x = self.rng.random(self.n) - 0.5
        y0 = self.rng.random(self.n) - 0.5
        prod = K.astype(np.longdouble) * x.astype(np.longdouble)[self.col]
        lens = np.diff(self.rowptr)
        ne = lens > 0
        P, mag = np.zeros(self.n, dtype=np.longdouble), np.zeros(self.n, dtype=np.longdouble)
        P[ne] = np.add.reduceat(prod, self.rowptr[:-1][ne])
        mag[ne] = np.add.reduceat(np.abs(prod), self.rowptr[:-1][ne])
        return {"K": K, "x": x, "y0": y0, "P": P, "mag": mag, "lens": lens}


def _swap_two_columns(f, i, g, ncp, F):
    def edit(rowptr, col):
        lo = rowptr[f * ncp + i]
        L = (rowptr[f * ncp + i + 1] - lo) // F
        col = col.copy()
        a, b = lo + g * L, lo + g * L + 1
        col[a], col[b] = col[b], col[a]
        return rowptr, col
    return edit


def _remove_one_entry(f, i, ncp):
    def edit(rowptr, col):
        at = rowptr[f * ncp + i] + 1
        rowptr = rowptr.copy()
        rowptr[f * ncp + i + 1:] -= 1
        return rowptr, np.delete(col, at)
    return edit


@functools.lru_cache(maxsize=None)
def mesh_cp_ids(name):
    """(cp_ids [itp, nel], ncp) of the three real meshes, numbered by the product's mesh_Classical"""
    from metafem_jl_amd import element, mesh as pm

    if name == "pikachu":
        z = np.load(os.path.join(GOLD, "pikachu_tet10.npz"))
        space = element.classical_space(3, "Serendipity", 2, 5, shape="SIMPLEX")
        vert, conn = z["vert"] / 100.0, z["conn"].astype(np.int64)
    elif name == "quad8_2d":
        space = element.classical_space(2, "Serendipity", 2, 3)
        vert, conn = pm.make_Square((1.0, 1.0), (12, 9))
        conn = conn[:, np.random.default_rng(0x5EED).permutation(conn.shape[1])]
    elif name == "hex27_u":
        space = element.classical_space(3, "Lagrange", 2, 3)
        vert, conn = pm.make_Brick((1.0, 1.0, 1.0), (5, 4, 3))
        conn = conn[:, np.random.default_rng(0x5EED).permutation(conn.shape[1])]
    else:
        raise KeyError(name)
    msh = pm.mesh_Classical(vert, conn, space)
    return np.asarray(msh.cp_ids).astype(np.int64), int(msh.ncp)


@functools.lru_cache(maxsize=None)
def graph(name, F, arg=0, ncp=0):
    """The systems of the table, built once per session."""
    if name in ("pikachu", "quad8_2d", "hex27_u"):
        cp, ncp = mesh_cp_ids(name)
        return Graph(name, *mesh_graph(cp, ncp), ncp, F, cp_ids=cp)
    if name == "hub":
        return Graph(f"hub{arg}_{ncp}", *hub(ncp, arg), ncp, F)
    if name == "trips":
        return Graph("trips", *hub(ncp, 129), ncp, F)
    if name == "ring":
        return Graph(f"ring{ncp}", *ring(ncp), ncp, F, ell_off=True)
    if name == "below":
        return Graph(f"below{ncp}", *ring(ncp), ncp, F, accepted=False, ell_off=True)
    if name == "empties":
        return Graph("empties", *emptied(*hub(200, 40), (3, 64, 65, 199)), 200, F)
    if name == "singles":
        return Graph("singles", *only_self(*hub(200, 40), (5, 64, 65, 130, 199)), 200, F)
    if name == "shuffled":
        return Graph("shuffled", *shuffled(*hub(200, 129), 5), 200, F)
    if name == "near_miss_a":
        return Graph("near_miss_a", *hub(200, 40), 200, F, accepted=False, edit=_swap_two_columns(2, 100, 1, 200, F))
    if name == "near_miss_b":
        return Graph("near_miss_b", *hub(200, 40), 200, F, accepted=False, edit=_remove_one_entry(1, 150, 200))
    raise KeyError(name)


SMALL = [("hub", F, H, ncp) for ncp in (200, 193) for H in (126, 127, 128, 129) for F in (2, 3, 4)]
SMALL += [("ring", 4, 0, 64), ("ring", 4, 0, 65), ("ring", 2, 0, 128), ("ring", 2, 0, 129)]
SMALL += [("below", 4, 0, 63), ("below", 3, 0, 85), ("below", 2, 0, 127), ("below", 3, 0, 64)]
SMALL += [("empties", 3, 0, 0), ("singles", 3, 0, 0), ("shuffled", 3, 0, 0), ("near_miss_a", 3, 0, 0), ("near_miss_b", 3, 0, 0)]
MESHES = [("quad8_2d", 2, 0, 0), ("quad8_2d", 3, 0, 0), ("hex27_u", 3, 0, 0)]
PIKACHU = [("pikachu", F, 0, 0) for F in (2, 3, 4)]
MAXL = {"pikachu": 130, "quad8_2d": 21, "hex27_u": 125, "ring": 3, "below": 3, "empties": 40, "singles": 40, "shuffled": 129, "near_miss_a": 40,
        "near_miss_b": 40}  # the longest node list (hub(H): H)
CALLER_FORMATS = ["i64b0", "i32b1", "i64b1"]  # row pointer width, index base
CASES = [(key, fmt) for key in SMALL for fmt in CALLER_FORMATS] + [(key, fmt) for key in MESHES for fmt in CALLER_FORMATS + ["built"]]
CASES += [(key, fmt) for key in PIKACHU for fmt in ("built", "i32b1")]


def _case_id(case):
    (name, F, arg, ncp), fmt = case
    return f"{name}{arg or ''}{'_' + str(ncp) if ncp else ''}-F{F}-{fmt}"


# -- device side ----------------------------------------------------------------------------------------------------------------------------------------
def new_pattern(mf, G, fmt):
    """A fresh handle of G's pattern: a caller's CSR in the given format, or ("built") what assemble_SparseID makes of the mesh's connectivity --
    which must be G's pattern, array for array."""
    import torch

    if fmt == "built":
        cp = torch.tensor((G.cp_ids.T + 1).astype(np.int32), device="cuda").contiguous()
        A = mf.assemble_SparseID(cp, G.ncp, n_fields=G.F, index_base=1, with_slots=False, ctx=mf.default_context())[0]
        assert np.array_equal(A.rowptr.cpu().numpy() - A.index_base, G.rowptr) and np.array_equal(A.colidx.cpu().numpy() - A.index_base, G.col)
        A._connectivity = cp  # (kept with the handle)
        return A
    dtype, base = {"i64b0": (torch.int64, 0), "i32b1": (torch.int32, 1), "i64b1": (torch.int64, 1)}[fmt]
    return mf.FEM_SpMat_CSR(torch.tensor(G.rowptr + base, dtype=dtype, device="cuda"), torch.tensor(G.col + base, dtype=torch.int32, device="cuda"),
                            G.n, index_base=base, ctx=mf.default_context())


def layout_of(mf, A):
    """(mode, padded_rows, entries, bytes, fields of the node-blocked form) of the planned solver layout"""
    from metafem_jl_amd import _lib

    lib, ctx = _lib.lib, A.ctx
    mode, padded, ent, sym, nbytes = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
    _lib.check(lib.mfem_csr_solver_layout(ctx._h, A._h, C.byref(mode), None, C.byref(padded), None))
    _lib.check(lib.mfem_csr_solver_layout_entries(ctx._h, A._h, C.byref(ent), C.byref(sym)))
    _lib.check(lib.mfem_csr_solver_layout_bytes(ctx._h, A._h, C.byref(nbytes)))
    return mode.value, padded.value, ent.value, nbytes.value, int(lib.mfem_debug_bsell_fields(A._h))


def assert_form(mf, G, A, node_blocked, tag, mode_wanted=3):
    """mode 3 and the form the case was written for; the node-blocked form's accounting, exact."""
    mode, padded, ent, nbytes, fields = layout_of(mf, A)
    assert mode == mode_wanted, (tag, mode)
    assert fields == (G.F if node_blocked else 0), (tag, fields)
    if node_blocked:
        assert gates(G.n, G.nnz, G.F * G.maxL, G.F, G.slots), tag  # (the restated plan passes the gates: the case is what its table row says)
        assert padded == -(-G.ncp // BSELL_B) * BSELL_B * G.F, (tag, padded)
        assert ent == G.slots * G.F * G.F, (tag, ent, G.slots)
        assert nbytes == ent * 8 + G.slots * 4 + G.n * 16 + G.ncp * 4, (tag, nbytes)


def _ratio(err, bound):
    """largest err / bound (a zero bound admits a zero error only)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    z = bound == 0
    if np.any(err[z] != 0):
        return np.inf
    return float((err[~z] / bound[~z]).max()) if np.any(~z) else 0.0


def products(mf, G, A, node_blocked, tag):
    """The four products of a configuration against the longdouble reference; returns (largest err / bound of y, of the dot)."""
    import torch
    from metafem_jl_amd import _lib

    lib, ctx, h = _lib.lib, A.ctx, G.host
    if "dev" not in h:
        h["dev"] = tuple(torch.tensor(h[k], device="cuda") for k in ("K", "x", "y0"))
    K, x, y0 = h["dev"]
    c0 = int(lib.mfem_debug_bsell_spmv_count())

    def run(alpha, beta, y, dot=False):
        if dot:
            d = C.c_double()
            _lib.check(lib.mfem_spmv_solver_layout_dot(ctx._h, A._h, K.data_ptr(), x.data_ptr(), y.data_ptr(), alpha, beta, C.byref(d)))
            return d.value
        _lib.check(lib.mfem_spmv_solver_layout(ctx._h, A._h, K.data_ptr(), x.data_ptr(), y.data_ptr(), alpha, beta))

    def nan():
        return torch.full((G.n,), float("nan"), dtype=torch.float64, device="cuda")

    y1, y1b, y2, y3 = nan(), nan(), y0.clone(), nan()
    run(1.0, 0.0, y1)
    run(1.0, 0.0, y1b)
    run(-0.5, 2.0, y2)
    dot = run(1.0, 0.0, y3, dot=True)
    torch.cuda.synchronize()
    assert int(lib.mfem_debug_bsell_spmv_count()) - c0 == (4 if node_blocked else 0), tag
    assert bool(torch.isfinite(y1).all()), (tag, "beta = 0 read y")
    assert torch.equal(y1, y1b), (tag, "two identical calls differ")
    assert torch.equal(y1, y3), (tag, "the fused dot changed y")
    ld = np.longdouble
    r1 = _ratio(np.abs(y1.cpu().numpy().astype(ld) - h["P"]), (h["lens"] + 4) * EPS * h["mag"])
    ref2 = ld(-0.5) * h["P"] + ld(2.0) * h["y0"].astype(ld)
    r2 = _ratio(np.abs(y2.cpu().numpy().astype(ld) - ref2), (h["lens"] + 4) * EPS * (0.5 * h["mag"] + np.abs(2.0 * h["y0"])))
    xy = h["x"].astype(ld) * y3.cpu().numpy().astype(ld)
    rd = _ratio([abs(ld(dot) - xy.sum())], [(G.n + 2) * EPS * np.abs(xy).sum()])
    print(f"\n{tag}: n={G.n} nnz={G.nnz} maxL={G.maxL} y(1,0) {r1:.3f} y(-0.5,2) {r2:.3f} dot {rd:.1e} of the bound")
    assert r1 <= 1.0, (tag, "y = A x", r1)
    assert r2 <= 1.0, (tag, "y = -0.5 A x + 2 y", r2)
    assert rd <= 1.0, (tag, "x . y", rd)


def knobs_for(G, **kw):
    H = _scale()
    kn = dict(layout_min_rows=(0, 0), **kw)
    if G.ell_off:
        kn["ell"] = 0  # (uniform rows: the inspector would take the slot-major copies, modes 1 / 2)
    return H._knobs(**kn)


# -- products: every system, format and form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_products_of_both_forms(mf, case):
    """y = alpha A x + beta y and the fused x . y through the node-blocked form with its default copy (bsell = 1), with the quad copy forced
    (bsell = 3) and through the row-sorted form of the same pattern (bsell = 0).  A system that is not node-blocked (below, near_miss_*) must be
    served by the row-sorted form whatever the knob says."""
    key, fmt = case
    G = graph(*key)
    assert gates(G.n, G.nnz, G.F * G.maxL, G.F, G.slots) == G.accepted or G.name.startswith("near_miss")
    # the longest node list decides the default copy, bsell_copy(maxL, F, knobs): the LDS transpose up to BSELL_T_MAXL, the lane quads beyond
    assert G.maxL == MAXL.get(key[0], key[2]) and G.ncp == (key[3] or {"pikachu": 23703, "quad8_2d": 367, "hex27_u": 693}.get(key[0], 200))
    assert (G.maxL > BSELL_T_MAXL) == (key[0] in ("pikachu", "shuffled") or key[2] in (128, 129))
    for bsell in (1, 3, 0):
        tag = f"{_case_id(case)}-bsell{bsell}"
        with knobs_for(G, bsell=bsell):
            A = new_pattern(mf, G, fmt)
            node_blocked = G.accepted and bsell != 0
            assert_form(mf, G, A, node_blocked, tag)
            products(mf, G, A, node_blocked, tag)
            del A


# -- knob sweeps ----------------------------------------------------------------------------------------------------------------------------------
# The word of mfem_debug_set("sell", word, 0) (csrc/sell_decide.h: SellKnobs); bit 0 = the layout on.
SELL_ON = 1
SELL_EXPLICIT_COLUMNS = 1 << 1   # offsets off: blocks with one diagonal list read their column stream too
SELL_XCD_WALK = 1 << 2           # xcd: every XCD walks a contiguous eighth of the block list (grids that are a multiple of 8)
SELL_WHOLE_COLUMN_STREAM = 1 << 3  # periodic off: field-periodic blocks read their whole column stream


def sell_window_log2(w):         # bits 8-13: rows sorted within windows of 2^w rows
    return w << 8


def sell_unroll(u):              # bits 16-20: k_spmv_sell<u>; anything but 4, 8, 9, 10, 15 resolves to 5
    return u << 16


def sell_per_u(v):               # bits 21-22: k_spmv_bsell<3, U> with U = 3, 2, 4, 1 for v = 0, 1, 2, 3 (field-periodic blocks: 3, 2, 4 slots in flight)
    return v << 21


def sell_wg_per_cu(w):           # bits 24-28: workgroups per CU of the product's grid (0 = 8)
    return w << 24


SWEEP = [  # (id, bsell, sell word, bitwise equal to the run with this id or None)
    ("bsell-default", 1, SELL_ON, None),
    ("bsell-U2", 1, SELL_ON | sell_per_u(1), None),
    ("bsell-U4", 1, SELL_ON | sell_per_u(2), None),
    ("bsell-U1", 1, SELL_ON | sell_per_u(3), None),
    ("sell-default", 0, SELL_ON, None),
    ("sell-U4", 0, SELL_ON | sell_unroll(4), None),
    ("sell-U8", 0, SELL_ON | sell_unroll(8), None),
    ("sell-U9", 0, SELL_ON | sell_unroll(9), None),
    ("sell-U10", 0, SELL_ON | sell_unroll(10), None),
    ("sell-U15", 0, SELL_ON | sell_unroll(15), None),
    ("sell-U7-is-5", 0, SELL_ON | sell_unroll(7), "sell-default"),  # an unlisted value: k_spmv_sell<5>, the same bits as the default
    ("sell-periodic-2-slots", 0, SELL_ON | sell_per_u(1), None),
    ("sell-periodic-4-slots", 0, SELL_ON | sell_per_u(2), None),
    # (windows of 128 rows are single blocks: on both systems of the sweep every block that holds a long row pads to it and sell_padding_ok refuses
    # the plan -- restated in row_sorted_accepted -- so the pattern stays on the CSR kernel; SWEEP_CASES adds quad8_2d, where both windows are accepted)
    ("sell-window-7", 0, SELL_ON | sell_window_log2(7), None),
    ("sell-window-10", 0, SELL_ON | sell_window_log2(10), None),
    ("sell-xcd", 0, SELL_ON | SELL_XCD_WALK, None),
    ("sell-explicit-columns", 0, SELL_ON | SELL_EXPLICIT_COLUMNS, None),
    ("sell-whole-column-stream", 0, SELL_ON | SELL_WHOLE_COLUMN_STREAM, None),
    ("sell-U4-explicit-whole", 0, SELL_ON | sell_unroll(4) | SELL_EXPLICIT_COLUMNS | SELL_WHOLE_COLUMN_STREAM, None),
]
_SWEEP_Y = {}
SWEEP_CASES = [(key, fmt, sw) for key, fmt in ((("hub", 3, 129, 193), "i64b0"), (("pikachu", 3, 0, 0), "built")) for sw in SWEEP]
SWEEP_CASES += [(("quad8_2d", 3, 0, 0), "built", sw) for sw in SWEEP if "window" in sw[0]]
WINDOW_REFUSED = {("hub129_193-F3", 7), ("pikachu-F3", 7)}  # (what row_sorted_accepted must find: no case changes its mind silently)


@pytest.mark.parametrize("key,fmt,sweep", SWEEP_CASES, ids=[f"{k[0]}{k[2] or ''}-{sw[0]}" for k, f, sw in SWEEP_CASES])
def test_knob_sweep_of_the_products(mf, key, fmt, sweep):
    """The instantiations and paths of the two product kernels that sit behind the "sell" knob, on a small graph whose Kb = 129 leaves a tail for
    every unroll and on the tetrahedral mesh."""
    import torch
    from metafem_jl_amd import _lib

    sid, bsell, word, same_as = sweep
    G = graph(*key)
    tag = f"{G.id}-{sid}"
    w = (word >> 8) & 63
    accepted = bsell != 0 or row_sorted_accepted(G.rowptr, w)
    assert accepted == ((G.id, w) not in WINDOW_REFUSED), tag
    with knobs_for(G, bsell=bsell, sell=word):
        A = new_pattern(mf, G, fmt)
        assert_form(mf, G, A, bsell != 0, tag, mode_wanted=3 if accepted else 0)
        products(mf, G, A, bsell != 0, tag)
        K, x, _ = G.host["dev"]
        y = torch.empty(G.n, dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib.mfem_spmv_solver_layout(A.ctx._h, A._h, K.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0))
        _SWEEP_Y[(G.id, sid)] = y
    if same_as is not None:
        if (G.id, same_as) not in _SWEEP_Y:
            other = next(s for s in SWEEP if s[0] == same_as)
            with knobs_for(G, bsell=other[1], sell=other[2]):
                A = new_pattern(mf, G, fmt)
                y0 = torch.empty(G.n, dtype=torch.float64, device="cuda")
                _lib.check(_lib.lib.mfem_spmv_solver_layout(A.ctx._h, A._h, K.data_ptr(), x.data_ptr(), y0.data_ptr(), 1.0, 0.0))
                _SWEEP_Y[(G.id, same_as)] = y0
        assert torch.equal(y, _SWEEP_Y[(G.id, same_as)]), tag


@pytest.mark.parametrize("bsell,word", [(1, SELL_ON | sell_wg_per_cu(1)), (0, SELL_ON | sell_wg_per_cu(1)),
                                        (0, SELL_ON | sell_wg_per_cu(1) | SELL_XCD_WALK)], ids=["node-blocked", "row-sorted", "row-sorted-xcd"])
def test_second_grid_stride_trip(mf, bsell, word):
    """wg_per_cu = 1: the product's grid is one workgroup (four waves) per CU, and the hub(129) graph on 64 * 4 * cus + 65 nodes has more blocks than
    that in both forms (64-node and 128-row blocks of a two-field matrix): a wave sweeps two blocks.  With the XCD walk on, the grid (= cus, a multiple
    of eight) takes the walk by contiguous eighths."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ncp = BSELL_B * 4 * cus + 65
    while ncp % 7 == 0:  # (row 0 = (0, 1, 7, ncp - 1) must not read as a lattice hint)
        ncp += 1
    G = graph("trips", 2, 0, ncp)
    nblk = G.nblk if bsell else -(-G.n // 128)
    assert nblk > 4 * cus and G.ncp > 64 * 4 * cus + 64
    if word & SELL_XCD_WALK:
        assert min(-(-nblk * 64 // 256), cus) % 8 == 0  # (sell_xcd_flag)
    tag = f"trips-bsell{bsell}-word{word:#x}"
    with knobs_for(G, bsell=bsell, sell=word):
        A = new_pattern(mf, G, "i64b0")
        assert_form(mf, G, A, bsell != 0, tag)
        products(mf, G, A, bsell != 0, tag)


# -- the scaled copies: solves against the oracle -------------------------------------------------------------------------------------------------
def _scaled_system(mf, G, fmt, symmetric):
    """S8's shifted graph Laplacian on G's pattern -- random negative couplings, each diagonal the sum of its row's couplings + 1e-2 -- scaled
    S M S (cg!) or M S (the nonsymmetric methods) with S = diag(s), s log-uniform in [0.5, 2]: the diagonal varies 16-fold, so a divisor taken
    from the wrong column moves the iterate at order 1."""
    import scipy.sparse as sp
    import torch

    H = _scale()
    R = sp.csr_matrix((-0.5 - np.random.default_rng(8).random(G.nnz), G.col, G.rowptr), shape=(G.n, G.n))
    R.setdiag(0.0)
    M = ((R + R.T) * 0.5).tocsr()
    M = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 1e-2)).tocsr()
    M.sort_indices()
    assert np.array_equal(M.indptr, G.rowptr) and np.array_equal(M.indices, G.col)  # (the pattern is symmetric, sorted and holds the diagonal)
    s = 2.0 ** np.random.default_rng(9).uniform(-1.0, 1.0, G.n)
    data = M.data * s[G.col]
    if symmetric:
        data = data * np.repeat(s, np.diff(G.rowptr))
    A0 = new_pattern(mf, G, "i64b0")  # (System reads its host arrays off a 0-based handle)
    return H.System(f"{G.id}-{'sym' if symmetric else 'nonsym'}", mf.default_context(), lambda: new_pattern(mf, G, fmt), A0,
                    torch.tensor(data, device="cuda"))


_SYSTEMS = {}
SOLVES = [  # (system key, pattern format, solver, s, Pl_func)
    (("pikachu", 3, 0, 0), "built", "idrs", 4, None),
    (("pikachu", 3, 0, 0), "built", "bicgstabl", 2, None),
    (("pikachu", 3, 0, 0), "built", "cg", 0, None),
    (("pikachu", 2, 0, 0), "built", "idrs", 4, None),
    (("hub", 2, 127, 193), "i32b1", "idrs", 4, None),
    (("hub", 4, 127, 193), "i32b1", "idrs", 4, None),
    (("hub", 2, 128, 193), "i32b1", "idrs", 4, None),
    (("hub", 4, 128, 193), "i32b1", "idrs", 4, None),
    (("hub", 4, 128, 193), "i64b1", "idrs", 4, "diag"),
]


@pytest.mark.parametrize("key,fmt,solver,s,pl", SOLVES, ids=[f"{k[0]}{k[2] or ''}-F{k[1]}-{f}-{sv}{s or ''}-{pl}" for k, f, sv, s, pl in SOLVES])
def test_scaled_copies_step_with_the_oracle(mf, key, fmt, solver, s, pl):
    """k steps of a Jacobi-preconditioned solve on the node-blocked form, as tests/test_gpu_krylov_scale.py runs them, against
    oracle.solvers.iterative_solve: the right Jacobi scale of the nonsymmetric methods is folded into the layout copy (dsc in k_bsell_fill and
    k_bsell_fill_t), cg! and the left-scaled solve bind an unscaled copy."""
    import torch
    from metafem_jl_amd import _lib

    H, G, lib = _scale(), graph(*key), _lib.lib
    sym = solver == "cg"
    if (key, fmt, sym) not in _SYSTEMS:
        _SYSTEMS[(key, fmt, sym)] = _scaled_system(mf, G, fmt, sym)
    S = _SYSTEMS[(key, fmt, sym)]
    k = H._k(solver, s)
    tag = f"{S.name}-{fmt}-{solver}{s}-{pl}"
    with knobs_for(G):
        A = S.new_pattern()
        assert_form(mf, G, A, True, tag)
        c0 = int(lib.mfem_debug_bsell_spmv_count())
        x, st = mf.iterative_Solve(A, S.K, S.b, 1e-300, Sv_func=getattr(mf, H.SOLVERS[solver]), Pr_func=mf.Pr_Jacobi_,
                                   Pl_func={None: mf.Identity, "diag": mf.Pl_Jacobi_}[pl], maxiter=H._maxiter(solver, s, k), max_pass=1, s=s,
                                   seed=H.SEED, cg_variant=0, fixed_iterations=solver == "cg")
        torch.cuda.synchronize()
        served = int(lib.mfem_debug_bsell_spmv_count()) - c0
        assert int(lib.mfem_debug_bsell_fields(A._h)) == G.F and served > 0, (tag, served)
    xd = x.cpu().numpy()
    xo, info, nprod = H._oracle(S, solver, s, k, "jacobi", pl)
    err = float(np.abs(xd - xo).max() / np.abs(xo).max())
    tres, floor = S.true_res(xd)
    print(f"\n{tag}: n={S.n} maxL={G.maxL} bsell products={served} err={err:.3e} it={st.iterations}/{info.iters} passes={st.passes}/{info.passes} "
          f"spmv={st.spmv_count}/{nprod} res={st.final_res:.6e}/{tres:.6e}/{info.res:.6e}")
    assert err <= H.TOL_X, (tag, err)
    assert st.passes == info.passes == 1
    assert st.iterations == info.iters, (st.iterations, info.iters)
    assert st.spmv_count == nprod - 1, (st.spmv_count, nprod)  # (the oracle forms r = b - K x0 with x0 = 0; the device knows x0 = 0)
    assert abs(st.final_res - tres) <= H.TOL_RES * tres + floor, (st.final_res, tres, floor)
    assert abs(info.res - tres) <= H.TOL_RES * tres + floor
