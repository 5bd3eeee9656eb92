"""GPU parity of the Krylov solvers with oracle.solvers, iterate by iterate, at the sizes where the vector reductions span many workgroups and the
solver layouts serve the SpMVs.

tests/test_gpu_krylov.py steps the solvers against the oracle on a few hundred unknowns: there every reduction folds ONE partial sum (G = 1 workgroup,
csrc/blas1.hip mfem_vec_grid) and every grid-stride loop runs one trip, and the SpMVs run on the CSR kernel.  Krylov methods correct their own errors, so
a dropped partial sum or a skipped trip only slows convergence and end-to-end checks cannot see it.  Here each case runs k steps (two or three sweeps /
cycles) with converge_tol = 1e-300 and max_pass = 1 on a system the product's brick assembly builds, and compares delta_x, the step and pass counts, the
SpMV count and the reported residual with the oracle run with the same arguments and shadow vectors:

  S0  hex-8 thermal (5, 6, 7)           n = 336       G = 1
  S1  hex-8 thermal (6, 6, 12) / 11     n = 637 / 588 G = 2, odd tail and its even control
  S2  hex-8 thermal (46, 46, 46) curved n = 103 823   G = 203, CSR kernel; graphs off
  S3  hex-8 thermal (84, 84, 84)        n = 614 125   G = 768 = cap, 2 grid-stride trips; diagonal slots, both symmetric sweeps (the patch sweep is
                                                      the bench's cg!); vec_grid 1 (G = 256, 5 trips) and 8 (G = 1 200 > 1 024: reduce_partials_bcast takes its second trip); graphs off
  S4  hex-8 elasticity (44, 44, 44)     n = 273 375   lattice tiles, mode 5
  S5  hex-27 thermal (32, 32, 32)       n = 274 625   lattice tiles, mode 4
  S6  hex-8 Nitsche thermal (64^3)      n = 274 625   nonsymmetric: tiles + the skew remainder
  S7  hex-8 elasticity (31, 31, 31)     n = 98 304    modes 1 and 3 with the size limits lifted
  S8  unstructured hex-20, 3 fields     n = 107 163   the node-blocked sliced layout (BSELL) and the row-sorted one, size limits lifted

The last test runs whatever case the session skipped and checks that the cases together reached every layout, sweep, graph mode, grid class and
parity listed in REQUIRED.
"""
import contextlib
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 7
K_COND, H, TENV = 0.6, 25.0, 293.15
H_PEN, TW = 1000.0, 1173.15
LAM, MU, TAU = 0.5769230769230769, 0.38461538461538464, 1000.0
X0 = 1 << 4
MAX_PARTIALS = 4096  # csrc/common.h MFEM_MAX_PARTIALS; the context's partial-sum buffer holds 8 rows of it
BLOCK = 256          # csrc/common.h MFEM_BLOCK

# max |x - x_oracle| / max |x_oracle| after k steps.  Observed on one MI355X: <= 3.4e-12 over all cases (IDR(4) on S2; CG 2.3e-15 after 64 steps).
# IDR(s) with s >= 8 runs one cycle: over two, round-off grew to 1.4e-9 for s = 11.
TOL_X = 1e-10
# |final_res - true residual| / true residual (the true one from longdouble products on the host)
TOL_RES = 1e-9

DEFAULT_KNOBS = {"layout_min_rows": (262144, 1000000), "ell": (1, 0), "sell": (1, 0), "bsell": (1, 0), "lat8": (1, 0), "lat27": (1, 0),
                 "remainder": (1, 0), "graphs": (1, 4000000), "vec_grid": (3, 0)}


def _restated_gmres():
    spec = importlib.util.spec_from_file_location("_gmres_restated", os.path.join(HERE, "test_gmres_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.gmres


@contextlib.contextmanager
def _knobs(**kw):
    from metafem_jl_amd import _lib

    try:
        for key, ab in kw.items():
            a, b = ab if isinstance(ab, tuple) else (ab, 0)
            _lib.check(_lib.lib.mfem_debug_set(key.encode(), int(a), int(b)))
        yield
    finally:
        for key in kw:
            a, b = DEFAULT_KNOBS[key]
            _lib.lib.mfem_debug_set(key.encode(), a, b)


# -- systems ----------------------------------------------------------------------------------------------------------------------------------------
class System:
    def __init__(self, name, ctx, new_pattern, A, K, keep=()):
        """new_pattern() makes a fresh handle of A's pattern (the same rows, columns and order); keep: what must outlive the system (the brick)."""
        self.name, self.ctx, self.new_pattern, self.A, self.K, self.keep = name, ctx, new_pattern, A, K, keep
        self.n = A.n
        self.b = mf_rand(A.n)
        self.rowptr = A.rowptr.cpu().numpy().astype(np.int64)
        self.col = A.colidx.cpu().numpy().astype(np.int32)
        self.K_h = K.cpu().numpy()
        self.b_h = self.b.cpu().numpy()

    def true_res(self, x):
        """normalized_norm(b - K x) with every product and sum in longdouble, and the round-off floor of any float64 evaluation of it:
        64 eps normalized_norm(|K| |x| + |b|)."""
        xl = x.astype(np.longdouble)
        prod = self.K_h.astype(np.longdouble) * xl[self.col]
        r = self.b_h.astype(np.longdouble) - np.add.reduceat(prod, self.rowptr[:-1])
        mag = np.add.reduceat(np.abs(prod), self.rowptr[:-1]) + np.abs(self.b_h)
        return float(np.sqrt((r * r).sum() / self.n)), 64 * np.finfo(np.float64).eps * float(np.sqrt((mag * mag).sum() / self.n))


def mf_rand(n):
    import metafem_jl_amd as mf

    return mf.FEM_rand(n, 11, 0) - 0.5


def _distort(brick):
    import torch

    c = [brick.coords_view(d).clone() for d in range(3)]
    brick.coords_view(0).add_(0.03 * torch.sin(3 * c[1]) * torch.cos(2 * c[2]))
    brick.coords_view(1).add_(0.02 * torch.sin(2 * c[0] + c[2]))
    brick.coords_view(2).add_(0.025 * c[0] * c[1])


def _build(mf, name):
    if name in ("S0", "S1o", "S1e", "S2", "S3"):
        dims = {"S0": (5, 6, 7), "S1o": (6, 6, 12), "S1e": (6, 6, 11), "S2": (46, 46, 46), "S3": (84, 84, 84)}[name]
        b = mf.make_Brick((1.0, 1.0, 1.0), dims)
        if name == "S2":
            _distort(b)
        A = b.pattern(1)
        return System(name, b.ctx, lambda: b.pattern(1), A, b.assemble_thermal(A, K_COND, H, TENV, 0x3F), keep=(b,))
    if name in ("S4", "S7"):
        b = mf.make_Brick((1.0, 0.7, 1.3), (44, 44, 44) if name == "S4" else (31, 31, 31), 1, 3)
        A = b.pattern(3)
        return System(name, b.ctx, lambda: b.pattern(3), A, b.assemble_elasticity(A, LAM, MU, TAU, X0), keep=(b,))
    if name == "S5":
        b = mf.make_Brick((1.0, 1.0, 1.0), (32, 32, 32), 2, 5)
        A = b.pattern(1)
        return System(name, b.ctx, lambda: b.pattern(1), A, b.assemble_thermal(A, K_COND, H, TENV, 0x3F), keep=(b,))
    if name == "S6":
        b = mf.make_Brick((1.0, 0.7, 1.3), (64, 64, 64), 1, 3)
        A = b.pattern(1)
        return System(name, b.ctx, lambda: b.pattern(1), A,
                      b.assemble_thermal(A, K_COND, H, TENV, 0x3F & ~X0, fixed_faces=X0, h_penalty=H_PEN, Tw=TW), keep=(b,))
    if name == "S8":
        return _unstructured_3field(mf)
    raise KeyError(name)


def _unstructured_3field(mf):
    """S8: the field-major 3-field pattern of an unstructured hex-20 mesh (20^3 serendipity elements, element order shuffled in blocks, as
    bench_legs.unstructured_mesh builds it) -- the pattern the node-blocked sliced layout is planned for -- with the values of a shifted graph
    Laplacian: random negative couplings, each diagonal the sum of its row's couplings + 1e-2 (symmetric positive definite, and slow enough to
    converge that k steps leave a residual far above round-off)."""
    import scipy.sparse as sp
    import torch
    from metafem_jl_amd import element, mesh as pm

    space = element.classical_space(3, "Serendipity", 2, 3)
    vert, conn = pm.make_Brick((1.0, 1.0, 1.0), (20, 20, 20))
    nel = conn.shape[1]
    block = 16
    perm = (np.random.default_rng(0x5EED).permutation((nel + block - 1) // block)[:, None] * block + np.arange(block)[None, :]).ravel()
    msh = pm.mesh_Classical(vert, conn[:, perm[perm < nel]], space)
    cp = torch.tensor((msh.cp_ids.T + 1).astype(np.int32), device="cuda").contiguous()
    ncp = int(msh.cp_ids.max()) + 1
    ctx = mf.default_context()

    def new_pattern():
        return mf.assemble_SparseID(cp, ncp, n_fields=3, index_base=1, with_slots=False, ctx=ctx)[0]

    A = new_pattern()
    rp = A.rowptr.cpu().numpy().astype(np.int64) - A.index_base
    ci = A.colidx.cpu().numpy().astype(np.int64) - A.index_base
    R = sp.csr_matrix((-0.5 - np.random.default_rng(8).random(ci.size), ci, rp), shape=(A.n, A.n))
    R.setdiag(0.0)
    M = ((R + R.T) * 0.5).tocsr()
    M = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 1e-2)).tocsr()
    M.sort_indices()
    assert np.array_equal(M.indptr, rp) and np.array_equal(M.indices, ci)  # (the pattern is symmetric and holds the diagonal)
    return System("S8", ctx, new_pattern, A, torch.tensor(M.data, device="cuda"), keep=(cp,))


@pytest.fixture(scope="module")
def systems(mf):
    """name -> System, built on the device by the product's brick assembly and copied to the host once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _build(mf, name)
        return cache[name]

    yield get
    cache.clear()


# -- one comparison ---------------------------------------------------------------------------------------------------------------------------------
SOLVERS = {"cg": "cg_", "bicgstabl": "bicgstabl_GS_", "idrs": "idrs_", "cgs2": "cgs2_", "gmres": "gmres_"}


def _k(solver, s):
    return 1 if solver == "idrs" and s >= 8 else 3 if solver == "cg" else 2


def _maxiter(solver, s, k):
    """k sweeps / cycles / steps as the oracle counts them (its stop rule: it >= maxiter; gmres: it > maxiter)."""
    if solver == "bicgstabl":
        return 1 + k * s
    if solver == "idrs":
        return k * (s + 1)
    if solver == "gmres":
        return 1 + (k - 1) * s
    return k


_ORACLE = {}


def _oracle(S, solver, s, k, pr, pl):
    """(x, SolveInfo, SpMV count) of oracle.solvers.iterative_solve with the device call's arguments; cached per system and arguments."""
    from oracle import solvers

    key = (S.name, solver, s, k, pr, pl)
    if key in _ORACLE:
        return _ORACLE[key]
    count = [0]
    mul0 = solvers.mul

    def mul(b, A, x, alpha=1.0, beta=0.0):
        count[0] += 1
        return mul0(b, A, x, alpha, beta)

    info = solvers.SolveInfo()
    maxiter = _maxiter(solver, s, k)
    solvers.mul = mul
    try:
        if solver == "cg" and pr == "jacobi":
            x = solvers.solve_cg_jacobi(S.rowptr, S.col, S.K_h, S.b_h, 1e-300, maxiter, max_pass=1, info=info)
        else:
            sv = {"cg": solvers.cg, "bicgstabl": solvers.bicgstabl_gs, "idrs": solvers.idrs, "cgs2": solvers.cgs2, "gmres": _restated_gmres()}[solver]
            plf = {None: None, "diag": solvers.pl_jacobi, "rownorm": lambda A: solvers.pl_jacobi(A, normalized_by_row=True)}[pl]
            x = solvers.iterative_solve(S.rowptr, S.col, S.K_h, S.b_h, 1e-300, Sv_func=sv, Pr_func=solvers.pr_jacobi if pr == "jacobi" else None,
                                        Pl_func=plf, max_pass=1, maxiter=maxiter, s=s, seed=SEED, info=info)
    finally:
        solvers.mul = mul0
    _ORACLE[key] = (x, info, count[0])
    return _ORACLE[key]


def _vec_grid(mf, n, mult):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = min(cus * mult, MAX_PARTIALS)
    want = -(-((n + 1) // 2) // BLOCK)
    G = max(1, min(want, cap))
    trips = -(-((n + 1) // 2) // (G * BLOCK))
    return G, cap, trips


def _grid_tags(G, cap, trips):
    tags = set()
    if G == 1:
        tags.add("G=1")
    elif G <= 256:
        tags.add("1<G<=256")
    elif G < cap:
        tags.add("256<G<cap")
    if G == cap and trips >= 2:
        tags.add("G=cap,trips>=2")
    if G > 1024:
        tags.add("G>1024")
    return tags


class Case:
    def __init__(self, sysname, solver, s=0, k=None, pr="jacobi", pl=None, cg_variant=0, knobs=None, expect=(), graphs_bitwise=False, caller_csr=False,
                 auto_is=None):
        self.sysname, self.solver, self.s, self.k, self.pr, self.pl = sysname, solver, s, k or _k(solver, s), pr, pl
        self.cg_variant, self.knobs, self.expect, self.graphs_bitwise = cg_variant, dict(knobs or {}), set(expect), graphs_bitwise
        self.caller_csr, self.auto_is = caller_csr, auto_is
        kn = ",".join(f"{a}={b}" for a, b in self.knobs.items())
        self.id = f"{sysname}-{solver}{s or ''}-v{cg_variant}-{pr}-{pl}-k{self.k}" + (f"-[{kn}]" if kn else "") + ("-csr" if caller_csr else "") + \
            ("-graphs-bitwise" if graphs_bitwise else "")


def _counters(lib):
    return {"sym": int(lib.mfem_debug_sym_spmv_count()), "lat8": int(lib.mfem_debug_lat8_spmv_count()), "lat27": int(lib.mfem_debug_lat27_spmv_count()),
            "rem": int(lib.mfem_debug_rem_spmv_count()), "bsell": int(lib.mfem_debug_bsell_spmv_count()), "graph": int(lib.mfem_debug_graph_launch_count())}


RAN = {}  # case id -> tags of the paths it took


def _run_case(mf, systems, case):
    import torch
    from metafem_jl_amd import _lib

    S = systems(case.sysname)
    lib = _lib.lib
    with _knobs(**case.knobs):
        A = S.A
        if case.caller_csr or case.knobs:  # (a fresh pattern: some knobs are read when a pattern's layout is planned)
            A = mf.FEM_SpMat_CSR(torch.tensor(S.rowptr, device="cuda"), torch.tensor(S.col, device="cuda"), S.n, ctx=S.ctx) if case.caller_csr else \
                S.new_pattern()
        mode, ent, sym = C.c_int32(), C.c_int64(), C.c_int32()
        _lib.check(lib.mfem_csr_solver_layout(S.ctx._h, A._h, C.byref(mode), None, None, None))
        _lib.check(lib.mfem_csr_solver_layout_entries(S.ctx._h, A._h, C.byref(ent), C.byref(sym)))
        bsell_F = int(lib.mfem_debug_bsell_fields(A._h))
        kw = dict(Sv_func=getattr(mf, SOLVERS[case.solver]), Pr_func=mf.Pr_Jacobi_ if case.pr == "jacobi" else mf.Identity,
                  Pl_func={None: mf.Identity, "diag": mf.Pl_Jacobi_, "rownorm": mf.Pl_Jacobi_rownorm_}[case.pl],
                  maxiter=_maxiter(case.solver, case.s, case.k), max_pass=1, s=case.s, seed=SEED, cg_variant=case.cg_variant,
                  fixed_iterations=case.solver == "cg")
        c0 = _counters(lib)
        x, st = mf.iterative_Solve(A, S.K, S.b, 1e-300, **kw)
        torch.cuda.synchronize()
        c1 = _counters(lib)
        d = {key: c1[key] - c0[key] for key in c0}
        rows, nent, asym = C.c_int64(), C.c_int64(), C.c_double()
        _lib.check(lib.mfem_debug_remainder_info(A._h, C.byref(rows), C.byref(nent), C.byref(asym)))
        if case.graphs_bitwise:  # the same solve with cycle graphs off: the direct launches must give the same bits
            with _knobs(graphs=(1, 1)):
                g0 = int(lib.mfem_debug_graph_launch_count())
                x2, st2 = mf.iterative_Solve(A, S.K, S.b, 1e-300, **kw)
                assert int(lib.mfem_debug_graph_launch_count()) == g0
            assert d["graph"] > 0 and torch.equal(x, x2) and st2.iterations == st.iterations and st2.spmv_count == st.spmv_count
        if case.auto_is is not None:  # cg_variant 0 must resolve to this variant: the same bits
            x3, _ = mf.iterative_Solve(A, S.K, S.b, 1e-300, **dict(kw, cg_variant=case.auto_is))
            assert torch.equal(x, x3), "cg_variant 0 did not resolve to the expected variant"
    mult = case.knobs.get("vec_grid", DEFAULT_KNOBS["vec_grid"])
    G, cap, trips = _vec_grid(mf, S.n, mult[0] if isinstance(mult, tuple) else mult)

    xd = x.cpu().numpy()
    xo, info, nprod = _oracle(S, case.solver, case.s, case.k, case.pr, case.pl)
    err = float(np.abs(xd - xo).max() / np.abs(xo).max())
    tres, floor = S.true_res(xd)
    print(f"\n{case.id}: n={S.n} G={G} trips={trips} mode={mode.value} sym={sym.value} bsell={bsell_F} rem_rows={rows.value} d={d} "
          f"err={err:.3e} it={st.iterations}/{info.iters} passes={st.passes}/{info.passes} spmv={st.spmv_count}/{nprod} "
          f"res={st.final_res:.6e}/{tres:.6e}/{info.res:.6e}")

    tags = {"odd" if S.n % 2 else "even", "graphs_on" if d["graph"] > 0 else "graphs_off"} | _grid_tags(G, cap, trips)
    if d["lat27"] > 0:
        tags.add("mode4")
    elif d["lat8"] > 0:
        tags.add("mode5")
    else:
        tags.add(f"mode{mode.value}")
    if d["rem"] > 0 and rows.value > 0:
        tags.add("remainder")
    if d["bsell"] > 0 and bsell_F > 0:
        tags.add("bsell")
    if d["sym"] > 0:  # (one counter for both sweeps; mfem_csr_solver_layout_entries tells which one the layout binds: 1 k_spmv_sym27, 2 k_spmv_symp)
        tags.add({1: "sym_sweep", 2: "symp"}.get(sym.value, "sym?"))
    RAN[case.id] = tags
    assert case.expect <= tags, (case.id, sorted(tags))

    assert err <= TOL_X, (case.id, err)
    assert st.passes == info.passes == 1
    assert st.iterations == info.iters, (st.iterations, info.iters)
    # the oracle forms r = b - K x0 with x0 = 0 at the start of the pass; the device knows x0 = 0 and needs no product there.  A solve on the lattice
    # tiles (other than cg!'s) recomputes the residual once more from the caller's CSR values before it ends the pass; the single-reduction CG (variant 2)
    # forms K r once before its first step
    extra = (1 if d["lat8"] + d["lat27"] > 0 and case.solver != "cg" else 0) + (1 if case.solver == "cg" and case.cg_variant == 2 else 0)
    assert st.spmv_count == nprod - 1 + extra, (st.spmv_count, nprod, extra)
    assert abs(st.final_res - tres) <= TOL_RES * tres + floor, (st.final_res, tres, floor)
    assert abs(info.res - tres) <= TOL_RES * tres + floor  # (the oracle's float64 residual agrees with the longdouble one: the reference value is sound)


# -- the cases ----------------------------------------------------------------------------------------------------------------------------------------
LIFT = {"layout_min_rows": (0, 0)}
ONE_RANK_SOLVERS = [("bicgstabl", 2), ("idrs", 4), ("cgs2", 0), ("gmres", 4)]

CASES = [
    Case("S0", "cg", expect={"G=1", "mode0"}),
    Case("S0", "idrs", 4, expect={"G=1"}),
]
for _sn, _par in (("S1o", "odd"), ("S1e", "even")):
    CASES += [Case(_sn, "cg", expect={_par, "1<G<=256"})] + [Case(_sn, sv, s, expect={_par}) for sv, s in ONE_RANK_SOLVERS]
CASES += [Case("S2", "cg", cg_variant=v, expect={"1<G<=256", "mode0"}) for v in (1, 2, 3, 4, 0)]
CASES += [Case("S2", "cg", pr="identity"), Case("S2", "idrs", 4, pr="identity")]
CASES += [Case("S2", "bicgstabl", l) for l in (1, 2, 4)] + [Case("S2", "idrs", s) for s in (1, 4, 8, 11)]
CASES += [Case("S2", "cgs2"), Case("S2", "gmres", 20)]
CASES += [Case("S2", sv, s, knobs={"graphs": (1, 50000)}, expect={"graphs_off"}) for sv, s in (("cg", 0), ("idrs", 8), ("bicgstabl", 2))]
CASES += [Case(sn, sv, s, graphs_bitwise=True, expect={"graphs_on"}) for sn in ("S2", "S3") for sv, s in (("idrs", 8), ("cg", 0))]
# S3: cap-sized grids on the diagonal-slotted layout; the CG variants on the plain kernel, and with the size limits lifted on the patch sweep
CASES += [Case("S3", "cg", cg_variant=v, expect={"G=cap,trips>=2", "mode2"}) for v in (1, 2, 3, 4, 0)]
# (the workgroup-tile sweep k_spmv_sym27: bit 23 of the "ell" knob)
CASES += [Case("S3", "cg", cg_variant=v, knobs=dict(LIFT, ell=1 | 1 << 23), expect={"sym_sweep", "mode2"}) for v in (3, 4)]
CASES += [Case("S3", "cg", cg_variant=4, knobs=LIFT, expect={"symp"}),
          Case("S3", "cg", k=64, cg_variant=0, knobs=LIFT, expect={"symp"}, auto_is=4),
          Case("S3", "cg", pr="identity"), Case("S3", "idrs", 4, pr="identity"), Case("S3", "gmres", 20, pr="identity")]
CASES += [Case("S3", "bicgstabl", l) for l in (2, 4)] + [Case("S3", "idrs", s) for s in (4, 8, 11)] + [Case("S3", "cgs2")]
CASES += [Case("S3", "gmres", s) for s in (4, 20, 32)]
CASES += [Case("S3", sv, s, knobs={"graphs": (1, 50000)}, expect={"graphs_off"}) for sv, s in (("cg", 0), ("idrs", 8))]
# vec_grid 1: the cap is the CU count (256 < 1 200 wanted), 5 grid-stride trips; vec_grid 8: G = 1 200, reduce_partials_bcast's second trip
CASES += [Case("S3", sv, s, knobs={"vec_grid": 1}, expect={"G=cap,trips>=2"}) for sv, s in (("cg", 0), ("idrs", 8), ("bicgstabl", 2))]
CASES += [Case("S3", sv, s, knobs={"vec_grid": 8}, expect={"G>1024"})
          for sv, s in (("cg", 0), ("idrs", 8), ("idrs", 11), ("bicgstabl", 4), ("cgs2", 0), ("gmres", 20))]
# lattice tiles: mode 5 (3-field hex-8), mode 4 (hex-27), the Nitsche brick (tiles + the skew remainder)
CASES += [Case("S4", "cg", expect={"mode5", "256<G<cap"}), Case("S4", "idrs", 4, expect={"mode5"}), Case("S4", "bicgstabl", 2, expect={"mode5"})]
CASES += [Case("S5", "cg", expect={"mode4", "odd"}), Case("S5", "idrs", 4, expect={"mode4"}), Case("S5", "bicgstabl", 2, expect={"mode4"})]
CASES += [Case("S6", sv, s, expect={"remainder"}) for sv, s in (("idrs", 4), ("idrs", 8), ("bicgstabl", 2), ("cgs2", 0), ("gmres", 20))]
CASES += [Case("S6", "gmres", 4), Case("S6", "idrs", 4, pl="diag"), Case("S6", "bicgstabl", 2, pl="rownorm"), Case("S6", "gmres", 20, pl="diag")]
# modes 1 and 3 on a 3-field pattern with the size limits lifted: no lattice tiles and no diagonal slots -> explicit columns; slot-major copies off
# as well -> the sliced layout, here for a caller-supplied CSR
CASES += [Case("S7", sv, s, knobs=dict(LIFT, lat8=0, ell=3), expect={"mode1"}) for sv, s in (("cg", 0), ("idrs", 4))]
CASES += [Case("S7", sv, s, knobs=dict(LIFT, lat8=0, ell=0), caller_csr=True, expect={"mode3"}) for sv, s in (("cg", 0), ("idrs", 4), ("bicgstabl", 2))]
# the node-blocked sliced layout (BSELL) of an unstructured 3-field pattern, and the row-sorted form of the same pattern
CASES += [Case("S8", sv, s, knobs=LIFT, expect={"mode3", "bsell"}) for sv, s in (("cg", 0), ("idrs", 4), ("idrs", 8), ("bicgstabl", 2), ("gmres", 20))]
CASES += [Case("S8", sv, s, knobs=dict(LIFT, bsell=0), expect={"mode3"}) for sv, s in (("cg", 0), ("idrs", 4))]

REQUIRED = {"mode0", "mode1", "mode2", "mode3", "mode4", "mode5", "remainder", "bsell", "sym_sweep", "symp", "graphs_on", "graphs_off",
            "G=1", "1<G<=256", "256<G<cap", "G=cap,trips>=2", "G>1024", "odd", "even"}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_solver_steps_match_the_oracle(mf, systems, case):
    _run_case(mf, systems, case)


def test_every_solver_path_ran(mf, systems):
    """The cases between them reached every layout, sweep, graph mode, grid class and parity of REQUIRED -- independent of test selection: the cases
    the session did not run are run here first."""
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        if c.id not in RAN:
            _run_case(mf, systems, c)
    ran = set().union(*RAN.values())
    assert REQUIRED <= ran, sorted(REQUIRED - ran)
