"""The ring of search directions of the classic CG pass (csrc/cg_decide.h, csrc/krylov_cg.hip): x is written once per m iterations, from the last m
directions, per element in iteration order with the per-iteration update's own fma -- so a solve with the depth forced to 2, 3, 8 or 16
(mfem_debug_set("cg_ring")) must return the solution AND the statistics of the m = 1 solve bit for bit, wherever the pass ends: fixed iteration counts
around the ring's edges, a tolerance stop inside a ring and on a flush position, a restart in mid-ring (max_pass = 2), check_every 5 and 32, captured
cycles on and off, every recurrence (cg_variant 0, 1, 3, 4: auto, plain Jacobi, z-carrying, scaled), the fused hex-27 iteration on the lattice tiles,
and two ranks on one GPU through the host transport (tests/cg_ring_worker.py).

The hex-8 brick is a 33 x 17 x 9 lattice: 5049 rows -- an odd count, padded to 5056 --, ten workgroups of the vector kernels."""
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K_COND, H, TENV = 0.6, 25.0, 293.15
DEPTHS = [2, 3, 8, 16]
VARIANTS = [0, 1, 3, 4]


@pytest.fixture(scope="module")
def small_layouts():
    """Solver layouts on small systems too: cg_variant 4 scales only on the diagonal-slotted layout, the hex-27 brick takes the lattice tiles."""
    from metafem_jl_amd import _lib

    _lib.lib.mfem_debug_set_layout_min_rows(0, 0)
    yield _lib
    _lib.lib.mfem_debug_set_layout_min_rows(262144, 1000000)
    _lib.lib.mfem_debug_set_cg_ring(0)
    _lib.lib.mfem_debug_set_graphs(1, 0)


class _System:
    """A matrix, a right-hand side and the m = 1 results of every solve asked for so far (computed once, shared, never changed)."""

    def __init__(self, mf, dims, order, itg):
        self.mf = mf
        b = mf.make_Brick((1.0, 0.8, 1.2), dims, order, itg)
        self.A = b.pattern(1)
        self.K = b.assemble_thermal(self.A, K_COND, H, TENV, 0x3F)
        self.rhs = mf.FEM_rand(self.A.n, 5, 0) - 0.5
        self.brick = b
        self.ref = {}

    def solve(self, _lib, m, graphs, tol, **kw):
        _lib.check(_lib.lib.mfem_debug_set_graphs(1 if graphs else 0, 0))
        _lib.check(_lib.lib.mfem_debug_set_cg_ring(m))
        x, st = self.mf.iterative_Solve(self.A, self.K, self.rhs, tol, Sv_func=self.mf.cg_, **kw)
        return x.cpu().numpy().tobytes(), (st.passes, st.iterations, st.final_res, st.initial_res, st.converged, st.spmv_count)

    def reference(self, _lib, graphs, tol, **kw):
        key = (graphs, tol, tuple(sorted(kw.items())))
        if key not in self.ref:
            self.ref[key] = self.solve(_lib, 1, graphs, tol, **kw)
        return self.ref[key]

    def same_as_m1(self, _lib, m, graphs, tol, **kw):
        c0 = int(_lib.lib.mfem_debug_cg_ring_count())
        want_x, want_st = self.reference(_lib, graphs, tol, **kw)
        assert int(_lib.lib.mfem_debug_cg_ring_count()) == c0  # (m = 1: no ring)
        got_x, got_st = self.solve(_lib, m, graphs, tol, **kw)
        assert int(_lib.lib.mfem_debug_cg_ring_count()) == c0 + got_st[0], "the pass did not run with the ring"  # (one per pass)
        assert got_st == want_st, (m, graphs, tol, kw, got_st, want_st)
        assert got_x == want_x, (m, graphs, tol, kw, "x differs in its bits")
        return want_st


@pytest.fixture(scope="module")
def hex8(mf, small_layouts):
    return _System(mf, (32, 16, 8), 1, 3)


@pytest.fixture(scope="module")
def hex27(mf, small_layouts):
    return _System(mf, (4, 4, 4), 2, 5)  # 9 x 9 x 9 points


_STOPS = {}


def _tolerance_stops(system, _lib, variant):
    """iteration count -> a tolerance at which the m = 1 pass stops there by its tolerance test (a sweep of tolerances, once per variant)"""
    key = (id(system), variant)
    if key not in _STOPS:
        res0 = float(np.sqrt(float((system.rhs * system.rhs).mean())))
        stops = {}
        for e in np.linspace(1.0, 9.0, 161):
            tol = res0 * 10.0 ** (-e)
            _, st = system.reference(_lib, True, tol, maxiter=4000, max_pass=1, cg_variant=variant)
            if 0 < st[1] < 4000:  # (ended by the tolerance test, not by maxiter)
                stops.setdefault(st[1], tol)
        _STOPS[key] = stops
    return _STOPS[key]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m", DEPTHS)
def test_fixed_iteration_counts_around_the_ring(hex8, small_layouts, m, variant):
    """0, 1, m - 1, m, m + 1 and 2 m + 3 iterations: nothing pending, a ring that never flushes, the flush itself, one past it, two rings and a tail"""
    for iters in sorted({0, 1, m - 1, m, m + 1, 2 * m + 3}):
        for check_every in (5, 32):
            for graphs in (True, False):
                st = hex8.same_as_m1(small_layouts, m, graphs, 1e-300, maxiter=iters, max_pass=1, fixed_iterations=True, check_every=check_every,
                                     cg_variant=variant)
                assert st[1] == iters


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m", DEPTHS)
def test_tolerance_stop_inside_a_ring_and_on_a_flush_position(hex8, small_layouts, m, variant):
    """A pass that its tolerance test ends after T iterations: T % m == 0 -- the last iteration is a flush position, k_cg_pupdate applies all m pending
    updates -- and T % m != 0 -- k_cg_xflush applies the T % m that are left"""
    stops = _tolerance_stops(hex8, small_layouts, variant)
    on = [t for t in sorted(stops) if t % m == 0 and t >= m]
    inside = [t for t in sorted(stops) if t % m != 0 and t > m]
    assert on and inside, (m, sorted(stops))
    for T in (on[0], inside[0], inside[-1]):
        for check_every in (5, 32):
            for graphs in (True, False):
                st = hex8.same_as_m1(small_layouts, m, graphs, stops[T], maxiter=4000, max_pass=1, check_every=check_every, cg_variant=variant)
                assert st[1] == T, (T, st)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m", DEPTHS)
def test_restart_in_mid_ring(hex8, small_layouts, m, variant):
    """max_pass = 2 with passes that maxiter ends after 3 m + 1 iterations: the first pass leaves one update pending, the second starts from its x"""
    for check_every in (5, 32):
        for graphs in (True, False):
            st = hex8.same_as_m1(small_layouts, m, graphs, 1e-300, maxiter=3 * m + 1, max_pass=2, check_every=check_every, cg_variant=variant)
            assert st[0] == 2 and st[1] == 2 * (3 * m + 1), st


@pytest.mark.parametrize("m", DEPTHS)
def test_fused_hex27_iteration_on_the_lattice_tiles(hex27, small_layouts, m):
    """The lat_fused branch of the pass (pass 2 of the tiles inside the residual update) hands the same ring to k_cg_pupdate"""
    _lib = small_layouts
    assert int(_lib.lib.mfem_debug_lat27_cg_fused()) == 1
    for variant in VARIANTS:
        for graphs in (True, False):
            c0 = int(_lib.lib.mfem_debug_lat27_spmv_count())
            for iters in sorted({0, 1, m - 1, m, m + 1, 2 * m + 3}):
                hex27.same_as_m1(_lib, m, graphs, 1e-300, maxiter=iters, max_pass=1, fixed_iterations=True, check_every=5, cg_variant=variant)
            assert int(_lib.lib.mfem_debug_lat27_spmv_count()) > c0  # (the tiles served these solves)
            res0 = float(np.sqrt(float((hex27.rhs * hex27.rhs).mean())))
            st = hex27.same_as_m1(_lib, m, graphs, 1e-9 * res0, maxiter=4000, max_pass=2, check_every=5, cg_variant=variant)
            assert st[4] == 1
            hex27.same_as_m1(_lib, m, graphs, 1e-300, maxiter=3 * m + 1, max_pass=2, check_every=32, cg_variant=variant)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_on_one_gpu():
    """Two slabs of the hex-8 brick on cuda:0 through the host-callback communicator: every rank's x and statistics for m = 2, 3, 8, 16 against its own
    m = 1 solve, bit for bit (the worker compares; its report lists every comparison)"""
    world, port = 2, _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    logs = [tempfile.TemporaryFile() for _ in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "cg_ring_worker.py"), str(world), str(r), str(port)], stdout=logs[r],
                              stderr=subprocess.STDOUT, env=env) for r in range(world)]
    deadline = time.monotonic() + 300
    try:
        for p in procs:
            try:
                p.wait(timeout=max(deadline - time.monotonic(), 0.1))
            except subprocess.TimeoutExpired:
                break
            if p.returncode != 0:  # a dead rank leaves the other waiting in a collective
                deadline = min(deadline, time.monotonic() + 20)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, f) in enumerate(zip(procs, logs)):
        f.seek(0)
        out = f.read().decode(errors="replace")
        f.close()
        line = [ln for ln in out.splitlines() if ln.startswith("CG_RING_REPORT ")]
        rep = json.loads(line[-1][len("CG_RING_REPORT "):]) if line else None
        assert p.returncode == 0 and rep is not None and rep["compared"] > 0 and not rep["failed"], (
            f"rank {r}: rc={p.returncode}, report {rep}\n--- output tail ---\n" + out[-3000:])
