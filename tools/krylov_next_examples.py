"""cgs! / tfqmr! / lsqr! timings, on the model of tools/gmres_examples.py.

  * the lid-driven cavity step of tools/cavity_solvers.py (oracle.cavity.build_cavity(40, Cb = 8), 2D_Script.jl's limits: maxiter 10000,
    max_pass 20, converge_tol 1e-8) with cgs! and tfqmr! next to cgs2!;
  * the 2D stress-concentration example (2D_Script.jl: maxiter 2000, max_pass 20, converge_tol 1e-8) with tfqmr! and lsqr! next to
    gmres!(20) and idrs!(20), on its first Newton system;
  * a hex-8 thermal brick of 128^3 nodes: ms per iteration of the three solvers (the difference of two fixed-iteration solves), tmul!
    against mul! on the same matrix (device events), the transpose plan's build time and bytes, and what the new vector kernels move by
    design, for the kernel times of a separate `rocprofv3 --kernel-trace --stats` run of `--large-only`.

  python tools/krylov_next_examples.py [--large-only] [--large N] [--json OUT]
  rocprofv3 --kernel-trace --stats -d PROF -o nx -- python tools/krylov_next_examples.py --large-only
  python tools/krylov_next_examples.py --prof-db PROF/nx_results.db [--large N]     (no GPU: the share of HBM peak from that trace)
Nothing here asserts a time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E spec

# vectors of n doubles each new kernel reads + writes per launch, by design (krylov_next.hip)
VEC_STREAMS = {"kcs_su": 5, "kcs_px": 5, "ktq_qv": 4, "ktq_rcgs": 4, "ktq_update": 10, "klq_lin_norm": 3, "klq_uscale": 2, "klq_xw": 6}


def _row(st, ms):
    return dict(solve_ms=ms, passes=st.passes, iterations=st.iterations, final_res=st.final_res, converged=bool(st.converged))


def _timed(mf, A, K, b, tol, reps=3, **kw):
    runs = []
    for _ in range(reps):  # (the first solve on a pattern captures the cycle graphs)
        dx, st = mf.iterative_Solve(A, K, b, tol, **kw)
        runs.append((st.solve_ms, st))
    ms = sorted(r[0] for r in runs)[len(runs) // 2]
    return _row(runs[-1][1], ms)


def cavity_example(mf):
    import torch

    import test_gpu_generic as tg
    from oracle import cavity

    od = cavity.build_cavity(40, Cb=8.0)
    gd = tg._gpu_domain(mf, od, "Serendipity", 2, 5)
    n = od.mesh.ncp
    od.controlpoints["u1"], od.controlpoints["u2"] = np.zeros(n), np.zeros(n)
    cavity.set_step_parameters(od, 0.1)
    for k in ("uw1", "uw2", "taum", "tauc"):
        gd.controlpoints[k] = torch.tensor(od.controlpoints[k], device="cuda")
    gd.K_linear_func(); gd.x_star.zero_(); gd.K_nonlinear_func()
    out = {}
    for name, sv in (("cgs2", mf.cgs2_), ("cgs", mf.cgs_), ("tfqmr", mf.tfqmr_)):
        out[name] = _timed(mf, gd.A, gd.K_total, gd.residue, 1e-8, 1, Sv_func=sv, maxiter=10000, max_pass=20)  # (seconds per solve)
        out[name]["dof"] = int(gd.residue.numel())
    return out


def stress_example(mf, reps=3):
    import gmres_examples as ge

    out = {}

    def solver(g):
        res = None
        for name, sv, s in (("gmres", mf.gmres_, 20), ("idrs", mf.idrs_, 20), ("tfqmr", mf.tfqmr_, 0), ("lsqr", mf.lsqr_, 0)):
            out[name] = _timed(mf, g.A, g.K_total, g.residue, g.converge_tol, reps, Sv_func=sv, maxiter=2000, max_pass=20, s=s)
            out[name]["dof"] = int(g.residue.numel())
            if name == "gmres":
                res, _ = mf.iterative_Solve(g.A, g.K_total, g.residue, g.converge_tol, Sv_func=sv, maxiter=2000, max_pass=20, s=s)
        return res

    gd = _stress_domain(mf, ge._wf)
    gd.linear_solver = solver
    gd.update_OneStep()
    return out


def _stress_domain(mf, _wf):
    import torch
    from metafem_jl_amd import element, generic as G, mesh as pm
    from oracle import problems, stress_concentration as scn
    from oracle.cantilever import traction_field

    z = np.load(os.path.join(ROOT, "tests", "golden", "stress_concentration_2d.npz"))
    space = element.classical_space(2, "Serendipity", 2, 5)
    msh = pm.mesh_Classical(z["vert"], z["conn"].astype(np.int64), space)
    fac = pm.get_BoundaryMesh(msh)
    E, nu, L, err = 210e9, 0.3, 5.0, 0.05
    lam, mu, tau = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu)), 10000 * E / L ** 2
    c = fac.centroid
    bnd = []
    for d in range(2):
        f = fac.select(np.abs(c[:, d]) < err)
        bnd.append((f.element_ID, f.element_eindex, _wf(scn.penalty_component(d, tau))))
    f = fac.select(np.abs(c[:, 1] - L) < err)
    bnd.append((f.element_ID, f.element_eindex, _wf(traction_field(2, "sl", rows=[1]))))
    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, 2, _wf(problems.elasticity_domain(2, lam, mu)), bnd)
    for v in (2, 3):
        gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device="cuda")
    gd.converge_tol = 1e-8
    return gd


def large(mf, nodes, k1=20, k2=120):
    import ctypes as C

    import torch
    from metafem_jl_amd import _lib

    b = mf.make_Brick((1.0, 1.0, 1.0), (nodes - 1,) * 3, 1, 3)
    A = b.pattern(1)
    K = b.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F)
    rhs = mf.FEM_rand(A.n, 5, 0) - 0.5
    out = dict(dof=int(A.n), nnz=int(A.nnz))
    for name, sv in (("cgs", mf.cgs_), ("tfqmr", mf.tfqmr_), ("lsqr", mf.lsqr_)):
        t = {}
        for k in (k1, k2, k1, k2):
            _, st = mf.iterative_Solve(A, K, rhs, 1e-30, Sv_func=sv, maxiter=k, max_pass=1, fixed_iterations=True)
            t[k] = min(t.get(k, 1e30), st.solve_ms)
        out[name] = dict(ms_per_iteration=(t[k2] - t[k1]) / (k2 - k1))
    nb, ms = C.c_int64(), C.c_double()
    _lib.lib.mfem_debug_csr_tplan(A._h, C.byref(nb), C.byref(ms))  # built by the lsqr! solves above
    A2 = b.pattern(1)  # a fresh handle: the first tmul! plans
    x = mf.FEM_rand(A.n, 7, 0)
    y = torch.zeros(A.n, dtype=torch.float64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    mf.tmul_(y, A2, K, x)
    e1.record()
    torch.cuda.synchronize()
    first_ms = e0.elapsed_time(e1)
    nb2, ms2 = C.c_int64(), C.c_double()
    _lib.lib.mfem_debug_csr_tplan(A2._h, C.byref(nb2), C.byref(ms2))
    out["tplan"] = dict(bytes=nb.value, build_ms_in_lsqr=ms.value, build_ms_first_tmul=ms2.value, first_tmul_ms=first_ms)
    for name, fn in (("mul", lambda: mf.mul_(y, A2, K, x)), ("tmul", lambda: mf.tmul_(y, A2, K, x))):
        for _ in range(3):
            fn()
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[f"{name}_ms"] = e0.elapsed_time(e1) / 20
    return out


def prof_share(db, nodes):
    """The new vector kernels of a rocprofv3 trace of `--large-only`: design bytes / kernel time."""
    import sqlite3

    n = nodes ** 3
    rows = sqlite3.connect(db).execute("select name, count(*), sum(end - start) from kernels group by name").fetchall()
    res = {}
    for key, streams in VEC_STREAMS.items():
        hit = [(k, t) for name, k, t in rows if key in name]
        if not hit:
            continue
        launches, secs = sum(k for k, _ in hit), sum(t for _, t in hit) * 1e-9
        byts = launches * streams * n * 8
        res[key] = dict(launches=launches, ms=secs * 1e3, TBps=byts / secs / 1e12, hbm_share=byts / secs / HBM_PEAK)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--large", type=int, default=128, help="nodes per edge of the hex-8 thermal brick")
    ap.add_argument("--json", default=None)
    ap.add_argument("--prof-db", default=None, help="rocprofv3 database of a --large-only run: the new vector kernels' share of HBM peak")
    a = ap.parse_args()
    if a.prof_db:
        for k, r in prof_share(a.prof_db, a.large).items():
            print(f"{k}: {r['launches']} launches, {r['ms']:.2f} ms, {r['TBps']:.2f} TB/s by design = {r['hbm_share']:.3f} of HBM peak (8 TB/s)")
        return
    import metafem_jl_amd as mf

    res = {}
    if not a.large_only:
        res["cavity"] = cavity_example(mf)
        for k, r in res["cavity"].items():
            print(f"cavity step ({r['dof']} DOF) {k}: {r['solve_ms']:.1f} ms, {r['passes']} pass(es), {r['iterations']} iterations, "
                  f"res {r['final_res']:.2e}, converged {r['converged']}", flush=True)
        res["stress_2d"] = stress_example(mf)
        for k, r in res["stress_2d"].items():
            print(f"stress_concentration 2D ({r['dof']} DOF) {k}: {r['solve_ms']:.1f} ms, {r['passes']} pass(es), {r['iterations']} iterations, "
                  f"res {r['final_res']:.2e}, converged {r['converged']}", flush=True)
    r = large(mf, a.large)
    res["large"] = r
    print(f"hex-8 thermal {a.large}^3 ({r['dof']} DOF): ms/iteration cgs! {r['cgs']['ms_per_iteration']:.3f}, tfqmr! {r['tfqmr']['ms_per_iteration']:.3f}, "
          f"lsqr! {r['lsqr']['ms_per_iteration']:.3f}; mul! {r['mul_ms']:.3f} ms, tmul! {r['tmul_ms']:.3f} ms (value gather included); transpose plan "
          f"{r['tplan']['bytes'] / 2 ** 20:.0f} MiB, built in {r['tplan']['build_ms_first_tmul']:.1f} ms", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
