"""gmres! timings: examples/linear_elasticity/stress_concentration/{2D,3D}_Script.jl as the scripts write them (gmres!, maxiter 2000,
max_pass 20, s = 20, converge_tol 1e-8) -- solve ms (device events), passes, iterations, ms per cycle -- next to idrs!(s = 20), the solver
3D_Script.jl uses, on the same first Newton system.  Then a hex-8 thermal brick whose Krylov basis is well over 256 MiB (128^3 nodes,
21 vectors of 2.1 M entries = 350 MB): what the orthogonalisation kernels move by design per cycle, for the kernel times of a separate
`rocprofv3 --kernel-trace --stats` run of `--large-only`.

  python tools/gmres_examples.py [--large-only] [--large N] [--json OUT]
  rocprofv3 --kernel-trace --stats -d PROF -o gmres -- python tools/gmres_examples.py --large-only
  python tools/gmres_examples.py --prof-db PROF/gmres_results.db [--large N]     (no GPU: the share of HBM peak from that trace)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E spec


def _wf(wf):
    from metafem_jl_amd import generic as G

    return G.WeakForm(inner_vars=list(wf.inner_vars), cp_ext_vars=list(wf.cp_ext_vars), normals=list(wf.normals),
                      residues=[G.ResTerm(r.dual_pos, r.dual_s, r.fn) for r in wf.residues],
                      linear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.linear_gradients],
                      nonlinear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.nonlinear_gradients])


def stress_example(mf, dim, reps=3):
    import torch
    from metafem_jl_amd import element, generic as G, mesh as pm
    from oracle import problems, stress_concentration as scn
    from oracle.cantilever import traction_field

    z = np.load(os.path.join(ROOT, "tests", "golden", f"stress_concentration_{dim}d.npz"))
    space = element.classical_space(dim, "Serendipity", 2, 5)
    msh = pm.mesh_Classical(z["vert"], z["conn"].astype(np.int64), space)
    fac = pm.get_BoundaryMesh(msh)
    E, nu, L, err = 210e9, 0.3, 5.0, 0.05
    lam, mu, tau = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu)), 10000 * E / L ** 2
    c = fac.centroid
    bnd = []
    for d in range(dim):
        f = fac.select(np.abs(c[:, d]) < err)
        bnd.append((f.element_ID, f.element_eindex, _wf(scn.penalty_component(d, tau))))
    f = fac.select(np.abs(c[:, 1] - L) < err)
    bnd.append((f.element_ID, f.element_eindex, _wf(traction_field(dim, "sl", rows=[1]))))
    gd = G.GenericDomain(mf.default_context(), space, msh.coords, msh.cp_ids, dim, _wf(problems.elasticity_domain(dim, lam, mu)), bnd)
    for v in {2: (2, 3), 3: (2, 4, 6)}[dim]:
        gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device="cuda")
    gd.converge_tol = 1e-8
    out = {}

    def solver(g):
        res = None
        for name, sv in (("gmres", mf.gmres_), ("idrs", mf.idrs_)):
            runs = []
            for _ in range(reps):  # (the first solve on a pattern captures the cycle graphs)
                dx, st = mf.iterative_Solve(g.A, g.K_total, g.residue, g.converge_tol, Sv_func=sv, maxiter=2000, max_pass=20, s=20)
                runs.append((st.solve_ms, st.passes, st.iterations, st.final_res, st.converged))
                if name == "gmres":
                    res = dx
            ms = sorted(r[0] for r in runs)[len(runs) // 2]
            _, passes, iters, fres, conv = runs[-1]
            row = dict(solve_ms=ms, passes=passes, iterations=iters, final_res=fres, converged=bool(conv), dof=int(g.residue.numel()))
            if name == "gmres":
                row["cycles"] = int(np.ceil(max(iters - passes, 0) / 20))
                row["ms_per_cycle"] = ms / max(row["cycles"], 1)
            out[name] = row
        return res

    gd.linear_solver = solver
    gd.update_OneStep()
    return out


def orth_bytes(n, s):
    """Design traffic of one cycle's orthogonalisation kernels (two CGS passes per step k: block dot (k + 1) n 8 B, update (k + 2) n 8 B;
    the normalisation 2 n 8 B)."""
    return sum(2 * (2 * k + 3) * n * 8 + 2 * n * 8 for k in range(1, s + 1))


def large(mf, nodes, cycles=4, s=20):
    b = mf.make_Brick((1.0, 1.0, 1.0), (nodes - 1,) * 3, 1, 3)
    A = b.pattern(1)
    K = b.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F)
    rhs = mf.FEM_rand(A.n, 5, 0) - 0.5
    maxiter = cycles * s
    runs = []
    for _ in range(2):
        _, st = mf.iterative_Solve(A, K, rhs, 1e-30, Sv_func=mf.gmres_, maxiter=maxiter - 1, max_pass=1, s=s, fixed_iterations=True)
        runs.append(st.solve_ms)
    nv = A.n
    return dict(dof=int(A.n), basis_MiB=(s + 1) * nv * 8 / 2 ** 20, cycles=cycles, solve_ms=min(runs), ms_per_cycle=min(runs) / cycles,
                orth_bytes_per_cycle=orth_bytes(A.n, s))


def prof_share(db, nodes, s=20):
    """Orthogonalisation kernels (kg_block_dot, kg_update, kg_normalize) of a rocprofv3 trace of `--large-only`: design bytes / kernel time."""
    import sqlite3

    rows = sqlite3.connect(db).execute("select name, count(*), sum(end - start) from kernels group by name").fetchall()
    pick = lambda *keys: [(k, t) for name, k, t in rows if any(key in name for key in keys)]
    t_orth = sum(t for _, t in pick("kg_block_dot", "kg_update", "kg_normalize")) * 1e-9
    cycles = sum(k for k, _ in pick("kg_normalize")) // s
    byts = cycles * orth_bytes(nodes ** 3, s)
    t_fold = sum(t for _, t in pick("kg_fold")) * 1e-9
    return dict(cycles=cycles, orth_ms=t_orth * 1e3, orth_GB=byts / 1e9, orth_TBps=byts / t_orth / 1e12, hbm_share=byts / t_orth / HBM_PEAK,
                fold_ms=t_fold * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--large", type=int, default=128, help="nodes per edge of the hex-8 thermal brick")
    ap.add_argument("--json", default=None)
    ap.add_argument("--prof-db", default=None, help="rocprofv3 database of a --large-only run: report the orthogonalisation kernels' share of HBM peak")
    a = ap.parse_args()
    if a.prof_db:
        r = prof_share(a.prof_db, a.large)
        print(f"orthogonalisation kernels, {r['cycles']} cycles at {a.large}^3: {r['orth_GB']:.1f} GB by design in {r['orth_ms']:.2f} ms = "
              f"{r['orth_TBps']:.2f} TB/s = {r['hbm_share']:.3f} of HBM peak (8 TB/s); the folds {r['fold_ms']:.2f} ms")
        return
    import metafem_jl_amd as mf

    res = {}
    if not a.large_only:
        for dim in (2, 3):
            r = stress_example(mf, dim)
            res[f"stress_{dim}d"] = r
            g, i = r["gmres"], r["idrs"]
            print(f"stress_concentration {dim}D ({g['dof']} DOF): gmres!(20) {g['solve_ms']:.2f} ms, {g['passes']} pass(es), {g['iterations']} iterations, "
                  f"{g['ms_per_cycle']:.3f} ms/cycle, res {g['final_res']:.2e} | idrs!(20) {i['solve_ms']:.2f} ms, {i['passes']} pass(es), "
                  f"{i['iterations']} iterations, res {i['final_res']:.2e}", flush=True)
    r = large(mf, a.large)
    res["large"] = r
    print(f"hex-8 thermal {a.large}^3 ({r['dof']} DOF, basis {r['basis_MiB']:.0f} MiB): gmres!(20) {r['ms_per_cycle']:.3f} ms/cycle; "
          f"orthogonalisation by design {r['orth_bytes_per_cycle'] / 1e9:.3f} GB/cycle (kernel times: rocprofv3 --kernel-trace --stats, "
          f"kg_block_dot + kg_update + kg_normalize)", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
