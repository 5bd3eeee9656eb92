"""K_nonlinear_func time of two nonlinear forms, table-free (GenericDomain(table_free=True): mfem_mesh_var_* / _res_* / _kval_*, geometry on the fly)
against the operator path (mfem_op_*_batch on the stored geometry tables), and the table bytes the table-free domain does not allocate:
  neo_hookean  the finite-strain Neo-Hookean domain form (9 residual + 81 nonlinear gradient terms, 3 fields) on bench.py's unstructured hex-20 mesh;
  cavity       the SUPG / PSPG cavity form with its Nitsche walls and lid (3 fields, nodal externals inside the expressions) on a quad-8 square.
Both paths evaluate the same coefficient expressions (torch broadcasts); one domain alive at a time.
usage: mesh_ops_time.py [n_hex20 = 48] [n_quad8 = 256] [reps = 5]"""
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import bench_legs as L  # noqa: E402
from metafem_jl_amd import element, generic as G, mesh as pm  # noqa: E402
from oracle import hyperelastic as he, problems  # noqa: E402  (the symbolic layer's output: the weak forms only)

n3 = int(sys.argv[1]) if len(sys.argv) > 1 else 48
n2 = int(sys.argv[2]) if len(sys.argv) > 2 else 256
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B = L.Bench(bench.parse_args([]))


def conv(wf):
    return G.WeakForm(inner_vars=list(wf.inner_vars), cp_ext_vars=list(wf.cp_ext_vars), normals=list(wf.normals),
                      residues=[G.ResTerm(r.dual_pos, r.dual_s, r.fn) for r in wf.residues],
                      linear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.linear_gradients],
                      nonlinear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.nonlinear_gradients])


def neo_hookean(table_free):
    space, msh, _ = B.unstructured_mesh(n3)
    gd = G.GenericDomain(B.ctx, space, msh.coords, msh.cp_ids, 3, conv(he.domain_weakform(dict(mu=1e6, lam=1e6), "neo_hookean")), [],
                         table_free=table_free)
    x = np.random.default_rng(1).uniform(-1.0, 1.0, gd.x_star.numel()) * 0.05 / n3  # (displacement gradients of a few percent)
    gd.x_star.copy_(torch.tensor(x))
    return gd


def cavity(table_free):
    rho, mu, Cb = 1e3, 1.0, 128.0
    dx = 1.0 / n2
    space = element.classical_space(2, "Serendipity", 2, 5)
    vert, conn = pm.make_Square((1.0, 1.0), (n2, n2))
    msh = pm.mesh_Classical(vert, conn, space)
    fac = pm.get_BoundaryMesh(msh)
    top = np.abs(fac.centroid[:, 1] - 1.0) < dx * 0.01
    wd, wfix, wtop = problems.cavity_weakforms(rho, mu, mu / rho * Cb / dx)
    walls, lid = fac.select(~top), fac.select(top)
    gd = G.GenericDomain(B.ctx, space, msh.coords, msh.cp_ids, 3, conv(wd), [(walls.element_ID, walls.element_eindex, conv(wfix)),
                                                                          (lid.element_ID, lid.element_eindex, conv(wtop))], table_free=table_free)
    rng = np.random.default_rng(2)
    f = lambda a: torch.tensor(a, dtype=torch.float64, device=B.dev)
    gd.controlpoints.update(uw1=f(np.full(msh.ncp, 0.05)), uw2=f(np.zeros(msh.ncp)), taum=f(rng.uniform(1e-3, 2e-3, msh.ncp)),
                            tauc=f(rng.uniform(1e-3, 2e-3, msh.ncp)))
    gd.dt = 0.2 * dx / 0.05
    gd.update_Time()
    gd.x_star.copy_(f(0.05 * rng.uniform(-1.0, 1.0, gd.x_star.numel())))
    return gd


def time_nonlinear(gd):
    gd.K_linear_func()
    gd.K_nonlinear_func()  # (first call: tables or adjacency, ranks, workspace)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        ev[0].record()
        gd.K_nonlinear_func()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms)), float(np.min(ms))


for name, build in (("neo_hookean", neo_hookean), ("cavity", cavity)):
    out, res = {"form": name}, {}
    for table_free in (True, False):
        tag = "table_free" if table_free else "operator"
        gd = build(table_free)
        out["nel"], out["ncp"] = int(gd.nel), int(gd.ncp)
        med, mn = time_nonlinear(gd)
        out[f"{tag}_ms"], out[f"{tag}_ms_min"] = round(med, 3), round(mn, 3)
        out[f"{tag}_table_bytes"] = gd.table_bytes
        if table_free:
            out["groups_fallen_back"] = sum(1 for g in gd.groups if not g.table_free)
        res[tag] = (gd.residue.cpu().numpy(), gd.K_total.cpu().numpy())
        del gd
        gc.collect()  # (the domain's table builders close over it)
        torch.cuda.empty_cache()
    out["table_bytes_not_allocated"] = out["operator_table_bytes"] - out["table_free_table_bytes"]
    out["table_free_over_operator"] = round(out["table_free_ms"] / out["operator_ms"], 3)
    out["residue_max_rel_diff"] = float(np.abs(res["table_free"][0] - res["operator"][0]).max() / np.abs(res["operator"][0]).max())
    out["K_max_rel_diff"] = float(np.abs(res["table_free"][1] - res["operator"][1]).max() / np.abs(res["operator"][1]).max())
    print(json.dumps(out), flush=True)
