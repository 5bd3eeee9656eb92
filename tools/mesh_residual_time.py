"""Residual (K_nonlinear_func) time of the unstructured legs with the fused mesh residual (GenericDomain(fused_residual=True): mfem_mesh_residual_elements
/ _facets, geometry on the fly) and with the operator path (mfem_op_var_batch + mfem_op_res_batch on the stored geometry tables), and the table bytes each
domain holds.  Meshes as bench.py's u20_* / tet10_* legs (bench_legs.Bench.unstructured_mesh), one domain alive at a time.
usage: mesh_residual_time.py [legs = u20_thermal_96,u20_elasticity_96,tet10_thermal_64,tet10_elasticity_64] [reps = 10]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import bench_legs as L  # noqa: E402
from metafem_jl_amd import generic as G, physics  # noqa: E402

legs = (sys.argv[1] if len(sys.argv) > 1 else "u20_thermal_96,u20_elasticity_96,tet10_thermal_64,tet10_elasticity_64").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = L.Bench(bench.parse_args([]))


def domain(space, msh, fac, fields, fused):
    if fields == 1:
        wf = physics.thermal_domain(3, L.K_COND)
        bnd = [(fac.element_ID, fac.element_eindex, physics.thermal_convection(L.H, L.TENV))]
    else:
        wf = physics.elasticity_domain(3, L.LAM, L.MU)
        c = fac.centroid
        wall, top = fac.select(np.abs(c[:, 0]) < 1e-9), fac.select(np.abs(c[:, 1] - 1.0) < 1e-9)
        bnd = [(wall.element_ID, wall.element_eindex, physics.penalty([0, 1, 2], L.TAU)),
               (top.element_ID, top.element_eindex, physics.traction(3, "sl", rows=[1]))]
    gd = G.GenericDomain(B.ctx, space, msh.coords, msh.cp_ids, fields, wf, bnd, fused_residual=fused)
    if fields == 1:
        gd.controlpoints["s"] = torch.full((msh.ncp,), L.SRC, dtype=torch.float64, device=B.dev)
    else:
        for v in (2, 4, 6):
            gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device=B.dev)
    gd.x_star.copy_(torch.linspace(-1.0, 1.0, gd.x_star.numel(), dtype=torch.float64, device=B.dev))
    return gd


def time_residual(gd):
    gd.K_nonlinear_func()  # (first call: analysis, adjacency, workspace)
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


for leg in legs:
    kind, phys, n = leg.split("_")
    n, fields = int(n), 1 if phys == "thermal" else 3
    space, msh, fac = B.unstructured_mesh(n, shape="CUBE" if kind == "u20" else "SIMPLEX")
    out = {"leg": leg, "nel": int(msh.cp_ids.shape[1]), "ncp": int(msh.ncp)}
    res = {}
    for fused in (True, False):
        tag = "fused" if fused else "operator"
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        gd = domain(space, msh, fac, fields, fused)
        out[f"{tag}_table_bytes_built"] = gd.table_bytes
        med, mn = time_residual(gd)
        torch.cuda.synchronize()
        out[f"{tag}_residual_ms"], out[f"{tag}_residual_ms_min"] = round(med, 3), round(mn, 3)
        out[f"{tag}_table_bytes"] = gd.table_bytes
        out[f"{tag}_domain_bytes"] = torch.cuda.memory_allocated() - m0
        res[tag] = gd.residue.cpu().numpy()
        del gd
        torch.cuda.empty_cache()
    out["max_rel_diff"] = float(np.abs(res["fused"] - res["operator"]).max() / np.abs(res["operator"]).max())
    print(json.dumps(out), flush=True)
