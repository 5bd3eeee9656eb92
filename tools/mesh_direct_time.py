"""K_linear_func time on bench.py's unstructured meshes with the direct row assembly (GenericDomain(direct_rows=True): mfem_mesh_assemble_elements_direct,
no element-matrix scratch) against the two-pass row-owner form (the default), per leg:
  hex-20 n^3 and tet-10 m^3 (the brick cut into tetrahedra), each with the thermal form (1 field) and linear elasticity (3 fields), facets included.
Recorded besides the times: the one-off plan time (mfem_mesh_direct_plan_create, host inspector + upload), the plan's device bytes, the context
workspace after the assemblies (the two-pass form's scratch lives there), geometry evaluations per element, and the largest difference of K.
A fresh context per domain, one domain alive at a time; warm-up, then the median of `reps` event-timed calls.
usage: mesh_direct_time.py [n_hex20 = 96] [n_tet10 = 64] [reps = 7] [budget_bytes = 0 (default)] [legs = u20_1,u20_3,tet10_1,tet10_3]"""
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import bench_legs as L  # noqa: E402
import metafem_jl_amd as mf  # noqa: E402
from metafem_jl_amd import _lib, generic as G, physics  # noqa: E402

n20 = int(sys.argv[1]) if len(sys.argv) > 1 else 96
n10 = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
budget = int(sys.argv[4]) if len(sys.argv) > 4 else 0
legs = sys.argv[5].split(",") if len(sys.argv) > 5 else ["u20_1", "u20_3", "tet10_1", "tet10_3"]
B = L.Bench(bench.parse_args([]))
_lib.check(_lib.lib.mfem_debug_set_mesh_direct_budget(budget))


def domain(ctx, shape, n, fields, direct):
    space, msh, fac = B.unstructured_mesh(n, shape=shape)
    if fields == 1:
        wf = physics.thermal_domain(3, L.K_COND)
        bnd = [(fac.element_ID, fac.element_eindex, physics.thermal_convection(L.H, L.TENV))]
    else:
        wf = physics.elasticity_domain(3, L.LAM, L.MU)
        c = fac.centroid
        wall, top = fac.select(np.abs(c[:, 0]) < 1e-9), fac.select(np.abs(c[:, 1] - 1.0) < 1e-9)
        bnd = [(wall.element_ID, wall.element_eindex, physics.penalty([0, 1, 2], L.TAU)),
               (top.element_ID, top.element_eindex, physics.traction(3, "sl", rows=[1]))]
    gd = G.GenericDomain(ctx, space, msh.coords, msh.cp_ids, fields, wf, bnd, direct_rows=direct)
    if fields == 1:
        gd.controlpoints["s"] = torch.full((msh.ncp,), L.SRC, dtype=torch.float64, device=B.dev)
    else:
        for v in (2, 4, 6):
            gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device=B.dev)
    gd.update_Time()
    return gd


def time_linear(gd):
    gd._row_ranks()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gd._direct()  # (None unless direct_rows: the plan, once per pattern)
    torch.cuda.synchronize()
    plan_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(2):
        gd.K_linear_func()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        ev[0].record()
        gd.K_linear_func()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms)), float(np.min(ms)), plan_ms


for leg in legs:
    tag, fields = leg.rsplit("_", 1)
    fields = int(fields)
    shape, n = ("CUBE", n20) if tag == "u20" else ("SIMPLEX", n10)
    out, Ks = {"leg": leg, "n": n, "fields": fields, "budget_bytes": budget}, {}
    for direct in (True, False):
        name = "direct" if direct else "two_pass"
        ctx = mf.Context(torch.cuda.current_device())
        gd = domain(ctx, shape, n, fields, direct)
        out["nel"], out["ncp"], out["nnz"] = int(gd.nel), int(gd.ncp), int(gd.A.nnz)
        n0 = int(_lib.lib.mfem_debug_mesh_direct_count())
        med, mn, plan_ms = time_linear(gd)
        out[f"{name}_ms"], out[f"{name}_ms_min"] = round(med, 3), round(mn, 3)
        out[f"{name}_ws_bytes"] = int(_lib.lib.mfem_debug_ws_bytes(ctx._h))
        if direct:
            st = gd.direct_stats()
            out["direct_took_the_form"] = st is not None and int(_lib.lib.mfem_debug_mesh_direct_count()) > n0
            if st:
                out.update(plan_ms=round(plan_ms, 1), plan_bytes=st["device_bytes"], batches=st["batches"], budget_doubles=st["budget_doubles"],
                           waves_per_workgroup=st["waves_per_workgroup"], lds_bytes=st["lds_bytes"], waves_per_trip=st["waves_per_trip"],
                           geometry_per_element=round(st["geometry_evaluations"] / gd.nel, 2))
        Ks[name] = gd.K_linear.cpu().numpy()
        del gd
        gc.collect()
        ctx.close()
        torch.cuda.empty_cache()
    out["direct_over_two_pass"] = round(out["direct_ms"] / out["two_pass_ms"], 3)
    out["ws_bytes_not_allocated"] = out["two_pass_ws_bytes"] - out["direct_ws_bytes"]
    out["K_max_rel_diff"] = float(np.abs(Ks["direct"] - Ks["two_pass"]).max() / np.abs(Ks["two_pass"]).max())
    print(json.dumps(out), flush=True)
_lib.lib.mfem_debug_set_mesh_direct_budget(0)
