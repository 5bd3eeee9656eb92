"""The matrix-free mesh operator (GenericDomain(matrix_free=True): MeshOperator, mfem_solve_operator) against the assembled path on bench.py's
unstructured meshes, per leg:
  hex-20 n^3 and tet-10 m^3 (the brick cut into tetrahedra), each with the thermal form (1 field) and linear elasticity (3 fields), facets included.
Per leg, a fresh context per domain, both domains alive, warm-up, then the median of `reps` repetitions with the two paths alternated:
  product    the operator product (event-timed mul_) against the Krylov loop's layout SpMV on the assembled K (the per-launch SpMV timing of a
             20-step fixed idrs!(8) solve: mfem_prof_spmv_*) and against the fused residual of the same form (event-timed K_nonlinear_func);
             condition: operator <= 1.1 x fused residual (the residual does strictly more: externals and the constant part)
  set-up     the operator's diagonal against K_linear_func (assembly) plus the layout fill (mfem_spmv_solver_layout minus one layout SpMV)
  solve      a 200-step idrs!(8) + Pr_Jacobi! solve both ways (stats.solve_ms), the residual ||b - K x|| / sqrt(n) recomputed with either product
             (the operator's solution also on the assembled K; IDR(s) residuals after a fixed number of steps differ between summation orders)
  bytes      torch.cuda.memory_allocated + mfem_debug_ws_bytes after the solve, both ways
With `capacity` > 0: the largest hex-20 thermal and elasticity meshes a matrix-free idrs!(8) solve completes on, stepping n up by `capacity` from the
size whose shape-derived byte count (mesh, adjacency, idrs!(8) vectors, scratch) reaches a quarter of the free memory; it stops at the first
allocation that fails and never repeats a failing step.
usage: mesh_operator_time.py [n_hex20 = 96] [n_tet10 = 64] [reps = 5] [legs = u20_1,u20_3,tet10_1,tet10_3] [capacity = 0]
The JSON lines go to stdout and, together, to profiles/mesh_operator_time.json."""
import ctypes as C
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
import metafem_jl_amd as mf  # noqa: E402
from metafem_jl_amd import _lib, generic as G, physics  # noqa: E402

n20 = int(sys.argv[1]) if len(sys.argv) > 1 else 96
n10 = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
legs = [s for s in (sys.argv[4].split(",") if len(sys.argv) > 4 else ["u20_1", "u20_3", "tet10_1", "tet10_3"]) if s]
capacity = int(sys.argv[5]) if len(sys.argv) > 5 else 0
B = L.Bench(bench.parse_args([]))


def domain(ctx, shape, n, fields, matrix_free):
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
    gd = G.GenericDomain(ctx, space, msh.coords, msh.cp_ids, fields, wf, bnd, matrix_free=matrix_free, fused_residual=True)
    if fields == 1:
        gd.controlpoints["s"] = torch.full((msh.ncp,), L.SRC, dtype=torch.float64, device=B.dev)
    else:
        for v in (2, 4, 6):
            gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 1.0 if v == 2 else 0.0, dtype=torch.float64, device=B.dev)
    gd.update_Time()
    return gd


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def solver_spmv_ms(gd, b, iters=20):
    """ms per product inside a fixed idrs!(8) solve: the per-launch SpMV timing of the library (the layout SpMV on the assembled path)"""
    h = gd.ctx._h
    _lib.check(_lib.lib.mfem_prof_spmv_enable(h, 1))
    try:
        mf.iterative_Solve(gd.A, gd.K_total, b, 1e-300, Sv_func=mf.idrs_, s=8, maxiter=iters, max_pass=1, fixed_iterations=True)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(_lib.lib.mfem_prof_spmv_read(h, C.byref(ms), C.byref(cnt), 1))
    finally:
        _lib.lib.mfem_prof_spmv_enable(h, 0)
    return ms.value / max(cnt.value, 1)


def device_bytes(ctx):
    torch.cuda.synchronize()
    return int(torch.cuda.memory_allocated()) + int(_lib.lib.mfem_debug_ws_bytes(ctx._h))


def run_leg(leg):
    tag, fields = leg.rsplit("_", 1)
    fields = int(fields)
    shape, n = ("CUBE", n20) if tag == "u20" else ("SIMPLEX", n10)
    out = {"leg": leg, "n": n, "fields": fields, "reps": reps}
    torch.cuda.synchronize()
    base = int(torch.cuda.memory_allocated())
    cm = mf.Context(torch.cuda.current_device())
    md = domain(cm, shape, n, fields, True)
    out["matrix_free"], out["matrix_free_reason"] = bool(md.matrix_free), md.matrix_free_reason
    md.K_linear_func()
    md.K_nonlinear_func()
    after_md = int(torch.cuda.memory_allocated())
    ca = mf.Context(torch.cuda.current_device())
    gd = domain(ca, shape, n, fields, False)
    out["nel"], out["ncp"], out["rows"], out["nnz"] = int(gd.nel), int(gd.ncp), int(gd.A.n), int(gd.A.nnz)
    nrows = gd.A.n
    x = torch.tensor(np.random.default_rng(1).uniform(-1.0, 1.0, nrows), device=B.dev)
    b = torch.tensor(np.random.default_rng(2).uniform(-1.0, 1.0, nrows), device=B.dev)
    y = torch.empty_like(x)
    # warm-up: every path once
    gd.K_linear_func()
    gd.K_nonlinear_func()
    md.A.mul_(y, x)
    md.A.diagonal()
    _lib.check(_lib.lib.mfem_spmv_solver_layout(ca._h, gd.A._h, gd.K_linear.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0))
    solver_spmv_ms(gd, b, 4)
    solver_spmv_ms(md, b, 4)
    y_csr = mf.mul_(torch.empty_like(x), gd.A, gd.K_linear, x)
    out["product_max_rel_diff"] = float((md.A.mul_(y, x) - y_csr).abs().max() / y_csr.abs().max())  # against the CSR kernel on the assembled K
    del y_csr
    T = {k: [] for k in ("op", "op_in_solve", "layout", "residual", "diag", "assembly", "layout_call")}
    for _ in range(reps):  # the two paths alternated
        T["op"].append(timed(lambda: md.A.mul_(y, x)))
        T["layout"].append(solver_spmv_ms(gd, b))
        T["op_in_solve"].append(solver_spmv_ms(md, b))
        T["residual"].append(timed(md.K_nonlinear_func))
        T["diag"].append(timed(md.A.diagonal))
        T["assembly"].append(timed(gd.K_linear_func))
        T["layout_call"].append(timed(lambda: _lib.check(_lib.lib.mfem_spmv_solver_layout(ca._h, gd.A._h, gd.K_linear.data_ptr(), x.data_ptr(),
                                                                                           y.data_ptr(), 1.0, 0.0))))
    m = {k: float(np.median(v)) for k, v in T.items()}
    out.update(operator_product_ms=round(m["op"], 3), operator_product_in_solve_ms=round(m["op_in_solve"], 3), layout_spmv_ms=round(m["layout"], 3),
               fused_residual_ms=round(m["residual"], 3), operator_over_layout=round(m["op"] / m["layout"], 2),
               operator_over_residual=round(m["op"] / m["residual"], 3), within_1p1_of_residual=bool(m["op"] <= 1.1 * m["residual"]),
               diagonal_ms=round(m["diag"], 3), assembly_ms=round(m["assembly"], 3), layout_fill_ms=round(max(m["layout_call"] - m["layout"], 0.0), 3))
    # the 200-step solve both ways, residual recomputed
    for name, d in (("operator", md), ("assembled", gd)):
        sol, st = mf.iterative_Solve(d.A, d.K_total, b, 1e-300, Sv_func=mf.idrs_, s=8, maxiter=200, max_pass=1, fixed_iterations=True)
        r = b - mf.mul_(torch.empty_like(b), d.A, d.K_total, sol)
        out[f"{name}_solve_ms"] = round(float(st.solve_ms), 2)
        out[f"{name}_solve_residual"] = float(r.norm()) / float(np.sqrt(nrows))
        out[f"{name}_spmv_count"] = int(st.spmv_count)
        if d is md:  # ... and the operator's solution once more on the assembled K
            r = b - mf.mul_(torch.empty_like(b), gd.A, gd.K_total, sol)
            out["operator_solve_residual_on_assembled_K"] = float(r.norm()) / float(np.sqrt(nrows))
    torch.cuda.synchronize()
    total = int(torch.cuda.memory_allocated())
    out["operator_bytes"] = after_md - base + int(_lib.lib.mfem_debug_ws_bytes(cm._h))
    out["assembled_bytes"] = total - after_md + int(_lib.lib.mfem_debug_ws_bytes(ca._h))
    out["bytes_ratio"] = round(out["assembled_bytes"] / max(out["operator_bytes"], 1), 2)
    md.A.close()
    del md, gd, x, b, y, sol, r
    gc.collect()
    cm.close()
    ca.close()
    torch.cuda.empty_cache()
    return out


def shape_bytes(n, fields):
    """hex-20 n^3, matrix-free idrs!(8): coordinates, connectivity (twice: host upload and adjacency), the x / dx / x_star / residue vectors, the solve's
    4 + 28 vectors, the scratch -- derived from the shapes alone"""
    nel, ncp = n ** 3, 4 * n ** 3 + 6 * n ** 2 + 3 * n + 1  # (vertices + one node per edge of the brick)
    rows = fields * ncp
    return 24 * ncp + 20 * nel * (4 + 4) + 8 * (ncp + 1) + 8 * rows * (4 + 32) + 8 * nel * 20 * fields


def run_capacity(fields, step):
    free, _ = torch.cuda.mem_get_info()
    n = 32
    while shape_bytes(n + step, fields) < free // 4:
        n += step
    out = {"capacity_fields": fields, "step": step, "first_n": n, "largest_n": None, "stopped_by": None}
    while True:
        ctx = mf.Context(torch.cuda.current_device())
        try:
            md = domain(ctx, "CUBE", n, fields, True)
            md.K_linear_func()
            b = torch.ones(md.A.n, dtype=torch.float64, device=B.dev)
            _, st = mf.iterative_Solve(md.A, None, b, 1e-300, Sv_func=mf.idrs_, s=8, maxiter=20, max_pass=1, fixed_iterations=True)
            out["largest_n"], out["largest_rows"], out["largest_bytes"] = n, int(md.A.n), device_bytes(ctx)
            md.A.close()
            del md, b
        except (torch.OutOfMemoryError, mf.MetaFEMError, MemoryError) as e:  # the first allocation that fails ends the search
            out["stopped_by"] = f"n = {n}: {type(e).__name__}"
            break
        finally:
            gc.collect()
            ctx.close()
            torch.cuda.empty_cache()
        n += step
    return out


results = []
for leg in legs:
    results.append(run_leg(leg))
    print(json.dumps(results[-1]), flush=True)
if capacity > 0:
    for fields in (1, 3):
        results.append(run_capacity(fields, capacity))
        print(json.dumps(results[-1]), flush=True)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "mesh_operator_time.json"), "w") as f:
    json.dump(results, f, indent=1)
