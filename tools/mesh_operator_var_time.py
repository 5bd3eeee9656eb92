"""The matrix-free mesh operator with VARIABLE terms (GenericDomain(matrix_free="any"): mfem_mesh_operator_set_variable_terms) on the finite-strain
Neo-Hookean domain form (9 residual + 81 nonlinear gradient terms, 3 fields, a penalty wall and a traction face) on bench.py's unstructured hex-20 mesh
of n^3 elements (n = 48: the size of tools/mesh_ops_time.py), against the assembled path.  One domain alive at a time, a fresh context each; warm-up,
then the median of `reps` repetitions:
  variable_product_ms         the operator product with the 81 coefficient arrays (event-timed mul_), and inside a fixed 20-step idrs!(8) solve
  constant_product_ms         the constant-coefficient elasticity operator (21 terms, matrix_free=True) on the same mesh
  coefficient_fill_ms         81 * 27 * 8 * nel bytes / the fill rate of this box (tools/write_bw_probe.py's fill_, measured here on 1 GiB)
  variable_over_model         variable product / (constant product + coefficient bytes / fill rate)
  variable_48_terms_ms / constant_same_48_entries_ms   the ablation with the coefficient loads skipped, at the 48 terms a constant part may hold: the
                              first 48 of the 81 terms as variable terms, and a constant operator with the same 48 entries (coefficients from the
                              kernel arguments; phases 1-3, 5, 6 and the gather identical): the difference is the coefficient loads
  layout_spmv_ms              the Krylov loop's layout SpMV on the assembled K_total (per-launch timing of a 20-step idrs!(8) solve)
  K_nonlinear_ms              K_nonlinear_func both ways (the assembled one on the default domain)
  newton_iteration_ms         K_nonlinear_func + a 50-step idrs!(8) + Pr_Jacobi! solve both ways (wall clock around both, synchronised)
  bytes                       torch.cuda.memory_allocated + mfem_debug_ws_bytes after that iteration, both ways
With `parent` (a checkout of the parent commit with its library built) the four legs of tools/mesh_operator_time.py -- constant terms only -- are run
on both trees in this session, sizes n_hex20 / n_tet10, and both sets are recorded with their ratios: they must agree within 10 %.
usage: mesh_operator_var_time.py [n = 48] [reps = 5] [parent = ""] [n_hex20 = 96] [n_tet10 = 64]
The JSON lines go to stdout and, together, to profiles/mesh_operator_var_time.json."""
import ctypes as C
import gc
import json
import os
import subprocess
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
from oracle import hyperelastic as he  # noqa: E402  (the symbolic layer's output: the weak forms only)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3] else ""
n20 = int(sys.argv[4]) if len(sys.argv) > 4 else 96
n10 = int(sys.argv[5]) if len(sys.argv) > 5 else 64
B = L.Bench(bench.parse_args([]))
MU, LAM = 1.0, 1.5


def conv(wf):
    return G.WeakForm(inner_vars=list(wf.inner_vars), cp_ext_vars=list(wf.cp_ext_vars), normals=list(wf.normals),
                      residues=[G.ResTerm(r.dual_pos, r.dual_s, r.fn) for r in wf.residues],
                      linear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.linear_gradients],
                      nonlinear_gradients=[G.GradTerm(g.dual_pos, g.dual_s, g.base_pos, g.base_s, g.fn, g.td_order) for g in wf.nonlinear_gradients])


def domain(ctx, form, **kw):
    space, msh, fac = B.unstructured_mesh(n)
    c = fac.centroid
    wall, top = fac.select(np.abs(c[:, 0]) < 1e-9), fac.select(np.abs(c[:, 1] - 1.0) < 1e-9)
    bnd = [(wall.element_ID, wall.element_eindex, physics.penalty([0, 1, 2], 37.0)), (top.element_ID, top.element_eindex, physics.traction(3, "sl", rows=[1]))]
    wf = conv(he.domain_weakform(dict(mu=MU, lam=LAM), "neo_hookean")) if form == "neo_hookean" else physics.elasticity_domain(3, LAM, MU)
    gd = G.GenericDomain(ctx, space, msh.coords, msh.cp_ids, 3, wf, bnd, **kw)
    for v in (2, 4, 6):
        gd.controlpoints[f"sl{v}"] = torch.full((msh.ncp,), 0.05 if v == 2 else 0.0, dtype=torch.float64, device=B.dev)
    x = np.concatenate([0.05 * np.sin(2.3 * msh.coords[:, (i + 1) % 3] + 1.1 * msh.coords[:, (i + 2) % 3] + 0.4 * i) for i in range(3)])
    gd.x_star.copy_(torch.tensor(x))  # (a smooth displacement: det F well above 0)
    gd.update_Time()
    gd.K_linear_func()
    gd.K_nonlinear_func()
    return gd


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def median(fn):
    fn()
    return float(np.median([timed(fn) for _ in range(reps)]))


def solver_spmv_ms(gd, b, iters=20):
    h = gd.ctx._h
    _lib.check(_lib.lib.mfem_prof_spmv_enable(h, 1))
    try:
        mf.iterative_Solve(gd.A, gd.K_total, b, 1e-300, Sv_func=mf.idrs_, s=8, maxiter=iters, max_pass=1, fixed_iterations=True)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(_lib.lib.mfem_prof_spmv_read(h, C.byref(ms), C.byref(cnt), 1))
    finally:
        _lib.lib.mfem_prof_spmv_enable(h, 0)
    return ms.value / max(cnt.value, 1)


def newton_iteration_ms(gd, b):
    def one():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gd.K_nonlinear_func()
        mf.iterative_Solve(gd.A, gd.K_total, b, 1e-300, Sv_func=mf.idrs_, s=8, maxiter=50, max_pass=1, fixed_iterations=True)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    one()
    return float(np.median([one() for _ in range(reps)]))


def device_bytes(ctx, base):
    torch.cuda.synchronize()
    return int(torch.cuda.memory_allocated()) - base + int(_lib.lib.mfem_debug_ws_bytes(ctx._h))


def fill_rate():
    """bytes / ms of a device fill (tools/write_bw_probe.py's fill_, on 1 GiB)"""
    x = torch.empty(1 << 27, dtype=torch.float64, device=B.dev)
    ms = median(lambda: x.fill_(1.5))
    return x.numel() * 8 / ms


def finish(ctx, *objs):
    for o in objs:
        if hasattr(o, "A") and hasattr(o.A, "close"):
            o.A.close()
    gc.collect()
    ctx.close()
    torch.cuda.empty_cache()


out = {"form": "neo_hookean", "n": n, "reps": reps}
torch.cuda.synchronize()
base = int(torch.cuda.memory_allocated())
ctx = mf.Context(torch.cuda.current_device())
md = domain(ctx, "neo_hookean", matrix_free="any")
out["matrix_free"], out["matrix_free_reason"], out["nel"], out["ncp"], out["rows"] = bool(md.matrix_free), md.matrix_free_reason, int(md.nel), int(md.ncp), int(md.A.n)
rng = np.random.default_rng(1)
x = torch.tensor(rng.uniform(-1.0, 1.0, md.A.n), device=B.dev)
b = torch.tensor(rng.uniform(-1.0, 1.0, md.A.n), device=B.dev)
y = torch.empty_like(x)
y_var = md.A.mul_(torch.empty_like(x), x).clone()
out["variable_product_ms"] = round(median(lambda: md.A.mul_(y, x)), 3)
solver_spmv_ms(md, b, 4)
out["variable_product_in_solve_ms"] = round(float(np.median([solver_spmv_ms(md, b) for _ in range(reps)])), 3)
out["variable_diagonal_ms"] = round(median(md.A.diagonal), 3)
out["K_nonlinear_operator_ms"] = round(median(md.K_nonlinear_func), 3)
out["newton_iteration_operator_ms"] = round(newton_iteration_ms(md, b), 2)
out["operator_bytes"] = device_bytes(ctx, base)
out["table_bytes"] = md.table_bytes
full = md._var_buf[0]
coefficient_bytes = full.numel() * 8
out["coefficient_bytes"], out["coefficient_bytes_per_element"] = coefficient_bytes, coefficient_bytes // md.nel
rate = fill_rate()
out["fill_GBps"] = round(rate / 1e6, 1)
out["coefficient_fill_ms"] = round(coefficient_bytes / rate, 3)
t48 = [(t.dual_s, t.base_s, t.dual_pos * 3 + t.base_pos) for t in md._op_parts[0].variable][:48]
assert md.A.set_variable_terms(0, t48, full[:48]) == 0
out["variable_48_terms_ms"] = round(median(lambda: md.A.mul_(y, x)), 3)
finish(ctx, md)
del md, full

torch.cuda.synchronize()
base_c = int(torch.cuda.memory_allocated())
cc = mf.Context(torch.cuda.current_device())
cd = domain(cc, "elasticity", matrix_free=True)
assert cd.matrix_free
out["constant_product_ms"] = round(median(lambda: cd.A.mul_(y, x)), 3)
out["constant_product_in_solve_ms"] = round(float(np.median([solver_spmv_ms(cd, b) for _ in range(reps)])), 3)
assert cd.A.set_terms(0, [(a, c, blk, 1.0) for a, c, blk in t48]) == 0
out["constant_same_48_entries_ms"] = round(median(lambda: cd.A.mul_(y, x)), 3)
finish(cc, cd)
del cd
model = out["constant_product_ms"] + out["coefficient_fill_ms"]
out["model_ms"] = round(model, 3)
out["variable_over_model"] = round(out["variable_product_ms"] / model, 3)
out["within_1p25_of_model"] = bool(out["variable_over_model"] <= 1.25)

torch.cuda.synchronize()
base = int(torch.cuda.memory_allocated())
ca = mf.Context(torch.cuda.current_device())
gd = domain(ca, "neo_hookean")
out["nnz"] = int(gd.A.nnz)
y_csr = mf.mul_(torch.empty_like(x), gd.A, gd.K_total, x)
out["product_max_rel_diff"] = float((y_var - y_csr).abs().max() / y_csr.abs().max())
solver_spmv_ms(gd, b, 4)
out["layout_spmv_ms"] = round(float(np.median([solver_spmv_ms(gd, b) for _ in range(reps)])), 3)
out["K_nonlinear_assembled_ms"] = round(median(gd.K_nonlinear_func), 3)
out["newton_iteration_assembled_ms"] = round(newton_iteration_ms(gd, b), 2)
out["assembled_bytes"] = device_bytes(ca, base)
out["assembled_table_bytes"] = gd.table_bytes
out["bytes_ratio"] = round(out["assembled_bytes"] / max(out["operator_bytes"], 1), 2)
out["variable_over_layout"] = round(out["variable_product_ms"] / out["layout_spmv_ms"], 2)
finish(ca)
del gd
results = [out]
print(json.dumps(out), flush=True)


def save():
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_operator_var_time.json"), "w") as f:
        json.dump(results, f, indent=1)


save()

if parent:  # the constant-term legs on the parent commit and on this one, in this session on this box
    keys = ("operator_product_ms", "operator_product_in_solve_ms", "diagonal_ms", "operator_solve_ms")
    runs = {}
    for tag, tree in (("parent", parent), ("this", ROOT)):
        p = subprocess.run([sys.executable, os.path.join(tree, "tools", "mesh_operator_time.py"), str(n20), str(n10), str(reps)], cwd=tree,
                           capture_output=True, text=True)
        if p.returncode:
            raise SystemExit(f"{tag}: mesh_operator_time.py failed\n{p.stderr[-2000:]}")
        runs[tag] = {r["leg"]: {k: r[k] for k in keys} for r in map(json.loads, (ln for ln in p.stdout.splitlines() if ln.startswith("{"))) if "leg" in r}
    cmp = {"constant_legs": runs, "n_hex20": n20, "n_tet10": n10}
    cmp["this_over_parent"] = {leg: {k: round(v / runs["parent"][leg][k], 3) for k, v in d.items()} for leg, d in runs["this"].items()}
    cmp["within_10_percent"] = all(abs(v - 1.0) <= 0.10 for d in cmp["this_over_parent"].values() for v in d.values())
    results.append(cmp)
    print(json.dumps(cmp), flush=True)
save()
