"""The matrix-free hex-27 brick operator (Brick.thermal_operator_hex27: Hex27BrickOperator, mfem_solve_operator) against the fused residual and the
assembled path on the C4 brick: hex-27, n^3 elements (128), itg 5, Robin on all faces.  Three legs, each in a child process of its own with a time
limit: `affine` (the brick as made), `distorted` (every element moved by a smooth map), `distorted_fixed` (the same with x = 0 a Nitsche face).  Warm-up,
then the median and the spread (min, max) of `reps` repetitions with the paths alternated:
  product    the operator product (event-timed mul_, beta = 0, no scaling: no partial sums, so not folded) against mfem_brick_residual_thermal with
             s = NULL on the same brick.  Condition: operator <= 1.1 R x residual, R = elements integrated / elements of the brick
             (csrc/brick_operator_hex27_decide.h; computed here from the header's constants the way b27_volume / b27_item do, and printed by
             tools/host_check_brick_operator_hex27.cpp), R <= 1.3.
  in a solve the product inside cg! (mfem_prof_spmv_*: with dotw, folded onto the capped grid) -- the ablation of dot and fold -- and, on the affine leg,
             the layout SpMV of the assembled path
  set-up     the operator's diagonal; on the affine leg assembly plus the layout fill
  solve      200 fixed cg! and idrs!(8) steps matrix-free (and assembled on the affine leg): solve_ms, final_res
  bytes      torch.cuda.memory_allocated + mfem_debug_ws_bytes, both ways (affine leg)
usage: brick_operator_hex27_time.py [n = 128] [reps = 7] [limit_s = 500] [legs = affine,distorted,distorted_fixed]
The JSON lines go to stdout and, together, to profiles/brick_operator_hex27_time.json."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_operator_hex27_time.json")
K_COND, H, TENV, SRC, H_PEN, TW = 0.6, 25.0, 293.15, 1600.0, 1000.0, 1173.15


def redundancy(n):
    """R of an n^3-element brick, from the constants of brick_operator_hex27_decide.h"""
    text = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "brick_operator_hex27_decide.h")).read()
    c = {k: int(re.search(r"#define " + k + r"\s+(\d+)", text).group(1)) for k in ("B27_TE", "B27_LMAX", "B27_LMIN", "B27_FILL")}
    nt = -(-n // c["B27_TE"])
    L = c["B27_LMAX"]
    while L > c["B27_LMIN"] and nt * nt * -(-n // L) < c["B27_FILL"]:
        L //= 2

    def integrated(T, count):  # elements a direction's pieces integrate: T per piece, + the low-side halo but for the first, clipped at the end
        return sum(min(T * (t + 1), n) - max(T * t - 1, 0) for t in range(count))

    return integrated(c["B27_TE"], nt) ** 2 * integrated(L, -(-n // L)) / n ** 3, L


def child(n, reps, leg):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib

    dev = f"cuda:{torch.cuda.current_device()}"
    R, L = redundancy(n)
    out = {"leg": leg, "n": n, "itg": 5, "reps": reps, "box": torch.cuda.get_device_name(), "R": round(R, 4), "segment_planes": L}

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def solver_spmv_ms(ctx, A, vals, b, iters=20):
        _lib.check(_lib.lib.mfem_prof_spmv_enable(ctx._h, 1))
        try:
            mf.iterative_Solve(A, vals, b, 1e-300, Sv_func=mf.cg_, maxiter=iters, max_pass=1, fixed_iterations=True)
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(_lib.lib.mfem_prof_spmv_read(ctx._h, C.byref(ms), C.byref(cnt), 1))
        finally:
            _lib.lib.mfem_prof_spmv_enable(ctx._h, 0)
        return ms.value / max(cnt.value, 1)

    def stats(v):
        return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}

    x0 = mf.FACE_BITS["x0"]
    robin, kw = (0x3F & ~x0, dict(fixed_faces=x0, h_penalty=H_PEN, Tw=TW)) if leg == "distorted_fixed" else (0x3F, {})
    torch.cuda.synchronize()
    base = int(torch.cuda.memory_allocated())
    cm = mf.Context(torch.cuda.current_device())
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 2, 5, ctx=cm)
    if leg != "affine":  # a smooth map that leaves no element an affine image of the reference cell
        c = [brick.coords_view(d).clone() for d in range(3)]
        brick.coords_view(0).add_(0.03 * torch.sin(3 * c[1]) * torch.cos(2 * c[2]))
        brick.coords_view(1).add_(0.02 * torch.sin(2 * c[0] + c[2]))
        brick.coords_view(2).add_(0.025 * c[0] * c[1])
        del c
    op = brick.thermal_operator_hex27(K_COND, H, TENV, robin, **kw)
    rows = op.n
    out["rows"] = rows
    g = torch.Generator(dev)
    x = torch.empty(rows, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g.manual_seed(1))
    b = torch.empty_like(x).uniform_(-1.0, 1.0, generator=g.manual_seed(2))
    y = torch.empty_like(x)
    residual = lambda: brick.residual_thermal(x, K_COND, H, TENV, robin, out=y, **kw)
    product = lambda: op.mul_(y, x)
    # the residual with s = NULL, Tenv = 0, Tw = 0 is the product (to the different summation orders): the two kernels are compared on the same numbers
    ref = brick.residual_thermal(x, K_COND, H, 0.0, robin, fixed_faces=kw.get("fixed_faces", 0), h_penalty=kw.get("h_penalty", 0.0), Tw=0.0).clone()
    out["product_vs_residual_max_rel_diff"] = float((op.mul_(y, x) - ref).abs().max() / ref.abs().max())
    del ref
    for _ in range(3):  # warm
        product()
        residual()
    op.diagonal()
    solver_spmv_ms(cm, op, None, b, 4)
    T = {k: [] for k in ("op", "residual", "op_in_solve", "diag")}
    for _ in range(reps):  # alternated
        T["op"].append(timed(product))
        T["residual"].append(timed(residual))
        T["op_in_solve"].append(solver_spmv_ms(cm, op, None, b))
        T["diag"].append(timed(op.diagonal))
    m = {k: float(np.median(v)) for k, v in T.items()}
    out.update(operator_product_ms=stats(T["op"]), residual_ms=stats(T["residual"]), operator_product_in_solve_ms=stats(T["op_in_solve"]),
               diagonal_ms=stats(T["diag"]), operator_over_residual=round(m["op"] / m["residual"], 3), bound_1p1_R=round(1.1 * R, 3),
               condition_met=bool(m["op"] <= 1.1 * R * m["residual"] and R <= 1.3),
               ablation={"unfolded_over_residual": round(m["op"] / m["residual"], 3), "per_integrated_element_over_residual": round(m["op"] / m["residual"] / R, 3),
                         "in_solve_with_dot_and_fold_over_residual": round(m["op_in_solve"] / m["residual"], 3),
                         "dot_and_fold_cost_over_residual": round((m["op_in_solve"] - m["op"]) / m["residual"], 3)})
    for sv, name, s in ((mf.cg_, "cg", 0), (mf.idrs_, "idrs8", 8)):
        _, st = mf.iterative_Solve(op, None, b, 1e-300, Sv_func=sv, s=s, maxiter=200, max_pass=1, fixed_iterations=True)
        out[f"operator_{name}200_solve_ms"], out[f"operator_{name}200_final_res"] = round(float(st.solve_ms), 2), float(st.final_res)
    torch.cuda.synchronize()
    out["operator_bytes"] = int(torch.cuda.memory_allocated()) - base - 3 * 8 * rows + int(_lib.lib.mfem_debug_ws_bytes(cm._h))  # (without this tool's x, b, y)
    out["largest_converged_cube"] = "not tried"
    if leg != "affine":
        return out
    # the assembled path of the same brick (the C4 leg of bench.py)
    after_op = int(torch.cuda.memory_allocated())
    ca = mf.Context(torch.cuda.current_device())
    brick_a = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 2, 5, ctx=ca)
    A = brick_a.pattern(1)
    K = brick_a.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    out["nnz"] = int(A.nnz)
    layout_call = lambda: _lib.check(_lib.lib.mfem_spmv_solver_layout(ca._h, A._h, K.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0))
    layout_call()
    solver_spmv_ms(ca, A, K, b, 4)
    y_csr = mf.mul_(torch.empty_like(x), A, K, x)
    out["product_vs_csr_max_rel_diff"] = float((op.mul_(y, x) - y_csr).abs().max() / y_csr.abs().max())
    del y_csr
    T = {k: [] for k in ("layout", "assembly", "layout_call", "op")}
    for _ in range(reps):
        T["op"].append(timed(product))
        T["layout"].append(solver_spmv_ms(ca, A, K, b))
        T["assembly"].append(timed(lambda: brick_a.assemble_thermal(A, K_COND, H, TENV, 0x3F, out=K)))
        T["layout_call"].append(timed(layout_call))
    m2 = {k: float(np.median(v)) for k, v in T.items()}
    out.update(layout_spmv_ms=stats(T["layout"]), assembly_ms=stats(T["assembly"]), layout_fill_ms=round(max(m2["layout_call"] - m2["layout"], 0.0), 3),
               operator_over_layout=round(m2["op"] / m2["layout"], 2))
    for sv, name, s in ((mf.cg_, "cg", 0), (mf.idrs_, "idrs8", 8)):
        _, st = mf.iterative_Solve(A, K, b, 1e-300, Sv_func=sv, s=s, maxiter=200, max_pass=1, fixed_iterations=True)
        out[f"assembled_{name}200_solve_ms"], out[f"assembled_{name}200_final_res"] = round(float(st.solve_ms), 2), float(st.final_res)
    torch.cuda.synchronize()
    out["assembled_bytes"] = int(torch.cuda.memory_allocated()) - after_op + int(_lib.lib.mfem_debug_ws_bytes(ca._h))
    out["bytes_ratio"] = round(out["assembled_bytes"] / max(out["operator_bytes"], 1), 2)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    legs = (sys.argv[4] if len(sys.argv) > 4 else "affine,distorted,distorted_fixed").split(",")
    results = []
    if os.path.exists(OUT):
        results = [r for r in json.load(open(OUT)) if not (r.get("n") == n and r.get("leg") in legs)]
    for leg in legs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps), leg], stdout=subprocess.PIPE, text=True, timeout=limit)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            r = json.loads(lines[-1]) if p.returncode == 0 and lines else {"leg": leg, "n": n, "failed": f"exit {p.returncode}"}
        except subprocess.TimeoutExpired:
            r = {"leg": leg, "n": n, "failed": f"time limit of {limit} s"}
        results.append(r)
        print(json.dumps(r), flush=True)
        if "failed" in r:  # (a child that faulted or hung: nothing more is started on the device)
            break
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    return 1 if any("failed" in r for r in results) else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        try:
            print(json.dumps(child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])), flush=True)
        except Exception as e:  # an allocation that fails is a result
            print(json.dumps({"leg": sys.argv[4], "n": int(sys.argv[2]), "failed": f"{type(e).__name__}: {str(e)[:300]}"}), flush=True)
        sys.exit(0)
    sys.exit(main())
