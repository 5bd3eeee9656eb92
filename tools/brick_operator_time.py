"""The matrix-free hex-8 brick operator (Brick.thermal_operator: BrickOperator, mfem_solve_operator) against the assembled path on the thermal brick.
Each size runs in a child process of its own with a time limit; the tool stops at the first failure (a size that fails to allocate is recorded and
nothing larger is tried).
  n <= 512 (Robin on all faces; at 256 also the Nitsche leg: x = 0 fixed, convection elsewhere), both paths alive, warm-up, then the median of `reps`
  repetitions with the two paths alternated:
    product    the operator product (event-timed mul_, beta = 0, no scaling: no partial sums, so not folded), the product inside a solve (the
               per-launch timing of a 20-step fixed cg! solve, mfem_prof_spmv_*: folded onto the capped grid; `ablation` sets the two side by side), mfem_brick_residual_thermal with s = NULL on the same brick, the layout SpMV of the assembled path
               (the same per-launch timing); condition: operator <= 1.1 x residual
    set-up     the operator's diagonal against assembly plus the layout fill (mfem_spmv_solver_layout minus one layout SpMV)
    solve      a 200-step cg! and a 200-step idrs!(8) solve both ways (stats.solve_ms, stats.final_res)
    bytes      torch.cuda.memory_allocated + mfem_debug_ws_bytes, both ways
  n > 512, matrix-free only: 200 fixed cg! iterations, then a converged cg! + Pr_Jacobi! solve of the source problem to 1e-6 |b| (final_res, iterations, device bytes).
usage: brick_operator_time.py [sizes = 256,512,768,1024] [reps = 5] [limit_s = 900]
The JSON lines go to stdout and, together, to profiles/brick_operator_time.json (results of sizes not asked for in this call are kept)."""
import ctypes as C
import gc
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_operator_time.json")
K_COND, H, TENV, SRC, H_PEN, TW = 0.6, 25.0, 293.15, 1600.0, 1000.0, 1173.15


def child(n, reps):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib

    def heartbeat():  # (a long solve is one library call: a line a minute tells whoever watches that the child is alive)
        import time
        t0 = time.time()
        while True:
            time.sleep(60)
            print(f"  n = {n}: running, {time.time() - t0:.0f} s", file=sys.stderr, flush=True)

    import threading
    threading.Thread(target=heartbeat, daemon=True).start()
    dev = f"cuda:{torch.cuda.current_device()}"
    out = {"n": n, "reps": reps, "box": torch.cuda.get_device_name()}

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

    def device_bytes(ctx, base):
        torch.cuda.synchronize()
        return int(torch.cuda.memory_allocated()) - base + int(_lib.lib.mfem_debug_ws_bytes(ctx._h))

    def ablation(o):
        """where the product's time goes against the residual's: the kernel itself (a product that leaves no partial sums launches the residual's
        grid, a workgroup per work item) and the fold (inside cg! the items are folded onto at most 3584 workgroups)"""
        items = (-(-(n + 1) // 15)) ** 2 * -(-(n + 1) // 32)  # 15 x 15 tiles, 32-plane segments (n >= 256: the grid fills the chip)
        rounds = -(-items // 3584)
        r = o["residual_ms"]
        o["ablation"] = {"work_items": items, "folded_workgroups": -(-items // rounds), "items_per_folded_workgroup": rounds,
                         "unfolded_over_residual": round(o["operator_product_ms"] / r, 3),
                         "folded_in_solve_over_residual": round(o["operator_product_in_solve_ms"] / r, 3),
                         "fold_costs": round((o["operator_product_in_solve_ms"] - o["operator_product_ms"]) / r, 3),
                         "in_solve_within_1p1_of_residual": bool(o["operator_product_in_solve_ms"] <= 1.1 * r)}

    torch.cuda.synchronize()
    base = int(torch.cuda.memory_allocated())
    cm = mf.Context(torch.cuda.current_device())
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 1, 3, ctx=cm)
    op = brick.thermal_operator(K_COND, H, TENV, 0x3F)
    rows = op.n
    out["rows"] = rows
    x = torch.empty(rows, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(1))
    y = torch.empty_like(x)
    if n > 512:  # matrix-free only
        zero = torch.zeros_like(x)
        s = torch.full_like(x, SRC)
        b = brick.residual_thermal(zero, K_COND, H, TENV, 0x3F, s=s)
        del zero, s
        op.mul_(y, x)
        T = [timed(lambda: op.mul_(y, x)) for _ in range(reps)]
        out["operator_product_ms"] = round(float(np.median(T)), 3)
        out["residual_ms"] = round(float(np.median([timed(lambda: brick.residual_thermal(x, K_COND, H, TENV, 0x3F, out=y)) for _ in range(reps)])), 3)
        del y
        solver_spmv_ms(cm, op, None, b, 4)
        out["operator_product_in_solve_ms"] = round(float(np.median([solver_spmv_ms(cm, op, None, b) for _ in range(reps)])), 3)
        ablation(out)
        _, st = mf.iterative_Solve(op, None, b, 1e-300, Sv_func=mf.cg_, maxiter=200, max_pass=1, fixed_iterations=True)
        out["cg200_solve_ms"], out["cg200_final_res"] = round(float(st.solve_ms), 2), float(st.final_res)
        tol = 1e-6 * mf.normalized_norm(b, cm)
        _, st = mf.iterative_Solve(op, None, b, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=6000, max_pass=2)
        out.update(converged=int(st.converged), converge_tol=tol, final_res=float(st.final_res), iterations=int(st.iterations), passes=int(st.passes),
                   solve_ms=round(float(st.solve_ms), 1), operator_bytes=device_bytes(cm, base))
        return out
    ca = mf.Context(torch.cuda.current_device())
    brick_a = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 1, 3, ctx=ca)
    after_op = int(torch.cuda.memory_allocated())
    A = brick_a.pattern(1)
    K = brick_a.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    out["nnz"] = int(A.nnz)
    b = torch.empty_like(x).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(2))
    layout_call = lambda: _lib.check(_lib.lib.mfem_spmv_solver_layout(ca._h, A._h, K.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0))
    residual = lambda: brick.residual_thermal(x, K_COND, H, TENV, 0x3F, out=y)
    # warm-up: every path once
    op.mul_(y, x)
    op.diagonal()
    residual()
    layout_call()
    solver_spmv_ms(ca, A, K, b, 4)
    solver_spmv_ms(cm, op, None, b, 4)
    y_csr = mf.mul_(torch.empty_like(x), A, K, x)
    out["product_max_rel_diff"] = float((op.mul_(y, x) - y_csr).abs().max() / y_csr.abs().max())
    del y_csr
    T = {k: [] for k in ("op", "op_in_solve", "layout", "residual", "diag", "assembly", "layout_call")}
    for _ in range(reps):  # the two paths alternated
        T["op"].append(timed(lambda: op.mul_(y, x)))
        T["layout"].append(solver_spmv_ms(ca, A, K, b))
        T["op_in_solve"].append(solver_spmv_ms(cm, op, None, b))
        T["residual"].append(timed(residual))
        T["diag"].append(timed(op.diagonal))
        T["assembly"].append(timed(lambda: brick_a.assemble_thermal(A, K_COND, H, TENV, 0x3F, out=K)))
        T["layout_call"].append(timed(layout_call))
    m = {k: float(np.median(v)) for k, v in T.items()}
    out.update(operator_product_ms=round(m["op"], 3), operator_product_in_solve_ms=round(m["op_in_solve"], 3), layout_spmv_ms=round(m["layout"], 3),
               residual_ms=round(m["residual"], 3), operator_over_layout=round(m["op"] / m["layout"], 2),
               operator_over_residual=round(m["op"] / m["residual"], 3), within_1p1_of_residual=bool(m["op"] <= 1.1 * m["residual"]),
               diagonal_ms=round(m["diag"], 3), assembly_ms=round(m["assembly"], 3), layout_fill_ms=round(max(m["layout_call"] - m["layout"], 0.0), 3))
    ablation(out)
    if n == 256:  # the Nitsche leg's faces
        x0 = mf.FACE_BITS["x0"]
        kw = dict(fixed_faces=x0, h_penalty=H_PEN, Tw=TW)
        opn = brick.thermal_operator(K_COND, H, TENV, 0x3F & ~x0, **kw)
        res_n = lambda: brick.residual_thermal(x, K_COND, H, TENV, 0x3F & ~x0, out=y, **kw)
        opn.mul_(y, x)
        res_n()
        to, tr = [], []
        for _ in range(reps):
            to.append(timed(lambda: opn.mul_(y, x)))
            tr.append(timed(res_n))
        mo, mr = float(np.median(to)), float(np.median(tr))
        out.update(nitsche_operator_product_ms=round(mo, 3), nitsche_residual_ms=round(mr, 3), nitsche_operator_over_residual=round(mo / mr, 3),
                   nitsche_within_1p1_of_residual=bool(mo <= 1.1 * mr))
        opn.close()
    for sv, name, s in ((mf.cg_, "cg", 0), (mf.idrs_, "idrs8", 8)):
        for way, (ctx, AA, vals) in (("operator", (cm, op, None)), ("assembled", (ca, A, K))):
            _, st = mf.iterative_Solve(AA, vals, b, 1e-300, Sv_func=sv, s=s, maxiter=200, max_pass=1, fixed_iterations=True)
            out[f"{way}_{name}200_solve_ms"] = round(float(st.solve_ms), 2)
            out[f"{way}_{name}200_final_res"] = float(st.final_res)
    torch.cuda.synchronize()
    total = int(torch.cuda.memory_allocated())
    out["operator_bytes"] = after_op - base - 2 * 8 * rows + int(_lib.lib.mfem_debug_ws_bytes(cm._h))  # (without this tool's x and y)
    out["assembled_bytes"] = total - after_op - 8 * rows + int(_lib.lib.mfem_debug_ws_bytes(ca._h))    # (without this tool's b)
    out["bytes_ratio"] = round(out["assembled_bytes"] / max(out["operator_bytes"], 1), 2)
    gc.collect()
    return out


def main():
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "256,512,768,1024").split(",") if v]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 900
    results = []
    if os.path.exists(OUT):
        results = [r for r in json.load(open(OUT)) if r.get("n") not in sizes]
    for n in sizes:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps)], stdout=subprocess.PIPE, text=True, timeout=limit)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            r = json.loads(lines[-1]) if p.returncode == 0 and lines else {"n": n, "failed": f"exit {p.returncode}"}
        except subprocess.TimeoutExpired:
            r = {"n": n, "failed": f"time limit of {limit} s"}
        results.append(r)
        print(json.dumps(r), flush=True)
        if "failed" in r:  # nothing larger is tried
            for rest in sizes[sizes.index(n) + 1:]:
                results.append({"n": rest, "not_measured": f"stopped after n = {n} failed"})
            break
    results.sort(key=lambda r: r["n"])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    return 1 if any("failed" in r for r in results) else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        try:
            print(json.dumps(child(int(sys.argv[2]), int(sys.argv[3]))), flush=True)
        except Exception as e:  # an allocation that fails is a result
            print(json.dumps({"n": int(sys.argv[2]), "failed": f"{type(e).__name__}: {str(e)[:300]}"}), flush=True)
        sys.exit(0)
    sys.exit(main())
