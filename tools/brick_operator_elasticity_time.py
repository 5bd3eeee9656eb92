"""The matrix-free hex-8 brick operator on elasticity (Brick.elasticity_operator, mfem_solve_operator) against mfem_brick_residual_elasticity and
against the assembled path.  Each size runs in a child process of its own with a time limit; the tool stops at the first failure.
The brick is the unit cube of n^3 elements, itg 3 (the 2-point rule: the plane sweep), lambda and mu of E = 1, nu = 0.3, the penalty tau = 1000 on x0.
  every size, warm-up, then the median of `reps` repetitions with the paths alternated:
    product    the operator product (event-timed mul_, beta = 0, no scaling: no partial sums, so not folded), the product inside a solve (the
               per-launch timing of a 20-step fixed cg! solve, mfem_prof_spmv_*: with the partial sums of p . A p; folded above 3584 work items), mfem_brick_residual_elasticity
               on the same brick and vector; condition: operator <= 1.1 x residual
    solve      200 fixed cg! iterations and 200 fixed idrs!(8) steps (stats.solve_ms, stats.final_res)
    converged  cg! + Pr_Jacobi! on the cantilever load (sigma_11 = 0.01 pulled on x1) to 1e-6 |b| (final_res, iterations); operator_bytes = what
               torch holds (the load, x) plus the context's workspace, which never shrinks: it is the one idrs!(8) grew (its 30-odd vectors), not cg!'s
  n <= assembled_upto, both paths alive: the layout SpMV of the assembled K (the same per-launch timing), the operator's diagonal against assembly
    plus the layout fill, the fixed solves on the assembled path, assembled_bytes = K, the vectors and that context's workspace (with the layout copy;
    the pattern's rowptr and colidx, library-owned, are NOT counted: 4 nnz + 8 n bytes more).
  n == 33 (always run first): SHA-256 of one thermal operator product and of one mfem_brick_residual_elasticity result, to compare trees bit for bit
    (`--hashes` prints them alone: run it from a copy of this file in the parent commit's tree and paste the record under "parent_tree").
usage: brick_operator_elasticity_time.py [sizes = 128,256] [reps = 5] [limit_s = 900] [assembled_upto = 128]
The JSON lines go to stdout and, together, to profiles/brick_operator_elasticity_time.json (results of sizes not asked for in this call are kept)."""
import ctypes as C
import gc
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_operator_elasticity_time.json")
E_MOD, NU = 1.0, 0.3
LAM, MU = E_MOD * NU / ((1 + NU) * (1 - 2 * NU)), E_MOD / (2 * (1 + NU))
TAU = 1000.0
SIG = (0.01, 0.0, 0.0, 0.0, 0.0, 0.0)


def hashes():
    """one 33^3 result of the thermal operator's product and of the elasticity residual: the same bits on every tree that leaves them alone"""
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf

    dev = f"cuda:{torch.cuda.current_device()}"
    brick = mf.make_Brick((1.0, 1.5, 0.75), (32, 32, 32), 1, 3)
    g = torch.Generator(dev).manual_seed(3)
    x = torch.empty(3 * brick.ncp, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g)
    top = brick.thermal_operator(0.6, 25.0, 293.15, 0x3F, fixed_faces=0, h_penalty=0.0, Tw=0.0)
    yt = top.mul_(torch.empty(brick.ncp, dtype=torch.float64, device=dev), x[: brick.ncp].contiguous())
    r = brick.residual_elasticity(x, LAM, MU, TAU, mf.FACE_BITS["x0"], mf.FACE_BITS["x1"], SIG)
    out = {"n": 33, "what": "bit-for-bit hashes of results this change must not move",
           "thermal_operator_product_sha256": hashlib.sha256(yt.cpu().numpy().tobytes()).hexdigest(),
           "residual_elasticity_sha256": hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest()}
    if hasattr(brick, "elasticity_operator"):
        ye = brick.elasticity_operator(LAM, MU, TAU, mf.FACE_BITS["x0"]).mul_(torch.empty_like(x), x)
        out["elasticity_operator_product_sha256"] = hashlib.sha256(ye.cpu().numpy().tobytes()).hexdigest()
    return out


def child(n, reps, assembled_upto):
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
    pen, tra = mf.FACE_BITS["x0"], mf.FACE_BITS["x1"]

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

    torch.cuda.synchronize()
    base = int(torch.cuda.memory_allocated())
    cm = mf.Context(torch.cuda.current_device())
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 1, 3, ctx=cm)
    op = brick.elasticity_operator(LAM, MU, TAU, pen)
    rows = op.n
    out["rows"] = rows
    x = torch.empty(rows, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(1))
    y = torch.empty_like(x)
    b = torch.empty_like(x).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(2))
    residual = lambda: brick.residual_elasticity(x, LAM, MU, TAU, pen, 0, out=y)
    both = n <= assembled_upto
    after_op = int(torch.cuda.memory_allocated())
    if both:
        ca = mf.Context(torch.cuda.current_device())
        brick_a = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 1, 3, ctx=ca)
        A = brick_a.pattern(3)
        K = brick_a.assemble_elasticity(A, LAM, MU, TAU, pen)
        out["nnz"] = int(A.nnz)
        layout_call = lambda: _lib.check(_lib.lib.mfem_spmv_solver_layout(ca._h, A._h, K.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0))
    # warm-up: every path once
    op.mul_(y, x)
    op.diagonal()
    residual()
    solver_spmv_ms(cm, op, None, b, 4)
    if both:
        layout_call()
        solver_spmv_ms(ca, A, K, b, 4)
        y_csr = mf.mul_(torch.empty_like(x), A, K, x)
        out["product_max_rel_diff"] = float((op.mul_(y, x) - y_csr).abs().max() / y_csr.abs().max())
        del y_csr
    T = {k: [] for k in ("op", "op_in_solve", "layout", "residual", "diag", "assembly", "layout_call")}
    for _ in range(reps):  # the paths alternated
        T["op"].append(timed(lambda: op.mul_(y, x)))
        T["residual"].append(timed(residual))
        T["op_in_solve"].append(solver_spmv_ms(cm, op, None, b))
        T["diag"].append(timed(op.diagonal))
        if both:
            T["layout"].append(solver_spmv_ms(ca, A, K, b))
            T["assembly"].append(timed(lambda: brick_a.assemble_elasticity(A, LAM, MU, TAU, pen, out=K)))
            T["layout_call"].append(timed(layout_call))
    m = {k: float(np.median(v)) for k, v in T.items() if v}
    out.update(operator_product_ms=round(m["op"], 3), residual_ms=round(m["residual"], 3), operator_over_residual=round(m["op"] / m["residual"], 3),
               within_1p1_of_residual=bool(m["op"] <= 1.1 * m["residual"]), operator_product_in_solve_ms=round(m["op_in_solve"], 3),
               in_solve_over_residual=round(m["op_in_solve"] / m["residual"], 3), diagonal_ms=round(m["diag"], 3),
               operator_product_all_ms=[round(v, 3) for v in T["op"]], residual_all_ms=[round(v, 3) for v in T["residual"]])
    if both:
        out.update(layout_spmv_ms=round(m["layout"], 3), operator_over_layout=round(m["op"] / m["layout"], 2), assembly_ms=round(m["assembly"], 3),
                   layout_fill_ms=round(max(m["layout_call"] - m["layout"], 0.0), 3))
    ways = [("operator", (cm, op, None))] + ([("assembled", (ca, A, K))] if both else [])
    for sv, name, s in ((mf.cg_, "cg", 0), (mf.idrs_, "idrs8", 8)):
        for way, (ctx, AA, vals) in ways:
            _, st = mf.iterative_Solve(AA, vals, b, 1e-300, Sv_func=sv, s=s, maxiter=200, max_pass=1, fixed_iterations=True)
            out[f"{way}_{name}200_solve_ms"] = round(float(st.solve_ms), 2)
            out[f"{way}_{name}200_final_res"] = float(st.final_res)
    torch.cuda.synchronize()
    total = int(torch.cuda.memory_allocated())
    if both:
        out["assembled_bytes"] = total - after_op + int(_lib.lib.mfem_debug_ws_bytes(ca._h))
        del K, A, brick_a, layout_call, ways, AA, vals  # (every name that holds K or A)
        ca.close()
        gc.collect()
    # the cantilever load, converged
    zero = torch.zeros_like(x)
    load = brick.residual_elasticity(zero, LAM, MU, TAU, pen, tra, SIG)
    del zero, x, y, b
    tol = 1e-6 * mf.normalized_norm(load, cm)
    _, st = mf.iterative_Solve(op, None, load, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=30000, max_pass=2)
    torch.cuda.synchronize()
    out.update(converged=int(st.converged), converge_tol=tol, final_res=float(st.final_res), iterations=int(st.iterations), passes=int(st.passes),
               solve_ms=round(float(st.solve_ms), 1),
               operator_bytes=int(torch.cuda.memory_allocated()) - base + int(_lib.lib.mfem_debug_ws_bytes(cm._h)))  # (brick, load, x and the workspace)
    if both:
        out["bytes_ratio"] = round(out["assembled_bytes"] / max(out["operator_bytes"], 1), 2)
    return out


def main():
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "128,256").split(",") if v]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 900
    upto = int(sys.argv[4]) if len(sys.argv) > 4 else 128
    results, parent = [], None
    if os.path.exists(OUT):
        old = json.load(open(OUT))
        parent = next((r.get("parent_tree") for r in old if r.get("n") == 33), None)  # (--hashes on the parent commit's tree, pasted in by hand: kept)
        results = [r for r in old if r.get("n") not in sizes + [33]]
    for n in [33] + sizes:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps), str(upto)], stdout=subprocess.PIPE, text=True,
                               timeout=limit)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            r = json.loads(lines[-1]) if p.returncode == 0 and lines else {"n": n, "failed": f"exit {p.returncode}"}
        except subprocess.TimeoutExpired:
            r = {"n": n, "failed": f"time limit of {limit} s"}
        if n == 33 and parent is not None and "failed" not in r:
            r["parent_tree"] = parent
            r["same_bits_as_parent"] = all(r[k] == v for k, v in parent.items() if k.endswith("_sha256"))
        results.append(r)
        print(json.dumps(r), flush=True)
        if "failed" in r:  # nothing larger is tried
            for rest in sizes[sizes.index(n) + 1:] if n in sizes else sizes:
                results.append({"n": rest, "not_measured": f"stopped after n = {n} failed"})
            break
    results.sort(key=lambda r: r["n"])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    return 1 if any("failed" in r for r in results) else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--hashes":  # (importable by a script that points ROOT's package at another tree)
        print(json.dumps(hashes()), flush=True)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        try:
            n = int(sys.argv[2])
            print(json.dumps(hashes() if n == 33 else child(n, int(sys.argv[3]), int(sys.argv[4]))), flush=True)
        except Exception as e:  # an allocation that fails is a result
            print(json.dumps({"n": int(sys.argv[2]), "failed": f"{type(e).__name__}: {str(e)[:300]}"}), flush=True)
        sys.exit(0)
    sys.exit(main())
