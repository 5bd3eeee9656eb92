"""The geometric multigrid preconditioner on the hex-27 THERMAL brick (Hex27BrickOperator.multigrid, Pr_Multigrid_) and the signed-diagonal sweep it
reads, timed on one device: n^3 hex-27 elements, itg 5, Robin on all faces, the affine brick and the brick with every element distorted, alternated
in one session.  Each (size, geometry) runs in a child process of its own with a time limit; medians of `reps` (>= 7) alternated repetitions with
min and max; nothing is tried twice.
  diagonal
      k_brick27_diagonal_sweep (mfem_debug_brick_operator_signed_diagonal: the sweep plus its face launch) against k_brick27_diagonal
      (mfem_brick_operator_diagonal, the kernel the sweep does not touch), alternated; condition: the sweep faster by more than the 10 % placement
      spread; the ratio to one operator product is recorded as a finding
  cycle against its parts
      model = sum over levels of [ products_l * t_prod(l) + S_l * 8 * points_l / B_copy ]
      t_prod(l)  the level's operator product timed alone (level 0: the hex-27 product; below it a hex-8 thermal operator on a brick of that level's
                 size and rule); products_l = 2 nu (nu_c - 1 on the coarsest); S_l = mg_cycle_streams; B_copy the copy rate measured here
      condition  cycle <= 1.15 x model
  time to solution
      the source problem (s = 1600) to 1e-6 |b| with cg_ + Pr_Multigrid_ (setup included) and with cg_ + Pr_Jacobi_ on the same operator:
      iterations, solve_ms, final_res, spmv_count; condition: multigrid faster by more than 10 %
  memory
      info.bytes, the context workspace after both solves
  bits
      SHA-256 of a hex-27 product and of mfem_brick_operator_diagonal on small bricks (the same on the parent commit and on this one)
usage: brick_multigrid_hex27_time.py [sizes = 128] [reps = 7] [limit_s = 900]
       brick_multigrid_hex27_time.py --record-diagonal FILE     (runs on any commit that has the hex-27 operator: the golden file of
                                                                tests/test_gpu_brick_multigrid_hex27.py::test_jacobi_diagonal_keeps_the_parents_bits)
The JSON lines go to stdout and, together, to profiles/brick_multigrid_hex27_time.json (results of sizes not asked for in this call are kept)."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_multigrid_hex27_time.json")
K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
X = (1.0, 1.5, 0.75)
ITG, NU, NU_C = 5, 2, 32
SHA_CASES = [((5, 4, 3), 5, True, 0x3F), ((9, 2, 9), 5, False, 0x15), ((2, 3, 2), 7, True, 0x3F), ((6, 2, 1), 5, True, 0)]


def streams(level, nlev):  # mg_cycle_streams
    s = (4 if NU_C == 1 else 5 + 6 * (NU_C - 1)) if level == nlev - 1 else 12 * NU + 2
    return s + (2 if level > 0 else 0)


def distort(brick):
    """every element distorted: _distort of tests/test_gpu_brick_operator.py on the library's own lattice"""
    import torch

    c = [brick.coords_view(d).clone() for d in range(3)]
    brick.coords_view(0).add_(0.03 * torch.sin(3 * c[1]) * torch.cos(2 * c[2]))
    brick.coords_view(1).add_(0.02 * torch.sin(2 * c[0] + c[2]))
    brick.coords_view(2).add_(0.025 * c[0] * c[1])


def sha_cases(mf):
    import torch

    out = []
    for n, itg, distorted, mask in SHA_CASES:
        brick = mf.make_Brick(X, n, 2, itg)
        if distorted:
            distort(brick)
        op = brick.thermal_operator_hex27(K_COND, H, TENV, mask)
        d = op.diagonal().cpu().numpy()
        x = torch.linspace(-1.0, 1.0, op.n, dtype=torch.float64, device="cuda")
        y = op.mul_(torch.empty_like(x), x).cpu().numpy()
        out.append({"n": list(n), "itg": itg, "distorted": distorted, "robin_faces": mask, "sha256": hashlib.sha256(d.tobytes()).hexdigest(),
                    "product_sha256": hashlib.sha256(y.tobytes()).hexdigest()})
        op.close()
    return out


def child(n, reps, distorted):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib

    lib = _lib.lib
    dev = f"cuda:{torch.cuda.current_device()}"
    out = {"n": n, "distorted": bool(distorted), "reps": reps, "itg": ITG, "box": torch.cuda.get_device_name()}

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def stat(ts):
        return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4), "max_ms": round(float(max(ts)), 4)}

    ctx = mf.Context(torch.cuda.current_device())
    brick = mf.make_Brick(X, (n, n, n), 2, ITG, ctx=ctx)
    if distorted:
        distort(brick)
    op = brick.thermal_operator_hex27(K_COND, H, TENV, 0x3F)
    mg = op.multigrid().setup()
    info = mg.info()
    levels = info["ne"]
    L = len(levels)
    out.update(rows=op.n, levels=L, ne=[list(e) for e in levels], sign=info["sign"], lambda_max=[round(v, 6) for v in info["lambda_max"]],
               hierarchy_bytes=info["bytes"])
    r = torch.empty(op.n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(1))
    z = torch.empty_like(r)
    # the diagonal: the sweep against the per-control-point kernel, alternated, with one product between them
    d_sweep, d_point = torch.zeros_like(r), torch.zeros_like(r)
    sweep = lambda: _lib.check(lib.mfem_debug_brick_operator_signed_diagonal(ctx._h, op._h, d_sweep.data_ptr()))
    point = lambda: _lib.check(lib.mfem_brick_operator_diagonal(ctx._h, op._h, d_point.data_ptr()))
    sweep(); point(); op.mul_(z, r)
    T = {"sweep": [], "point": [], "product": []}
    for _ in range(reps):
        T["sweep"].append(timed(sweep))
        T["point"].append(timed(point))
        T["product"].append(timed(lambda: op.mul_(z, r)))
    agree = float((d_sweep + d_point).abs().max() / d_point.abs().max())
    out["diagonal"] = {"sweep": stat(T["sweep"]), "per_control_point": stat(T["point"]), "product": stat(T["product"]),
                       "per_control_point_over_sweep": round(float(np.median(T["point"]) / np.median(T["sweep"])), 2),
                       "sweep_over_product": round(float(np.median(T["sweep"]) / np.median(T["product"])), 2),
                       "sweep_faster_by_more_than_10_percent": bool(np.median(T["point"]) > 1.1 * np.median(T["sweep"])),
                       "max_abs_K_ii_plus_abs_K_ii_over_max": agree}
    del d_sweep, d_point
    # the cycle against its parts
    ops = [op]
    for ne in levels[1:]:
        ops.append(mf.make_Brick(X, ne, 1, ITG, ctx=ctx).thermal_operator(K_COND, H, TENV, 0x3F))
    vec = [(r[:o.n], z[:o.n]) for o in ops]
    for o, (a, b) in zip(ops, vec):
        o.mul_(b, a)
    mg.apply(r, z)
    z.copy_(r)
    T_prod, T_cycle, T_copy = [[] for _ in ops], [], []
    for _ in range(reps):  # alternated: a cycle, every level's product, the copy
        T_cycle.append(timed(lambda: mg.apply(r, z)))
        for l, (o, (a, b)) in enumerate(zip(ops, vec)):
            T_prod[l].append(timed(lambda: o.mul_(b, a, -1.0, 1.0)))
        T_copy.append(timed(lambda: z.copy_(r)))
    t_prod = [float(np.median(t)) for t in T_prod]
    b_copy = 2 * 8 * op.n / (float(np.median(T_copy)) * 1e-3)
    per_level, model = [], 0.0
    for l, o in enumerate(ops):
        products = NU_C - 1 if l == L - 1 else 2 * NU
        t_p = products * t_prod[l]
        t_s = streams(l, L) * 8 * o.n / b_copy * 1e3
        model += t_p + t_s
        per_level.append({"ne": list(levels[l]), "points": o.n, "products": products, "t_prod_ms": round(t_prod[l], 4), "products_ms": round(t_p, 4),
                          "streams": streams(l, L), "streams_ms": round(t_s, 4)})
    cycle = float(np.median(T_cycle))
    out.update(cycle=stat(T_cycle), model_ms=round(model, 3), cycle_over_model=round(cycle / model, 3), copy_GBps=round(b_copy / 1e9, 1),
               cycle_within_1p15_of_model=bool(cycle <= 1.15 * model), per_level=per_level)
    del ops, vec, z
    # time to solution, both ways on the same operator, alternated
    zero = torch.zeros_like(r)
    b = brick.residual_thermal(zero, K_COND, H, TENV, 0x3F, s=torch.full_like(r, SRC))
    del zero, r
    tol = 1e-6 * mf.normalized_norm(b, ctx)
    runs = {"multigrid": [], "jacobi": []}
    for _ in range(reps):
        for name, pr, maxiter in (("multigrid", mf.Pr_Multigrid_, 200), ("jacobi", mf.Pr_Jacobi_, 6000)):
            _, st = mf.iterative_Solve(op, None, b, tol, Sv_func=mf.cg_, Pr_func=pr, maxiter=maxiter, max_pass=2)
            torch.cuda.synchronize()
            runs[name].append((float(st.solve_ms), int(st.iterations), float(st.final_res), int(st.converged), int(st.spmv_count),
                               int(lib.mfem_debug_ws_bytes(ctx._h))))
    for name, rs in runs.items():
        ts = [v[0] for v in rs]
        out[name] = {"solve_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2), "iterations": rs[-1][1],
                     "final_res": rs[-1][2], "converged": rs[-1][3], "spmv_count": rs[-1][4], "workspace_bytes": rs[-1][5]}
    out["converge_tol"] = tol
    out["jacobi_over_multigrid"] = round(out["jacobi"]["solve_ms"] / out["multigrid"]["solve_ms"], 2)
    out["multigrid_faster_by_more_than_10_percent"] = bool(out["jacobi"]["solve_ms"] > 1.1 * out["multigrid"]["solve_ms"])
    out["memory"] = {"hierarchy_bytes": info["bytes"], "level0_vector_bytes": 8 * op.n, "hierarchy_in_level0_vectors": round(info["bytes"] / (8 * op.n), 3),
                     "workspace_after_both_solves": out["jacobi"]["workspace_bytes"]}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--record-diagonal":
        sys.path.insert(0, ROOT)
        import metafem_jl_amd as mf

        json.dump({"tool": "tools/brick_multigrid_hex27_time.py --record-diagonal", "what": "SHA-256 of mfem_brick_operator_diagonal (and of a product of "
                   "x = linspace(-1, 1)) on hex-27 bricks of size (1, 1.5, 0.75), k = 0.6, h = 25, Tenv = 293.15", "cases": sha_cases(mf)},
                  open(sys.argv[2], "w"), indent=1)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        res = child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        if not int(sys.argv[4]):
            sys.path.insert(0, ROOT)
            import metafem_jl_amd as mf

            res["bits"] = sha_cases(mf)
        print("RESULT " + json.dumps(res), flush=True)
        return
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "128").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 900
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}  # (other keys, such as the record of what did not move against the parent, are kept)
    results = doc.get("runs", {})
    for n in sizes:
        for distorted in (0, 1):
            key = f"{n}-{'distorted' if distorted else 'affine'}"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps), str(distorted)], capture_output=True, text=True,
                                   timeout=limit)
            except subprocess.TimeoutExpired:
                print(json.dumps({"run": key, "error": f"time limit of {limit} s"}), flush=True)
                return
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(json.dumps({"run": key, "error": (p.stderr or p.stdout)[-600:]}), flush=True)
                return
            results[key] = json.loads(line[0][len("RESULT "):])
            print(json.dumps(results[key]), flush=True)
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            doc.update(tool="tools/brick_multigrid_hex27_time.py", runs={k: results[k] for k in sorted(results)})
            json.dump(doc, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
