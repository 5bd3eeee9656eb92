"""gmres_ with the multigrid V-cycle on a hex-8 thermal brick with a Nitsche face (BrickOperator.multigrid(nonsymmetric=True), Pr_Multigrid_) timed on
one device: the unit brick, itg 3, x0 fixed (h_penalty 1000, Tw 1173.15), Robin on the other five faces.  Each size runs in a child process of its
own with a time limit; medians of `reps` (>= 7) alternated repetitions.
  condition 1: time to solution
      the source problem (s = 1600) to 1e-6 |b| with gmres_(20) + Pr_Multigrid_ (the setup included) against what a user has without it on the same
      matrix-free operator: idrs_(8) + Pr_Jacobi_ and gmres_(20) + Pr_Jacobi_, whichever is faster; iterations, spmv_count, final_res of all three;
      condition: the multigrid solve faster than that baseline by more than 10 %
  condition 2: one cycle on the Nitsche operator against its parts
      model = sum over levels of [ products_l * t_prod(l) + S_l * 8 n_l / B_copy ]  (tools/brick_multigrid_time.py's model: the level's product
      timed alone on a Nitsche operator of that size, mg_cycle_streams at the copy rate measured in the run); condition: cycle <= 1.15 x model
  finding: one restart of s Arnoldi steps (fixed_iterations, maxiter = s) minus the setup, its s + 1 cycles and its s + 2 products, against the vector
      streams of its own kernels at the copy rate: step k moves 4 k + 8 vectors (two block dots of k + 1, two updates of k + 2, the normalisation's 2),
      the restart 2 (Q_1) + s + 1 (u) + 3 (x += z) + 3 (the residual's finish), the wrapper's residual 3 more
usage: brick_multigrid_nonsym_time.py [sizes = 256,512] [reps = 7] [limit_s = 900]
The JSON lines go to stdout and, together, to profiles/brick_multigrid_nonsym_time.json (results of sizes not asked for in this call are kept)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_multigrid_nonsym_time.json")
K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
ROBIN, FIXED = 0x2F, dict(fixed_faces=0x10, h_penalty=1000.0, Tw=1173.15)
NU, NU_C, S = 2, 32, 20


def streams(level, nlev):  # mg_cycle_streams
    s = (4 if NU_C == 1 else 5 + 6 * (NU_C - 1)) if level == nlev - 1 else 12 * NU + 2
    return s + (2 if level > 0 else 0)


def child(n, reps):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf

    dev = f"cuda:{torch.cuda.current_device()}"
    out = {"n": n, "reps": reps, "box": torch.cuda.get_device_name()}

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    ctx = mf.Context(torch.cuda.current_device())
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 1, 3, ctx=ctx)
    op = brick.thermal_operator(K_COND, H, TENV, ROBIN, **FIXED)
    mg = op.multigrid(nonsymmetric=True).setup()
    info = mg.info()
    levels = info["ne"]
    L = len(levels)
    out.update(rows=op.n, levels=L, sign=info["sign"], lambda_max=[round(v, 6) for v in info["lambda_max"]], hierarchy_bytes=info["bytes"])
    # condition 2: the parts -- a product per level on a Nitsche operator of that size, the copy rate
    r = torch.empty(op.n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(1))
    z = torch.empty_like(r)
    ops = [op]
    for ne in levels[1:]:
        ops.append(mf.make_Brick((1.0, 1.0, 1.0), ne, 1, 3, ctx=ctx).thermal_operator(K_COND, H, TENV, ROBIN, **FIXED))
    vec = [(r[:o.n], z[:o.n]) for o in ops]
    for o, (a, b) in zip(ops, vec):
        o.mul_(b, a)
    mg.apply(r, z)
    z.copy_(r)
    T_prod, T_cycle, T_copy, T_setup = [[] for _ in ops], [], [], []
    for _ in range(reps):  # alternated: a cycle, every level's product, the copy, a setup
        T_cycle.append(timed(lambda: mg.apply(r, z)))
        for l, (o, (a, b)) in enumerate(zip(ops, vec)):
            T_prod[l].append(timed(lambda: o.mul_(b, a, -1.0, 1.0)))
        T_copy.append(timed(lambda: z.copy_(r)))
        T_setup.append(timed(lambda: mg.setup()))
    t_prod = [float(np.median(t)) for t in T_prod]
    copy_ms = float(np.median(T_copy))
    setup_ms = float(np.median(T_setup))
    b_copy = 2 * 8 * op.n / (copy_ms * 1e-3)  # bytes per second, read + write
    per_level, model = [], 0.0
    for l, o in enumerate(ops):
        products = NU_C - 1 if l == L - 1 else 2 * NU
        t_p = products * t_prod[l]
        t_s = streams(l, L) * 8 * o.n / b_copy * 1e3
        model += t_p + t_s
        per_level.append({"ne": list(levels[l]), "products": products, "t_prod_ms": round(t_prod[l], 4), "products_ms": round(t_p, 4),
                          "streams": streams(l, L), "streams_ms": round(t_s, 4)})
    cycle = float(np.median(T_cycle))
    out.update(cycle_ms=round(cycle, 3), model_ms=round(model, 3), cycle_over_model=round(cycle / model, 3), copy_GBps=round(b_copy / 1e9, 1),
               setup_ms=round(setup_ms, 3), cycle_within_1p15_of_model=bool(cycle <= 1.15 * model), per_level=per_level)
    del ops, vec, z
    # condition 1: time to solution, three ways on the same operator, alternated
    zero = torch.zeros_like(r)
    b = brick.residual_thermal(zero, K_COND, H, TENV, ROBIN, s=torch.full_like(r, SRC), **FIXED)
    del zero, r
    tol = 1e-6 * mf.normalized_norm(b, ctx)
    ways = (("gmres_multigrid", dict(Sv_func=mf.gmres_, Pr_func=mf.Pr_Multigrid_, s=S, maxiter=200, max_pass=4)),
            ("idrs8_jacobi", dict(Sv_func=mf.idrs_, Pr_func=mf.Pr_Jacobi_, s=8, maxiter=20000, max_pass=10)),
            ("gmres20_jacobi", dict(Sv_func=mf.gmres_, Pr_func=mf.Pr_Jacobi_, s=S, maxiter=3000, max_pass=1)))
    runs = {name: [] for name, _ in ways}
    solve_reps = max(3, reps // 2) if n >= 512 else reps
    for rep in range(solve_reps):
        for name, kw in ways:
            if name == "gmres20_jacobi" and rep >= 3:  # (thousands of steps with up to 20 basis vectors each: three repetitions)
                continue
            _, st = mf.iterative_Solve(op, None, b, tol, **kw)
            torch.cuda.synchronize()
            runs[name].append((float(st.solve_ms), int(st.iterations), float(st.final_res), int(st.converged), int(st.spmv_count), int(st.passes)))
    for name, rs in runs.items():
        out[name] = {"solve_ms": round(float(np.median([v[0] for v in rs])), 2), "iterations": rs[-1][1], "final_res": rs[-1][2], "converged": rs[-1][3],
                     "spmv_count": rs[-1][4], "passes": rs[-1][5], "solve_reps": len(rs)}
    out["converge_tol"] = tol
    conv = [k for k in ("idrs8_jacobi", "gmres20_jacobi") if out[k]["converged"]]
    base = min(conv, key=lambda k: out[k]["solve_ms"]) if conv else None
    out["baseline"] = base
    if base:
        out["baseline_over_multigrid"] = round(out[base]["solve_ms"] / out["gmres_multigrid"]["solve_ms"], 2)
        out["multigrid_faster_by_more_than_10_percent"] = bool(out["gmres_multigrid"]["converged"] and
                                                               out[base]["solve_ms"] > 1.1 * out["gmres_multigrid"]["solve_ms"])
    # finding: one restart of S steps without its cycles and products, against its vector streams
    T_fixed = []
    for _ in range(solve_reps):
        _, st = mf.iterative_Solve(op, None, b, tol, Sv_func=mf.gmres_, Pr_func=mf.Pr_Multigrid_, s=S, maxiter=S, max_pass=1, fixed_iterations=True)
        T_fixed.append(float(st.solve_ms))
    fixed_ms = float(np.median(T_fixed))
    rest = fixed_ms - setup_ms - (S + 1) * cycle - (S + 2) * t_prod[0]
    nstreams = sum(4 * k + 8 for k in range(1, S + 1)) + 2 + (S + 1) + 3 + 3 + 3
    streams_ms = nstreams * 8 * op.n / b_copy * 1e3
    out["arnoldi"] = {"fixed_restart_ms": round(fixed_ms, 2), "without_setup_cycles_products_ms": round(rest, 2), "vector_streams": nstreams,
                      "streams_ms": round(streams_ms, 2), "over_streams": round(rest / streams_ms, 3), "per_step_ms": round(rest / S, 3)}
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(child(int(sys.argv[2]), int(sys.argv[3]))), flush=True)
        return
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "256,512").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 900
    results, extra = {}, {}
    if os.path.exists(OUT):
        old = json.load(open(OUT))
        results = {int(k): v for k, v in old.get("sizes", {}).items()}
        extra = {k: v for k, v in old.items() if k not in ("tool", "sizes")}
    for n in sizes:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"n": n, "error": f"time limit of {limit} s"}), flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(json.dumps({"n": n, "error": (p.stderr or p.stdout)[-600:]}), flush=True)
            break
        results[n] = json.loads(line[0][len("RESULT "):])
        print(json.dumps(results[n]), flush=True)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        json.dump({"tool": "tools/brick_multigrid_nonsym_time.py", "sizes": {str(k): results[k] for k in sorted(results)}, **extra}, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
