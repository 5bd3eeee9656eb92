"""The geometric multigrid preconditioner on the hex-8 ELASTICITY brick (ElasticityBrickOperator.multigrid, Pr_Multigrid_) timed on one device: the
unit brick, itg 3, E = 1, Poisson 0.3, penalty tau = 1000 on x0, sigma_11 = 0.01 pulled on x1 (the README's cantilever load).  Each size runs in a
child process of its own with a time limit; medians of `reps` (>= 7) alternated repetitions; nothing is tried twice.
  cycle against its parts
      model = sum over levels of [ products_l * t_prod(l) + S_l * 8 * fields * points_l / B_copy ]
      t_prod(l)  mfem_brick_operator_apply of the elasticity operator timed alone on a brick of that level's size; products_l = 2 nu (nu_c - 1 on
                 the coarsest)
      B_copy     the device-to-device copy rate on a level-0 vector (read + write bytes per second), measured here
      S_l        the vector streams per cycle on the level (csrc/brick_multigrid_decide.h: mg_cycle_streams, unchanged; a level vector holds
                 fields x points doubles)
      condition  cycle <= 1.15 x model; the per-level terms are recorded either way
  transfers
      one 3-field restriction and one 3-field prolongation (level 0 <-> 1, mfem_debug_brick_multigrid_transfer) against three launches of the
      one-field kernel on the same lattice (a thermal hierarchy on the same brick); recorded, no condition
  time to solution
      the cantilever load to 1e-6 |b| with cg_ + Pr_Multigrid_ and with cg_ + Pr_Jacobi_ on the same operator: iterations, solve_ms (the multigrid's
      setup included), final_res, spmv_count, workspace bytes; condition: multigrid faster by more than 10 %
  memory
      info.bytes plus the solve workspace against the Jacobi solve's workspace
usage: brick_multigrid_elasticity_time.py [sizes = 128,256] [reps = 7] [limit_s = 900]
The JSON lines go to stdout and, together, to profiles/brick_multigrid_elasticity_time.json (results of sizes not asked for in this call are kept)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_multigrid_elasticity_time.json")
E_MOD, POISSON, TAU, SIGMA = 1.0, 0.3, 1000.0, 0.01
LAM, MU = E_MOD * POISSON / ((1 + POISSON) * (1 - 2 * POISSON)), E_MOD / (2 * (1 + POISSON))
NU, NU_C, FIELDS = 2, 32, 3


def streams(level, nlev):  # mg_cycle_streams
    s = (4 if NU_C == 1 else 5 + 6 * (NU_C - 1)) if level == nlev - 1 else 12 * NU + 2
    return s + (2 if level > 0 else 0)


def child(n, reps):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib

    lib = _lib.lib
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
    pen, tra = mf.FACE_BITS["x0"], mf.FACE_BITS["x1"]
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 1, 3, ctx=ctx)
    op = brick.elasticity_operator(LAM, MU, TAU, pen)
    mg = op.multigrid().setup()
    info = mg.info()
    levels = info["ne"]
    L = len(levels)
    out.update(rows=op.n, fields=FIELDS, levels=L, sign=info["sign"], lambda_max=[round(v, 6) for v in info["lambda_max"]], hierarchy_bytes=info["bytes"])
    # the parts: a product per level, the copy rate
    r = torch.empty(op.n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=torch.Generator(dev).manual_seed(1))
    z = torch.empty_like(r)
    ops = [op]
    for ne in levels[1:]:
        ops.append(mf.make_Brick((1.0, 1.0, 1.0), ne, 1, 3, ctx=ctx).elasticity_operator(LAM, MU, TAU, pen))
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
    copy_ms = float(np.median(T_copy))
    b_copy = 2 * 8 * op.n / (copy_ms * 1e-3)  # bytes per second, read + write
    per_level, model = [], 0.0
    for l, o in enumerate(ops):
        products = NU_C - 1 if l == L - 1 else 2 * NU
        t_p = products * t_prod[l]
        t_s = streams(l, L) * 8 * o.n / b_copy * 1e3  # (o.n = fields x points)
        model += t_p + t_s
        per_level.append({"ne": list(levels[l]), "products": products, "t_prod_ms": round(t_prod[l], 4), "products_ms": round(t_p, 4),
                          "streams": streams(l, L), "streams_ms": round(t_s, 4)})
    cycle = float(np.median(T_cycle))
    out.update(cycle_ms=round(cycle, 3), model_ms=round(model, 3), cycle_over_model=round(cycle / model, 3), copy_GBps=round(b_copy / 1e9, 1),
               cycle_within_1p15_of_model=bool(cycle <= 1.15 * model), per_level=per_level)
    del ops, vec
    # the transfers: one 3-field launch against three launches of the one-field kernel on the same lattice
    if L > 1:
        pts_f, pts_c = op.n // FIELDS, (levels[1][0] + 1) * (levels[1][1] + 1) * (levels[1][2] + 1)
        top = brick.thermal_operator(0.6, 25.0, 293.15, 0x3F)
        tmg = top.multigrid(max_levels=2)
        coarse = torch.empty(FIELDS * pts_c, dtype=torch.float64, device=dev)

        def transfer(handle, restriction, src, dst):
            _lib.check(lib.mfem_debug_brick_multigrid_transfer(ctx._h, handle, 0, restriction, src.data_ptr(), dst.data_ptr()))

        def three(restriction, src, dst, ps, pd):
            for f in range(FIELDS):
                transfer(tmg._h, restriction, src[f * ps:(f + 1) * ps], dst[f * pd:(f + 1) * pd])

        legs = {"restrict_3field": lambda: transfer(mg._h, 1, r, coarse), "restrict_3x1field": lambda: three(1, r, coarse, pts_f, pts_c),
                "prolong_3field": lambda: transfer(mg._h, 0, coarse, z), "prolong_3x1field": lambda: three(0, coarse, z, pts_c, pts_f)}
        for fn in legs.values():
            fn()
        T = {k: [] for k in legs}
        for _ in range(reps):
            for k, fn in legs.items():
                T[k].append(timed(fn))
        out["transfers_ms"] = {k: round(float(np.median(v)), 4) for k, v in T.items()}
        del coarse
        tmg.close()
        top.close()
    del z
    # time to solution, both ways on the same operator, alternated
    zero = torch.zeros_like(r)
    b = brick.residual_elasticity(zero, LAM, MU, TAU, pen, tra, (SIGMA, 0.0, 0.0, 0.0, 0.0, 0.0))
    del zero, r
    tol = 1e-6 * mf.normalized_norm(b, ctx)
    runs = {"multigrid": [], "jacobi": []}
    solve_reps = max(3, reps // 2) if n >= 384 else reps
    for _ in range(solve_reps):
        for name, pr, maxiter in (("multigrid", mf.Pr_Multigrid_, 300), ("jacobi", mf.Pr_Jacobi_, 8000)):
            _, st = mf.iterative_Solve(op, None, b, tol, Sv_func=mf.cg_, Pr_func=pr, maxiter=maxiter, max_pass=2)
            torch.cuda.synchronize()
            runs[name].append((float(st.solve_ms), int(st.iterations), float(st.final_res), int(st.converged), int(st.spmv_count),
                               int(lib.mfem_debug_ws_bytes(ctx._h))))
    for name, rs in runs.items():
        out[name] = {"solve_ms": round(float(np.median([v[0] for v in rs])), 2), "iterations": rs[-1][1], "final_res": rs[-1][2], "converged": rs[-1][3],
                     "spmv_count": rs[-1][4], "workspace_bytes": rs[-1][5], "solve_reps": len(rs)}
    out["converge_tol"] = tol
    out["jacobi_over_multigrid"] = round(out["jacobi"]["solve_ms"] / out["multigrid"]["solve_ms"], 2)
    out["multigrid_faster_by_more_than_10_percent"] = bool(out["jacobi"]["solve_ms"] > 1.1 * out["multigrid"]["solve_ms"])
    out["memory"] = {"hierarchy_bytes": info["bytes"], "workspace_is_the_larger_of_both_solves": out["multigrid"]["workspace_bytes"],
                     "level0_vector_bytes": 8 * op.n, "hierarchy_in_level0_vectors": round(info["bytes"] / (8 * op.n), 3)}
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(child(int(sys.argv[2]), int(sys.argv[3]))), flush=True)
        return
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "128,256").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 900
    results = {}
    if os.path.exists(OUT):
        results = {int(k): v for k, v in json.load(open(OUT)).get("sizes", {}).items()}
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
        json.dump({"tool": "tools/brick_multigrid_elasticity_time.py", "sizes": {str(k): results[k] for k in sorted(results)}}, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
