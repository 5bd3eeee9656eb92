"""The matrix-free hex-27 elasticity brick operator (Brick.elasticity_operator_hex27: Hex27ElasticityBrickOperator) against the hex-27 THERMAL operator
on the same brick, rule and session: n^3 elements (64, 128), itg 5, penalty tau = 1000 on x0.  Two legs, each in a child process of its own with a
time limit: `affine` (the brick as made) and `distorted` (every element moved by a smooth map).  Warm-up, then the median and the spread (min, max)
of `reps` repetitions with the paths alternated:
  condition A  the elasticity product (event-timed mul_, beta = 0, no scaling) <= 3.0 x the thermal hex-27 product (tools/brick_operator_hex27_time.py's
               kernel, Robin on all faces).  Beside it the ablation: the product at the alternative arrangement (8 waves per workgroup: 123.7 KB of LDS
               where the shipped 12 waves take 155.7 KB; one workgroup per CU both ways) and with the stress stage reduced to one field (timing only).
  condition B  the product is faster, by more than the 10 % placement and clock spread, than the only other device route: a MeshOperator
               (GenericDomain(matrix_free=True)) of the same form on the same hex-27 lattice, built with make_Brick and mesh_Classical and moved by the
               same map, timed alternately with the product in the same process; its device bytes stand beside the brick operator's.  The two
               products are cross-checked through the energy x' K x of the same smooth field (their unknowns are ordered differently).
  findings     the product inside cg! (mfem_prof_spmv_*: with dotw, folded), the diagonal (the per-control-point form ships) against one product, 200
               fixed cg! and idrs!(8) steps with final_res, the cantilever problem (sigma_11 = 0.01 pulled on x1) with cg! + Pr_Jacobi! to 1e-6 |b| (64^3
               only by default), the device bytes, R, the LDS bytes and waves of both arrangements.
usage: brick_operator_elasticity_hex27_time.py [n = 128] [reps = 7] [limit_s = 500] [legs = affine,distorted] [cantilever = 0|1] [mesh = 1|0]
The JSON lines go to stdout and, together, to profiles/brick_operator_elasticity_hex27_time.json."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "brick_operator_elasticity_hex27_time.json")
E_MOD, NU, TAU = 1.0, 0.3, 1000.0
LAM, MU = E_MOD * NU / ((1 + NU) * (1 - 2 * NU)), E_MOD / (2 * (1 + NU))
K_COND, H, TENV = 0.6, 25.0, 293.15

sys.path.insert(0, os.path.join(ROOT, "tools"))


def distort_(c0, c1, c2):
    """the smooth map of the `distorted` leg (tools/brick_operator_hex27_time.py's), on three coordinate arrays of one kind (torch or numpy)"""
    import numpy as np
    import torch

    sin, cos = (torch.sin, torch.cos) if isinstance(c0, torch.Tensor) else (np.sin, np.cos)
    return c0 + 0.03 * sin(3 * c1) * cos(2 * c2), c1 + 0.02 * sin(2 * c0 + c2), c2 + 0.025 * c0 * c1


def child(n, reps, leg, cantilever, mesh_leg=True):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import metafem_jl_amd as mf
    from brick_operator_hex27_time import redundancy
    from metafem_jl_amd import _lib

    dev = f"cuda:{torch.cuda.current_device()}"
    R, L = redundancy(n)
    waves = mf.brick_operator_elasticity_hex27_waves(3)
    out = {"leg": leg, "n": n, "itg": 5, "reps": reps, "box": torch.cuda.get_device_name(), "R": round(R, 4), "segment_planes": L,
           "diagonal_form": "a thread per control point (the pair-form sweep is not built)",
           "shipped": {"waves": waves, "lds_bytes": mf.brick_operator_elasticity_hex27_lds_bytes(3, waves), "workgroups_per_cu": 1},
           "alternative": {"waves": 8, "lds_bytes": mf.brick_operator_elasticity_hex27_lds_bytes(3, 8), "workgroups_per_cu": 1},
           "condition_B": "not run"}
    out["min_max"] = "every *_ms entry holds median, min and max of the repetitions"

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def knob(word, fn):
        _lib.check(_lib.lib.mfem_debug_set(b"elasticity_hex27", word, 0))
        try:
            return timed(fn)
        finally:
            _lib.lib.mfem_debug_set(b"elasticity_hex27", 0, 0)

    def solver_spmv_ms(ctx, A, b, iters=20):
        _lib.check(_lib.lib.mfem_prof_spmv_enable(ctx._h, 1))
        try:
            mf.iterative_Solve(A, None, b, 1e-300, Sv_func=mf.cg_, maxiter=iters, max_pass=1, fixed_iterations=True)
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(_lib.lib.mfem_prof_spmv_read(ctx._h, C.byref(ms), C.byref(cnt), 1))
        finally:
            _lib.lib.mfem_prof_spmv_enable(ctx._h, 0)
        return ms.value / max(cnt.value, 1)

    def stats(v):
        return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}

    x0f, x1f = mf.FACE_BITS["x0"], mf.FACE_BITS["x1"]
    torch.cuda.synchronize()
    base = int(torch.cuda.memory_allocated())
    cm = mf.Context(torch.cuda.current_device())
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n), 2, 5, ctx=cm)
    if leg != "affine":  # a smooth map that leaves no element an affine image of the reference cell (tools/brick_operator_hex27_time.py's)
        c = distort_(*[brick.coords_view(d).clone() for d in range(3)])
        for d in range(3):
            brick.coords_view(d).copy_(c[d])
        del c
    sig = (0.01, 0.0, 0.0, 0.0, 0.0, 0.0)
    op = brick.elasticity_operator_hex27(LAM, MU, TAU, x0f, x1f, sig)
    th = brick.thermal_operator_hex27(K_COND, H, TENV, 0x3F)
    rows = op.n
    out["rows"] = rows
    g = torch.Generator(dev)
    x = torch.empty(rows, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g.manual_seed(1))
    b = torch.empty_like(x).uniform_(-1.0, 1.0, generator=g.manual_seed(2))
    y = torch.empty_like(x)
    xt, yt = x[: th.n], y[: th.n]
    product = lambda: op.mul_(y, x)
    thermal = lambda: th.mul_(yt, xt)
    for _ in range(3):  # warm
        product()
        thermal()
    knob(8 << 8, product)
    knob(2, product)
    op.diagonal()
    solver_spmv_ms(cm, op, b, 4)
    T = {k: [] for k in ("op", "thermal", "op_8_waves", "op_one_field", "op_in_solve", "diag")}
    for _ in range(reps):  # alternated
        T["op"].append(timed(product))
        T["thermal"].append(timed(thermal))
        T["op_8_waves"].append(knob(8 << 8, product))
        T["op_one_field"].append(knob(2, product))
        T["op_in_solve"].append(solver_spmv_ms(cm, op, b))
        T["diag"].append(timed(op.diagonal))
    m = {k: float(np.median(v)) for k, v in T.items()}
    out.update(product_ms=stats(T["op"]), thermal_hex27_product_ms=stats(T["thermal"]), product_8_waves_ms=stats(T["op_8_waves"]),
               product_one_field_stress_ms=stats(T["op_one_field"]), product_in_solve_ms=stats(T["op_in_solve"]), diagonal_ms=stats(T["diag"]),
               product_over_thermal=round(m["op"] / m["thermal"], 3), condition_A_bound=3.0, condition_A_met=bool(m["op"] <= 3.0 * m["thermal"]),
               ablation={"8_waves_over_thermal": round(m["op_8_waves"] / m["thermal"], 3), "one_field_stress_over_thermal": round(m["op_one_field"] / m["thermal"], 3),
                         "in_solve_with_dot_and_fold_over_product": round(m["op_in_solve"] / m["op"], 3)},
               diagonal_over_product=round(m["diag"] / m["op"], 2))
    for sv, name, s in ((mf.cg_, "cg", 0), (mf.idrs_, "idrs8", 8)):
        _, st = mf.iterative_Solve(op, None, b, 1e-300, Sv_func=sv, s=s, maxiter=200, max_pass=1, fixed_iterations=True)
        out[f"{name}200_solve_ms"], out[f"{name}200_final_res"] = round(float(st.solve_ms), 2), float(st.final_res)
    torch.cuda.synchronize()
    out["operator_bytes"] = int(torch.cuda.memory_allocated()) - base - 3 * 8 * rows + int(_lib.lib.mfem_debug_ws_bytes(cm._h))  # (without this tool's x, b, y)
    if mesh_leg:
        condition_b(out, mf, cm, brick, op, product, timed, stats, n, reps, leg, dev)
    out["cantilever"] = "not run"
    if cantilever:
        f = op.residual(torch.zeros_like(x))  # the load: K 0 + f
        tol = 1e-6 * float(f.norm()) / np.sqrt(rows)
        cap = int(60e3 / m["op_in_solve"])  # (a minute of products at the most)
        sol, st = mf.iterative_Solve(op, None, f, tol, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=min(20000, cap), max_pass=1)
        torch.cuda.synchronize()
        out["cantilever"] = {"tol_normalized": tol, "converged": int(st.converged), "iterations": int(st.iterations), "solve_s": round(float(st.solve_ms) / 1e3, 2),
                             "final_res": float(st.final_res), "max_abs_u": float(sol.abs().max()),
                             "bytes": int(torch.cuda.memory_allocated()) - base - 3 * 8 * rows + int(_lib.lib.mfem_debug_ws_bytes(cm._h))}
    return out


def condition_b(out, mf, cm, brick, op, product, timed, stats, n, reps, leg, dev):
    """the MeshOperator of the same form on the same lattice: time, bytes, and the energy cross-check"""
    import numpy as np
    import torch

    from metafem_jl_amd import element, generic as G, mesh as pm, physics as P

    torch.cuda.synchronize()
    before = int(torch.cuda.memory_allocated())
    try:
        space = element.classical_space(3, "Lagrange", 2, 5, shape="CUBE")
        vert, conn = pm.make_Brick((1.0, 1.0, 1.0), (n, n, n), "CUBE")
        msh = pm.mesh_Classical(vert, conn, space)
        fac = pm.get_BoundaryMesh(msh)
        x0 = fac.select(np.abs(fac.centroid[:, 0]) < 1e-9)
        coords = np.asarray(msh.coords, dtype=np.float64)
        if leg != "affine":
            coords = np.stack(distort_(coords[:, 0], coords[:, 1], coords[:, 2]), axis=1)
        gd = G.GenericDomain(cm, space, coords, msh.cp_ids, 3, P.elasticity_domain(3, LAM, MU), [(x0.element_ID, x0.element_eindex, P.penalty([0, 1, 2], TAU))],
                             matrix_free=True)
        gd.update_Time()
        gd.K_linear_func()
        assert gd.matrix_free and isinstance(gd.A, mf.MeshOperator) and gd.A.n == op.n, gd.matrix_free_reason
        smooth = lambda c: torch.cat([torch.sin(2 * c[0] + c[1]) * (1 + c[2]), torch.cos(c[1] - 3 * c[2]) + c[0], c[0] * c[1] - torch.sin(c[2])])
        xm = smooth([torch.tensor(np.ascontiguousarray(coords[:, d]), device=dev) for d in range(3)])
        xb = smooth([brick.coords_view(d).clone() for d in range(3)])
        ym, yb = torch.empty_like(xm), torch.empty_like(xb)
        mesh_product = lambda: mf.mul_(ym, gd.A, None, xm)
        mesh_product()
        op.mul_(yb, xb)
        em, eb = float(xm @ ym), float(xb @ yb)
        out["mesh_operator_energy_rel_diff"] = abs(em - eb) / abs(eb)
        for _ in range(2):
            mesh_product()
        T = {"op": [], "mesh": []}
        for _ in range(reps):  # alternated
            T["op"].append(timed(product))
            T["mesh"].append(timed(mesh_product))
        torch.cuda.synchronize()
        mo, mm = float(np.median(T["op"])), float(np.median(T["mesh"]))
        out.update(mesh_operator_product_ms=stats(T["mesh"]), product_beside_mesh_operator_ms=stats(T["op"]), mesh_operator_over_product=round(mm / mo, 2),
                   mesh_operator_bytes=int(torch.cuda.memory_allocated()) - before - 4 * 8 * op.n,  # (without this leg's xm, ym, xb, yb)
                   condition_B="met" if mo * 1.1 < mm else "condition not met")
        out["condition_B_rule"] = "product x 1.1 < MeshOperator product"
    except Exception as e:  # (an allocation that fails at this size is a result)
        out["condition_B"] = f"not run: {type(e).__name__}: {str(e)[:200]}"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    legs = (sys.argv[4] if len(sys.argv) > 4 else "affine,distorted").split(",")
    cantilever = sys.argv[5] if len(sys.argv) > 5 else "0"
    mesh = sys.argv[6] if len(sys.argv) > 6 else "1"
    results = []
    if os.path.exists(OUT):
        results = [r for r in json.load(open(OUT)) if not (r.get("n") == n and r.get("leg") in legs)]
    for leg in legs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps), leg, cantilever, mesh], stdout=subprocess.PIPE, text=True,
                               timeout=limit)
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
            print(json.dumps(child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5] == "1", sys.argv[6] == "1")), flush=True)
        except Exception as e:  # an allocation that fails is a result
            print(json.dumps({"leg": sys.argv[4], "n": int(sys.argv[2]), "failed": f"{type(e).__name__}: {str(e)[:300]}"}), flush=True)
        sys.exit(0)
    sys.exit(main())
