"""One rank of tests/test_gpu_cg_ring.py::test_two_ranks_on_one_gpu (started `world` times on cuda:0).

The rank owns a slab of the hex-8 thermal brick (33 x 17 x 9 lattice points, cut along the first direction), attaches the host-callback communicator
(gloo moves the staged data: ranks that share a GPU cannot use RCCL) and solves with the classic CG recurrences -- plain Jacobi, z-carrying, scaled --
once with the ring of search directions off (m = 1) and once per depth m = 2, 3, 8, 16.  Every m > 1 solve must return this rank's x and the statistics
of the m = 1 solve bit for bit: fixed iteration counts around the ring's edges, a tolerance stop, a restart in mid-ring.  Exit code 0 = all equal.

usage: cg_ring_worker.py <world> <rank> <port>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
DEPTHS = [2, 3, 8, 16]


def main():
    world, rank, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib, parallel as par

    _lib.lib.mfem_debug_set_layout_min_rows(0, 0)  # the solver layouts on this small system (cg_variant 4 scales on the diagonal-slotted one)
    ctx = mf.Context(0)
    sb = mf.Brick((2.0, 1.0, 1.0), (32, 16, 8), 1, 3, ctx=ctx)
    m0, m1, m2 = sb.m
    lo, hi = par.slab_planes(m0, world, rank, 1)
    sb.set_slab(lo, hi)
    A = sb.pattern(1)
    nloc = par.local_vector_length(lo, hi, m1, m2, 1, 1)
    comm = par.HostSlabComm(ctx, sb, rank, world, n_fields=1, poison=True)
    K = sb.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    s_loc = torch.full((nloc,), SRC, dtype=torch.float64, device="cuda:0")
    R = sb.residual_thermal(torch.zeros(nloc, dtype=torch.float64, device="cuda:0"), K_COND, H, TENV, 0x3F, s=s_loc)

    def solve(m, tol, **kw):
        _lib.check(_lib.lib.mfem_debug_set_cg_ring(m))
        x, st = mf.iterative_Solve(A, K, R, tol, Sv_func=mf.cg_, **kw)
        return x.cpu().numpy().tobytes(), (st.passes, st.iterations, st.final_res, st.initial_res, st.converged, st.spmv_count)

    ring0 = int(_lib.lib.mfem_debug_cg_ring_count())
    res0 = solve(1, 1e-300, cg_variant=1, maxiter=0, max_pass=1)[1][3]  # the initial residual of the whole system
    compared, failed = 0, []
    for variant in (1, 3, 4):
        # every rank walks the same list of solves: each one holds collectives
        cases = [dict(maxiter=it, max_pass=1, fixed_iterations=True, check_every=5) for it in (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 19, 35)]
        cases += [dict(maxiter=4000, max_pass=1, check_every=ce) for ce in (5, 32)]  # a tolerance stop
        cases += [dict(maxiter=10, max_pass=2, check_every=32), dict(maxiter=25, max_pass=2, check_every=5)]  # 25: a restart in mid-ring for every depth
        for kw in cases:
            tol = 1e-6 * res0 if kw["maxiter"] == 4000 else 1e-300
            want = solve(1, tol, cg_variant=variant, **kw)
            for m in DEPTHS:
                got = solve(m, tol, cg_variant=variant, **kw)
                compared += 1
                if got != want:
                    failed.append({"variant": variant, "m": m, "case": kw, "stats": [list(got[1]), list(want[1])], "x_equal": got[0] == want[0]})
    _lib.lib.mfem_debug_set_cg_ring(0)
    ring_passes = int(_lib.lib.mfem_debug_cg_ring_count()) - ring0
    callbacks = comm.calls["exchange"] > 10 and comm.calls["allreduce"] > 10
    comm.close()
    dist.barrier()
    dist.destroy_process_group()
    print("CG_RING_REPORT " + json.dumps({"rank": rank, "compared": compared, "failed": failed[:8], "callbacks_ran": callbacks, "ring_passes": ring_passes}), flush=True)
    sys.exit(0 if not failed and callbacks and ring_passes >= compared else 1)


if __name__ == "__main__":
    main()
