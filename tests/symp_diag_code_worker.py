"""One rank of tests/test_gpu_symp_diag_code.py::test_two_ranks_on_one_gpu (started `world` times on cuda:0).

The rank owns a slab of a hex-8 thermal brick (48 x 20 x 40 lattice points, cut along the first direction: 24 planes per rank, enough for the slot-major
layout and four swept planes between the ghost planes), attaches the host-callback communicator (gloo moves the staged data: ranks that share a GPU
cannot use RCCL) and solves with the scaled CG (cg_variant 4) once on the coded-diagonal copy of the patch sweep and once with the stored form forced (bit 21
of the "ell" knob), for one and two bands, ring depth 1 and 8: x and the statistics must be the same bit for bit, and every unforced solve must have bound
the coded form.  Exit code 0 = all equal.

usage: symp_diag_code_worker.py <world> <rank> <port>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
B1, B2, STORED = 1 << 24, 1 << 25, 1 << 21


def main():
    world, rank, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib, parallel as par

    _lib.lib.mfem_debug_set_layout_min_rows(0, 0)
    ctx = mf.Context(0)
    sb = mf.Brick((2.0, 1.0, 1.0), (47, 19, 39), 1, 3, ctx=ctx)
    m0, m1, m2 = sb.m
    lo, hi = par.slab_planes(m0, world, rank, 1)
    sb.set_slab(lo, hi)
    A = sb.pattern(1)
    nloc = par.local_vector_length(lo, hi, m1, m2, 1, 1)
    comm = par.HostSlabComm(ctx, sb, rank, world, n_fields=1, poison=True)
    K = sb.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    s_loc = torch.full((nloc,), SRC, dtype=torch.float64, device="cuda:0")
    R = sb.residual_thermal(torch.zeros(nloc, dtype=torch.float64, device="cuda:0"), K_COND, H, TENV, 0x3F, s=s_loc)

    def solve(word, ring, iters):
        _lib.check(_lib.lib.mfem_debug_set_ell(1 | word))
        _lib.check(_lib.lib.mfem_debug_set_cg_ring(ring))
        c0, s0 = int(_lib.lib.mfem_debug_symp_coded_count()), int(_lib.lib.mfem_debug_sym_spmv_count())
        x, st = mf.iterative_Solve(A, K, R, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=iters, max_pass=1, fixed_iterations=True, cg_variant=4)
        stats = (st.passes, st.iterations, st.final_res, st.initial_res, st.converged, st.spmv_count)
        return (x.cpu().numpy().tobytes(), repr(stats)), int(_lib.lib.mfem_debug_symp_coded_count()) - c0, int(_lib.lib.mfem_debug_sym_spmv_count()) - s0

    compared, coded_binds, failed = 0, 0, []
    for bands in (B1, B2):   # every rank walks the same list of solves: each one holds collectives
        for ring in (1, 8):
            for iters in (12, 40):
                got, nc, swept = solve(bands, ring, iters)
                want, ns, swept_s = solve(bands | STORED, ring, iters)
                compared += 1
                coded_binds += nc
                if got != want or nc != 1 or ns != 0 or swept <= 0 or swept_s <= 0:
                    failed.append({"bands": bands >> 24, "ring": ring, "iters": iters, "coded_binds": [nc, ns], "sweeps": [swept, swept_s], "x_equal": got[0] == want[0],
                                   "stats": [got[1], want[1]]})
    _lib.lib.mfem_debug_set_ell(1)
    _lib.lib.mfem_debug_set_cg_ring(0)
    callbacks = comm.calls["exchange"] > 10 and comm.calls["allreduce"] > 10
    comm.close()
    dist.barrier()
    dist.destroy_process_group()
    print("DIAG_CODE_REPORT " + json.dumps({"rank": rank, "compared": compared, "coded_binds": coded_binds, "failed": failed[:8], "callbacks_ran": callbacks}), flush=True)
    sys.exit(0 if not failed and callbacks else 1)


if __name__ == "__main__":
    main()
