"""One rank of tests/test_gpu_symp_trim.py::test_two_ranks_on_one_gpu (started `world` times on cuda:0).

The rank owns a slab of the hex-8 thermal brick (64 x 17 x 33 lattice points, cut along the first direction), attaches the host-callback communicator
(gloo moves the staged data: ranks that share a GPU cannot use RCCL) and runs a few fixed CG iterations with Pr_Jacobi! -- cg_variant 4, 3 and 1 -- on the
trimmed patch sweep (bit 3 of the "ell" knob: the rim rows go with the boundary part of the split SpMV), on the untrimmed one (bit 2) and on the plain
per-row kernel (bit 22), with one and two bands.  Every sweep's x must lie within 1e-10 * max |x| of the plain kernel's on this rank, with the same
statistics up to the residual's last digits, and the trimmed binds must have had rim rows.  Exit code 0 = all within.

usage: symp_trim_worker.py <world> <rank> <port>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
B1, B2, PLAIN, UNTRIMMED, TRIM = 1 << 24, 1 << 25, 1 << 22, 1 << 2, 1 << 3
TOL_X = 1e-10


def main():
    world, rank, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    import numpy as np
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib, parallel as par

    _lib.lib.mfem_debug_set_layout_min_rows(0, 0)
    ctx = mf.Context(0)
    sb = mf.Brick((2.0, 1.0, 1.0), (63, 16, 32), 1, 3, ctx=ctx)
    m0, m1, m2 = sb.m
    lo, hi = par.slab_planes(m0, world, rank, 1)
    sb.set_slab(lo, hi)
    A = sb.pattern(1)
    nloc = par.local_vector_length(lo, hi, m1, m2, 1, 1)
    comm = par.HostSlabComm(ctx, sb, rank, world, n_fields=1, poison=True)
    K = sb.assemble_thermal(A, K_COND, H, TENV, 0x3F)
    s_loc = torch.full((nloc,), SRC, dtype=torch.float64, device="cuda:0")
    R = sb.residual_thermal(torch.zeros(nloc, dtype=torch.float64, device="cuda:0"), K_COND, H, TENV, 0x3F, s=s_loc)

    def solve(word, variant, iters):
        _lib.check(_lib.lib.mfem_debug_set_ell(1 | word))
        s0, t0 = int(_lib.lib.mfem_debug_sym_spmv_count()), int(_lib.lib.mfem_debug_symp_trim_count())
        x, st = mf.iterative_Solve(A, K, R, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=iters, max_pass=1, fixed_iterations=True, cg_variant=variant)
        torch.cuda.synchronize()
        return (x.cpu().numpy(), (st.passes, st.iterations, st.spmv_count), st.final_res, int(_lib.lib.mfem_debug_sym_spmv_count()) - s0,
                int(_lib.lib.mfem_debug_symp_trim_count()) - t0)

    compared, failed = 0, []
    for variant in (4, 3, 1):
        for iters in (3, 9):
            # every rank walks the same list of solves: each one holds collectives
            xp, stp, resp, symp, _ = solve(PLAIN, variant, iters)
            for word in (B2 | TRIM, B1 | TRIM, B2 | UNTRIMMED, B2 | TRIM | 1 << 26):
                x, st, res, sym, trims = solve(word, variant, iters)
                compared += 1
                err = float(np.abs(x - xp).max() / np.abs(xp).max())
                ok = (np.all(np.isfinite(x)) and err <= TOL_X and st == stp and abs(res - resp) <= 1e-9 * abs(resp) and sym > 0 and symp == 0
                      and (trims > 0) == bool(word & TRIM))
                if not ok:
                    failed.append({"variant": variant, "iters": iters, "word": hex(word), "err": err, "stats": [list(st), list(stp)], "res": [res, resp],
                                   "sym": sym, "trims": trims})
    _lib.lib.mfem_debug_set_ell(1)
    callbacks = comm.calls["exchange"] > 10 and comm.calls["allreduce"] > 10
    comm.close()
    dist.barrier()
    dist.destroy_process_group()
    print("SYMP_TRIM_REPORT " + json.dumps({"rank": rank, "compared": compared, "failed": failed[:8], "callbacks_ran": callbacks}), flush=True)
    sys.exit(0 if not failed and callbacks else 1)


if __name__ == "__main__":
    main()
