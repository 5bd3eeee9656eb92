"""One rank of tests/test_gpu_symp_const.py::test_two_ranks_on_one_gpu (started `world` times on cuda:0).

The rank owns a slab of the hex-8 thermal brick on a dyadic lattice (Brick((0.25, 0.25, 1.0), (32, 32, 128)): h = 2^-7, 33 x 33 x 129 lattice points, cut
along the first direction), attaches the host-callback communicator (gloo moves the staged data: ranks that share a GPU cannot use RCCL) and runs a few
fixed CG iterations with Pr_Jacobi! -- cg_variant 4 and 1 -- on the patch sweep in its constant form (csrc/symp_const_decide.h; forced by bit 5 of the
"ell" knob: the slabs' share of interior steps lies under the gate), in its forced stored form
(bit 4 of the "ell" knob) and on the plain per-row kernel (bit 22), with one and two bands.  Every sweep's x must lie within 1e-10 * max |x| of the plain
kernel's on this rank, with the same statistics up to the residual's last digits; the constant form's x must be the stored form's byte for byte, and its
binds must have flagged steps and ended in the constant form.  Exit code 0 = all within.

usage: symp_const_worker.py <world> <rank> <port>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_COND, H, TENV, SRC = 0.6, 25.0, 293.15, 1600.0
B1, B2, PLAIN, TRIM, FORCE_STORED, FORCE_CONST = 1 << 24, 1 << 25, 1 << 22, 1 << 3, 1 << 4, 1 << 5
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
    sb = mf.Brick((0.25, 0.25, 1.0), (32, 32, 128), 1, 3, ctx=ctx)
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
        s0, c0 = int(_lib.lib.mfem_debug_sym_spmv_count()), int(_lib.lib.mfem_debug_symp_const_count())
        x, st = mf.iterative_Solve(A, K, R, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=iters, max_pass=1, fixed_iterations=True, cg_variant=variant)
        torch.cuda.synchronize()
        return (x.cpu().numpy(), (st.passes, st.iterations, st.spmv_count), st.final_res, int(_lib.lib.mfem_debug_sym_spmv_count()) - s0,
                int(_lib.lib.mfem_debug_symp_const_count()) - c0, int(_lib.lib.mfem_debug_symp_const_steps()))

    compared, failed, const_binds = 0, [], 0
    for variant in (4, 1):
        for iters in (3, 9):
            # every rank walks the same list of solves: each one holds collectives
            xp, stp, resp, symp, _, _ = solve(PLAIN, variant, iters)
            for bands in (B2, B1):
                x, st, res, sym, binds, steps = solve(bands | TRIM | FORCE_CONST, variant, iters)
                xs, sts, ress, syms, binds_s, steps_s = solve(bands | TRIM | FORCE_STORED, variant, iters)
                compared += 1
                const_binds += binds
                err = float(np.abs(x - xp).max() / np.abs(xp).max())
                ok = (np.all(np.isfinite(x)) and err <= TOL_X and st == stp and abs(res - resp) <= 1e-9 * abs(resp) and sym > 0 and syms > 0 and symp == 0
                      and binds > 0 and steps > 0 and binds_s == 0 and steps_s == 0 and x.tobytes() == xs.tobytes() and st == sts and res == ress)
                if not ok:
                    failed.append({"variant": variant, "iters": iters, "bands": hex(bands), "err": err, "stats": [list(st), list(stp), list(sts)],
                                   "res": [res, resp, ress], "sym": [sym, syms, symp], "binds": [binds, binds_s], "steps": [steps, steps_s],
                                   "same_bytes": x.tobytes() == xs.tobytes()})
    _lib.lib.mfem_debug_set_ell(1)
    callbacks = comm.calls["exchange"] > 10 and comm.calls["allreduce"] > 10
    comm.close()
    dist.barrier()
    dist.destroy_process_group()
    print("SYMP_CONST_REPORT " + json.dumps({"rank": rank, "compared": compared, "failed": failed[:8], "const_binds": const_binds, "callbacks_ran": callbacks}),
          flush=True)
    sys.exit(0 if not failed and callbacks else 1)


if __name__ == "__main__":
    main()
