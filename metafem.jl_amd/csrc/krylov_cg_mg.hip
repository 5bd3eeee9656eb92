// cg! with the geometric multigrid V-cycle as its preconditioner (MFEM_PRECOND_MULTIGRID; the cycle: brick_multigrid.hip): the classic PCG
// recurrence with z = Cycle(0, r), a fixed symmetric positive operator.  The fused, ring-carrying mfem_cg_pass (krylov_cg.hip) is not involved.
//   per iteration:  A p (+ p . A p partials, dotw = p as the Jacobi pass asks for them) | x += alpha p, r -= alpha A p (+ r . r partials) | the stop test |
//                   z = Cycle(r) | r . z | p = z + beta p
// Scalars and the stop flag stay on the device; every sum goes through the partial sums and their folds in a fixed order.  The host reads the flag
// after EVERY iteration, whatever check_every says: a cycle is some dozens of launches and far more work than the read, and an iteration that stops
// the pass must not launch a cycle.  No cycle graph is captured.  fixed_iterations runs exactly maxiter iterations.
// Level-0 products of a pass (mfem_solve_stats.spmv_count, mg_pass_products): x0 + it + c it for it >= 1 -- one A p per iteration and one cycle of
// c = 2 nu products (nu_c - 1 on a brick that does not coarsen) per iteration, the first before iteration 1, none after the last -- and x0 for it = 0;
// the restart wrapper adds the true residual's.
#include "krylov.h"
#include "brick_multigrid.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

struct CgMgArgs {
  int64_t n2;    // padded length / 2
  double n_inv;  // 1 / n
  double tol;
  int32_t maxiter, fixed;
};

// one thread: the state a pass starts from (S[S_RR] holds r . r)
__global__ void k_cgmg_start(CgMgArgs a, const double* __restrict__ S, int32_t* __restrict__ flags) {
  flags[F_ITER] = 0;
  flags[F_DONE] = (!a.fixed && sqrt(S[S_RR] * a.n_inv) <= a.tol) ? 1 : 0;
}

// p = z + beta p, beta = r . z / (the previous r . z): S[S_TMP0] holds the new r . z, S[S_RZ0 + (wr ^ 1)] the previous one; first: p = z.  Workgroup 0
// leaves the new value in S[S_RZ0 + wr], a slot no workgroup of this kernel reads.
__global__ __launch_bounds__(MFEM_BLOCK) void k_cgmg_p(CgMgArgs a, int first, int wr, const d2_t* __restrict__ z, d2_t* __restrict__ p, double* __restrict__ S) {
  const double rz = S[S_TMP0];
  const double beta = first ? 0.0 : rz / S[S_RZ0 + (wr ^ 1)];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) p[i] = first ? z[i] : z[i] + beta * p[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) S[S_RZ0 + wr] = rz;
}

// alpha = r . z / p . A p ; x += alpha p ; r -= alpha A p ; partials of r . r
__global__ __launch_bounds__(MFEM_BLOCK) void k_cgmg_update(CgMgArgs a, int cur, const double* __restrict__ pap_partials, int np, const d2_t* __restrict__ p,
                                                              const d2_t* __restrict__ Ap, d2_t* __restrict__ x, d2_t* __restrict__ r,
                                                              const double* __restrict__ S, double* __restrict__ partials) {
  __shared__ double red[4];
  const double pap = reduce_partials_bcast(pap_partials, np, red);
  const double alpha = S[S_RZ0 + cur] / pap;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double rr = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
    x[i] = x[i] + alpha * p[i];
    const d2_t rv = r[i] - alpha * Ap[i];
    r[i] = rv;
    rr += rv.x * rv.x + rv.y * rv.y;
  }
  const double s = block_reduce_sum(rr, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one workgroup: r . r, the iteration count and the stop flag
__global__ __launch_bounds__(MFEM_BLOCK) void k_cgmg_check(CgMgArgs a, const double* __restrict__ partials, int np, double* __restrict__ S, int32_t* __restrict__ flags) {
  __shared__ double red[4];
  const double rr = reduce_partials_bcast(partials, np, red);
  if (threadIdx.x != 0) return;
  S[S_RR] = rr;
  const int iter = flags[F_ITER] + 1;
  flags[F_ITER] = iter;
  flags[F_DONE] = ((!a.fixed && sqrt(rr * a.n_inv) <= a.tol) || iter >= a.maxiter) ? 1 : 0;
}

int mfem_cg_mg_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int, double tol, int64_t n_global,
                    int* iters_out, int* spmv_out) {
  mfem_brick_multigrid_s* mg = mfem_mg_of(A);
  MFEM_REQUIRE(mg, "no multigrid hierarchy is attached to the bound operator");
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  double *r = V.w[0], *p = V.w[1], *Ap = V.w[2], *z = V.w[3];
  CgMgArgs a;
  a.n2 = V.nv / 2;
  a.n_inv = 1.0 / (double)n_global;
  a.tol = tol;
  a.maxiter = o->maxiter;
  a.fixed = o->fixed_iterations;
  double* part1 = ctx->d_partials;                     // p . A p, from the product
  double* part2 = ctx->d_partials + MFEM_MAX_PARTIALS;  // r . r
  int rc = mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out);
  if (rc) return rc;
  hipLaunchKernelGGL(k_cgmg_start, dim3(1), dim3(1), 0, ctx->stream, a, (const double*)S, F);
  MFEM_CHECK_LAUNCH();
  rc = mfem_read_flags(ctx);
  if (rc) return rc;
  const int G = mfem_vec_grid(ctx, V.nv);
  int it = 0, cycles = 0;
  bool done = ctx->h_flags[F_DONE] != 0 || o->maxiter <= 0;
  while (!done) {
    // z = Cycle(r); p = z (+ beta p)
    rc = mfem_mg_cycle(ctx, mg, r, z);
    if (rc) return rc;
    ++cycles;
    rc = mfem_dot_device(ctx, V.n, r, z, S + S_TMP0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cgmg_p, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, it == 0 ? 1 : 0, it & 1, (const d2_t*)z, (d2_t*)p, S);
    MFEM_CHECK_LAUNCH();
    int np1 = 0;
    rc = mfem_spmv_launch(ctx, A, vals, p, Ap, 1.0, 0.0, p, part1, &np1, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cgmg_update, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, it & 1, (const double*)part1, np1, (const d2_t*)p, (const d2_t*)Ap, (d2_t*)V.x,
                       (d2_t*)r, (const double*)S, part2);
    MFEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cgmg_check, dim3(1), dim3(MFEM_BLOCK), 0, ctx->stream, a, (const double*)part2, G, S, F);
    MFEM_CHECK_LAUNCH();
    ++it;
    rc = mfem_read_flags(ctx);  // after every iteration (see the head of the file)
    if (rc) return rc;
    done = ctx->h_flags[F_DONE] != 0;
  }
  *iters_out = it;
  *spmv_out += it + cycles * mfem_mg_level0_products(mg);
  return MFEM_OK;
}
