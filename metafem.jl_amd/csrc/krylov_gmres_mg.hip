// gmres! with the geometric multigrid V-cycle as its RIGHT preconditioner (MFEM_SOLVER_GMRES + MFEM_PRECOND_MULTIGRID on a hex-8 thermal brick operator
// with a hierarchy of mfem_brick_multigrid_create_nonsymmetric attached; the cycle: brick_multigrid.hip): restarted GMRES(s) on A M^-1 u = b,
// x = M^-1 u, M^-1 = one cycle -- a fixed linear operator, symmetric or not, so K may carry Nitsche (fixed_faces) rows.  The residual the Arnoldi
// process minimises is the TRUE one, b - A x.
//   per restart:  Q_1 = r / |r|, g = (|r|, 0, ...)
//     step k:     z = Cycle(Q_k) | w = A z | CGS2 of krylov_gmres_kernels.h against Q_1..Q_k into column k of H, Q_(k+1) = w / |w| |
//                 kgm_step: the stored Givens rotations on column k, the new rotation, g rotated; the estimate |g_(k+1)| of |b - A x|, the iteration
//                 count and the stop flag (the estimate meets the tolerance, the cap is reached, or H[k+1, k] == 0 exactly)
//     at a stop or at k = s:  kgm_solve: R y = g on the width reached | u = sum_j y_j Q_j (kgm_combine, j in order) | z = Cycle(u) | x += z |
//                 r = b - A x and the test on it; a failed test starts the next restart
// H, g, y and the rotations stay on the device; every sum goes through partials folded in a fixed order: the same bits on every run.  The host reads
// the flags after EVERY step, as krylov_cg_mg.hip does and for its reason: a cycle is some dozens of launches, and the step that stops must not be
// followed by one.  No graph is captured.  fixed_iterations runs exactly maxiter steps (short of an exact breakdown).
// Level-0 products of a pass (mfem_solve_stats.spmv_count, mg_gmres_pass_products): x0 + it (1 + c) + restarts (c + 1), c the cycle's level-0
// products; cycles = it + restarts.  Work vectors: r (which holds u between the least-squares solve and the true residual), Q_1..Q_(s+1), z.
#include "krylov_gmres_kernels.h"
#include "brick_multigrid.h"
#include "brick_multigrid_decide.h"

enum { S_GMG_C = S_SOLVER, S_GMG_S = S_SOLVER + MFEM_MAX_S, S_GMG_EST = S_SOLVER + 2 * MFEM_MAX_S };  // the rotations, the residual estimate
static_assert(S_GMG_EST < S_SOLVER + 100, "below the slots a multigrid setup reports its estimates in");
enum { F_GMG_STOP = 4, F_GMG_WIDTH = 5 };  // (the second bank of flags, which only the classic cg! alternates to): 1 stop, 2 exact breakdown; columns so far
static_assert(MG_GMRES_DEFAULT_S == 20 && MG_GMRES_MAX_S == MFEM_MAX_S, "brick_multigrid_decide.h states the restart lengths");

// one thread: the state a pass starts from (S[S_RR] holds r . r): nothing to do for a zero or a converged residual
__global__ void kgm_start(GmArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  F[F_DONE] = (S[S_RR] == 0.0 || kk_converged(a, S[S_RR])) ? 1 : 0;
  F[F_ITER] = 0;
  F[F_SPMV] = 0;
  F[F_GM_WIDTH] = 0;
  F[F_GMG_STOP] = 0;
  F[F_GMG_WIDTH] = 0;
}

// One wave, after step k0 + 1 (column k0, 0-based, rows 0 .. k0 + 1, is complete): the rotations of the earlier columns on it, its own rotation,
// g rotated, the estimate, the count and the stop flag.  The column goes back as column k0 of R.
__global__ __launch_bounds__(MFEM_WAVE) void kgm_step(GmArgs a, int k0, double* __restrict__ H, double* __restrict__ g, double* __restrict__ S,
                                                       int32_t* __restrict__ F) {
  __shared__ double col[GM_LD];
  const int t = threadIdx.x;
  double* Hc = H + GM_LD * k0;
  if (t <= k0 + 1) col[t] = Hc[t];
  __syncthreads();
  if (t == 0) {
    for (int j = 0; j < k0; ++j) {
      const double c = S[S_GMG_C + j], sn = S[S_GMG_S + j];
      const double tmp = -sn * col[j] + c * col[j + 1];
      col[j] = c * col[j] + sn * col[j + 1];
      col[j + 1] = tmp;
    }
    const bool breakdown = col[k0 + 1] == 0.0;  // (|w| itself: no rotation has touched the row yet)
    double c, sn;
    gm_givens(col[k0], col[k0 + 1], &c, &sn);
    col[k0] = c * col[k0] + sn * col[k0 + 1];
    col[k0 + 1] = 0.0;
    const double g0 = g[k0], g1 = g[k0 + 1];
    g[k0] = c * g0 + sn * g1;
    const double gn = -sn * g0 + c * g1;
    g[k0 + 1] = gn;
    S[S_GMG_C + k0] = c;
    S[S_GMG_S + k0] = sn;
    S[S_GMG_EST] = fabs(gn);
    const int iter = F[F_ITER] + 1;
    F[F_ITER] = iter;
    F[F_GMG_WIDTH] = k0 + 1;
    F[F_GMG_STOP] = breakdown ? 2 : ((kk_converged(a, gn * gn) || iter >= a.maxiter) ? 1 : 0);
  }
  __syncthreads();
  if (t <= k0 + 1) Hc[t] = col[t];
}

// One wave: R y = g on the width reached (R: the rotated columns of H, upper triangular), column by column as krylov_gmres.hip's back substitution;
// y[width .. s] = 0
__global__ __launch_bounds__(MFEM_WAVE) void kgm_solve(const double* __restrict__ H, const double* __restrict__ g, double* __restrict__ y, int s,
                                                        const int32_t* __restrict__ F) {
  __shared__ double h[GM_LD * MFEM_MAX_S];
  __shared__ double rhs[GM_LD];
  const int width = F[F_GMG_WIDTH];
  const int t = threadIdx.x;
  for (int i = t; i < GM_LD * width; i += MFEM_WAVE) h[i] = H[i];
  if (t < width) rhs[t] = g[t];
  __syncthreads();
  for (int j = width - 1; j >= 0; --j) {
    if (t == 0) rhs[j] = rhs[j] / h[j + GM_LD * j];
    __syncthreads();
    if (t < j) rhs[t] -= h[t + GM_LD * j] * rhs[j];
    __syncthreads();
  }
  if (t <= s) y[t] = t < width ? rhs[t] : 0.0;
}

// u = sum_j y_j Q_j, j < K, in the order of j
template <int K>
__global__ __launch_bounds__(MFEM_BLOCK) void kgm_combine(int64_t n2v, GmBasis B, const double* __restrict__ y, d2_t* __restrict__ u) {
  double c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c[j] = y[j];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2v; i += stride) {
    d2_t q[K];
#pragma unroll
    for (int j = 0; j < K; ++j) q[j] = KB_LD(B.q[j], i);
    d2_t acc = q[0] * c[0];
#pragma unroll
    for (int j = 1; j < K; ++j) acc += q[j] * c[j];
    u[i] = acc;
  }
}
static int gmg_combine(mfem_context_s* ctx, int G, int K, int64_t nv, const GmBasis& B, const double* y, double* u) {
  switch (K) {
#define GMG_CB(K_) case K_: hipLaunchKernelGGL(kgm_combine<K_>, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, nv / 2, B, y, (d2_t*)u); break;
    GM_CASES(GMG_CB)
#undef GMG_CB
    default: mfem_set_error("gmres: %d basis vectors", K); return MFEM_ERR_INVALID;
  }
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// one thread, after the true residual (S[S_RR] = r . r): the end of the pass, or the next restart
__global__ void kgm_final(GmArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  const double rr = S[S_RR];
  F[F_DONE] = (rr == 0.0 || kk_converged(a, rr) || F[F_ITER] >= a.maxiter || F[F_GMG_STOP] == 2) ? 1 : 0;
  F[F_GMG_STOP] = 0;
}

int mfem_gmres_mg_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int s, double tol,
                       int64_t n_global, int* iters_out, int* spmv_out) {
  mfem_brick_multigrid_s* mg = mfem_mg_of(A);
  MFEM_REQUIRE(mg, "no multigrid hierarchy is attached to the bound operator");
  MFEM_REQUIRE(s >= 1 && s <= MFEM_MAX_S, "gmres: 1 <= s <= 32 supported");
  MFEM_REQUIRE(!ctx->comm, "gmres: no multi-rank form (refused with a communicator attached)");
  MFEM_REQUIRE(V.nwork >= s + 3 && V.gm, "gmres: workspace");
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  const int64_t nv = V.nv, n = V.n;
  double* r = V.w[0];
  double** Q = V.w + 1;  // Q_1 .. Q_(s+1)
  double* z = V.w[s + 2];
  double* H = V.gm + GM_H;
  double* g = V.gm + GM_Y;
  double* h2 = V.gm + GM_H2;  // the second CGS pass's coefficients; after the last step of a restart: y
  double* part = V.gm + GM_PART;
  double* part_nrm = part + (int64_t)MFEM_MAX_S * MFEM_MAX_PARTIALS;
  const int G = mfem_vec_grid(ctx, nv);
  const GmArgs a{kk_args(tol, n_global, o), s};
  KK k{ctx, nv, n, G, S, F, ctx->stream};

  RC(mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out));
  K1(kgm_start, a, S, F);
  RC(mfem_read_flags(ctx));
  int it = 0, restarts = 0, cycles = 0;
  bool done = ctx->h_flags[F_DONE] != 0 || o->maxiter <= 0;
  GmBasis B;
  for (int j = 0; j < s; ++j) B.q[j] = (const d2_t*)Q[j];
  while (!done) {
    KV(kg_start, nv / 2, (const d2_t*)r, (d2_t*)Q[0], g, s, S, F);
    int width = 0;
    for (int kk = 1; kk <= s; ++kk) {
      RC(mfem_mg_cycle(ctx, mg, Q[kk - 1], z));
      ++cycles;
      RC(k.spmv(A, vals, z, Q[kk]));
      RC(gm_orthogonalise(ctx, G, kk, n, nv, B, Q[kk], H + GM_LD * (kk - 1), h2, part, part_nrm, F));
      hipLaunchKernelGGL(kgm_step, dim3(1), dim3(MFEM_WAVE), 0, ctx->stream, a, kk - 1, H, g, S, F);
      MFEM_CHECK_LAUNCH();
      ++it;
      width = kk;
      RC(mfem_read_flags(ctx));  // after every step (see the head of the file)
      if (ctx->h_flags[F_GMG_STOP]) break;
    }
    hipLaunchKernelGGL(kgm_solve, dim3(1), dim3(MFEM_WAVE), 0, ctx->stream, (const double*)H, (const double*)g, h2, s, (const int32_t*)F);
    MFEM_CHECK_LAUNCH();
    RC(gmg_combine(ctx, G, width, nv, B, h2, r));
    RC(mfem_mg_cycle(ctx, mg, r, z));
    ++cycles;
    RC(k.axpby(coef_imm(1.0), z, coef_imm(1.0), V.x));  // x += z
    RC(mfem_true_residual(ctx, A, vals, V.b, V.x, r, S + S_RR));
    ++restarts;
    K1(kgm_final, a, S, F);
    RC(mfem_read_flags(ctx));
    done = ctx->h_flags[F_DONE] != 0;
  }
  *iters_out = it;
  *spmv_out += it + restarts + cycles * mfem_mg_level0_products(mg);
  return MFEM_OK;
}
