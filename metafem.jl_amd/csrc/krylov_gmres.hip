// gmres!  -- restarted GMRES(s) (reference linear_solver/05_GMRES.jl:48-100, Hessenberg :7-37); what
// examples/linear_elasticity/stress_concentration/2D_Script.jl:63 selects (and 3D_Script.jl:68 as its alternative).
// Same cycle as the reference: Q1 = r / |r|, s Arnoldi steps, the (s+1) x s least-squares problem by Givens rotations,
// x += Q y, the true residual r = b - A x, and the stop test on it -- only at the end of a cycle.  Every scalar stays on
// the device (H, y and the rotations in a small region of the solve workspace) and the kernels are DONE-guarded, so a
// whole cycle has constant kernel arguments and is captured and replayed as one graph.
//
// Orthogonalisation: classical Gram-Schmidt applied twice (CGS2) instead of the reference's modified Gram-Schmidt order.
// One pass of step k = one block dot  h = Q_(1..k)' w  (a single read of the k basis vectors and w, k partials per
// workgroup), a one-workgroup fold into H's column, and one fused update  w -= Q h  -- (2k + 3) n 8 B and 2 reductions
// per step where the MGS order moves 5 k n 8 B through k dependent reductions.  The second pass's update also leaves
// the partials of |w|^2; one grid kernel folds them (every workgroup the same sum), writes H[k+1, k], flags an exact
// breakdown and scales w.  mfem_debug_set("gmres", 1, 0) runs the reference's MGS order instead (one dot, then one axpy,
// per basis vector) for step-by-step comparison with the oracle.
#include "krylov_gmres_kernels.h"

size_t mfem_gmres_workspace_bytes() { return sizeof(double) * (size_t)GM_DOUBLES; }

// r = b - A x is in place and S[S_RR] = r.r: iter = 1, or 0 iterations if normalized_norm(r) <= tol (:49-52)
__global__ void kg_init(GmArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  kk_start(S[S_RR] == 0.0 || kk_converged(a, S[S_RR]), F);
  F[F_GM_WIDTH] = 0;
}

// Hessenberg(H, y) (:7-37) on the cycle's width columns (s, or k after an exact breakdown at step k): Givens rotations to upper triangular,
// applied to y as well, then the back substitution.  One wave; column t of H belongs to lane t.  y[width..s] = 0 on return.
__global__ __launch_bounds__(MFEM_WAVE) void kg_lsq(double* __restrict__ H, double* __restrict__ y, int s, const int32_t* __restrict__ F) {
  __shared__ double h[GM_LD * MFEM_MAX_S];
  __shared__ double rhs[GM_LD];
  __shared__ double rot[2];
  if (F[F_DONE]) return;
  const int width = F[F_GM_WIDTH] ? F[F_GM_WIDTH] : s;
  const int t = threadIdx.x;
  for (int i = t; i < GM_LD * width; i += MFEM_WAVE) h[i] = H[i];
  if (t <= width) rhs[t] = y[t];
  __syncthreads();
  for (int i = 0; i < width; ++i) {
    if (t == 0) {
      double c, sn;
      gm_givens(h[i + GM_LD * i], h[i + 1 + GM_LD * i], &c, &sn);
      h[i + GM_LD * i] = c * h[i + GM_LD * i] + sn * h[i + 1 + GM_LD * i];
      const double tmp = -sn * rhs[i] + c * rhs[i + 1];
      rhs[i] = c * rhs[i] + sn * rhs[i + 1];
      rhs[i + 1] = tmp;
      rot[0] = c;
      rot[1] = sn;
    }
    __syncthreads();
    if (t > i && t < width) {
      const double c = rot[0], sn = rot[1];
      double* col = h + GM_LD * t;
      const double tmp = -sn * col[i] + c * col[i + 1];
      col[i] = c * col[i] + sn * col[i + 1];
      col[i + 1] = tmp;
    }
    __syncthreads();
  }
  for (int j = width - 1; j >= 0; --j) {  // ldiv!(UpperTriangular(H[1:width, 1:width]), y[1:width]), column by column
    if (t == 0) rhs[j] = rhs[j] / h[j + GM_LD * j];
    __syncthreads();
    if (t < j) rhs[t] -= h[t + GM_LD * j] * rhs[j];
    __syncthreads();
  }
  if (t <= s) y[t] = t < width ? rhs[t] : 0.0;
}

// x += y_j Q_j, j < K, in the order of j (:83-85; columns past an exact breakdown carry y_j = 0)
template <int K>
__global__ __launch_bounds__(MFEM_BLOCK) void kg_xupdate(int64_t n2v, GmBasis B, const double* __restrict__ y, d2_t* __restrict__ x,
                                                         const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  double c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c[j] = y[j];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2v; i += stride) {
    d2_t q[K];
#pragma unroll
    for (int j = 0; j < K; ++j) q[j] = KB_LD(B.q[j], i);
    d2_t acc = KB_LD(x, i);
#pragma unroll
    for (int j = 0; j < K; ++j) acc += q[j] * c[j];
    x[i] = acc;
  }
}

// before the true residual: iter += s, or iter += width and return after an exact breakdown (:74-76, :87)
__global__ void kg_cycle_end(GmArgs a, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const int width = F[F_GM_WIDTH];
  if (width) {
    F[F_ITER] += width;
    F[F_SPMV] += width;
    F[F_DONE] = 1;
    return;
  }
  F[F_ITER] += a.s;
}
// after it (S[S_RR] = r.r): stop if normalized_norm(r) <= tol || iter > maxiter (:91)
__global__ void kg_cycle_test(GmArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  F[F_SPMV] += a.s + 1;
  if (kk_converged(a, S[S_RR]) || F[F_ITER] > a.maxiter) F[F_DONE] = 1;
}

static std::atomic<int> g_gmres_literal{0};
extern "C" int mfem_debug_set_gmres(int literal_mgs) try {
  ++mfem_debug_epoch;
  g_gmres_literal = literal_mgs ? 1 : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_gmres")

static int gm_xupdate(mfem_context_s* ctx, int G, int K, int64_t nv, const GmBasis& B, const double* y, double* x, const int32_t* F) {
  switch (K) {
#define GM_XU(K_) case K_: hipLaunchKernelGGL(kg_xupdate<K_>, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, nv / 2, B, y, (d2_t*)x, F); break;
    GM_CASES(GM_XU)
#undef GM_XU
    default: mfem_set_error("gmres: %d basis vectors", K); return MFEM_ERR_INVALID;
  }
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

int mfem_gmres_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int s, double tol,
                    int64_t n_global, int* iters_out, int* spmv_out) {
  MFEM_REQUIRE(s >= 1 && s <= MFEM_MAX_S, "gmres: 1 <= s <= 32 supported");
  MFEM_REQUIRE(!ctx->comm, "gmres: no multi-rank form (refused with a communicator attached)");
  MFEM_REQUIRE(V.nwork >= s + 2 && V.gm, "gmres: workspace");
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  const int64_t nv = V.nv, n = V.n;
  double* r = V.w[0];
  double** Q = V.w + 1;  // Q_1 .. Q_(s+1)
  double* H = V.gm + GM_H;
  double* y = V.gm + GM_Y;
  double* h2 = V.gm + GM_H2;
  double* part = V.gm + GM_PART;
  double* part_nrm = part + (int64_t)MFEM_MAX_S * MFEM_MAX_PARTIALS;
  const int G = mfem_vec_grid(ctx, nv);
  const bool literal = g_gmres_literal != 0;
  const GmArgs a{kk_args(tol, n_global, o), s};
  KK k{ctx, nv, n, G, S, F, ctx->stream};

  RC(mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out));  // :49-51
  K1(kg_init, a, S, F);
  // one cycle: s Arnoldi steps (s SpMVs), the least-squares solve, x += Q y and the true residual -- constant kernel arguments
  auto cycle = [&](int) -> int {
    KV(kg_start, nv / 2, (const d2_t*)r, (d2_t*)Q[0], y, s, S, F);
    GmBasis B;
    for (int j = 0; j < s; ++j) B.q[j] = (const d2_t*)Q[j];
    for (int kk = 1; kk <= s; ++kk) {  // Q_(kk+1) = A Q_kk, orthogonalised against Q_1..Q_kk into column kk of H (:61-80)
      double* w = Q[kk];
      double* col = H + GM_LD * (kk - 1);
      RC(k.spmv(A, vals, Q[kk - 1], w));
      if (!literal) {  // CGS2 and the normalisation (krylov_gmres_kernels.h)
        RC(gm_orthogonalise(ctx, G, kk, n, nv, B, w, col, h2, part, part_nrm, F));
        continue;
      }
      {  // the reference's order: for each j one dot product, then one update (:65-68)
        for (int j = 0; j < kk; ++j) {
          GmBasis Bj;
          Bj.q[0] = (const d2_t*)Q[j];
          RC(gm_block_dot(ctx, G, 1, n, Bj, w, part, F));
          hipLaunchKernelGGL(kg_fold, dim3(1), dim3(GM_FOLD_BLOCK), 0, ctx->stream, part, G, 1, col + j, (double*)nullptr, F);
          MFEM_CHECK_LAUNCH();
          RC(gm_update(ctx, G, 1, false, n, nv, Bj, col + j, w, nullptr, F));
        }
        GmBasis Bw;
        Bw.q[0] = (const d2_t*)w;
        RC(gm_block_dot(ctx, G, 1, n, Bw, w, part, F));  // |w|^2 (:71)
      }
      hipLaunchKernelGGL(kg_normalize, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, nv / 2, (const double*)part, G, col + kk, kk, (d2_t*)w, F);
      MFEM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(kg_lsq, dim3(1), dim3(MFEM_WAVE), 0, ctx->stream, H, y, s, F);  // Hessenberg(H, y) (:82)
    MFEM_CHECK_LAUNCH();
    RC(gm_xupdate(ctx, G, s, nv, B, y, V.x, F));
    K1(kg_cycle_end, a, F);
    // r = b - A x (:88-90).  Not DONE-guarded, which is harmless: once DONE is set x no longer changes, so it recomputes the same r.
    RC(mfem_true_residual(ctx, A, vals, V.b, V.x, r, S + S_RR));
    K1(kg_cycle_test, a, S, F);
    return MFEM_OK;
  };
  uint64_t key = mfem_pass_key(MFEM_SOLVER_GMRES, A, vals, V, tol, n_global, o);
  key = mfem_hash(key, s); key = mfem_hash(key, V.gm); key = mfem_hash(key, (int)literal);
  // (kg_cycle_test stops once the iteration count passes maxiter; check_every counts iterations, a poll every ceil(check / s) cycles)
  return kk_drive(ctx, o, key, s, (int64_t)o->maxiter + 1, cycle, kc_main, iters_out, spmv_out);
}
