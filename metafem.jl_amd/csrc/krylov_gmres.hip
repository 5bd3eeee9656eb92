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
#include "krylov_kernels.h"

#define GM_LD (MFEM_MAX_S + 1)  // leading dimension of H (column-major, rows 0..s)
enum {
  GM_H = 0,                            // H[j + GM_LD * c], (s+1) x s
  GM_Y = GM_LD * MFEM_MAX_S,           // y (right-hand side / solution of the least-squares problem), s + 1
  GM_H2 = GM_Y + GM_LD,                // the second CGS pass's coefficients of the current step
  GM_PART = 1152,                      // block-dot partials, row j at GM_PART + j * MFEM_MAX_PARTIALS; row MFEM_MAX_S: |w|^2
  GM_DOUBLES = GM_PART + (MFEM_MAX_S + 1) * MFEM_MAX_PARTIALS
};
static_assert(GM_H2 + GM_LD <= GM_PART, "gmres region layout");
size_t mfem_gmres_workspace_bytes() { return sizeof(double) * (size_t)GM_DOUBLES; }

enum { F_GM_WIDTH = F_AUX };  // columns of the cycle after an exact breakdown (0: none)

struct GmArgs : KrylovArgs {
  int32_t s;
};
struct GmBasis {
  const d2_t* q[MFEM_MAX_S];
};

// r = b - A x is in place and S[S_RR] = r.r: iter = 1, or 0 iterations if normalized_norm(r) <= tol (:49-52)
__global__ void kg_init(GmArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  kk_start(S[S_RR] == 0.0 || kk_converged(a, S[S_RR]), F);
  F[F_GM_WIDTH] = 0;
}

// y = 0, y[1] = |r| ; Q1 = r / |r|  (:56-58, :94-96)
__global__ __launch_bounds__(MFEM_BLOCK) void kg_start(int64_t n2v, const d2_t* __restrict__ r, d2_t* __restrict__ q1, double* __restrict__ y,
                                                       int s, const double* __restrict__ S, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const double nr = sqrt(S[S_RR]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int j = 0; j <= s; ++j) y[j] = 0.0;
    y[0] = nr;
    F[F_GM_WIDTH] = 0;
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2v; i += stride) q1[i] = r[i] / nr;
}

// part[j * MFEM_MAX_PARTIALS + blockIdx] = partial of Q_j . w, j < K: one read of the K basis vectors and w.  Only the first n entries count.
template <int K>
__global__ __launch_bounds__(MFEM_BLOCK) void kg_block_dot(int64_t n, GmBasis B, const d2_t* __restrict__ w, double* __restrict__ part,
                                                           const int32_t* __restrict__ F) {
  __shared__ double red[K][MFEM_BLOCK / MFEM_WAVE];
  if (F[F_DONE]) return;
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += stride) {
    const d2_t wi = KB_LD(w, i);
    d2_t q[K];
#pragma unroll
    for (int j = 0; j < K; ++j) q[j] = KB_LD(B.q[j], i);
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] += q[j].x * wi.x + q[j].y * wi.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd n: the last entry shares its 16 bytes with the first pad entry
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] += B.q[j][n2].x * w[n2].x;
  }
  const int lane = threadIdx.x & (MFEM_WAVE - 1), wv = threadIdx.x / MFEM_WAVE;
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = wave_reduce_sum(acc[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) red[j][wv] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double v = 0.0;
    for (int i = 0; i < MFEM_BLOCK / MFEM_WAVE; ++i) v += red[threadIdx.x][i];
    part[(int64_t)threadIdx.x * MFEM_MAX_PARTIALS + blockIdx.x] = v;
  }
}

// One workgroup: out[j] = sum of the G partials of row j (fixed order), j < K; add_to[j] += out[j] when add_to is given.  One wave per row.
#define GM_FOLD_BLOCK 1024
__global__ __launch_bounds__(GM_FOLD_BLOCK) void kg_fold(const double* __restrict__ part, int G, int K, double* __restrict__ out,
                                                         double* __restrict__ add_to, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const int lane = threadIdx.x & (MFEM_WAVE - 1), wv = threadIdx.x / MFEM_WAVE;
  for (int j = wv; j < K; j += GM_FOLD_BLOCK / MFEM_WAVE) {
    const double* p = part + (int64_t)j * MFEM_MAX_PARTIALS;
    double acc = 0.0;
    for (int i = lane; i < G; i += 4 * MFEM_WAVE) {  // four loads in flight, added in the order of the plain loop
      const double v0 = p[i], v1 = i + MFEM_WAVE < G ? p[i + MFEM_WAVE] : 0.0, v2 = i + 2 * MFEM_WAVE < G ? p[i + 2 * MFEM_WAVE] : 0.0,
                   v3 = i + 3 * MFEM_WAVE < G ? p[i + 3 * MFEM_WAVE] : 0.0;
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) {
      out[j] = acc;
      if (add_to) add_to[j] += acc;
    }
  }
}

// w -= sum_j h[j] Q_j, j < K (in the order of j).  NORM: the partials of |w|^2 (new w, first n entries) to part_nrm[blockIdx].
template <int K, bool NORM>
__global__ __launch_bounds__(MFEM_BLOCK) void kg_update(int64_t n, int64_t n2v, GmBasis B, const double* __restrict__ h, d2_t* __restrict__ w,
                                                        double* __restrict__ part_nrm, const int32_t* __restrict__ F) {
  __shared__ double red[MFEM_BLOCK / MFEM_WAVE];
  if (F[F_DONE]) return;
  double c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c[j] = h[j];
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
  double nacc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2v; i += stride) {
    d2_t q[K];
#pragma unroll
    for (int j = 0; j < K; ++j) q[j] = KB_LD(B.q[j], i);
    d2_t acc = KB_LD(w, i);
#pragma unroll
    for (int j = 0; j < K; ++j) acc -= c[j] * q[j];
    w[i] = acc;
    if constexpr (NORM) {
      if (i < n2) nacc += acc.x * acc.x + acc.y * acc.y;
      else if (i == n2 && (n & 1)) nacc += acc.x * acc.x;
    }
  }
  if constexpr (NORM) {
    const double sum = block_reduce_sum(nacc, red);
    if (threadIdx.x == 0) part_nrm[blockIdx.x] = sum;
  }
}

// H[k+1, k] = |w| (every workgroup folds the same G partials in the same order); an exact zero is the reference's "problem exactly solved"
// (:69): the cycle's width becomes k and w is left as it is (zero).  Otherwise w /= |w| (:79).
__global__ __launch_bounds__(MFEM_BLOCK) void kg_normalize(int64_t n2v, const double* __restrict__ part_nrm, int G, double* __restrict__ hsub, int k,
                                                           d2_t* __restrict__ w, int32_t* __restrict__ F) {
  __shared__ double red[MFEM_BLOCK / MFEM_WAVE];
  if (F[F_DONE]) return;
  const double nrm = sqrt(reduce_partials_bcast(part_nrm, G, red));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *hsub = nrm;
    if (nrm == 0.0 && F[F_GM_WIDTH] == 0) F[F_GM_WIDTH] = k;
  }
  if (nrm == 0.0) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2v; i += stride) w[i] = w[i] / nrm;
}

// LinearAlgebra.givensAlgorithm (LAPACK dlartg): c, s with [c s; -s c] [f; g] = [r; 0]
__device__ void gm_givens(double f, double g, double* cs, double* sn) {
  const double safmn2 = 0x1p-511, safmx2 = 0x1p511;  // floatmin2(Float64) and its inverse
  if (g == 0.0) { *cs = 1.0; *sn = 0.0; return; }
  if (f == 0.0) { *cs = 0.0; *sn = 1.0; return; }
  double f1 = f, g1 = g, scale = fmax(fabs(f1), fabs(g1)), c, s;
  if (scale >= safmx2) {
    int count = 0;
    do { ++count; f1 *= safmn2; g1 *= safmn2; scale = fmax(fabs(f1), fabs(g1)); } while (scale >= safmx2 && count < 20);
  } else if (scale <= safmn2) {
    do { f1 *= safmx2; g1 *= safmx2; scale = fmax(fabs(f1), fabs(g1)); } while (scale <= safmn2);
  }
  const double r = sqrt(f1 * f1 + g1 * g1);
  c = f1 / r;
  s = g1 / r;
  if (fabs(f) > fabs(g) && c < 0.0) { c = -c; s = -s; }
  *cs = c;
  *sn = s;
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

#define GM_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
  X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
static int gm_block_dot(mfem_context_s* ctx, int G, int K, int64_t n, const GmBasis& B, const double* w, double* part, const int32_t* F) {
  switch (K) {
#define GM_DOT(K_) case K_: hipLaunchKernelGGL(kg_block_dot<K_>, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, n, B, (const d2_t*)w, part, F); break;
    GM_CASES(GM_DOT)
#undef GM_DOT
    default: mfem_set_error("gmres: %d basis vectors", K); return MFEM_ERR_INVALID;
  }
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
static int gm_update(mfem_context_s* ctx, int G, int K, bool norm, int64_t n, int64_t nv, const GmBasis& B, const double* h, double* w,
                     double* part_nrm, const int32_t* F) {
  switch (K) {
#define GM_UPD(K_)                                                                                                                       \
  case K_:                                                                                                                               \
    if (norm) hipLaunchKernelGGL((kg_update<K_, true>), dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, n, nv / 2, B, h, (d2_t*)w, part_nrm, F); \
    else hipLaunchKernelGGL((kg_update<K_, false>), dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, n, nv / 2, B, h, (d2_t*)w, part_nrm, F); \
    break;
    GM_CASES(GM_UPD)
#undef GM_UPD
    default: mfem_set_error("gmres: %d basis vectors", K); return MFEM_ERR_INVALID;
  }
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
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
      const double* nrm_part = part_nrm;
      if (literal) {  // the reference's order: for each j one dot product, then one update (:65-68)
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
        nrm_part = part;
      } else {
        RC(gm_block_dot(ctx, G, kk, n, B, w, part, F));  // CGS pass 1: H[1:kk, kk] = Q' w ; w -= Q H[1:kk, kk]
        hipLaunchKernelGGL(kg_fold, dim3(1), dim3(GM_FOLD_BLOCK), 0, ctx->stream, part, G, kk, col, (double*)nullptr, F);
        MFEM_CHECK_LAUNCH();
        RC(gm_update(ctx, G, kk, false, n, nv, B, col, w, nullptr, F));
        RC(gm_block_dot(ctx, G, kk, n, B, w, part, F));  // pass 2: h2 = Q' w ; H[1:kk, kk] += h2 ; w -= Q h2, with the partials of |w|^2
        hipLaunchKernelGGL(kg_fold, dim3(1), dim3(GM_FOLD_BLOCK), 0, ctx->stream, part, G, kk, h2, col, F);
        MFEM_CHECK_LAUNCH();
        RC(gm_update(ctx, G, kk, true, n, nv, B, h2, w, part_nrm, F));
      }
      hipLaunchKernelGGL(kg_normalize, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, nv / 2, nrm_part, G, col + kk, kk, (d2_t*)w, F);
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
