// The kernels of one Arnoldi step that gmres! (krylov_gmres.hip) and gmres! with the multigrid V-cycle (krylov_gmres_mg.hip) share: the start of a
// cycle, the CGS2 orthogonalisation (block dot, fold, fused update, normalise), the Givens rotation, and the layout of the small device region that
// holds H, y and the block-dot partials.  Both passes launch the same kernels with the same grids: a step's sums have one order.
#pragma once
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

enum { F_GM_WIDTH = F_AUX };  // columns of the cycle after an exact breakdown (0: none)

struct GmArgs : KrylovArgs {
  int32_t s;
};
struct GmBasis {
  const d2_t* q[MFEM_MAX_S];
};

// y = 0, y[1] = |r| ; Q1 = r / |r|  (:56-58, :94-96)
static __global__ __launch_bounds__(MFEM_BLOCK) void kg_start(int64_t n2v, const d2_t* __restrict__ r, d2_t* __restrict__ q1, double* __restrict__ y,
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
static __global__ __launch_bounds__(MFEM_BLOCK) void kg_block_dot(int64_t n, GmBasis B, const d2_t* __restrict__ w, double* __restrict__ part,
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
static __global__ __launch_bounds__(GM_FOLD_BLOCK) void kg_fold(const double* __restrict__ part, int G, int K, double* __restrict__ out,
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
static __global__ __launch_bounds__(MFEM_BLOCK) void kg_update(int64_t n, int64_t n2v, GmBasis B, const double* __restrict__ h, d2_t* __restrict__ w,
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
static __global__ __launch_bounds__(MFEM_BLOCK) void kg_normalize(int64_t n2v, const double* __restrict__ part_nrm, int G, double* __restrict__ hsub, int k,
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
static __device__ void gm_givens(double f, double g, double* cs, double* sn) {
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

// Step kk (1-based) of the Arnoldi process by CGS2: w, which holds the new direction, is orthogonalised against B's first kk vectors into column
// kk of H (col = H + GM_LD * (kk - 1)) and normalised -- pass 1: col[0..kk) = Q' w, w -= Q col; pass 2: h2 = Q' w, col += h2, w -= Q h2 with the
// partials of |w|^2; col[kk] = |w|, w /= |w| (kg_normalize).  The launches of krylov_gmres.hip's cycle, in its order.
static int gm_orthogonalise(mfem_context_s* ctx, int G, int kk, int64_t n, int64_t nv, const GmBasis& B, double* w, double* col, double* h2, double* part,
                            double* part_nrm, int32_t* F) {
  RC(gm_block_dot(ctx, G, kk, n, B, w, part, F));
  hipLaunchKernelGGL(kg_fold, dim3(1), dim3(GM_FOLD_BLOCK), 0, ctx->stream, part, G, kk, col, (double*)nullptr, F);
  MFEM_CHECK_LAUNCH();
  RC(gm_update(ctx, G, kk, false, n, nv, B, col, w, nullptr, F));
  RC(gm_block_dot(ctx, G, kk, n, B, w, part, F));
  hipLaunchKernelGGL(kg_fold, dim3(1), dim3(GM_FOLD_BLOCK), 0, ctx->stream, part, G, kk, h2, col, F);
  MFEM_CHECK_LAUNCH();
  RC(gm_update(ctx, G, kk, true, n, nv, B, h2, w, part_nrm, F));
  hipLaunchKernelGGL(kg_normalize, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, nv / 2, part_nrm, G, col + kk, kk, (d2_t*)w, F);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
