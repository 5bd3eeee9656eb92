// y = alpha A' x + beta y: tmul! (reference misc/04_GPU_Utils.jl:132, CUSPARSE mv!('T', ...)) without floating-point atomics.
//
// A scatter of A's rows into y would need atomics and lose the library's fixed summation order (the Krylov tests compare graph
// replay with direct launches bit for bit).  Instead the pattern is transposed once, on the device, and cached on the handle
// (mfem_tplan_s): the transposed row pointers (int64: nnz passes 2^31 at 512^3), the transposed columns and the permutation
// perm from transposed slots back to the caller's nnz slots.  A stable radix sort of the column indices keeps, inside every
// transposed row, the entries in increasing original row order.  A product is then a value gather  valsT[k] = vals[perm[k]]
// (divided by up to two row scalings of A': the Jacobi vectors of lsqr!, krylov_next.hip) followed by the ordinary CSR kernel
// family on the transposed arrays -- the same row-block inspection, the same fixed order.  Nothing is planned before the first
// product: the plan costs (ncols + 1) 8 B + nnz (4 + 4 or 8) B of device memory.
#include <hipcub/hipcub.hpp>
#include <chrono>
#include "blas1.h"

int mfem_csr_plan(mfem_context_s* ctx, mfem_csr_s* A);

template <typename PT>
__global__ __launch_bounds__(MFEM_BLOCK) void k_t_iota(int64_t nnz, PT* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nnz; k += stride) out[k] = (PT)k;
}

// rowptrT[c] = first sorted slot whose column is >= c + base, c = 0 .. ncols (columns outside [base, ncols + base) fall outside every row)
__global__ __launch_bounds__(MFEM_BLOCK) void k_t_rowptr(int64_t ncols, int64_t nnz, const int32_t* __restrict__ sorted, int base,
                                                          int64_t* __restrict__ rowptrT) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c <= ncols; c += stride) {
    const int64_t key = c + base;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)sorted[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    rowptrT[c] = lo;
  }
}

// colT[k] = the row of original slot perm[k] (0-based): the last row r with rowptr[r] - base <= perm[k]
template <typename RP, typename PT>
__global__ __launch_bounds__(MFEM_BLOCK) void k_t_cols(int64_t n, int64_t nnz, const RP* __restrict__ rowptr, int base, const PT* __restrict__ perm,
                                                        int32_t* __restrict__ colT) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nnz; k += stride) {
    const int64_t slot = (int64_t)perm[k];
    int64_t lo = 0, hi = n + 1;  // first index with rowptr - base > slot
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)rowptr[mid] - base <= slot) lo = mid + 1;
      else hi = mid;
    }
    colT[k] = (int32_t)(lo - 1);
  }
}

// valsT[k] = (src ? src[perm[k]] : valsT[k]) / d1[i] / d2[i] for the slots k of transposed row i (d1, d2 optional).  One wave per row:
// the writes of a row are contiguous, the reads of src are the gather.
template <typename PT>
__global__ __launch_bounds__(MFEM_BLOCK) void k_t_gather(int64_t nT, const int64_t* __restrict__ rowptrT, const PT* __restrict__ perm,
                                                          const double* __restrict__ src, double* __restrict__ valsT, const double* __restrict__ d1,
                                                          const double* __restrict__ d2) {
  const int lane = threadIdx.x & (MFEM_WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / MFEM_WAVE;
  const int64_t waves = (int64_t)gridDim.x * blockDim.x / MFEM_WAVE;
  for (int64_t i = wave; i < nT; i += waves) {
    const int64_t k0 = rowptrT[i], k1 = rowptrT[i + 1];
    const double s1 = d1 ? d1[i] : 1.0, s2 = d2 ? d2[i] : 1.0;
    for (int64_t k = k0 + lane; k < k1; k += MFEM_WAVE) {
      double v = src ? src[perm[k]] : valsT[k];
      if (d1) v = v / s1;
      if (d2) v = v / s2;
      valsT[k] = v;
    }
  }
}

void mfem_tplan_free(mfem_csr_s* A) {
  mfem_tplan_s* P = A->tplan;
  if (!P) return;
  if (P->AT) mfem_csr_destroy(P->AT);  // (frees the owned rowptrT / colT and the AT handle's own inspection)
  if (P->perm) hipFree(P->perm);
  if (P->vals) hipFree(P->vals);
  delete P;
  A->tplan = nullptr;
}

int mfem_tplan_get(mfem_context_s* ctx, mfem_csr_s* A, mfem_tplan_s** out) {
  if (A->tplan) {
    *out = A->tplan;
    return MFEM_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t n = A->n, nnz = A->nnz, ncols = A->ncols > 0 ? A->ncols : A->n;
  MFEM_REQUIRE(ncols < ((int64_t)1 << 31) - 1 && n < ((int64_t)1 << 31) - 1, "transposed pattern: rows and columns must fit int32");
  mfem_host_alloc_probe();
  mfem_tplan_s* P = new mfem_tplan_s();
  memset(P, 0, sizeof(*P));
  A->tplan = P;  // (mfem_tplan_free releases whatever a failed build below leaves)
  const bool p64 = nnz >= ((int64_t)1 << 31);
  P->perm_bits = p64 ? 64 : 32;
  const size_t pb = p64 ? 8 : 4;
  int64_t* rowptrT = nullptr;
  int32_t* colT = nullptr;
  void* iota = nullptr;
  void* tmp = nullptr;
  auto fail = [&](hipError_t e, int line) -> int {
    if (rowptrT) hipFree(rowptrT);
    if (colT) hipFree(colT);
    if (iota) hipFree(iota);
    if (tmp) hipFree(tmp);
    mfem_tplan_free(A);
    mfem_set_error("spmv_t.hip:%d: transpose plan: %s", line, hipGetErrorString(e));
    return MFEM_ERR_HIP;
  };
#define TP_CHECK(expr)                          \
  do {                                          \
    hipError_t _e = (expr);                     \
    if (_e != hipSuccess) return fail(_e, __LINE__); \
  } while (0)
  TP_CHECK(hipMalloc(&rowptrT, sizeof(int64_t) * (size_t)(ncols + 1)));
  TP_CHECK(hipMalloc(&colT, sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1)));
  TP_CHECK(hipMalloc(&P->perm, pb * (size_t)(nnz > 0 ? nnz : 1)));
  TP_CHECK(hipMalloc(&iota, pb * (size_t)(nnz > 0 ? nnz : 1)));
  const int gk = mfem_grid_for(nnz, MFEM_BLOCK, 4096);
  if (nnz > 0) {
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) <= ncols + A->index_base) ++bits;
    size_t tb = 0;
    if (p64) {
      hipLaunchKernelGGL(k_t_iota<int64_t>, dim3(gk), dim3(MFEM_BLOCK), 0, ctx->stream, nnz, (int64_t*)iota);
      TP_CHECK(hipGetLastError());
      TP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, A->colidx, colT, (const int64_t*)iota, (int64_t*)P->perm, nnz, 0, bits, ctx->stream));
      TP_CHECK(hipMalloc(&tmp, tb ? tb : 16));
      TP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, A->colidx, colT, (const int64_t*)iota, (int64_t*)P->perm, nnz, 0, bits, ctx->stream));
    } else {
      hipLaunchKernelGGL(k_t_iota<int32_t>, dim3(gk), dim3(MFEM_BLOCK), 0, ctx->stream, nnz, (int32_t*)iota);
      TP_CHECK(hipGetLastError());
      TP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, A->colidx, colT, (const int32_t*)iota, (int32_t*)P->perm, (int)nnz, 0, bits, ctx->stream));
      TP_CHECK(hipMalloc(&tmp, tb ? tb : 16));
      TP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, A->colidx, colT, (const int32_t*)iota, (int32_t*)P->perm, (int)nnz, 0, bits, ctx->stream));
    }
  }
  // row pointers from the sorted columns, then the sorted columns are replaced by the rows they came from
  hipLaunchKernelGGL(k_t_rowptr, dim3(mfem_grid_for(ncols + 1, MFEM_BLOCK, 4096)), dim3(MFEM_BLOCK), 0, ctx->stream, ncols, nnz, colT, A->index_base, rowptrT);
  TP_CHECK(hipGetLastError());
  if (nnz > 0) {
#define TP_COLS(RP, PT) \
  hipLaunchKernelGGL((k_t_cols<RP, PT>), dim3(gk), dim3(MFEM_BLOCK), 0, ctx->stream, n, nnz, (const RP*)A->rowptr, A->index_base, (const PT*)P->perm, colT)
    if (A->rowptr_bits == 64) {
      if (p64) TP_COLS(int64_t, int64_t); else TP_COLS(int64_t, int32_t);
    } else {
      if (p64) TP_COLS(int32_t, int64_t); else TP_COLS(int32_t, int32_t);
    }
#undef TP_COLS
    TP_CHECK(hipGetLastError());
  }
  TP_CHECK(hipStreamSynchronize(ctx->stream));
  hipFree(iota);
  iota = nullptr;
  if (tmp) hipFree(tmp);
  tmp = nullptr;
  mfem_csr_s* AT = new mfem_csr_s();
  memset(AT, 0, sizeof(*AT));
  AT->ctx = ctx;
  AT->n = ncols;
  AT->nnz = nnz;
  AT->rowptr = rowptrT;
  AT->rowptr_bits = 64;
  AT->colidx = colT;
  AT->index_base = 0;
  AT->ncols = n != ncols ? n : 0;
  AT->owned_rowptr = rowptrT;
  AT->owned_colidx = colT;
  P->AT = AT;  // (owns the two arrays from here on)
  rowptrT = nullptr;
  colT = nullptr;
  const int rc = mfem_csr_plan(ctx, AT);
  if (rc) {
    mfem_tplan_free(A);
    return rc;
  }
  P->bytes = (int64_t)(sizeof(int64_t) * (ncols + 1) + sizeof(int32_t) * nnz + pb * nnz);
  P->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = P;
  return MFEM_OK;
#undef TP_CHECK
}

int mfem_tplan_gather(mfem_context_s* ctx, const mfem_tplan_s* P, const double* src, double* valsT, const double* d1, const double* d2) {
  const mfem_csr_s* AT = P->AT;
  if (AT->n == 0 || AT->nnz == 0) return MFEM_OK;
  const int grid = mfem_grid_for(AT->n, MFEM_BLOCK / MFEM_WAVE, ctx->num_cus * 16);
  if (P->perm_bits == 64)
    hipLaunchKernelGGL(k_t_gather<int64_t>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, AT->n, (const int64_t*)AT->rowptr, (const int64_t*)P->perm, src,
                       valsT, d1, d2);
  else
    hipLaunchKernelGGL(k_t_gather<int32_t>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, AT->n, (const int64_t*)AT->rowptr, (const int32_t*)P->perm, src,
                       valsT, d1, d2);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

extern "C" int mfem_spmv_csr_t(mfem_context ctx, mfem_csr A, const double* vals, const double* x, double* y, double alpha, double beta) try {
  MFEM_REQUIRE(ctx && A, "null handle");
  MFEM_REQUIRE(A->ctx == ctx, "the pattern belongs to another context");
  const int64_t ncols = A->ncols > 0 ? A->ncols : A->n;
  if (ncols == 0) return MFEM_OK;
  MFEM_REQUIRE(y && (A->n == 0 || (x && (A->nnz == 0 || vals))), "null vector");
  mfem_tplan_s* P = nullptr;
  int rc = mfem_tplan_get(ctx, A, &P);
  if (rc) return rc;
  if (!P->vals && A->nnz > 0) MFEM_CHECK_HIP(hipMalloc(&P->vals, sizeof(double) * (size_t)A->nnz));  // (kept with the plan: one gather per call)
  rc = mfem_tplan_gather(ctx, P, vals, P->vals, nullptr, nullptr);
  if (rc) return rc;
  return mfem_spmv_launch(ctx, P->AT, P->vals, x, y, alpha, beta, nullptr, nullptr, nullptr);
} MFEM_API_CATCH("mfem_spmv_csr_t")

extern "C" int mfem_debug_csr_tplan(mfem_csr A, int64_t* bytes, double* build_ms) try {
  MFEM_REQUIRE(A, "null handle");
  const mfem_tplan_s* P = A->tplan;
  if (bytes) *bytes = P ? P->bytes : 0;
  if (build_ms) *build_ms = P ? P->build_ms : 0.0;
  return P ? 1 : 0;
} MFEM_API_CATCH("mfem_debug_csr_tplan")
