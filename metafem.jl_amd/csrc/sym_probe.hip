// The symmetry measure shared by the lattice-tile layouts (modes 4 and 5: spmv_lat27.hip, spmv_lat8.hip) and their skew remainder (spmv_rem.hip).
// The layout stores one triangle and mirrors it; whether that is the caller's matrix is measured with a probe product: x with entries of magnitude
// in [0.75, 1.25) and a random SIGN each (zero mean: a skew part with zero row sums -- convection-like terms -- is not attenuated the way a
// nearly constant probe would), y1 = (layout) x, y2 = (CSR kernel on the caller's values) x.  y1 - y2 = (L - U^T) x: an entry pair that differs by
// delta shows up as >= 0.75 |delta| in its row (the other terms of that row are the other pairs' differences: no cancellation for a generic x).
// The two products round differently (a few 1e-15 of the row's entries for rows of up to 125 entries), so the layout is taken when
//     max over rows r of |y1 - y2|_r / |a_rr|  <=  LAT_SYM_GATE (lat_decide.h)
// -- the difference is weighed PER ROW by that row's diagonal entry (badly scaled matrices: a penalty or Robin row of 1e5 no longer hides an
// asymmetric pair in a row of 1e-3); rows without a stored non-zero diagonal are weighed by the global max |a|.
#include "blas1.h"
#include "krylov.h"  // mfem_fill

__global__ __launch_bounds__(MFEM_BLOCK) void k_probe_vector(int64_t n, double* __restrict__ x) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t z = (uint64_t)i + 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double mag = 0.75 + 0.5 * (double)(z >> 11) * (1.0 / 9007199254740992.0);
    x[i] = (z & 1ull) ? mag : -mag;
  }
}
__global__ __launch_bounds__(MFEM_BLOCK) void k_probe_diff(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                             const double* __restrict__ scale, unsigned long long* __restrict__ out) {
  double d = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double e = fabs(a[i] - b[i]) / scale[i];  // (scale > 0: |diagonal| or the preset max |a|)
    if (!(e == e)) e = __builtin_huge_val();
    d = fmax(d, e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d = fmax(d, __shfl_down(d, o, MFEM_WAVE));
  if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(d));
}

// *dmax = max over rows of |y1 - y2|_r / |a_rr|.  The rows' weights go into x (the probe vector has served): |a_rr|, amax where no non-zero diagonal
// is stored.  One stream synchronisation.
static int probe_measure(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double amax, const double* y1, const double* y2, double* x, double* dmax) {
  unsigned long long* d_stat = (unsigned long long*)(ctx->d_flags + 12);
  int rc = mfem_fill(ctx, A->n, amax, x);
  if (!rc) rc = mfem_jacobi_diag_launch(ctx, A, vals, x, 0);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_probe_diff, dim3(mfem_vec_grid(ctx, A->n)), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, y1, y2, x, d_stat);
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 12, d_stat, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(dmax, ctx->h_flags + 12, sizeof(double));
  return MFEM_OK;
}

// scratch: ncols + 2 n doubles (x carries the ghost entries of a slab pattern).  T must be bound for `vals` with no column scaling and be the only
// layout bound: the second product runs with T's pointers put aside, on the CSR kernel.
int mfem_sym_probe(mfem_context_s* ctx, mfem_csr_s* A, LatTiles* T, const double* vals, double* scratch, double amax, double* asym, int rem_fields) {
  A->rem_active = 0;
  A->rem_asym_before = 0.0;
  A->rem_last_rows = A->rem_last_ent = 0;
  const int64_t n = A->n, nc = A->ncols > n ? A->ncols : n;
  double *x = scratch, *y1 = scratch + nc, *y2 = y1 + n;
  const int prof = ctx->prof_on;
  ctx->prof_on = 0;  // (not SpMVs of the solve: bench.py's per-launch timing must not see them)
  ctx->probe_active = 1;
  hipLaunchKernelGGL(k_probe_vector, dim3(mfem_vec_grid(ctx, nc)), dim3(MFEM_BLOCK), 0, ctx->stream, nc, x);
  int rc = mfem_spmv_launch(ctx, A, vals, x, y1, 1.0, 0.0, nullptr, nullptr, nullptr);
  if (!rc) {
    const LatTiles bound = *T;
    mfem_lat_unbind(A, *T);
    rc = mfem_spmv_launch(ctx, A, vals, x, y2, 1.0, 0.0, nullptr, nullptr, nullptr);
    T->vals = bound.vals;
    T->dump = bound.dump;
    T->src = bound.src;
  }
  ctx->prof_on = prof;
  ctx->probe_active = 0;
  if (rc) return rc;
  const bool finite = amax < __builtin_huge_val() && amax == amax;
  if (!(amax > 0.0) || !finite) {  // an all-zero matrix is symmetric; a non-finite one is not taken
    *asym = finite ? 0.0 : 1.0;
    return MFEM_OK;
  }
  double dmax;
  rc = probe_measure(ctx, A, vals, amax, y1, y2, x, &dmax);
  if (rc) return rc;
  *asym = dmax;
  A->rem_asym_before = dmax;
  if (lat_accepts(dmax) || rem_fields <= 0 || !(dmax < __builtin_huge_val())) return MFEM_OK;
  // A = S + N (spmv_rem.hip): the rows above the gate get a remainder N[r][c] = A[r][c] - A[c][r] on their mirrored entries; accepted when the SAME
  // probe passes on S + N.  (x holds the rows' weights now, y1 / y2 the two products.)
  bool built = false;
  rc = mfem_rem_build(ctx, A, vals, rem_fields, y1, y2, x, LAT_SYM_GATE, &built);
  if (rc || !built) return rc;
  hipLaunchKernelGGL(k_probe_vector, dim3(mfem_vec_grid(ctx, nc)), dim3(MFEM_BLOCK), 0, ctx->stream, nc, x);  // the probe vector again (the weights took its place)
  MFEM_CHECK_LAUNCH();
  ctx->probe_active = 1;
  rc = mfem_rem_apply(ctx, A, x, nullptr, y1, 1.0, nullptr, nullptr, nullptr, nullptr);
  ctx->probe_active = 0;
  double dmax2;
  if (!rc) rc = probe_measure(ctx, A, vals, amax, y1, y2, x, &dmax2);
  if (rc) return rc;
  if (lat_accepts(dmax2)) {
    *asym = dmax2;
    A->rem_active = 1;
    A->rem_last_rows = A->rem_nrows;
    A->rem_last_ent = A->rem_nent;
  }
  return MFEM_OK;
}
