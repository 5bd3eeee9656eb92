// The SpMV behind mul! and every Krylov loop: y = alpha A x + beta y on whatever serves the values -- the solver layout bound to them (layout.hip) or
// the CSR kernels on the caller's arrays (spmv_csr.hip) --, its optional timing bracket, and the slab form that overlaps the halo exchange of x with
// the rows that need no ghost entry.
#include "blas1.h"
#include "operator.h"

// Internal launcher: y = alpha*A*x + beta*y, optionally partial sums of (dotw . y) into `partials`
// (*n_partials receives the number written).
static int spmv_launch_inner(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y,
                             double alpha, double beta, const double* dotw, double* partials, int* n_partials,
                             const int32_t* done_flag, const SpmvPart& part);

static const SpmvPart kAllRows = {0, 0, {0}, {0}};

struct ProfScope {  // optional hip-event bracket around one SpMV (bench.py's roofline): a split SpMV counts as one launch
  mfem_context_s* ctx;
  int k;
  int begin() {
    k = -1;
    if (!ctx->prof_on) return MFEM_OK;
    if (ctx->prof_used == MFEM_PROF_PAIRS) {
      int rc = mfem_prof_flush(ctx);
      if (rc) return rc;
    }
    k = ctx->prof_used;
    MFEM_CHECK_HIP(hipEventRecord(ctx->prof_ev[2 * k], ctx->stream));
    return MFEM_OK;
  }
  int end() {
    if (k < 0) return MFEM_OK;
    MFEM_CHECK_HIP(hipEventRecord(ctx->prof_ev[2 * k + 1], ctx->stream));
    ctx->prof_used = k + 1;
    return MFEM_OK;
  }
};

int mfem_spmv_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y,
                     double alpha, double beta, const double* dotw, double* partials, int* n_partials,
                     const int32_t* done_flag) {
  ProfScope prof{ctx, -1};
  int rc = prof.begin();
  if (rc) return rc;
  rc = spmv_launch_inner(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, kAllRows);
  if (rc) return rc;
  return prof.end();
}

// The SpMV of a Krylov loop on a slab: y = alpha A x + beta y where x carries ghost blocks that the neighbours' boundary
// planes must fill first.  The exchange is started on the communicator's stream, the rows that reference no ghost column
// run beside it, the few planes of rows that do run after it has arrived (one extra small launch).  The row-sorted sliced layout
// splits by blocks instead of zones: its ghost-reading rows are sorted behind all others when the pattern is planned.  Without a
// communicator this is mfem_spmv_launch.
static std::atomic<int> g_halo_overlap{1};
extern "C" int mfem_debug_set_halo_overlap(int on) try {
  ++mfem_debug_epoch;
  g_halo_overlap = on ? 1 : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_halo_overlap")

int mfem_spmv_halo(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* x, double* y, double alpha, double beta,
                   const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  if (mfem_comm_world(ctx) == 1) return mfem_spmv_launch(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag);
  ProfScope prof{ctx, -1};
  int rc = prof.begin();
  if (rc) return rc;
  const mfem_layout bound = mfem_layout_bound(A, vals);
  if (bound == MFEM_LAYOUT_LAT27 || bound == MFEM_LAYOUT_LAT8) {
    // lattice tiles split by i-LAYERS of tiles, not by row zones: the layers that stage no ghost plane run beside the exchange (part 1), the top
    // layers and the gather pass -- which reads the lower ghost planes for the first owned rows -- after it (part 2)
    rc = mfem_comm_halo_begin(ctx, x);
    if (rc) return rc;
    SpmvPart P;
    memset(&P, 0, sizeof(P));
    if (g_halo_overlap) {
      P.part = 1;
      rc = spmv_launch_inner(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, P);
      if (rc) {
        mfem_comm_halo_end(ctx);
        return rc;
      }
      P.part = 2;
    }
    rc = mfem_comm_halo_end(ctx);
    if (rc) return rc;
    rc = spmv_launch_inner(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, P);
    if (rc) return rc;
    return prof.end();
  }
  rc = mfem_comm_halo_begin(ctx, x);
  if (rc) return rc;
  // an error between begin and end must not leave the exchange "in flight": the communicator would refuse every later one
  auto fail = [&](int code) {
    mfem_comm_halo_end(ctx);
    return code;
  };
  SpmvPart P;
  memset(&P, 0, sizeof(P));
  const int F = ctx->halo_fields;
  const bool split = g_halo_overlap && A->n > 0 && 2 * F <= MFEM_MAX_ZONES && A->n == (int64_t)F * mfem_comm_owned_nodes(ctx);
  if (split) {
    const int64_t NO = mfem_comm_owned_nodes(ctx), PL = ctx->halo_plane_len;
    const int rank = mfem_comm_rank(ctx), world = mfem_comm_world(ctx);
    for (int f = 0; f < F; ++f) {
      if (rank > 0) { P.lo[P.nz] = f * NO; P.hi[P.nz] = f * NO + PL; ++P.nz; }
      if (rank < world - 1) { P.lo[P.nz] = (f + 1) * NO - PL; P.hi[P.nz] = (f + 1) * NO; ++P.nz; }
    }
    int np1 = 0, np2 = 0;
    P.part = 1;
    rc = spmv_launch_inner(ctx, A, vals, x, y, alpha, beta, dotw, partials, &np1, done_flag, P);
    if (rc) return fail(rc);
    rc = mfem_comm_halo_end(ctx);
    if (rc) return rc;
    P.part = 2;
    rc = spmv_launch_inner(ctx, A, vals, x, y, alpha, beta, dotw, partials ? partials + np1 : nullptr, &np2, done_flag, P);
    if (rc) return rc;
    if (n_partials) *n_partials = np1 + np2;
    if (np1 + np2 > MFEM_MAX_PARTIALS) {
      mfem_set_error("split SpMV wrote %d partial sums (> %d)", np1 + np2, MFEM_MAX_PARTIALS);
      return MFEM_ERR_INVALID;
    }
  } else {
    rc = mfem_comm_halo_end(ctx);
    if (rc) return rc;
    rc = spmv_launch_inner(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, kAllRows);
    if (rc) return rc;
  }
  return prof.end();
}

static int spmv_launch_inner(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y,
                             double alpha, double beta, const double* dotw, double* partials, int* n_partials,
                             const int32_t* done_flag, const SpmvPart& part) {
  if (n_partials) *n_partials = 0;
  if (A->n == 0) return MFEM_OK;
  int launched = 0;  // (a layout launcher returns 1 if it launched, < 0 on error)
  switch (ctx->force_csr ? MFEM_LAYOUT_CSR : mfem_layout_bound(A, vals)) {
    case MFEM_LAYOUT_CSR: break;
    case MFEM_LAYOUT_ELL:
    case MFEM_LAYOUT_DIA: launched = mfem_spmv_ell_launch(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, part); break;
    // (the sliced layout splits by BLOCKS: its ghost-reading rows are sorted behind all others, whatever the zones say)
    case MFEM_LAYOUT_SELL: launched = mfem_spmv_sell_launch(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, part.part); break;
    case MFEM_LAYOUT_LAT27: launched = mfem_spmv_lat27_launch(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, part.part); break;
    case MFEM_LAYOUT_LAT8: launched = mfem_spmv_lat8_launch(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, part.part); break;
    // (a matrix-free operator has no CSR arrays to fall back to: its launcher launches or fails)
    case MFEM_LAYOUT_OPERATOR: {
      const mfem_operator_interface* I = mfem_operator_interface_of(A->op);
      MFEM_REQUIRE(I, "the bound operator's handle carries no known kind tag");
      return I->launch(ctx, A, x, y, alpha, beta, dotw, partials, n_partials, done_flag);
    }
  }
  if (launched != 0) return launched < 0 ? launched : MFEM_OK;
  return mfem_spmv_csr_launch(ctx, A, vals, x, y, alpha, beta, dotw, partials, n_partials, done_flag, part);  // (also what a layout that did not launch falls back to)
}

extern "C" int mfem_spmv_csr(mfem_context ctx, mfem_csr A, const double* vals, const double* x, double* y,
                             double alpha, double beta) try {
  MFEM_REQUIRE(ctx && A, "null handle");
  MFEM_REQUIRE(A->n == 0 || (x && y && (A->nnz == 0 || vals)), "null vector");
  return mfem_spmv_launch(ctx, A, vals, x, y, alpha, beta, nullptr, nullptr, nullptr, nullptr);
} MFEM_API_CATCH("mfem_spmv_csr")
