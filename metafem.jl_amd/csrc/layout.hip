// The solver layouts of a CSR handle, planned, bound, released and accounted for here only: mfem_solve (the stages of its driver, krylov.hip), the layout query and the diagnostic product
// below take the same rules.  At most one layout is bound at a time; which one serves a product is read off the per-layout pointers, never cached
// beside them: the tile binds' symmetry probe (sym_probe.hip) puts the tiles' pointers aside for its CSR product.  Nothing here issues a
// collective: a refusal of the tiles is a rank-local verdict (krylov.hip: bind_tiles, solve_inner).
#include "blas1.h"
#include "layouts.h"

// The symmetric lattice tiles first: the hex-27 tiles, else the F-field tiles.  While a pattern's values have never been refused by the tiles, the
// row layouts are not even planned (their inspections and column copies cost 20 - 40 ms and 2 - 4 GB at the BASELINE sizes).  Then the slot-major
// copy for near-uniform rows, else the row-sorted sliced layout.
int mfem_layout_plan(mfem_context_s* ctx, mfem_csr_s* A, bool is_cg, bool allow_tiles, mfem_layout_plan_s* P) {
  *P = mfem_layout_plan_s{MFEM_LAYOUT_CSR, MFEM_LAYOUT_CSR, 0, 0};
  int rc = MFEM_OK;
  if (allow_tiles) {  // (both also on slab patterns: the plans read the pattern's lattice hint)
    rc = mfem_lat27_plan(ctx, A);
    if (rc) return rc;
    P->tile_bytes = mfem_lat27_bytes(A);
    if (P->tile_bytes) {
      P->tile = MFEM_LAYOUT_LAT27;
    } else if (mfem_lat8_for_method(A, is_cg)) {  // (asked first: the plan's entry-by-entry check of the pattern costs 27 ms at 512^3)
      rc = mfem_lat8_plan(ctx, A);
      if (rc) return rc;
      if (mfem_lat8_for_method(A, is_cg)) P->tile_bytes = mfem_lat8_bytes(A);  // (again: the plan may have inferred the number of fields)
      if (P->tile_bytes) P->tile = MFEM_LAYOUT_LAT8;
    }
  }
  if (P->tile_bytes && !A->lat_refused) return MFEM_OK;
  rc = mfem_ell_plan(ctx, A);
  if (rc) return rc;
  P->rows_bytes = mfem_ell_vals_bytes(A);
  if (P->rows_bytes) {
    P->rows = mfem_dia_layout_planned(A) ? MFEM_LAYOUT_DIA : MFEM_LAYOUT_ELL;
    return MFEM_OK;
  }
  rc = mfem_sell_plan(ctx, A);  // rows of uneven length
  if (rc) return rc;
  P->rows_bytes = mfem_sell_vals_bytes(A);
  if (P->rows_bytes) P->rows = MFEM_LAYOUT_SELL;
  return MFEM_OK;
}

int mfem_layout_bind(mfem_context_s* ctx, mfem_csr_s* A, mfem_layout mode, const double* vals, double* buf, const double* dsc, const double* ssym,
                     double* scratch, bool allow_rem) {
  mfem_layout_unbind(A);
  switch (mode) {
    case MFEM_LAYOUT_CSR: return MFEM_OK;
    case MFEM_LAYOUT_ELL:
    case MFEM_LAYOUT_DIA: return mfem_ell_bind(ctx, A, vals, buf, dsc, ssym);
    case MFEM_LAYOUT_SELL: return mfem_sell_bind(ctx, A, vals, buf, dsc);
    case MFEM_LAYOUT_LAT27: return mfem_lat27_bind(ctx, A, vals, buf, dsc, scratch, allow_rem);
    case MFEM_LAYOUT_LAT8: return mfem_lat8_bind(ctx, A, vals, buf, dsc, scratch, allow_rem);
    case MFEM_LAYOUT_OPERATOR: break;  // (bound by mfem_mesh_operator_bind, never through a plan)
  }
  return MFEM_OK;
}

mfem_layout mfem_layout_bound(const mfem_csr_s* A, const double* vals) {
  if (A->op) return MFEM_LAYOUT_OPERATOR;  // (the operator's own pattern-less handle: there are no values to tell apart)
  if (A->lat8.vals && vals == A->lat8.src) return MFEM_LAYOUT_LAT8;
  if (A->ell_vals && vals == A->ell_src) return A->ell_bound_mode == 2 ? MFEM_LAYOUT_DIA : MFEM_LAYOUT_ELL;
  if (A->lat27.vals && vals == A->lat27.src) return MFEM_LAYOUT_LAT27;
  if (A->sell.vals && vals == A->sell.src) return MFEM_LAYOUT_SELL;
  return MFEM_LAYOUT_CSR;
}

void mfem_layout_unbind(mfem_csr_s* A) {
  mfem_ell_unbind(A);
  mfem_sell_unbind(A);
  mfem_lat_unbind(A, A->lat27);
  mfem_lat_unbind(A, A->lat8);
}

void mfem_layout_drop(mfem_csr_s* A) {
  mfem_layout_unbind(A);
  mfem_ell_free(A);
  mfem_sell_free(A);
  mfem_rem_free(A);
  A->lat27.state = A->lat8.state = A->lat_refused = A->sym_state = A->symp_state = 0;
  if (A->lat_inferred) {  // (a hint read off the arrays goes with them)
    A->lat_fields = A->lat_m0 = A->lat_m1 = A->lat_m2 = A->lat_plo = A->lat_gw = 0;
    A->lat_inferred = 0;
  }
}

// A pattern without a lattice hint (lat_fields == 0, no ghost columns: a caller-supplied pattern, mfem_csr_create with the reference's own K_J_ptr /
// K_J) gets the one its row 0 proposes (lat_decide.h: lattice_from_row0); lat_fields = -1 afterwards if there is none, so that the question is asked
// once per pattern.  Both tile plans call this; mfem_layout_drop forgets the answer with the arrays.
int mfem_lattice_hint_from_row0(mfem_context_s* ctx, mfem_csr_s* A) {
  if (A->lat_fields != 0) return MFEM_OK;
  A->lat_fields = -1;
  A->lat_inferred = 1;
  if (A->n < 8 || (A->ncols > A->n)) return MFEM_OK;
  int64_t rp[2] = {0, 0};
  const int rc = mfem_by_rowptr(A, [&](auto w) -> int {
    decltype(w) r[2];
    MFEM_CHECK_HIP(hipMemcpyAsync(r, A->rowptr, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    rp[0] = r[0];
    rp[1] = r[1];
    return MFEM_OK;
  });
  if (rc) return rc;
  const int64_t len = rp[1] - rp[0];
  if (!lattice_row0_len(len)) return MFEM_OK;
  int32_t c[27];
  MFEM_CHECK_HIP(hipMemcpyAsync(c, A->colidx + (rp[0] - A->index_base), (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < len; ++i) c[i] -= A->index_base;
  const LatHint H = lattice_from_row0(len, c, A->n);
  if (!H.fields) return MFEM_OK;
  A->lat_fields = H.fields;
  A->lat_m0 = H.m0;
  A->lat_m1 = H.m1;
  A->lat_m2 = H.m2;
  A->lat_plo = H.plo;
  A->lat_gw = H.gw;
  return MFEM_OK;
}

// What the Krylov loop of the next mfem_solve will run on this pattern: 0 = CSR tile kernel, 1 = slot-major copy with explicit
// columns, 2 = slot-major copy with diagonal-slotted regular blocks, 3 = row-sorted sliced layout, 4 / 5 = symmetric lattice tiles (one rank;
// the values of each solve decide, modes 3 / 2 serve it otherwise).  Answers for cg!.  Plans what it reports if that has not happened yet.
extern "C" int mfem_csr_solver_layout(mfem_context ctx, mfem_csr A, int32_t* mode, int32_t* slots, int64_t* padded_rows,
                                      int64_t* regular_rows) try {
  MFEM_REQUIRE(ctx && A, "null handle");
  mfem_layout_plan_s P;
  const int rc = mfem_layout_plan(ctx, A, true, true, &P);
  if (rc) return rc;
  const mfem_layout m = P.tile != MFEM_LAYOUT_CSR ? P.tile : P.rows;
  const bool ell = m == MFEM_LAYOUT_ELL || m == MFEM_LAYOUT_DIA;
  if (mode) *mode = m;
  if (slots) *slots = ell ? A->ell_K : m >= MFEM_LAYOUT_SELL ? A->max_row_nnz : 0;
  if (padded_rows) *padded_rows = ell ? A->ell_npad : m == MFEM_LAYOUT_SELL ? sell_padded_rows(A->sell) : 0;
  if (regular_rows) *regular_rows = m == MFEM_LAYOUT_DIA ? (int64_t)A->dia_regular_blocks * 128 : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_csr_solver_layout")

// The accounting of the planned solver layout, per layout (layouts.h).  Entries: matrix entries (8-byte values) one SpMV reads from memory; sweep: 0 none,
// 1 / 2 the structure allows the workgroup-tile / patch sweep of mode 2 (whether it runs is decided per solve by the bitwise symmetry check of the
// values), 3 symmetric tiles.  Bytes: what one SpMV moves by design (bench.py's roofline numerator) -- matrix entries, 4-byte columns where the kernel
// reads them, x as often as the kernel fetches it from memory by design, y once.
static int layout_account(mfem_context ctx, mfem_csr A, int64_t* entries, int32_t* sweep, int64_t* bytes) {
  int32_t mode = 0, sym = 0;
  const int rc = mfem_csr_solver_layout(ctx, A, &mode, nullptr, nullptr, nullptr);
  if (rc) return rc;
  int64_t e = A->nnz, b = A->nnz * 12 + A->n * 16 + (A->n + 1) * (A->rowptr_bits / 8);
  switch ((mfem_layout)mode) {
    case MFEM_LAYOUT_CSR: break;
    case MFEM_LAYOUT_ELL:
    case MFEM_LAYOUT_DIA: e = mfem_ell_entries(ctx, A, &sym); b = mfem_ell_design_bytes(ctx, A); break;
    case MFEM_LAYOUT_SELL: e = mfem_sell_entries(A); b = mfem_sell_design_bytes(A); break;
    case MFEM_LAYOUT_LAT27: e = mfem_lat27_entries(A); b = mfem_lat27_design_bytes(A); sym = 3; break;
    case MFEM_LAYOUT_LAT8: e = mfem_lat8_entries(A); b = mfem_lat8_design_bytes(A); sym = 3; break;
    case MFEM_LAYOUT_OPERATOR: break;  // (never planned)
  }
  if (entries) *entries = e;
  if (sweep) *sweep = sym;
  if (bytes) *bytes = b;
  return MFEM_OK;
}
extern "C" int mfem_csr_solver_layout_entries(mfem_context ctx, mfem_csr A, int64_t* entries, int32_t* symmetric_sweep) try {
  MFEM_REQUIRE(ctx && A, "null argument");
  return layout_account(ctx, A, entries, symmetric_sweep, nullptr);
} MFEM_API_CATCH("mfem_csr_solver_layout_entries")
extern "C" int mfem_csr_solver_layout_bytes(mfem_context ctx, mfem_csr A, int64_t* bytes) try {
  MFEM_REQUIRE(ctx && A && bytes, "null argument");
  return layout_account(ctx, A, nullptr, nullptr, bytes);
} MFEM_API_CATCH("mfem_csr_solver_layout_bytes")

// y = alpha A x + beta y through the layout mfem_solve would use for this pattern with cg! (the one-off conversion of `vals` included): the tiles if
// these values pass their probe, the row layout otherwise.  A test / diagnostic entry point -- production SpMVs of caller-supplied values go
// through mfem_spmv_csr.
static int spmv_solver_layout(mfem_context ctx, mfem_csr A, const double* vals, const double* x, double* y, double alpha, double beta, double* xdoty) {
  MFEM_REQUIRE(ctx && A, "null handle");
  MFEM_REQUIRE(A->n == 0 || (x && y && (A->nnz == 0 || vals)), "null vector");
  if (xdoty) *xdoty = 0.0;
  if (A->n == 0) return MFEM_OK;
  struct Release { mfem_csr_s* A; ~Release() { mfem_layout_unbind(A); } } release{A};  // nothing stays bound on any way out
  mfem_layout_plan_s P;
  int rc = mfem_layout_plan(ctx, A, true, true, &P);
  if (rc) return rc;
  if (P.tile != MFEM_LAYOUT_CSR) {
    const size_t lay = (P.tile_bytes + 255) & ~(size_t)255;
    rc = mfem_ws_reserve(ctx, lay + (2 * (size_t)A->n + (size_t)(A->ncols > A->n ? A->ncols : A->n)) * sizeof(double));
    if (!rc) rc = mfem_layout_bind(ctx, A, P.tile, vals, (double*)ctx->ws, nullptr, nullptr, (double*)((char*)ctx->ws + lay), mfem_rem_diag());
    if (rc) return rc;
  }
  if (mfem_layout_bound(A, vals) == MFEM_LAYOUT_CSR) {  // no tiles, or they refused these values: the row layout (planned now if it was not)
    rc = mfem_layout_plan(ctx, A, true, false, &P);
    if (!rc && P.rows != MFEM_LAYOUT_CSR) rc = mfem_ws_reserve(ctx, P.rows_bytes);
    if (!rc && P.rows != MFEM_LAYOUT_CSR) rc = mfem_layout_bind(ctx, A, P.rows, vals, (double*)ctx->ws, nullptr, nullptr, nullptr, false);
    if (rc) return rc;
  }
  if (!xdoty) return mfem_spmv_launch(ctx, A, vals, x, y, alpha, beta, nullptr, nullptr, nullptr, nullptr);
  // with the product's fused x . y, as cg! takes p . Ap: one partial sum per workgroup, added on the host in workgroup order
  int np = 0;
  rc = mfem_spmv_launch(ctx, A, vals, x, y, alpha, beta, x, ctx->d_partials, &np, nullptr);
  if (rc) return rc;
  MFEM_REQUIRE(np > 0 && np <= MFEM_MAX_PARTIALS, "the product left no partial sums");
  std::vector<double> h((size_t)np);
  MFEM_CHECK_HIP(hipMemcpyAsync(h.data(), ctx->d_partials, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  double s = 0.0;
  for (double v : h) s += v;
  *xdoty = s;
  return MFEM_OK;
}
extern "C" int mfem_spmv_solver_layout(mfem_context ctx, mfem_csr A, const double* vals, const double* x, double* y, double alpha,
                                       double beta) try {
  return spmv_solver_layout(ctx, A, vals, x, y, alpha, beta, nullptr);
} MFEM_API_CATCH("mfem_spmv_solver_layout")
extern "C" int mfem_spmv_solver_layout_dot(mfem_context ctx, mfem_csr A, const double* vals, const double* x, double* y, double alpha,
                                           double beta, double* xdoty) try {
  MFEM_REQUIRE(xdoty, "null argument");
  return spmv_solver_layout(ctx, A, vals, x, y, alpha, beta, xdoty);
} MFEM_API_CATCH("mfem_spmv_solver_layout_dot")

// TEST / DIAGNOSTIC entry point: one product y = alpha (S^-1 A S^-1) x + beta y on the row layout bound the way the scaled CG (cg_variant 4) binds it --
// the symmetric scaling ssym = 1 / S folded into the copy -- with the fused dotw . y: its per-workgroup partial sums (at most `cap`) go to
// partials_out, their count to *n_partials.  *form: -1 the bind did not end on the patch sweep, 0 / 1 its copy carries the diagonal stored / as one-byte
// codes (spmv_symp.h; bit 21 of the "ell" knob forces the stored form).  Nothing stays bound.
extern "C" int mfem_debug_spmv_scaled_layout(mfem_context ctx, mfem_csr A, const double* vals, const double* ssym, const double* x, double* y, double alpha,
                                             double beta, const double* dotw, double* partials_out, int32_t cap, int32_t* n_partials, int32_t* form) try {
  MFEM_REQUIRE(ctx && A && vals && ssym && x && y && form, "null argument");
  *form = -1;
  if (n_partials) *n_partials = 0;
  struct Release { mfem_csr_s* A; ~Release() { mfem_layout_unbind(A); } } release{A};
  mfem_layout_plan_s P;
  int rc = mfem_layout_plan(ctx, A, true, false, &P);
  if (rc) return rc;
  MFEM_REQUIRE(P.rows == MFEM_LAYOUT_DIA, "the pattern has no diagonal-slotted layout");
  rc = mfem_ws_reserve(ctx, P.rows_bytes);
  if (!rc) rc = mfem_layout_bind(ctx, A, P.rows, vals, (double*)ctx->ws, nullptr, ssym, nullptr, false);
  if (rc) return rc;
  MFEM_REQUIRE(mfem_layout_bound(A, vals) == MFEM_LAYOUT_DIA, "the layout was not bound");
  if (A->symp_vals) *form = A->symp_DC;
  int np = 0;
  rc = mfem_spmv_launch(ctx, A, vals, x, y, alpha, beta, dotw, dotw ? ctx->d_partials : nullptr, &np, nullptr);
  if (rc) return rc;
  if (dotw && partials_out) {
    MFEM_REQUIRE(np > 0 && np <= MFEM_MAX_PARTIALS && np <= cap, "partial sums: none, or more than the caller's buffer holds");
    MFEM_CHECK_HIP(hipMemcpyAsync(partials_out, ctx->d_partials, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    if (n_partials) *n_partials = np;
  }
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_spmv_scaled_layout")
