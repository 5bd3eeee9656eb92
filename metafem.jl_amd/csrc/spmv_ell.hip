// Inspector-executor SpMV for matrices whose rows have (nearly) the same length -- every matrix the structured assembly
// produces (27 entries per row for hex-8 thermal, 81 for 3-field elasticity, fewer only on the boundary).
//
// The caller's contract is unchanged: CSR pattern + values in CSR order (`mul!(b, A, x)`, 04_GPU_Utils.jl:131).  The
// reference's own linear solver starts every solve with a gather copy of the values (K_total[K_val_ids],
// 02_Preconditioner.jl:35); here that one pass per solve transposes the (already preconditioner-scaled) values into a
// slot-major padded layout  ell_vals[s][row]  next to a column table  ell_cols[s][row]  built once per pattern.
// In the Krylov loop lane <-> row, the slot loop runs in registers:
//   * the value / column streams are unit-stride across the lanes of a wave (512-byte and 256-byte runs), no LDS
//     staging, no workgroup barrier, no cross-lane reduction;
//   * the gather x[col] of one slot touches 64 CONSECUTIVE-ish entries (neighbouring rows have neighbouring columns):
//     4-5 cache lines per instruction instead of ~12 in CSR order (tools/gather_probe.hip, modes 0 vs 5);
//   * the row sum is accumulated in slot order = the plain sequential CSR row sum (deterministic).
// Padding entries carry value 0 and the row's own index as column.  Eligible when padding <= 10 % of nnz and
// max_row_nnz <= 128; rows of uneven length (hex-27: 27..125 entries) take the row-sorted sliced layout of spmv_sell.hip,
// small systems stay on the CSR kernels of spmv_csr.hip (size thresholds below).
#include "blas1.h"
#include "spmv_ell.h"

// Size thresholds: below them the Krylov loop is launch-bound and the CSR tile kernel, which spreads the nonzeros of few rows
// over many lanes, is as fast or faster than a lane-per-row layout whose slots are walked one dependent batch after the other
// (tools/probe_ell.py, tools/probe_small_solve.py: crossover ~3e5 rows with diagonal slots, ~1e6 rows with explicit columns).
std::atomic<int64_t> g_layout_min_rows_dia{262144};
std::atomic<int64_t> g_layout_min_rows_cols{1000000};
// hex-27 lattice tiles (spmv_lat27.hip): crossover against the CSR tile kernel + cycle graphs between 1.2e5 rows (41 / 45 us per CG iteration)
// and 2.7e5 (70 / 54 us); at 9.1e5 rows 183 / 110 us (tools/probe_lat_threshold.py, profiles/r03_lat_tiles_thresholds.txt)
#define LAT27_MIN_ROWS 180000
std::atomic<int64_t> g_layout_min_rows_lat27{LAT27_MIN_ROWS};
extern "C" int mfem_debug_set_layout_min_rows(int64_t diagonal_slots, int64_t explicit_columns) try {
  ++mfem_debug_epoch;
  g_layout_min_rows_dia = diagonal_slots;
  g_layout_min_rows_cols = explicit_columns;
  g_layout_min_rows_lat27 = explicit_columns < LAT27_MIN_ROWS ? explicit_columns : LAT27_MIN_ROWS;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_layout_min_rows")

// The "ell" knob word, decoded here and nowhere else (fields: spmv_ell.h; bits: include/metafem_mi355x_debug.h).  Bits 6-7, 16-19 (other than the value
// 8) and 24-25 selected kernel variants of the round-1 sweeps (profiles/r01_spmv_sweep.txt): the winners alone are left, the bits are ignored.
EllKnobs g_ell;
extern "C" int mfem_debug_set_ell(int enable) try {
  ++mfem_debug_epoch;
  g_ell.enable = enable & 1;
  g_ell.dia = (enable & 2) ? 0 : 1;
  g_ell.symp_trim = (enable & 4) ? 2 : (enable & 8) ? 1 : 0;
  g_ell.symp_const = (enable & 16) ? 2 : (enable & 32) ? 1 : 0;
  if ((enable >> 8) & 255) g_ell.grid_mult = (enable >> 8) & 255;
  g_ell.shared_x = ((enable >> 16) & 15) == 8 ? 0 : 1;
  g_ell.xcd = (enable >> 20) & 1;
  g_ell.symp_coded = ((enable >> 21) & 1) ? 0 : 1;
  g_ell.sym = ((enable >> 22) & 1) ? 0 : 1;
  g_ell.symp = ((enable >> 23) & 1) ? 0 : 1;
  g_ell.symp_bands = ((enable >> 24) & 1) ? 1 : ((enable >> 25) & 1) ? 2 : 0;
  g_ell.symp_tail = ((enable >> 26) & 1) ? 0 : 1;
  g_ell.symp_direct = ((enable >> 27) & 1) ? 0 : 1;
  g_ell.dia_pipe = ((enable >> 28) & 1) ? 0 : 1;
  g_ell.dia_fast = ((enable >> 29) & 1) ? 0 : 1;
  g_ell.symp_fingerprint = ((enable >> 30) & 1) ? 0 : 1;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_ell")

// cols[s][r] (0-based) for s < K; pad: the row index itself
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_ell_cols(int64_t n, int64_t npad, int K, const RP* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, int base, int32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < npad; r += stride) {
    int64_t lo = 0;
    int len = 0;
    if (r < n) {
      lo = (int64_t)rowptr[r] - base;
      len = (int)((int64_t)rowptr[r + 1] - base - lo);
    }
    const int32_t self = (int32_t)(r < n ? r : 0);
    for (int s = 0; s < K; ++s) out[ell_base(r, K) + s * ELL_B] = s < len ? col[lo + s] - base : self;
  }
}

// Transposition of the values through LDS: a wave owns 64 consecutive rows, whose CSR values are one contiguous run -> read with
// unit-stride lanes into the wave's LDS block, written out slot by slot with lane <-> row (both sides coalesced).
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_ell_vals_lds(int64_t n, int64_t npad, int K, const RP* __restrict__ rowptr,
                                                               const double* __restrict__ vals, int base, double* __restrict__ out,
                                                               const int32_t* __restrict__ col, const double* __restrict__ dsc) {
  // dsc != nullptr: the copy is the right-Jacobi-scaled matrix, entry / dsc[its column] (Mat_Div_Jacobi folded into this pass)
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double* T = lds + (size_t)w * 64 * K;
  const int64_t ntiles = npad >> 6;
  for (int64_t tile = (int64_t)blockIdx.x * nw + w; tile < ntiles; tile += (int64_t)gridDim.x * nw) {
    const int64_t r0 = tile << 6, r = r0 + lane;
    const int64_t rend = (r0 + 64 < n) ? r0 + 64 : n;
    int64_t lo = 0;
    int len = 0;
    if (r < n) {
      lo = (int64_t)rowptr[r] - base;
      len = (int)((int64_t)rowptr[r + 1] - base - lo);
    }
    const int64_t s0 = r0 < n ? (int64_t)rowptr[r0] - base : 0;
    const int cnt = r0 < n ? (int)((int64_t)rowptr[rend] - base - s0) : 0;  // <= 64 K
    constexpr int NB = 28;  // loads in flight per lane: a tile of 27-entry rows in ONE round trip (with 8 the kernel waited 79 % of its wave cycles)
    for (int i0 = lane; i0 < cnt; i0 += 64 * NB) {
      double tv[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + 64 * u;
        tv[u] = i < cnt ? vals[s0 + i] : 0.0;
        if (dsc && i < cnt) tv[u] /= dsc[col[s0 + i] - base];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + 64 * u;
        if (i < cnt) T[i] = tv[u];
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    const int off = (int)(lo - s0);
    for (int s = 0; s < K; ++s) out[ell_base(r, K) + s * ELL_B] = s < len ? T[off + s] : 0.0;
    __builtin_amdgcn_wave_barrier();
  }
}

// RPT rows per lane (1: 8-byte value / 4-byte column loads; 2: 16-byte / 8-byte loads of two neighbouring rows), U slots in
// flight per batch.  npad is a multiple of 64, so row pairs (even r) are 16-byte aligned in every slot plane.
template <int RPT, int U>
__global__ __launch_bounds__(MFEM_BLOCK) void k_spmv_ell(int64_t n, int64_t npad, int K, const int32_t* __restrict__ cols,
                                                           const double* __restrict__ vals, const double* __restrict__ x,
                                                           double* __restrict__ y, double alpha, double beta,
                                                           const double* __restrict__ dotw, double* __restrict__ partials,
                                                           const int32_t* __restrict__ done_flag, SpmvPart part) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * RPT;
  for (int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * RPT; r < n; r += stride) {
    if (spmv_part_skip(part, r, r + RPT)) continue;
    const double* v = vals + ell_base(r, K);
    const int32_t* c = cols + ell_base(r, K);
    if (RPT == 1) {
      double acc = 0.0;
      int s = 0;
      for (; s + U <= K; s += U) {
        double vv[U];
        int32_t cc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          vv[u] = __builtin_nontemporal_load(v + (s + u) * ELL_B);
          cc[u] = __builtin_nontemporal_load(c + (s + u) * ELL_B);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += vv[u] * x[cc[u]];
      }
      for (; s < K; ++s) acc += __builtin_nontemporal_load(v + s * ELL_B) * x[__builtin_nontemporal_load(c + s * ELL_B)];
      double yv = alpha * acc;
      if (beta != 0.0) yv += beta * y[r];
      y[r] = yv;
      if (dotw) dot_acc += yv * dotw[r];
    } else {
      // rows r, r + 1 (r even; row r + 1 may be the pad row n when n is odd: its slots are zero-valued and point at row 0)
      e_d2 acc = {0.0, 0.0};
      int s = 0;
      for (; s + U <= K; s += U) {
        e_d2 vv[U];
        e_i2 cc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          vv[u] = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + (s + u) * ELL_B));
          cc[u] = __builtin_nontemporal_load(reinterpret_cast<const e_i2*>(c + (s + u) * ELL_B));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          acc.x += vv[u].x * x[cc[u].x];
          acc.y += vv[u].y * x[cc[u].y];
        }
      }
      for (; s < K; ++s) {
        const e_d2 v1 = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + s * ELL_B));
        const e_i2 c1 = __builtin_nontemporal_load(reinterpret_cast<const e_i2*>(c + s * ELL_B));
        acc.x += v1.x * x[c1.x];
        acc.y += v1.y * x[c1.y];
      }
      double y0 = alpha * acc.x, y1 = alpha * acc.y;
      const bool two = r + 1 < n;
      if (beta != 0.0) {
        y0 += beta * y[r];
        if (two) y1 += beta * y[r + 1];
      }
      y[r] = y0;
      if (two) y[r + 1] = y1;
      if (dotw) {
        dot_acc += y0 * dotw[r];
        if (two) dot_acc += y1 * dotw[r + 1];
      }
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// d[r] = |A_rr| read from the bound slot-major copy (n values instead of a scan of all nonzeros); rows without a stored
// diagonal keep 1.0 (Jacobi_By_Diagonal, 02_Preconditioner.jl:122-130)
__global__ __launch_bounds__(MFEM_BLOCK) void k_ell_diag(int64_t n, int K, const DiaOffsets* __restrict__ Op,
                                                           const int32_t* __restrict__ flags, const int32_t* __restrict__ cols,
                                                           const double* __restrict__ vals, double* __restrict__ d) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += stride) {
    const int64_t b = ell_base(r, K);
    const int cls = flags ? flags[r >> 7] - 1 : -1;
    double out = 1.0;
    if (cls >= 0) {
      const int D = Op->D[cls];
      for (int s = 0; s < D; ++s)
        if (Op->off[cls][s] == 0) {
          const double v = vals[b + s * ELL_B];
          if (v != 0.0) out = fabs(v);
          break;
        }
    } else {
      for (int s = 0; s < K; ++s)
        if (cols[b + s * ELL_B] == (int32_t)r) {
          const double v = vals[b + s * ELL_B];
          if (v != 0.0) out = fabs(v);  // a padding slot (col = self, value 0) is not a stored diagonal
          break;
        }
    }
    d[r] = out;
  }
}

// Plan, once per pattern: eligibility and the column table.  A->max_row_nnz must be known (mfem_csr_plan).
static int ell_plan_columns(mfem_context_s* ctx, mfem_csr_s* A) {
  A->ell_state = -1;
  const int K = A->max_row_nnz;
  if (A->n < 1 || K < 1 || K > 128) return MFEM_OK;
  const int64_t npad = (A->n + ELL_B - 1) & ~(int64_t)(ELL_B - 1);
  if ((double)K * (double)npad > 1.10 * (double)A->nnz + 64.0 * K) return MFEM_OK;  // > 10 % padding
  MFEM_CHECK_HIP(hipMalloc(&A->ell_cols, sizeof(int32_t) * (size_t)K * (size_t)npad));
  const int grid = mfem_grid_for(npad, MFEM_BLOCK, ctx->num_cus * 16);
  mfem_by_rowptr(A, [&](auto t) {
    hipLaunchKernelGGL(k_ell_cols<decltype(t)>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, npad, K, (const decltype(t)*)A->rowptr, A->colidx,
                       A->index_base, A->ell_cols);
  });
  MFEM_CHECK_LAUNCH();
  A->ell_K = K;
  A->ell_npad = npad;
  A->ell_state = 1;
  return MFEM_OK;
}
int mfem_ell_plan(mfem_context_s* ctx, mfem_csr_s* A) {
  if (A->ell_state != 0) return MFEM_OK;
  if (A->n < g_layout_min_rows_dia && A->n < g_layout_min_rows_cols) return MFEM_OK;  // launch-bound sizes: CSR tile kernel
  // The inspection allocates on the host (std::vector, mfem_host_alloc_probe) after it has begun to record its verdict: an exception on the way
  // must leave the pattern UNPLANNED -- the next solve inspects again -- not half-planned on the slower path for good.  Same for an error return.
  struct Undo {
    mfem_csr_s* A;  // (nullptr: disarmed)
    ~Undo() {
      if (!A) return;
      mfem_ell_free(A);  // (also resets ell_state / dia_state to "not inspected")
      A->sym_state = A->symp_state = 0;
    }
  } undo{A};
  int rc = ell_plan_columns(ctx, A);
  if (!rc && A->ell_state == 1) rc = mfem_dia_plan(ctx, A);  // diagonal structure?  Then the structure of the two symmetric sweeps
  if (!rc) undo.A = nullptr;
  return rc;
}

bool mfem_dia_layout_planned(const mfem_csr_s* A) { return A->ell_state == 1 && g_ell.enable && A->dia_state == 1 && g_ell.dia; }
DiaKernel mfem_dia_kernel_wanted(const mfem_csr_s* A, DiaKernel refused, bool* direct) {
  DiaKernel k = DIA_ROWS;
  if (A->dia_triples && g_ell.shared_x) {  // (both sweeps share the x loads of three consecutive diagonals too)
    k = DIA_ROWS_TRIPLES;
    if (refused != DIA_SYM27 && mfem_sym_wanted(A, DIA_SYM27)) k = DIA_SYM27;
    if (refused == DIA_NONE && mfem_sym_wanted(A, DIA_SYMP)) k = DIA_SYMP;  // (its refusal leaves the tile sweep to try, not the other way round)
  }
  if (direct) *direct = k == DIA_SYMP && g_ell.symp_direct;
  return k;
}
// Bands per patch of the patch sweep, decided here once per bind (dia_bind stores it with the copy): two 4-line bands move 6 % fewer matrix bytes
// and a sixth less x, but leave three resident waves per CU instead of seven.  Measured at 512^3 (1.3e8 swept rows), parent and change alternated on
// one box: 1073-1083 against 1128-1153 ms per benchmark step (profiles/r07_symp_bands_ab_512.txt).  Smaller lattices were not measured with two
// bands and keep one: the limit lies between the two benchmark sizes (256^3: 1.7e7 swept rows).
#define SYMP_BANDS2_MIN_ROWS 100000000
int mfem_symp_bands_wanted(const mfem_csr_s* A) {
  if (g_ell.symp_bands) return g_ell.symp_bands;
  return A->symp_state == 1 && (int64_t)(A->symp_p1 - A->symp_p0) * A->symp_PL >= SYMP_BANDS2_MIN_ROWS ? 2 : 1;
}
int mfem_symp_bands(const mfem_csr_s* A) { return A->symp_B ? A->symp_B : mfem_symp_bands_wanted(A); }
// Whole patches only (symp_trim_decide.h: a remainder of <= 2 points per line or of one line per plane leaves the sweep and is computed row by row), decided
// here once per bind.  Measured at 512^3 (B = 2: 1105 -> 1024 patches per plane, 2 -> 3 runs per patch) and 256^3 (B = 1: 585 -> 512 patches), parent and
// change alternated on one box: profiles/r10_symp_trim_ab_512.txt.  Smaller lattices were not measured and keep every row in a patch: the limit is the
// smaller measured size (256^3: 1.67e7 swept rows).  Bit 2 of the "ell" knob forces the untrimmed form, bit 3 the trimmed one at any size (the tests).
#define SYMP_TRIM_MIN_ROWS 16000000
int mfem_symp_trim_wanted(const mfem_csr_s* A) {
  if (g_ell.symp_trim) return g_ell.symp_trim == 1 ? 1 : 0;
  return A->symp_state == 1 && (int64_t)(A->symp_p1 - A->symp_p0) * A->symp_PL >= SYMP_TRIM_MIN_ROWS ? 1 : 0;
}
int mfem_symp_trim(const mfem_csr_s* A) { return A->symp_B ? A->symp_trim : mfem_symp_trim_wanted(A); }
static std::atomic<long long> g_symp_trim_binds{0};  // binds that ended on the patch sweep with rim rows outside its patches (tests, the A/B)
extern "C" long long mfem_debug_symp_trim_count(void) { return g_symp_trim_binds; }
// Form of the diagonal in the patch-major copy, decided here once per bind.  Coded (one signed byte per row instead of a double: 0.95 of the 19.7 GB a 512^3
// product streams) where the fill writes S^-1 A S^-1 itself -- the values of every other bind have an arbitrary diagonal.  Measured:
// profiles/r09_symp_diag_code_ab_512.txt.  The fill's gate (a diagonal without a code) sends a bind back to the stored form: dia_bind.
int mfem_symp_coded_wanted(DiaKernel k, bool fast, const double* ssym) { return k == DIA_SYMP && fast && ssym && g_ell.symp_coded ? 1 : 0; }
int mfem_symp_coded(const mfem_csr_s* A) { return A->symp_vals ? A->symp_DC : A->symp_dc_last; }
static std::atomic<long long> g_symp_coded_binds{0};  // binds that ended on the patch sweep with the coded form (tests, the A/B)
extern "C" long long mfem_debug_symp_coded_count(void) { return g_symp_coded_binds; }
// The constant form of the patch sweep, decided here once per bind (spc_form, symp_const_decide.h) from the fill's count of flagged steps.
static std::atomic<long long> g_symp_const_binds{0}, g_symp_const_steps{0};  // binds that ended in the constant form; flagged steps of the last patch-sweep bind (tests, the A/B)
extern "C" long long mfem_debug_symp_const_count(void) { return g_symp_const_binds; }
extern "C" long long mfem_debug_symp_const_steps(void) { return g_symp_const_steps; }
size_t mfem_ell_vals_bytes(const mfem_csr_s* A) {
  if (A->ell_state != 1 || !g_ell.enable) return 0;
  const bool dia = mfem_dia_layout_planned(A);
  if (A->n < (dia ? g_layout_min_rows_dia : g_layout_min_rows_cols)) return 0;
  size_t bytes = sizeof(double) * (size_t)A->ell_K * (size_t)A->ell_npad;
  if (dia && mfem_dia_kernel_wanted(A) == DIA_SYMP) {  // patch-major copy of the swept planes: room for either band count (the count is decided per bind)
    size_t pm = 0;
    for (int B = 1; B <= SP_BMAX; ++B)
      for (int trim = 0; trim <= 1; ++trim) pm = std::max(pm, sizeof(double) * (size_t)mfem_symp_copy_doubles(A, B, trim));  // (and either extent: the knob is read by the bind)
    bytes += pm;
  }
  return bytes;
}
// Bind of mode 2, once per solve: choose the kernel, make its copies, obtain the symmetry verdict of these values, fall back to the next kernel if
// they are refused.  The copy is bound only once the kernel that serves it is known.
static int dia_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, const double* ssym) {
  bool direct = false, fp_made = false, flags_made = false;
  SympConst cst{};
  int64_t flagged = 0;
  DiaKernel k = mfem_dia_kernel_wanted(A, DIA_NONE, &direct);
  A->symp_trim = mfem_symp_trim_wanted(A);
  A->symp_B = mfem_symp_bands_wanted(A);  // (A is unbound here: the geometry below is this count's)
  A->symp_DC = mfem_symp_coded_wanted(k, mfem_dia_fill_fast(A, dsc, direct), ssym);
  A->symp_dneg = 0;
  double* pvals = buf + (size_t)A->ell_K * (size_t)A->ell_npad;
  SympGeom G = k == DIA_SYMP ? mfem_symp_geom(ctx, A) : SympGeom{};
  // the rim rows' compact copy lies behind the patch-major one (whose length depends on the form of the diagonal: placed per copy)
  auto rim_of = [&](const SympGeom& g) -> double* { return k == DIA_SYMP && g.rim_units > 0 ? pvals + (int64_t)g.NR * g.NPk * (g.p1 - g.p0) * sp_step(g.B, g.DC) : nullptr; };
  // the step flags of the constant form lie behind the rim copy; the fill makes them unless the knob forces the stored form
  auto flags_of = [&](const SympGeom& g) -> unsigned char* { return k == DIA_SYMP && direct && g_ell.symp_const != 2 ? mfem_symp_flags_of(pvals, g) : nullptr; };
  int rc = mfem_dia_copy(ctx, A, vals, buf, dsc, ssym, G, direct ? pvals : nullptr, rim_of(G), g_ell.symp_fingerprint != 0, &fp_made, flags_of(G), &flags_made);
  while (!rc && (k == DIA_SYMP || k == DIA_SYM27)) {  // a sweep: are the pairs it mirrors bitwise equal?
    bool ok = false, dc_refused = false;
    rc = mfem_sym_verdict(ctx, A, k, buf, pvals, G, direct, fp_made, &ok, &dc_refused, &A->symp_dneg, flags_made, &cst, &flagged);
    if (rc) break;
    if (dc_refused) {  // a swept row's scaled diagonal has no code: the same copy in the stored form, and its verdict
      A->symp_DC = 0;
      G = mfem_symp_geom(ctx, A);
      rc = mfem_dia_copy(ctx, A, vals, buf, dsc, ssym, G, pvals, rim_of(G), g_ell.symp_fingerprint != 0, &fp_made, flags_of(G), &flags_made);
      continue;
    }
    if (ok) break;
    // the other kernels read all rows from the slot-major copy: after a direct fill the swept rows go there now
    if (k == DIA_SYMP && direct) rc = mfem_dia_copy(ctx, A, vals, buf, dsc, ssym, SympGeom{}, nullptr, nullptr, false, &fp_made);
    k = mfem_dia_kernel_wanted(A, k);
  }
  if (rc) return rc;
  A->ell_vals = buf;
  A->ell_src = vals;
  A->ell_bound_mode = 2;
  A->dia_kernel = k;
  A->symp_vals = k == DIA_SYMP ? pvals : nullptr;
  if (k != DIA_SYMP) A->symp_B = A->symp_DC = A->symp_trim = 0;
  if (!A->symp_DC) A->symp_dneg = 0;
  A->symp_CS = 0;
  A->symp_flagged = 0;
  if (k == DIA_SYMP) {  // (the byte accounting of the unbound pattern answers for this bind)
    const int64_t steps = mfem_symp_steps(A);
    if (!flags_made) flagged = 0;
    // the sweep's path for flagged steps multiplies by the reference row's values where the stored form reads the mirrored entry: only behind the fingerprint's
    // verdict (every pair among the swept rows bitwise equal; the check pass lets +0.0 meet -0.0) and with a reference row that is its own mirror image
    // (no flagged step: nothing to ask)
    bool mirror = fp_made || flagged == 0;
    for (int sl = 0; sl < 13 && mirror && flagged > 0; ++sl) mirror = memcmp(&cst.v[sl], &cst.v[26 - sl], sizeof(double)) == 0;
    A->symp_CS = spc_form(flags_made && mirror, flags_made && cst.valid != 0, flagged, steps, g_ell.symp_const == 2, g_ell.symp_const == 1);
    A->symp_flagged = flagged;
    memcpy(A->symp_cst, cst.v, sizeof(A->symp_cst));
    A->symp_ccode = cst.code;
    A->symp_cs_last = A->symp_CS;
    A->symp_flagged_last = flagged;
    g_symp_const_steps = flagged;
    if (A->symp_CS) ++g_symp_const_binds;
    A->symp_dc_last = A->symp_DC;
    if (A->symp_DC) ++g_symp_coded_binds;
    if (G.rim_units > 0) ++g_symp_trim_binds;
    return mfem_symp_sched_bind(ctx, A, G);  // which wave sweeps which run of the constant form (symp_sched_decide.h): from the flags of THESE values
  }
  return MFEM_OK;
}

// Transpose CSR-ordered values into `buf` and route subsequent mfem_spmv_launch calls with these `vals` to this layout's kernels.
// dsc (optional): right Jacobi column scaling applied on the way (copy = vals[j] / dsc[col[j]]): the Krylov loop then runs on the scaled
// matrix without a scaled CSR copy ever existing (krylov.hip: plan_layouts, bind_rows).  `vals` stays the identity of the bound values.
int mfem_ell_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, const double* ssym) {
  mfem_ell_unbind(A);
  if (A->ell_state != 1 || !g_ell.enable || !buf) return MFEM_OK;
  if (mfem_dia_layout_planned(A)) return dia_bind(ctx, A, vals, buf, dsc, ssym);
  int waves = 4;  // mode 1: the values transposed through LDS
  while (waves > 1 && sizeof(double) * 64 * (size_t)A->ell_K * waves > 64 * 1024) waves >>= 1;
  const size_t lds = sizeof(double) * 64 * (size_t)A->ell_K * waves;
  const int64_t ntiles = A->ell_npad >> 6;
  int grid = (int)((ntiles + waves - 1) / waves);
  if (grid > ctx->num_cus * 16) grid = ctx->num_cus * 16;
  mfem_by_rowptr(A, [&](auto t) {
    hipLaunchKernelGGL(k_ell_vals_lds<decltype(t)>, dim3(grid), dim3(64 * waves), lds, ctx->stream, A->n, A->ell_npad, A->ell_K,
                       (const decltype(t)*)A->rowptr, vals, A->index_base, buf, A->colidx, dsc);
  });
  MFEM_CHECK_LAUNCH();
  A->ell_vals = buf;
  A->ell_src = vals;
  A->ell_bound_mode = 1;
  return MFEM_OK;
}
void mfem_ell_unbind(mfem_csr_s* A) {
  A->ell_bound_mode = A->dia_kernel = DIA_NONE;
  A->ell_vals = A->symp_vals = nullptr;
  A->ell_src = nullptr;
  A->symp_B = A->symp_DC = A->symp_dneg = A->symp_trim = A->symp_CS = 0;
  A->symp_flagged = 0;
  A->symp_sched = nullptr;
  A->symp_sched_grid = 0;
}
void mfem_ell_free(mfem_csr_s* A) {
  if (A->ell_cols) hipFree(A->ell_cols);
  if (A->dia_flags) hipFree(A->dia_flags);
  if (A->dia_dev) hipFree(A->dia_dev);
  A->ell_cols = nullptr;
  A->dia_flags = nullptr;
  A->dia_dev = nullptr;
  A->ell_state = A->dia_state = 0;
}
int mfem_ell_diag(mfem_context_s* ctx, mfem_csr_s* A, double* d) {
  if (!A->ell_vals) return MFEM_ERR_INVALID;
  const int grid = mfem_grid_for(A->n, MFEM_BLOCK, ctx->num_cus * 16);
  hipLaunchKernelGGL(k_ell_diag, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, A->ell_K, (const DiaOffsets*)A->dia_dev,
                     A->ell_bound_mode == 2 ? A->dia_flags : nullptr, A->ell_cols, A->ell_vals, d);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

static std::atomic<int64_t> g_sym_launches{0};
extern "C" int64_t mfem_debug_sym_spmv_count(void) { return g_sym_launches; }
// returns 1 if launched, 0 if the CSR kernel should be used, an error code otherwise.  Mode 2 runs the kernel its bind recorded.
int mfem_spmv_ell_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha, double beta,
                         const double* dotw, double* partials, int* n_partials, const int32_t* done_flag, const SpmvPart& part) {
  if (!A->ell_vals || vals != A->ell_src) return 0;
  int cap = ctx->num_cus * g_ell.grid_mult;  // partial sums = workgroups of the per-row kernels
  if (cap > MFEM_MAX_PARTIALS) cap = MFEM_MAX_PARTIALS;
  if (part.part != 0) cap /= 2;  // the two parts of a split SpMV share one partial-sum array
  if (part.part == 2) {          // a few planes of rows: no point in a chip-filling persistent grid
    int64_t rows = 0;
    for (int z = 0; z < part.nz; ++z) rows += part.hi[z] - part.lo[z];
    const int64_t want = rows / 512 + 2 * part.nz + 1;
    if (want < cap) cap = (int)want;
  }
  const SpmvArgs a{x, y, alpha, beta, dotw, partials, n_partials, done_flag, part};
  int rc = MFEM_OK;
  switch (A->ell_bound_mode == 2 ? A->dia_kernel : DIA_NONE) {
    case DIA_SYMP:
    case DIA_SYM27:
      if (part.part != 2) ++g_sym_launches;
      rc = mfem_sym_launch(ctx, A, (DiaKernel)A->dia_kernel, a);
      break;
    case DIA_ROWS_TRIPLES:
    case DIA_ROWS: rc = mfem_dia_launch(ctx, A, A->dia_kernel == DIA_ROWS_TRIPLES, cap, a); break;
    default: {  // mode 1
      const int grid = mfem_grid_for((A->n + 1) / 2, MFEM_BLOCK, cap);
      hipLaunchKernelGGL((k_spmv_ell<2, 1>), dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, A->ell_npad, A->ell_K, A->ell_cols, A->ell_vals, x,
                         y, alpha, beta, dotw, partials, done_flag, part);
      MFEM_CHECK_LAUNCH();
      if (n_partials && partials) *n_partials = grid;
    }
  }
  return rc ? rc : 1;
}

// Accounting (mfem_csr_solver_layout_entries / _bytes, layout.hip).  Matrix entries (8-byte values) one SpMV reads from memory: K * padded rows,
// less what a symmetric sweep takes from LDS.  *sweep: 2 / 1 if the structure allows the patch sweep / the workgroup-tile sweep (whether it
// runs is decided per solve by the symmetry of the values), else 0.
int64_t mfem_ell_entries(const mfem_context_s* ctx, const mfem_csr_s* A, int32_t* sweep) {
  const DiaKernel k = mfem_dia_layout_planned(A) ? mfem_dia_kernel_wanted(A) : DIA_NONE;
  if (sweep) *sweep = k == DIA_SYMP ? 2 : k == DIA_SYM27 ? 1 : 0;
  return k == DIA_SYMP || k == DIA_SYM27 ? mfem_sym_entries(ctx, A, k) : (int64_t)A->ell_K * A->ell_npad;
}
// Bytes one SpMV moves by design: the entries, 4-byte columns where the kernel reads them, x as often as the kernel fetches it, y once
int64_t mfem_ell_design_bytes(const mfem_context_s* ctx, const mfem_csr_s* A) {
  int32_t sym = 0;
  const int64_t ent = mfem_ell_entries(ctx, A, &sym);
  if (!mfem_dia_layout_planned(A)) return ent * 12 + A->n * 16;
  const int64_t reg = (int64_t)A->dia_regular_blocks * 128;
  int64_t b = ent * 8 + A->n * 16 + (A->n > reg ? A->n - reg : 0) * (int64_t)A->ell_K * 4;  // (rows in generic blocks read their columns)
  // the patch sweep stages a (4 B + 2) x (32 + 2) neighbourhood of x per step instead of reading each swept entry once
  // (a rim row of a trimmed sweep reads x like a row outside the swept planes)
  if (sym == 2) b += mfem_symp_steps(A) * (int64_t)sp_xn(mfem_symp_bands(A)) * 8 - mfem_symp_swept_rows(A) * 8;
  return b;
}
