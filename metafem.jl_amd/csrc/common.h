// Shared internals of libmetafem_mi355x.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <unordered_map>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "metafem_mi355x is written for gfx950 (MI355X) only: counted s_waitcnt vmcnt(k) pipelines assume loads and stores share one in-order counter, global_load_lds_dwordx4 and v_mfma_f64 are used directly -- build with --offload-arch=gfx950"
#endif
#include "../../include/metafem_mi355x.h"
#include "../../include/metafem_mi355x_debug.h"
#include "csr_decide.h"
#include "sell_decide.h"
#include "lat_decide.h"

#define MFEM_WAVE 64
#define MFEM_BLOCK 256
#define MFEM_MAX_PARTIALS 4096
static_assert(LAT_MAX_GATHER_GRID == MFEM_MAX_PARTIALS, "a workgroup of the tiles' gather pass writes one partial sum");
#define MFEM_NFLAGS 80           // 32-bit device flags of a context (mfem_context_s::d_flags)
#define MFEM_NSCALARS 4096      // device-resident Krylov scalars (doubles)  // upper bound on per-launch partial sums of a fused reduction

void mfem_set_error(const char* fmt, ...);

// Every `extern "C" int` entry point is a function-try-block closed by this handler: no C++ exception leaves the library (include/metafem_mi355x.h,
// error convention).  mfem_api_exception (api.hip) rethrows the exception in flight, maps it to a status and sets mfem_last_error().
int mfem_api_exception(const char* entry) noexcept;
#define MFEM_API_CATCH(entry) catch (...) { return mfem_api_exception(entry); }
// Called in front of the library's host allocations (new / std::vector): throws std::bad_alloc when mfem_debug_fail_host_alloc armed it -- the
// test hook that shows the handler above at work (tests/test_gpu_round4_abi.py).
void mfem_host_alloc_probe();

#define MFEM_CHECK_HIP(expr)                                                                  \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      mfem_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));    \
      return MFEM_ERR_HIP;                                                                    \
    }                                                                                         \
  } while (0)

#define MFEM_REQUIRE(cond, msg)                                      \
  do {                                                               \
    if (!(cond)) {                                                   \
      mfem_set_error("%s:%d: %s (%s)", __FILE__, __LINE__, msg, #cond); \
      return MFEM_ERR_INVALID;                                       \
    }                                                                \
  } while (0)

#define MFEM_CHECK_LAUNCH() MFEM_CHECK_HIP(hipGetLastError())

// Owner of one device allocation, move-only: freed when it goes out of scope unless release() has handed the pointer on (to a handle).
template <typename T> struct __attribute__((visibility("hidden"))) DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t count) { reset(); return hipMalloc((void**)&p, sizeof(T) * count); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }
  T* release() { T* q = p; p = nullptr; return q; }
  operator T*() const { return p; }
};

struct mfem_comm_s;

// Row split of a slab SpMV (multi-GPU): the rows that reference ghost columns -- the first / last halo_plane_len owned rows
// of every field next to a neighbour rank ("boundary zones") -- against all other rows.  The interior part runs while the
// halo exchange is in flight, the boundary part after it (spmv.hip: mfem_spmv_halo).  Kernels test whole work units
// (tiles / chunks / a lane's rows): a unit that touches a zone belongs to the boundary part, so every row is computed once.
#define MFEM_MAX_ZONES 8
struct SpmvPart {
  int part;  // 0 = all rows, 1 = interior units only, 2 = boundary units only
  int nz;
  int64_t lo[MFEM_MAX_ZONES], hi[MFEM_MAX_ZONES];
};
__host__ __device__ __forceinline__ bool spmv_part_skip(const SpmvPart& P, int64_t r0, int64_t r1) {
  if (P.part == 0) return false;
  bool bnd = false;
  for (int z = 0; z < P.nz; ++z) bnd = bnd || (r0 < P.hi[z] && r1 > P.lo[z]);
  return P.part == 1 ? bnd : !bnd;
}


#define MFEM_GRAPH_SLOTS 4
struct mfem_context_s {
  int device;
  hipStream_t stream;
  int num_cus;
  // reduction scratch: partial sums (device) + a small block of device scalars + pinned host mirror
  double* d_partials;   // [MFEM_MAX_PARTIALS * 8]
  double* d_scalars;    // [256] device-resident Krylov scalars
  double* h_scalars;    // pinned, [256]
  int32_t* d_flags;     // [MFEM_NFLAGS] device flags (16-17: the symmetry fingerprint of k_symp_fill, 64 bits; 18: its coded-diagonal gate, 19: the codes' unit is -1.0; 20: its count of
                        // constant steps, 22-77: the reference row of the constant form, a SympConst -- symp_const_decide.h): 0-7 the Krylov loop's two banks (done, iteration count, ...); 9 mirrored-sweep check; 10 ring self-test; 11 mesh
                        // assembly; 12-15 one-shot statistics, each user clears the slots it reads before its launch and synchronises after it (layout binds:
                        // 12-13 max |a| / symmetry measure, krylov.hip (try_scaled_cg): 12-15 extremes of S, assemble_hex27.hip: 14 count of non-affine elements)
  int32_t* h_flags;     // pinned
  // generic workspace (grown on demand, never shrunk)
  void* ws;        // (ws_raw + the placement offset, see mfem_ws_reserve)
  void* ws_raw;    // what hipMalloc returned
  size_t ws_bytes;
  // placement of a large workspace (krylov.hip: ws_trial; the decision: solve_decide.h): the solver SpMV runs at one of two speeds depending on the physical memory an
  // allocation received (profiles/r03_placement_probe.txt); the first big solve on a workspace times it, tries ONE second allocation and keeps
  // the faster.  ws_try: candidates allocated after the first (the best so far kept in ws_alt*); 99: decided.
  int ws_try;
  void* ws_alt;
  void* ws_alt_raw;
  float ws_try_ms;
  float ws_log[4];  // the candidates' times (ms for two SpMVs), in the order tried; [3]: which one was kept (0-based)
  // optional user shadow vectors
  const double* shadow;
  int32_t shadow_count;
  // multi-GPU
  mfem_comm_s* comm;
  int64_t halo_plane_len;
  int32_t halo_fields;
  hipEvent_t ev0, ev1;
  // optional per-launch timing of the SpMV kernel (bench.py roofline): event pairs on ctx->stream
  int prof_on;
  int prof_used;
  hipEvent_t* prof_ev;      // [2 * MFEM_PROF_PAIRS]
  double prof_ms;
  int64_t prof_count;
  // hipGraph replay of launch-bound Krylov cycles (krylov.h: mfem_cycle_run): one cached executable graph, keyed by a
  // hash of everything its kernel arguments depend on; graph_stream stands in for the legacy null stream, which cannot
  // be captured
  hipGraphExec_t graph_exec[MFEM_GRAPH_SLOTS];   // small cache: a coupled problem alternates between a few matrices / solvers
  uint64_t graph_key[MFEM_GRAPH_SLOTS];
  int graph_next;                                // round-robin replacement
  hipStream_t graph_stream;
  hipEvent_t graph_ev;
  int graph_active;   // set by mfem_solve for the duration of a solve when cycles may be captured
  int force_csr;      // set while a product must run the CSR kernel on the caller's arrays whatever layout is bound (the residual a tile solve reports, krylov.hip: csr_true_residual)
  int probe_active;   // set while a measuring product runs on this context (symmetry probe, placement trial): not an SpMV a solver asked for -- the usage counters skip it
};
#define MFEM_PROF_PAIRS 1024
int mfem_prof_flush(mfem_context_s* ctx);

struct mfem_operator_head;  // operator.h: the kind tag every matrix-free operator handle starts with
struct mfem_csr_s {
  mfem_context_s* ctx;
  uint64_t serial;          // unique per created pattern (cycle-graph cache key)
  int64_t n, nnz;
  const void* rowptr;
  int rowptr_bits;
  const int32_t* colidx;
  int index_base;
  // what the CSR kernels know of the pattern (csr.hip: mfem_csr_plan; the decisions: csr_decide.h)
  int32_t max_row_nnz;
  CsrPlan plan;             // the inspections the plan built: row blocks (k_spmv_csr_rb), their elision flags, the wave tiles' (k_spmv_csr_w)
  // node-blocked form of a field-major multi-field pattern (round 6): nb_F = fields F > 1 when the F rows of every node list the node's coupled nodes once
  // per column field (mfem_node_block_fields: checked entry by entry once per pattern -- nb_checked), 0 = no or not asked
  int nb_F, nb_checked;
  int64_t rb_ntiles;
  int64_t rb_elided;        // tiles of them whose columns the kernel derives from the tile's first two rows (bit 31 of rb_rows[t])
  int32_t* rb_rows;         // owned, [rb_ntiles + 1]: first row of every tile
  uint8_t* cw_elide;        // owned: one flag per tile of plan.w_elide_Rw rows of the fixed-row-count wave-tile kernel (k_spmv_csr_w): columns derivable from the tile's first row
  int32_t lat_m1, lat_m2, lat_fields;  // lattice hint of a structured pattern (0 = none): points per lattice plane = lat_m1 * lat_m2 (brick.hip)
  int32_t lat_m0, lat_plo, lat_gw;     // ... planes of the whole lattice, first owned plane of a slab, ghost planes per side (0 = not given)
  int32_t lat_inferred;                // the hint was read off row 0 of a caller-supplied pattern (mfem_lattice_hint_from_row0), not given by mfem_brick_pattern
  uint16_t* diag_off;       // owned, [n], built on first use: offset of the diagonal entry inside its row (0xFFFF = none stored): |diag| is then an
                            // n-sized gather instead of a scan of all nonzeros (Jacobi_By_Diagonal of every solve)
  // owned storage (mfem_brick_pattern) -- freed in destroy
  void* owned_rowptr;
  void* owned_colidx;
  // slab info (multi-GPU): rows = owned nodes, x has ghost planes; 0 for single GPU
  int64_t x_offset;  // offset of the first owned entry inside the local x (per field)
  int64_t ncols;     // columns the pattern addresses: n, or n + ghost entries for a slab pattern (0 = n)
  // slot-major padded copy for near-uniform rows (spmv_ell.hip; shared declarations: spmv_ell.h): ell_state 0 = not planned, -1 = not eligible, 1 = ready
  int ell_state, ell_K;
  int64_t ell_npad;
  int32_t* ell_cols;        // owned, [K][npad], 0-based
  const double* ell_src;    // the CSR-ordered values the bound copy mirrors (identity of the `vals` argument)
  double* ell_vals;         // not owned (solver workspace), [K][npad]
  // diagonal-slotted variant (spmv_dia.hip; all entries on <= 32 diagonals): dia_state 0 = not inspected, -1 = no, 1 = yes
  int dia_state, dia_classes;
  void* dia_dev;            // owned, device copy of the diagonal lists (DiaOffsets, spmv_ell.h)
  int32_t* dia_flags;       // owned, one int per 128-row block: 1 = regular (diagonal-slotted), 0 = explicit columns
  int32_t dia_regular_blocks;
  int dia_triples;          // the diagonals come in runs of three consecutive offsets
  // symmetric sweep variant of the diagonal-slotted SpMV (spmv_sym.hip; 27-point lattice stencil): sym_state 0 = not inspected, -1 = no, 1 = structure ok
  int sym_state;
  int64_t sym_c0, sym_c1;   // chunks (512 rows) [c0, c1) whose blocks are all regular
  int sym_cls;              // the diagonal list (class) with the lattice form
  int sym_S;                // chunks per lattice plane (rounded): a workgroup sweeps chunks c, c + S, c + 2 S, ...
  int64_t sym_mx, sym_myz;  // matrix entries per chunk the sweep kernel takes from LDS: previous-plane diagonals / in-chunk -y, -z
  int ell_bound_mode;       // 0 none, 1 slot-major with explicit columns, 2 diagonal-slotted
  int dia_kernel;           // mode 2: the product kernel the bound values got, after their symmetry verdict (DiaKernel, spmv_ell.h; 0 = nothing bound)
  // wave-private (j, k)-patch form of the symmetric sweep (spmv_sym.hip: k_spmv_symp): symp_state 0 = not inspected, -1 = no, 1 = structure ok
  int symp_state;
  int symp_m1, symp_m2;     // lattice lines per plane, points per line
  int64_t symp_PL;          // rows per lattice plane (m1 * m2)
  int symp_p0, symp_p1;     // regular lattice planes [p0, p1) (plane = row / PL): the rows the sweep computes
  int symp_NS, symp_NPk;    // strips of 4 lines, patches of 32 points per line
  int symp_B;               // bands (strips) per patch of the bound patch-major copy: decided once per bind (dia_bind), 0 while none is bound
  int symp_trim;            // the bound patch-major copy covers whole patches only, the rim rows have a compact copy behind it (symp_trim_decide.h; mfem_symp_trim_wanted)
  int symp_DC;              // form of the bound patch-major copy's main part (spmv_symp.h): 1 = the diagonal as one-byte codes (mfem_symp_coded_wanted), 0 stored / none bound
  int symp_dneg;            // symp_DC = 1: the codes count from -1.0 (the first swept row's diagonal is negative), not from +1.0
  int symp_CS;              // the bound patch sweep takes the values of its flagged steps from kernel arguments (symp_const_decide.h), 0 stored form / none bound
  int symp_cs_last;         // symp_CS and the flagged steps of the last bind that ended on the patch sweep (accounting of an unbound pattern, as symp_dc_last)
  int64_t symp_flagged, symp_flagged_last;  // flagged steps of the bound copy (counted by the fill whether or not the constant form is taken)
  double symp_cst[27];      // symp_CS = 1: the reference row's 27 values as the fill forms them
  int symp_ccode;           // ... and, coded diagonal, its diagonal's code
  const int32_t* symp_sched;  // symp_CS = 1: the schedule of the bound copy's runs (symp_sched_decide.h; not owned: in the solver workspace behind the step flags), null = the arithmetic form
  int symp_sched_grid;      // ... and the sweep's grid it was built for
  int symp_dc_last;         // symp_DC of the last bind that ended on the patch sweep (the byte accounting of an unbound pattern answers for that bind)
  double* symp_vals;        // not owned (solver workspace, behind ell_vals): [plane - p0][patch][27 x 128 + edge block]; set while dia_kernel is the patch sweep
  // solver layout mode 3 for rows of uneven length: the row-sorted sliced layout (spmv_sell.hip) or its node-blocked form (spmv_bsell.hip) -- sell.form
  // tells which, and each form has its own members; sell.state 0 = not planned, -1 = no, 1 = ready.  The record and the decisions: sell_decide.h
  SellLayout sell;
  // symmetric lattice tiles of the hex-27 lattice matrix (spmv_lat27.hip) and of the F-field 27-point lattice matrix (hex-8; spmv_lat8.hip): what the
  // plan found and what is bound.  The record and the decisions: lat_decide.h
  LatTiles lat27, lat8;
  int lat_refused;          // a lattice-tile bind has refused values of this pattern once (not symmetric): solves plan the other layouts too from then on
  // A = S + N (spmv_rem.hip): the sparse skew remainder a lattice-tile bind carries when the values are nonsymmetric in a few rows only (Nitsche / SUPG
  // faces): owned device storage, grown on demand and kept between solves; rem_active: the CURRENT bind applies it after the tiles' gather pass
  int rem_active;
  int64_t rem_nrows, rem_nent, rem_cap_rows, rem_cap_ent;
  int32_t* rem_rows;   // [rem_nrows] the rows of N
  int64_t* rem_ptr;    // [rem_nrows] first entry of each
  int32_t* rem_len;    // [rem_nrows] entries of each
  int32_t* rem_col;    // [rem_nent] 0-based columns
  double* rem_val;     // [rem_nent] A[r][c] - A[c][r]
  unsigned long long* rem_cnt;  // device counters of the build
  void* rem_sort_tmp;           // owned: radix-sort scratch of the build, grown on demand (a nonsymmetric K rebuilds the remainder at every solve)
  size_t rem_sort_bytes;
  double rem_asym_before;       // what the probe measured on the tiles alone (the asymmetry the remainder repairs)
  int64_t rem_last_rows, rem_last_ent;  // what the last ACCEPTED remainder of the last probe held (0: none) -- survives the unbind at the end of a solve (tests, bench.py)
  // transposed pattern for A' x (spmv_t.hip): built by the first mfem_spmv_csr_t or lsqr! solve, dropped by replan / destroy
  struct mfem_tplan_s* tplan;
  // the internal pattern-less handle (n rows, nnz = 0) of a matrix-free operator (operator.h: mesh_operator.hip, brick_operator.hip): op is set while
  // the operator is bound for a solve -- every product then goes to its kind's launcher --, with the scratch and the column scaling of that solve;
  // op_epoch counts the operator's term / parameter changes (a captured cycle bakes them in)
  struct mfem_operator_head* op;
  double* op_scratch;
  const double* op_dsc;
  uint64_t op_epoch;
};
// The transpose plan of a pattern (spmv_t.hip): AT is an internal CSR handle over the owned transposed arrays (rows = the columns of A,
// int64 row pointers, 0-based), perm maps its slots to A's slots (int32 below 2^31 entries, int64 above).
struct mfem_tplan_s {
  mfem_csr_s* AT;
  void* perm;
  int perm_bits;
  double* vals;      // values buffer of mfem_spmv_csr_t (allocated by its first call; lsqr! gathers into its workspace instead)
  int64_t bytes;     // device bytes of the plan (row pointers, columns, perm)
  double build_ms;   // host time of the build, synchronised
};
static inline CsrShape mfem_csr_shape(const mfem_csr_s* A) { return {A->n, A->nnz, A->max_row_nnz}; }
// f(int64_t{}) or f(int32_t{}): the width of the pattern's row pointers, for the kernels that are templates on it
template <typename F> static inline auto mfem_by_rowptr(const mfem_csr_s* A, F&& f) { return A->rowptr_bits == 64 ? f(int64_t{}) : f(int32_t{}); }
int mfem_tplan_get(mfem_context_s* ctx, mfem_csr_s* A, mfem_tplan_s** out);
void mfem_tplan_free(mfem_csr_s* A);
// valsT[k] = (src ? src[perm[k]] : valsT[k]) / d1[i] / d2[i] over the slots of transposed row i; d1, d2 may be null
int mfem_tplan_gather(mfem_context_s* ctx, const mfem_tplan_s* P, const double* src, double* valsT, const double* d1, const double* d2);
bool mfem_rem_enabled();
bool mfem_rem_diag();
void mfem_rem_clear(mfem_csr_s* A);
void mfem_rem_free(mfem_csr_s* A);
int mfem_rem_build(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, int n_fields, const double* y1, const double* y2, const double* scale,
                   double gate, bool* built);
int mfem_rem_apply(mfem_context_s* ctx, mfem_csr_s* A, const double* x, const double* dsc, double* y, double alpha, const double* dotw,
                   double* partials, int* n_partials, const int32_t* done_flag);
int64_t mfem_rem_design_bytes(const mfem_csr_s* A);
int mfem_spmv_lat8_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha, double beta,
                          const double* dotw, double* partials, int* n_partials, const int32_t* done_flag, int part);
int64_t mfem_lat8_design_bytes(const mfem_csr_s* A);
int64_t mfem_lat8_entries(const mfem_csr_s* A);
int mfem_lattice_hint_from_row0(mfem_context_s* ctx, mfem_csr_s* A);  // proposes lat_* for a pattern without a hint (layout.hip; lat_decide.h: lattice_from_row0)
static inline LatShape mfem_lat_shape(const mfem_csr_s* A, int64_t min_rows) {
  return {A->n, A->ncols, A->max_row_nnz, A->lat_m0, A->lat_m1, A->lat_m2, A->lat_fields, A->lat_plo, A->lat_gw, min_rows};
}
// releases the tiles `T` of A (A->lat27 or A->lat8); the remainder belongs to the bind
static inline void mfem_lat_unbind(mfem_csr_s* A, LatTiles& T) {
  if (T.vals) A->rem_active = 0;
  T.vals = T.dump = nullptr;
  T.src = T.dsc = nullptr;
}
// The symmetry probe of a tile bind (sym_probe.hip): T = the tiles just filled from `vals` and bound without a column scaling.  rem_fields > 0: rows above
// the gate may be repaired by a remainder built for that many fields (then *asym is the measure of tiles + remainder and A->rem_active is set); 0:
// symmetric values only
int mfem_sym_probe(mfem_context_s* ctx, mfem_csr_s* A, LatTiles* T, const double* vals, double* scratch, double amax, double* asym, int rem_fields);
int mfem_spmv_lat27_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha,
                           double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag, int part);
int64_t mfem_lat27_design_bytes(const mfem_csr_s* A);
int64_t mfem_lat27_entries(const mfem_csr_s* A);
int mfem_node_block_fields(mfem_context_s* ctx, mfem_csr_s* A);  // fills A->nb_F (spmv_bsell.hip)
int mfem_spmv_sell_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha,
                          double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag, int part);
int mfem_ell_diag(mfem_context_s* ctx, mfem_csr_s* A, double* d);
int mfem_spmv_ell_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha,
                         double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag,
                         const SpmvPart& part);
// a product y = alpha A x + beta y (+ partial sums of y . dotw), as mfem_spmv_ell_launch and mfem_spmv_csr_launch receive it
struct SpmvArgs {
  const double* x; double* y; double alpha, beta; const double* dotw; double* partials; int* n_partials; const int32_t* done_flag; const SpmvPart& part;
};
// The CSR kernels on the caller's arrays (spmv_csr.hip; the handle and its plan: csr.hip).  Both stay out of the library's dynamic symbols.
__attribute__((visibility("hidden"))) int mfem_spmv_csr_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha,
                                                             double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag,
                                                             const SpmvPart& part);
__attribute__((visibility("hidden"))) CsrKnobs mfem_csr_knobs();  // what mfem_debug_set_spmv last set

// The solver layouts of a pattern (layout.hip): which copy of the values a solve runs on, and its binding and release.  The values are the
// mode numbers of mfem_csr_solver_layout: the CSR tile kernel on the caller's values (no copy), slot-major copy with explicit columns / with
// diagonal-slotted regular blocks (spmv_ell.hip, spmv_dia.hip and the sweeps of spmv_sym.hip), row-sorted sliced ELL or its node-blocked form (spmv_sell.hip, spmv_bsell.hip), symmetric lattice tiles (spmv_lat27.hip with spmv_lat27_gather.hip, spmv_lat8.hip)
enum mfem_layout : int32_t { MFEM_LAYOUT_CSR = 0, MFEM_LAYOUT_ELL = 1, MFEM_LAYOUT_DIA = 2, MFEM_LAYOUT_SELL = 3, MFEM_LAYOUT_LAT27 = 4, MFEM_LAYOUT_LAT8 = 5,
                             MFEM_LAYOUT_OPERATOR = 6 /* no copy of any values: a bound matrix-free operator (operator.h) */ };
// What a pattern offers a solve: a tile layout (taken if the values pass its symmetry probe) and a row layout, each with the workspace bytes of
// its copy (MFEM_LAYOUT_CSR, 0: none)
struct mfem_layout_plan_s {
  mfem_layout tile, rows;
  size_t tile_bytes, rows_bytes;
};
int mfem_layout_plan(mfem_context_s* ctx, mfem_csr_s* A, bool is_cg, bool allow_tiles, mfem_layout_plan_s* P);
// Releases whatever is bound, then copies `vals` into buf in `mode` and binds the copy (mfem_layout_bound tells whether it was taken).  dsc: right
// Jacobi scaling (nullptr: none); ssym: symmetric scaling of the diagonal-slotted copy (ELL / DIA only); scratch: 3 n doubles for a tile layout's
// symmetry probe, left dirty; allow_rem: the tiles may carry a sparse remainder (spmv_rem.hip)
int mfem_layout_bind(mfem_context_s* ctx, mfem_csr_s* A, mfem_layout mode, const double* vals, double* buf, const double* dsc, const double* ssym,
                     double* scratch, bool allow_rem);
mfem_layout mfem_layout_bound(const mfem_csr_s* A, const double* vals);  // the layout that serves products with these values (CSR: none)
void mfem_layout_unbind(mfem_csr_s* A);
void mfem_layout_drop(mfem_csr_s* A);  // frees and resets every layout's plan (unbound first)

int mfem_ws_reserve(mfem_context_s* ctx, size_t bytes);
int mfem_ws_next_candidate(mfem_context_s* ctx);
int mfem_ws_decide(mfem_context_s* ctx, bool keep_current);
uint64_t mfem_next_csr_serial();
bool mfem_context_alive(mfem_context_s* ctx);       // false once mfem_context_destroy has run (api.hip)
void mfem_graphs_invalidate(mfem_context_s* ctx);  // drops every cached cycle graph of the context (api.hip)
extern std::atomic<int> mfem_debug_epoch;  // bumped by every mfem_debug_set_*: part of the cycle-graph cache key (api.hip)

// ---- device helpers ---------------------------------------------------------------------
__device__ __forceinline__ double wave_reduce_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, MFEM_WAVE);
  return v;
}

// Block-wide sum for blockDim.x == MFEM_BLOCK (4 waves). Result valid in thread 0.
// Workgroup barrier for data the waves exchange through LDS ONLY.  __syncthreads() is s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier: it also waits until every
// global load of the wave has returned and every global STORE has reached memory -- in a kernel that requests the next plane's data early, or streams its
// results out with stores, that is a memory round trip per barrier (round 5: found in k_hex27_rows_gq with the counters, then in the plane sweeps).  Here only
// the LDS counter is drained; global loads into registers are waited for where the registers are used (the compiler's own s_waitcnt), stores never.
// NOT for barriers that order global-memory accesses between the waves of a workgroup.
__device__ __forceinline__ void mfem_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Pass 1 of the lattice tiles: a launch of 8 * ceil(tcount / 8) workgroups covers tcount tiles.  Workgroups with equal blockIdx % 8 share an XCD
// (round-robin dispatch): each XCD walks a contiguous eighth of the tiles, so the neighbourhoods that overlap are staged through one L2.  tsub = this
// workgroup's tile; false: it has none (the whole workgroup leaves: no barrier is left waiting).
__device__ __forceinline__ bool mfem_xcd_tile(int tcount, int& tsub) {
  const int chunk = (tcount + 7) >> 3;
  tsub = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  return !((int)(blockIdx.x >> 3) >= chunk || tsub >= tcount);
}

__device__ __forceinline__ double block_reduce_sum(double v, double* smem /* >= 4 doubles */) {
  v = wave_reduce_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();  // a slower wave may still be reading smem from a preceding reduce_partials_bcast / block_reduce_sum
  if (lane == 0) smem[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int i = 0; i < nw; ++i) r += smem[i];
  }
  __syncthreads();
  return r;
}

// Workgroups of `kernel` a CU holds at once (registers, LDS, waves), from the runtime, cached per kernel; `fallback` when the query fails.  A PERSISTENT grid must
// be a multiple of what is resident: one workgroup more per CU than fits runs as a second round while the others idle (round 5: k_lat8_gather<F = 1> at 75
// VGPRs holds 6 workgroups per CU and was launched with 8 -- two rounds for the work of 1.33).
static inline int mfem_resident_per_cu(const void* kernel, int block_threads, size_t dyn_lds, int fallback) {
  static std::mutex mu;
  static std::unordered_map<const void*, int> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(kernel);
  if (it != cache.end()) return it->second;
  int occ = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, block_threads, dyn_lds);
  const int v = (e == hipSuccess && occ >= 1) ? occ : fallback;
  cache[kernel] = v;
  return v;
}
static inline int mfem_grid_for(int64_t work_items, int per_block, int cap) {
  int64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}
