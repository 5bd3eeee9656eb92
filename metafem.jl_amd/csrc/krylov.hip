// The driver behind mfem_solve -- the linear-solver seam
//   delta_x = fem_domain.linear_solver(globalfield)           (reference solver/04_Time_Domain.jl:76)
//   iterative_Solve!(globalfield; Sv_func!, Pr_func!, ...)    (linear_solver/02_Preconditioner.jl:32-76)
// -- and what every solver file uses: mfem_fill, the residual at the start of and between passes, the read-back of scalars and flags, the small vector
// kernels.  The driver is a sequence of stages over one SolveRun (solve_attempt lists them); its two decisions that are host arithmetic alone are in
// solve_decide.h.  The solvers themselves are reached through mfem_pass_fn (krylov.h), one file each: krylov_cg.hip, krylov_bicgstabl.hip,
// krylov_idrs.hip, krylov_cgs2.hip, krylov_gmres.hip, krylov_next.hip (cgs!, tfqmr!, lsqr!).
//
// The reference returns every dot/norm to the host (CUBLAS scalar readback = one sync per reduction).
// Here all recurrence scalars stay in ctx->d_scalars: a reduction leaves per-workgroup partial sums
// and the NEXT kernel's workgroups each re-reduce those partials (<= 4096 doubles, L2 resident) in a
// fixed order, so there is no finalize launch, no atomic and the result is bitwise reproducible.  The
// convergence test of the reference (normalized_norm(r) <= tol || iter >= maxiter, evaluated every
// iteration) is evaluated on device into a DONE flag that turns the remaining enqueued kernels into
// no-ops; the host polls it every `check_every` iterations.
#include "krylov.h"
#include "solve_decide.h"
#include "operator.h"
#include "mesh_operator_decide.h"
#include "brick_multigrid.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------
// generic small kernels
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MFEM_BLOCK) void k_fill(int64_t n, double v, double* __restrict__ x) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) x[i] = v;
}

// d <- sqrt(d), t <- 1 / sqrt(d) ; out[0] = max, out[1] = min over the new d (bit patterns of non-negative doubles; out[1] starts huge)
__global__ __launch_bounds__(MFEM_BLOCK) void k_sqrt_max(int64_t n, double* __restrict__ d, double* __restrict__ t, unsigned long long* __restrict__ out) {
  double m = 0.0, lo = __builtin_huge_val();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = sqrt(d[i]);
    d[i] = v;
    t[i] = 1.0 / v;
    m = fmax(m, v == v ? v : __builtin_huge_val());
    lo = fmin(lo, v == v ? v : 0.0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmax(m, __shfl_down(m, o, MFEM_WAVE));
    lo = fmin(lo, __shfl_down(lo, o, MFEM_WAVE));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(out, (unsigned long long)__double_as_longlong(m));
    atomicMin(out + 1, (unsigned long long)__double_as_longlong(lo));
  }
}

// y = 1 / x  (only the first n entries; the pad stays 0)
__global__ __launch_bounds__(MFEM_BLOCK) void k_recip(int64_t n, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) y[i] = 1.0 / x[i];
}

// y = x ./ d
__global__ __launch_bounds__(MFEM_BLOCK) void k_div(int64_t n, const double* x, const double* __restrict__ d,
                                                      double* y) {  // y may alias x
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) y[i] = x[i] / d[i];
}

// y = x .* d
__global__ __launch_bounds__(MFEM_BLOCK) void k_mul(int64_t n, const double* x, const double* __restrict__ d,
                                                      double* y) {  // y may alias x
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) y[i] = x[i] * d[i];
}

int mfem_fill(mfem_context_s* ctx, int64_t n, double v, double* x) {
  if (n == 0) return MFEM_OK;
  hipLaunchKernelGGL(k_fill, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, v, x);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// r = b - A x  and  S[slot] = r.r   (start of every Sv body: mul!(r, A, x, -1.); r .+= b)
// n = owned entries: behind them r may carry ghost entries (stale copies of neighbours' values) that must not be summed
__global__ __launch_bounds__(MFEM_BLOCK) void k_resid_finish(int64_t n, const d2_t* __restrict__ b, d2_t* __restrict__ r,
                                                               double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n2 = n >> 1;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += stride) {
    const d2_t v = r[i] + b[i];
    r[i] = v;
    acc += v.x * v.x + v.y * v.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double* rs = reinterpret_cast<double*>(r);
    const double v = rs[n - 1] + reinterpret_cast<const double*>(b)[n - 1];
    rs[n - 1] = v;
    acc += v * v;
  }
  const double s = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

int mfem_true_residual(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* b, const double* x,
                       double* r, double* d_rr) {
  // r = -A x ; r += b ; *d_rr = r.r  (device scalar, all-reduced over ranks when a communicator is attached)
  int rc = mfem_spmv_halo(ctx, A, vals, const_cast<double*>(x), r, -1.0, 0.0, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const int grid = mfem_vec_grid(ctx, A->n);
  hipLaunchKernelGGL(k_resid_finish, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, (const d2_t*)b, (d2_t*)r,
                     ctx->d_partials);
  MFEM_CHECK_LAUNCH();
  rc = mfem_sum_partials(ctx, ctx->d_partials, grid, d_rr);
  if (rc) return rc;
  if (ctx->comm) return mfem_comm_allreduce(ctx, d_rr, 1);
  return MFEM_OK;
}

// r = b, partial sums of b.b: k_resid_finish without its read of r (the SpMV of a zero vector leaves +-0 there: r + b = b)
__global__ __launch_bounds__(MFEM_BLOCK) void k_resid_from_b(int64_t n, const d2_t* __restrict__ b, d2_t* __restrict__ r, double* __restrict__ partials) {
  __shared__ double red[MFEM_BLOCK / MFEM_WAVE];
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += stride) {
    const d2_t v = b[i];
    r[i] = v;
    acc += v.x * v.x + v.y * v.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double v = reinterpret_cast<const double*>(b)[n - 1];
    reinterpret_cast<double*>(r)[n - 1] = v;
    acc += v * v;
  }
  const double s = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

int mfem_pass_residual(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const KrylovVecs& V, double* r, double* d_rr, int* spmv_out) {
  if (!V.x_zero) {
    ++*spmv_out;
    return mfem_true_residual(ctx, A, vals, V.b, V.x, r, d_rr);
  }
  const int grid = mfem_vec_grid(ctx, A->n);
  hipLaunchKernelGGL(k_resid_from_b, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, (const d2_t*)V.b, (d2_t*)r, ctx->d_partials);
  MFEM_CHECK_LAUNCH();
  int rc = mfem_sum_partials(ctx, ctx->d_partials, grid, d_rr);
  if (rc) return rc;
  if (ctx->comm) return mfem_comm_allreduce(ctx, d_rr, 1);
  return MFEM_OK;
}

int mfem_read_scalars(mfem_context_s* ctx, int first, int count) {
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_scalars + first, ctx->d_scalars + first, sizeof(double) * count,
                                hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return MFEM_OK;
}

// A host number summed over the ranks of the attached communicator: up through S[S_TMP0], one all-reduce, read back
static int sum_over_ranks(mfem_context_s* ctx, double mine, double* sum) {
  ctx->h_scalars[S_TMP0] = mine;
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->d_scalars + S_TMP0, ctx->h_scalars + S_TMP0, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  int rc = mfem_comm_allreduce(ctx, ctx->d_scalars + S_TMP0, 1);
  if (!rc) rc = mfem_read_scalars(ctx, S_TMP0, 1);
  if (rc) return rc;
  *sum = ctx->h_scalars[S_TMP0];
  return MFEM_OK;
}

int mfem_read_flags(mfem_context_s* ctx) {
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags, ctx->d_flags, sizeof(int32_t) * 8, hipMemcpyDeviceToHost, ctx->stream));  // two banks of 4 (classic CG alternates)
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return MFEM_OK;
}

// ------------------------------------------------------------------------------------------
// iterative_Solve! wrapper
// ------------------------------------------------------------------------------------------
extern "C" int mfem_solve_set_shadow(mfem_context ctx, const double* shadow, int32_t count) try {
  MFEM_REQUIRE(ctx, "null ctx");
  MFEM_REQUIRE(count >= 0, "negative count");
  ctx->shadow = shadow;
  ctx->shadow_count = shadow ? count : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_solve_set_shadow")

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static std::atomic<int> g_ws_trial{0};           // timed choice between allocations of a large workspace: OPT-IN since round 4 (mfem_debug_set_ws_trial)
extern "C" int mfem_debug_set_ws_trial(int on) try {
  g_ws_trial = on ? 1 : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_ws_trial")
extern "C" int mfem_debug_ws_trial_log(mfem_context ctx, double* out4) try {  // times of the candidates tried (ms for two SpMVs; 0: not tried)
  MFEM_REQUIRE(ctx && out4, "null argument");
  for (int i = 0; i < 4; ++i) out4[i] = ctx->ws_log[i];
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_ws_trial_log")
static std::atomic<int64_t> g_cg_single_max_rows{20000000};  // rows per rank below which the auto choice with a communicator is the single-reduction CG (mfem_debug_set_cg_single_max_rows)
extern "C" int mfem_debug_set_cg_single_max_rows(int64_t rows) try {
  g_cg_single_max_rows = rows;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_cg_single_max_rows")
std::atomic<int> mfem_graph_comm_broken{0};    // a capture with RCCL calls failed once: never tried again in this process
std::atomic<long long> mfem_graph_comm_captures{0};  // cycles captured with a communicator attached (tests)
std::atomic<long long> mfem_graph_launches{0};       // cycle graphs launched, first launches after a capture included (tests)
static std::atomic<int> g_graphs{1};             // hipGraph replay of solver cycles (mfem_debug_set_graphs)
static std::atomic<int64_t> g_graph_max_n{4000000};  // above this size kernels are long enough that launch latency is hidden anyway
// Cycle graphs WITH a communicator (round 6): off unless asked for -- MFEM_GRAPH_COMM=1 in the environment or bit 1 of
// mfem_debug_set_graphs -- because RCCL with more than one rank has never executed on this pool (no >= 2-GPU box): the un-captured sequence stays the
// reference, tests/test_gpu_multirank.py (armed, skipif < 2 GPUs) compares the two.  What is captured: ncclAllReduce on the context stream, and the halo
// exchange's fork (event on the context stream -> halo stream: grouped ncclSend / ncclRecv) and join (event back); a capture that fails falls back to
// the direct launches for the rest of the process (mfem_cycle_run).
static std::atomic<int> g_graph_comm{-1};  // -1: ask the environment on first use
static bool graph_comm_wanted() {
  int v = g_graph_comm;
  if (v < 0) {
    const char* e = getenv("MFEM_GRAPH_COMM");
    v = (e && e[0] == '1') ? 1 : 0;
    g_graph_comm = v;
  }
  return v == 1;
}
extern "C" int mfem_debug_graph_comm_count(void) { return (int)mfem_graph_comm_captures; }
extern "C" long long mfem_debug_graph_launch_count(void) { return mfem_graph_launches; }
extern "C" int mfem_debug_set_graphs(int on, int64_t max_n) try {
  ++mfem_debug_epoch;
  g_graphs = (on & 1) ? 1 : 0;
  g_graph_comm = (on & 2) ? 1 : 0;
  if (max_n > 0) g_graph_max_n = max_n;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_graphs")

// TEST HOOK: the residual recomputed from the caller's CSR values (the recheck of a tile solve) is multiplied by this factor -- 1.2 makes the two residuals
// straddle the tolerance after a pass that the tiles' copy ends, the situation the tightened next pass exists for (tests/test_gpu_remainder.py)
static std::atomic<double> g_recheck_scale{1.0};
extern "C" int mfem_debug_set_recheck_scale(double scale) try {
  ++mfem_debug_epoch;
  g_recheck_scale = scale > 0.0 ? scale : 1.0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_recheck_scale")

// The solvers, per mfem_solver_kind: the l_or_s a zero selects, the work vectors for it, whether a communicator is refused, the pass
struct KrylovMethod {
  const char* name;
  int default_s;
  int max_s;  // (tfqmr!: l_or_s is checkiter, not a vector count)
  int (*nwork)(int s);
  bool one_rank;
  mfem_pass_fn* pass;
};
static const KrylovMethod k_methods[] = {
    {"cg!", 2, MFEM_MAX_S, [](int) { return 3; }, false, mfem_cg_pass},  // r, p, Ap (+ m - 1 further slots of the ring of directions: cg_work_vectors)
    {"bicgstabl_GS!", 2, MFEM_MAX_S, [](int l) { return 2 * (l + 1) + 1; }, false, mfem_bicgstabl_pass},  // R[0..l], U[0..l], r~
    {"idrs!", 4, MFEM_MAX_S, [](int s) { return 3 * s + 4; }, false, mfem_idrs_pass},
    {"cgs2!", 2, MFEM_MAX_S, [](int) { return 9; }, false, mfem_cgs2_pass},
    // gmres!: s = 20 by default (05_GMRES.jl:48).  No multi-rank form: it would need an all-reduce of up to s + 1 scalars per orthogonalisation pass
    {"gmres!", 20, MFEM_MAX_S, [](int s) { return s + 2; }, true, mfem_gmres_pass},  // r, Q_1 .. Q_(s+1)
    // cgs!, tfqmr!, lsqr!: one rank as well (lsqr!'s transposed product would need the halo reduction of mfem_halo_reduce)
    {"cgs!", 2, MFEM_MAX_S, [](int) { return 6; }, true, mfem_cgs_pass},  // r, r0, u, p, s, v
    {"tfqmr!", 200, INT32_MAX, [](int) { return 9; }, true, mfem_tfqmr_pass},  // r, r0, r_cgs, p, q, u, v, d, tmp; checkiter 200 by default (08_QMR.jl:4)
    {"lsqr!", 2, MFEM_MAX_S, [](int) { return 5; }, true, mfem_lsqr_pass},  // r, u, v, w, tmp
};
// cg! with one reduction group per iteration: r, p, s, u, w
static const KrylovMethod k_cg_single = {"cg!", 2, MFEM_MAX_S, [](int) { return 5; }, false, mfem_cg_single_pass};
// cg! with the multigrid V-cycle (MFEM_PRECOND_MULTIGRID, one rank, a hex-8 thermal brick operator): r, p, Ap, z
static const KrylovMethod k_cg_mg = {"cg!", 2, MFEM_MAX_S, [](int) { return 4; }, true, mfem_cg_mg_pass};
// gmres! with the multigrid V-cycle as its right preconditioner (a nonsymmetric hierarchy attached: mg_solve_refusal_nonsym): r, Q_1 .. Q_(s+1), z
static const KrylovMethod k_gmres_mg = {"gmres!", 20, MFEM_MAX_S, [](int s) { return s + 3; }, true, mfem_gmres_mg_pass};
static_assert(sizeof(k_methods) / sizeof(k_methods[0]) == MFEM_SOLVER_LSQR + 1, "one row per mfem_solver_kind");

// The work vectors of this solve and how many of them (with the four in front) start cleared.  mfem_cg_pass keeps a ring of m search directions
// (cg_decide.h): its slots beyond p follow the method's three vectors.  Every slot is written in full before it is read (k_cg_init, k_cg_pupdate), so
// they are left out of the per-solve clear -- 1.3 ms per solve at 512^3 with m = 8.
static void cg_work_vectors(const KrylovMethod* method, int s_param, KrylovVecs& V, int* nclear) {
  V.nwork = method->nwork(s_param);
  *nclear = 4 + V.nwork;
  V.cg_ring = 1;
  if (method->pass == mfem_cg_pass) {
    V.cg_ring = mfem_cg_ring_depth(V.nv);
    V.nwork += V.cg_ring - 1;
  }
}

// What the stages of one mfem_solve share: the arguments, what choose_method derives from them once per solve, and what one attempt sets up.  A stage
// that cannot go on with this attempt says so in `next`; solve_inner then runs the set-up again from plan_layouts.
enum SolveNext { GO_ON = 0, START_OVER, START_OVER_NO_TILES };
struct SolveRun {
  mfem_context_s* ctx;
  mfem_csr_s* A;
  double* vals;
  const double* b;
  double* x_out;
  const mfem_solve_options* o;
  mfem_solve_stats* stats;
  // per solve (choose_method)
  const KrylovMethod* method;
  int s_param;
  int64_t n_global;  // rows of the whole system
  double n_inv;      // 1 / n_global
  bool is_cg, jac, left, is_lsqr;
  bool mg = false;  // MFEM_PRECOND_MULTIGRID (mfem_solve_operator on a hex-8 thermal or elasticity brick operator: the gate has passed)
  bool allow_lat;  // false: the symmetric lattice tiles have refused this solve's values (they are not tried again in this call)
  // per attempt
  SolveNext next;
  bool fused_scale, need_copy, scaled_copy, gather_early;
  mfem_layout_plan_s lp;
  mfem_tplan_s* tplan;  // lsqr!: the transposed pattern
  size_t vec_bytes, csr_copy_bytes, layout_bytes, gm_offset, total;
  int nclear;  // vectors at the front of the workspace that start cleared (cg_work_vectors)
  KrylovVecs V;
  double* dinv_buf;        // CG: 1 / d (scaled CG: 1 / S); otherwise the left scaling dl
  double* vals_work;       // the values the passes run on: the caller's, or the working copy
  const double* vals_src;  // what the right scaling is computed from
  double* lay;             // the layout copy
  bool tiles_bound, rows_bound, cg_scaled;
  mfem_operator_head* op = nullptr;  // mfem_solve_operator: A is the operator's pattern-less handle, vals is null
  const mfem_operator_interface* opi = nullptr;  // ... and its kind's table (operator.h)
};

// 1. the options; the method (with a communicator: the one all-reduce of n, every rank must take the same decisions)
static int choose_method(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  const mfem_solve_options* o = R.o;
  double *vals = R.vals, *x_out = R.x_out;
  const double* b = R.b;
  MFEM_REQUIRE(A->n == 0 || ((vals || R.op) && b && x_out), "null array");
  MFEM_REQUIRE(o->maxiter >= 0 && o->max_pass >= 1, "maxiter >= 0 and max_pass >= 1 required");
  MFEM_REQUIRE(o->method >= MFEM_SOLVER_CG && o->method <= MFEM_SOLVER_LSQR, "unknown method");
  MFEM_REQUIRE((o->precond >= MFEM_PRECOND_NONE && o->precond <= MFEM_PRECOND_JACOBI_RIGHT_COLNORM) || R.mg, "unknown precond");
  MFEM_REQUIRE(o->left_precond >= MFEM_LEFT_NONE && o->left_precond <= MFEM_LEFT_JACOBI_ROWNORM, "unknown left_precond");
  MFEM_REQUIRE(!(o->left_precond && o->method == MFEM_SOLVER_CG), "left Jacobi would break the symmetry CG needs");
  if (R.stats) memset(R.stats, 0, sizeof(*R.stats));
  const int64_t n = A->n;
  if (n == 0) return MFEM_OK;
  const KrylovMethod* method = &k_methods[o->method];
  if (method->one_rank && ctx->comm) {
    mfem_set_error("%s runs on one rank only: no communicator may be attached", method->name);
    return MFEM_ERR_INVALID;
  }
  const int s_param = o->l_or_s > 0 ? o->l_or_s : method->default_s;
  MFEM_REQUIRE(o->cg_variant >= 0 && o->cg_variant <= 4, "cg_variant must be 0 (auto), 1 (classic), 2 (single reduction), 3 (classic, preconditioned residual carried) or 4 (plain CG on the symmetrically scaled matrix)");
  R.n_global = n;
  if (ctx->comm) {
    double sum = 0.0;
    const int rcg = sum_over_ranks(ctx, (double)n, &sum);
    if (rcg) return rcg;
    R.n_global = (int64_t)(sum + 0.5);
  }
  // One reduction group per CG iteration where a reduction costs an all-reduce -- as long as the all-reduce it saves (~30 us on a node) is worth more than
  // the vector stream the single-reduction form adds (9 against 8: n * 8 B at ~5.3 TB/s).  Break-even near 2e7 rows per rank (round 4: design figures,
  // no multi-GPU box): above it -- 512^3 per rank: 0.2 ms of stream against 0.03 ms of all-reduce per iteration -- the classic recurrence runs with a
  // communicator too.  Decided on n_global / world: the same on every rank.
  const int world_ranks = mfem_comm_world(ctx);
  if (o->method == MFEM_SOLVER_CG &&
      (o->cg_variant == 2 || (o->cg_variant == 0 && world_ranks > 1 && R.n_global / world_ranks < g_cg_single_max_rows)))
    method = &k_cg_single;
  if (R.mg) method = o->method == MFEM_SOLVER_GMRES ? &k_gmres_mg : &k_cg_mg;  // (the gate admits no other method)
  R.n_inv = 1.0 / (double)R.n_global;
  MFEM_REQUIRE(s_param <= method->max_s, "l_or_s too large");
  R.method = method;
  R.s_param = s_param;
  R.is_lsqr = o->method == MFEM_SOLVER_LSQR;
  R.is_cg = o->method == MFEM_SOLVER_CG;
  R.jac = o->precond != MFEM_PRECOND_NONE && !R.mg;  // (the cycle is applied by the pass itself: no diagonal scaling)
  R.left = o->left_precond != MFEM_LEFT_NONE;
  return MFEM_OK;
}

// 2a. the layouts this attempt may bind, whether the scaling is left to their bind or needs a working copy, the size of the workspace: x, b (padded
// copies), d, dinv (CG) / left scaling dl, work vectors, optional matrix copy, the layout copy
static int plan_layouts(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  const mfem_solve_options* o = R.o;
  const bool is_cg = R.is_cg, jac = R.jac, left = R.left;
  R.tiles_bound = R.rows_bound = R.cg_scaled = false;
  R.V = KrylovVecs{};
  R.V.n = A->n;
  // x may carry ghost entries behind the owned rows (slab decomposition)
  const int64_t ghosts = ctx->comm ? 2 * ctx->halo_plane_len * ctx->halo_fields : 0;
  const int64_t nv = R.V.nv = (int64_t)align_up((size_t)(A->n + ghosts), 32);  // padded vector length (even => d2 kernels)
  cg_work_vectors(R.method, R.s_param, R.V, &R.nclear);
  const int nwork = R.V.nwork;
  // lsqr!: the transposed pattern, planned on the first lsqr! solve (or mfem_spmv_csr_t) and kept on the handle
  R.tplan = nullptr;
  if (R.is_lsqr) {
    const int rct = mfem_tplan_get(ctx, A, &R.tplan);
    if (rct) return rct;
  }
  // Right Jacobi on a solver layout: the column scaling is applied while the layout copy is made (Mat_Div_Jacobi folded into the bind), so
  // the scaled matrix exists only in that copy -- no scaled CSR copy, no scaling pass.  Not with a left preconditioner (it reads the
  // scaled CSR values) and not with scale_in_place (the caller wants `vals` scaled, Pr_Jacobi! semantics).
  R.fused_scale = jac && !is_cg && !left && !o->scale_in_place;
  const bool need_copy_unfused = ((jac && !is_cg) || left) && !o->scale_in_place;
  R.vec_bytes = (size_t)nv * sizeof(double);
  // Solver layouts (layout.hip): symmetric lattice tiles first, one rank, solver on the unscaled or right-scaled matrix -- taken if this solve's
  // values are symmetric (decided by the bind); a right Jacobi scaling is applied to x there, not to the stored matrix.  While a pattern's values have
  // never been refused, the row layouts are not even planned; the first refusal plans them and the solve starts over.  A row layout's copy of the
  // working values is made once per solve after the scaling.
  int rc = mfem_layout_plan(ctx, A, is_cg, R.allow_lat && !left && (is_cg || !jac || R.fused_scale), &R.lp);
  if (rc) return rc;
  // (the CSR kernel of small systems reads the caller's array: it needs the scaled copy.  Planned tiles keep the scaling fused -- they take the caller's
  // UNSCALED values and apply a right scaling to x; should they refuse the values with no other layout to carry the fused scaling, the solve starts
  // over without them, bind_tiles)
  R.fused_scale = R.fused_scale && (R.lp.tile || R.lp.rows);
  R.need_copy = need_copy_unfused && !R.fused_scale;
  // The tiles are never bound from a scaled working copy (it lives in the workspace and is filled only further down); cannot happen with the rule
  // above, kept as the invariant's guard
  if (R.need_copy && jac && !is_cg) R.lp = mfem_layout_plan_s{MFEM_LAYOUT_CSR, R.lp.rows, 0, R.lp.rows_bytes};
  R.csr_copy_bytes = R.need_copy ? align_up((size_t)A->nnz * sizeof(double), 256) : 0;
  R.layout_bytes = R.lp.tile_bytes > R.lp.rows_bytes ? R.lp.tile_bytes : R.lp.rows_bytes;
  R.total = R.vec_bytes * (4 + nwork) + R.csr_copy_bytes + R.layout_bytes;
  R.gm_offset = align_up(R.total, 256);  // gmres!: H, y and the block-dot partials behind everything else
  if (o->method == MFEM_SOLVER_GMRES) R.total = R.gm_offset + mfem_gmres_workspace_bytes();
  if (R.is_lsqr) R.total = R.gm_offset + (size_t)A->nnz * sizeof(double);  // lsqr!: the values of the transposed working matrix, behind everything else
  return MFEM_OK;
}

// 2b. the workspace reserved, cleared and carved; the working copy started, b copied
static int carve_workspace(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  const mfem_solve_options* o = R.o;
  KrylovVecs& V = R.V;
  const int64_t n = A->n;
  const int nwork = V.nwork;
  int rc = mfem_ws_reserve(ctx, R.total);
  if (rc) return rc;
  char* base = (char*)ctx->ws;
  MFEM_CHECK_HIP(hipMemsetAsync(base, 0, R.vec_bytes * R.nclear, ctx->stream));
  V.x = (double*)(base);
  V.b = (double*)(base + R.vec_bytes);
  V.d = (double*)(base + 2 * R.vec_bytes);
  R.dinv_buf = (double*)(base + 3 * R.vec_bytes);
  for (int i = 0; i < nwork; ++i) V.w[i] = (double*)(base + (4 + i) * R.vec_bytes);
  if (o->method == MFEM_SOLVER_GMRES) V.gm = (double*)(base + R.gm_offset);
  if (R.is_lsqr) {
    V.AT = R.tplan->AT;
    V.valsT = (double*)(base + R.gm_offset);
  }
  R.vals_work = R.vals;
  // right Jacobi scaling of a working copy: the scaling kernel writes the copy straight from the caller's values (no copy pass first)
  R.scaled_copy = R.need_copy && R.jac && !R.is_cg;
  R.lay = (double*)(base + R.vec_bytes * (4 + nwork) + R.csr_copy_bytes);
  if (R.need_copy) {
    R.vals_work = (double*)(base + R.vec_bytes * (4 + nwork));
    if (!R.scaled_copy) MFEM_CHECK_HIP(hipMemcpyAsync(R.vals_work, R.vals, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  R.vals_src = R.scaled_copy ? R.vals : R.vals_work;
  MFEM_CHECK_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  MFEM_CHECK_HIP(hipMemcpyAsync(V.b, R.b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  // lsqr!'s A' is built from the caller's values, not from the working matrix (left_precond).  scale_in_place overwrites them: gather them first.
  R.gather_early = R.is_lsqr && o->scale_in_place && (R.jac || R.left);
  if (R.gather_early) {
    rc = mfem_tplan_gather(ctx, R.tplan, R.vals, V.valsT, nullptr, nullptr);
    if (rc) return rc;
  }
  return MFEM_OK;
}

// 3. symmetric lattice tiles: bound first, before anything is communicated (a refusal starts over) -- the Jacobi step then takes |diag| from the CSR
// values; only the pointer of the column scaling is handed over here, the SpMVs read it after it has been filled.
// (the first three work vectors serve the bind's probe product and are cleared again)
static int bind_tiles(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  if (!R.lp.tile) return MFEM_OK;
  // (values that are nonsymmetric in a few rows only -- Nitsche / SUPG faces -- keep the tiles and carry a sparse remainder, spmv_rem.hip; not for cg!,
  // which is not defined on such a matrix: its refusal keeps the reproducible layouts)
  const int rc = mfem_layout_bind(ctx, A, R.lp.tile, R.vals_work, R.lay, R.fused_scale ? R.V.d : nullptr, nullptr, R.V.w[0], !R.is_cg);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipMemsetAsync(R.V.w[0], 0, R.vec_bytes * 3, ctx->stream));
  R.tiles_bound = mfem_layout_bound(A, R.vals_work) == R.lp.tile;
  if (!R.tiles_bound && (!A->lat_refused || (R.fused_scale && !R.lp.rows))) {
    // refused: no other layout was planned beside the tiles (first refusal on this pattern), or none exists at this size to carry the fused
    // scaling -- start over without the tiles (the other layouts get planned; a scaled copy is made where the CSR kernel serves)
    // (lat_refused only makes later solves on this pattern plan the other layouts up front -- the tiles are still tried first by every solve, and
    // serve it again as soon as the values pass: tests/test_gpu_remainder.py::test_refusal_is_not_sticky)
    A->lat_refused = 1;
    R.next = START_OVER_NO_TILES;
  }
  return MFEM_OK;
}

// 4a. cg_variant 4: plain CG on S^-1 A S^-1, S = sqrt|diag A| -- the Jacobi-preconditioned iteration in the variables S x, without the stream of
// 1 / d in its vector kernels (8 instead of 9 per iteration).  The scaling is folded into the diagonal-slotted layout copy (mode 2: plain or
// mirrored kernels alike -- a bitwise symmetric matrix stays one), one rank; otherwise cg_scaled stays false and the classic recurrence runs.
// (auto: not for passes of fewer than 64 iterations -- the scaled copy and its S vectors cost 1.2 ms more per solve at 256^3 than the plain
// path, an iteration saves 0.026 ms there: tools/cg_per_solve.py)
static int try_scaled_cg(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  const mfem_solve_options* o = R.o;
  KrylovVecs& V = R.V;
  const int64_t n = A->n;
  if (!(R.jac && R.is_cg && (o->cg_variant == 4 || (o->cg_variant == 0 && o->maxiter >= 64)) && o->precond != MFEM_PRECOND_JACOBI_RIGHT_COLNORM && !R.left &&
        R.lp.rows == MFEM_LAYOUT_DIA && !R.tiles_bound))
    return MFEM_OK;
  int rc = mfem_fill(ctx, n, 1.0, V.d);
  if (!rc) rc = mfem_jacobi_diag_launch(ctx, A, R.vals_work, V.d, 0);
  if (rc) return rc;
  unsigned long long* d_stat = (unsigned long long*)(ctx->d_flags + 12);  // [12,13]: max, [14,15]: min
  MFEM_CHECK_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long), ctx->stream));
  MFEM_CHECK_HIP(hipMemsetAsync(d_stat + 1, 0x7f, sizeof(unsigned long long), ctx->stream));  // (0x7f7f...: a huge finite double)
  hipLaunchKernelGGL(k_sqrt_max, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, V.d, R.dinv_buf, d_stat);  // S and 1 / S
  MFEM_CHECK_LAUNCH();
  if (ctx->comm) {  // the ghost columns are scaled by their owners' 1 / S
    rc = mfem_comm_halo(ctx, R.dinv_buf);
    if (rc) return rc;
  }
  rc = mfem_layout_bind(ctx, A, R.lp.rows, R.vals_work, R.lay, nullptr, R.dinv_buf, nullptr, false);  // (synchronises: the check's verdict)
  if (rc) return rc;
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 12, d_stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  double s_max = 1.0, s_min = 0.0;
  memcpy(&s_max, ctx->h_flags + 12, sizeof(double));
  memcpy(&s_min, ctx->h_flags + 14, sizeof(double));
  bool ok = mfem_layout_bound(A, R.vals_work) == MFEM_LAYOUT_DIA && s_min > 0.0 && s_max < __builtin_huge_val();
  if (ctx->comm) {  // every rank iterates on the same system: scaled only if all of them can
    double sum = 0.0;
    rc = sum_over_ranks(ctx, ok ? 1.0 : 0.0, &sum);
    if (rc) return rc;
    ok = (int)(sum + 0.5) == mfem_comm_world(ctx);
  }
  if (!ok) {
    mfem_layout_unbind(A);  // (no diagonal-slotted copy after all, or a zero / non-finite diagonal: the classic recurrence on an unscaled copy)
    return MFEM_OK;
  }
  R.cg_scaled = true;
  R.rows_bound = true;
  V.cg_s = V.d;
  V.cg_smax = s_max;
  V.cg_smin = s_min;
  hipLaunchKernelGGL(k_mul, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, V.b, R.dinv_buf, V.b);  // b^ = S^-1 b
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// 4b. Pr = Pr_func!(A)   (02_Preconditioner.jl:38, 103-120): the Jacobi vector; 1 / d for CG, else the matrix scaled by it unless a layout bind does that
static int right_jacobi(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  const mfem_solve_options* o = R.o;
  KrylovVecs& V = R.V;
  const int64_t n = A->n;
  int rc;
  if (o->precond == MFEM_PRECOND_JACOBI_RIGHT_COLNORM && !R.is_cg) {
    rc = mfem_jacobi2_by_column(ctx, A, R.vals_src, V.d);
  } else if (R.is_cg && (R.lp.rows == MFEM_LAYOUT_ELL || R.lp.rows == MFEM_LAYOUT_DIA) && !R.tiles_bound) {
    // CG does not scale the matrix: transpose first and read |diag| from the copy (n values instead of all nonzeros)
    rc = mfem_layout_bind(ctx, A, R.lp.rows, R.vals_work, R.lay, nullptr, nullptr, nullptr, false);
    if (!rc && mfem_layout_bound(A, R.vals_work) != MFEM_LAYOUT_CSR) {
      R.rows_bound = true;
      rc = mfem_ell_diag(ctx, A, V.d);
    } else if (!rc) {
      rc = mfem_fill(ctx, n, 1.0, V.d);
      if (!rc) rc = mfem_jacobi_diag_launch(ctx, A, R.vals_work, V.d, 0);
    }
  } else {
    rc = mfem_fill(ctx, n, 1.0, V.d);
    if (!rc) rc = mfem_jacobi_diag_launch(ctx, A, R.vals_src, V.d, 0);
  }
  if (rc) return rc;
  if (R.is_cg) {
    hipLaunchKernelGGL(k_recip, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, V.d, R.dinv_buf);
    MFEM_CHECK_LAUNCH();
    V.dinv = R.dinv_buf;
    return MFEM_OK;
  }
  if (ctx->comm && o->precond != MFEM_PRECOND_JACOBI_RIGHT_COLNORM) {  // ghost columns need their owners' d (the column
    rc = mfem_comm_halo(ctx, V.d);                                      // norm comes with them, mfem_jacobi2_by_column)
    if (rc) return rc;
  }
  if (!R.fused_scale) rc = mfem_mat_div_jacobi_from(ctx, A, R.vals_src, R.vals_work, V.d);
  return rc;
}

// 5. Pl = Pl_func(A)   (:40, 155-168), taken from the matrix Pr has already scaled.  D_l^-1 (A v) == (D_l^-1 A) v, so the
// rows of the working matrix and b are divided once instead of dividing every mat-vec result.  Then lsqr!'s transposed working values.
static int left_precond(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  KrylovVecs& V = R.V;
  const int64_t n = A->n;
  double* dl = R.dinv_buf;
  int rc = MFEM_OK;
  if (R.left) {
    if (R.o->left_precond == MFEM_LEFT_JACOBI_ROWNORM) {
      rc = mfem_jacobi_diag_launch(ctx, A, R.vals_work, dl, 1);
    } else {
      rc = mfem_fill(ctx, n, 1.0, dl);
      if (!rc) rc = mfem_jacobi_diag_launch(ctx, A, R.vals_work, dl, 0);
    }
    if (!rc) rc = mfem_mat_div_rows(ctx, A, R.vals_work, dl);
    if (rc) return rc;
    hipLaunchKernelGGL(k_div, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, V.b, dl, V.b);
    MFEM_CHECK_LAUNCH();
  }
  // lsqr!: the reference's v = Pl(tmul!(A_r, u)) (06_LSQR.jl:23-24, 42-43) is P A_r' u, A_r = A C the Pr_Jacobi!-scaled matrix (C = 1 / d) and
  // P = 1 / dl the left scaling taken from A_r -- not the transpose of the row-scaled working matrix (P A_r)' = A_r' P.  Row i of the transposed
  // working matrix is therefore (a(j, i) / d_i) / dl_i, gathered from the caller's values on every path: the fused-scale layouts keep no scaled
  // CSR copy, the lattice tiles apply the right scaling to x, and scale_in_place has overwritten them (gathered in carve_workspace, divided here).
  if (R.is_lsqr) rc = mfem_tplan_gather(ctx, R.tplan, R.gather_early ? nullptr : R.vals, V.valsT, R.jac ? V.d : nullptr, R.left ? dl : nullptr);
  return rc;
}

// 6. bind the row layout's copy: every mfem_spmv_launch(A, vals_work, ...) from here on runs its kernel
// (fused_scale: vals_work is the caller's unscaled array and only names the bound values; every SpMV runs on the scaled copy)
static int bind_rows(SolveRun& R) {
  if (!R.lp.rows || R.rows_bound || R.tiles_bound) return MFEM_OK;
  const int rc = mfem_layout_bind(R.ctx, R.A, R.lp.rows, R.vals_work, R.lay, R.fused_scale ? R.V.d : nullptr, nullptr, nullptr, false);
  if (rc) return rc;
  if (R.fused_scale && mfem_layout_bound(R.A, R.vals_work) == MFEM_LAYOUT_CSR) {
    mfem_set_error("solver layout could not be bound for the fused Jacobi scaling");
    return MFEM_ERR_INVALID;
  }
  return MFEM_OK;
}

// logical OR over the ranks
static int agree(mfem_context_s* ctx, bool mine, bool* any) {
  if (!ctx->comm) { *any = mine; return MFEM_OK; }
  double sum = 0.0;
  const int rc = sum_over_ranks(ctx, mine ? 1.0 : 0.0, &sum);
  if (rc) return rc;
  *any = sum > 0.5;
  return MFEM_OK;
}

// the time of two SpMVs on the bound layout in this workspace (after one that warms tables and code)
static int time_two_spmvs(SolveRun& R, float* ms) {
  mfem_context_s* ctx = R.ctx;
  KrylovVecs& V = R.V;
  const int prof = ctx->prof_on;
  ctx->prof_on = 0;
  ctx->probe_active = 1;
  hipEvent_t e0, e1;
  MFEM_CHECK_HIP(hipEventCreate(&e0));
  MFEM_CHECK_HIP(hipEventCreate(&e1));
  int rc = mfem_spmv_launch(ctx, R.A, R.vals_work, V.w[0], V.w[1], 1.0, 0.0, nullptr, nullptr, nullptr);  // (warm: tables, code)
  MFEM_CHECK_HIP(hipEventRecord(e0, ctx->stream));
  for (int k = 0; k < 2 && !rc; ++k) rc = mfem_spmv_launch(ctx, R.A, R.vals_work, V.w[0], V.w[1], 1.0, 0.0, nullptr, nullptr, nullptr);
  MFEM_CHECK_HIP(hipEventRecord(e1, ctx->stream));
  MFEM_CHECK_HIP(hipEventSynchronize(e1));
  MFEM_CHECK_HIP(hipEventElapsedTime(ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  ctx->prof_on = prof;
  ctx->probe_active = 0;
  if (rc) return rc;
  MFEM_CHECK_HIP(hipMemsetAsync(V.w[1], 0, R.vec_bytes, ctx->stream));  // (A * 0: zero anyway; the work vectors start clear)
  return MFEM_OK;
}

// 7. Placement of a large workspace (one rank; >= 8 GB: where the effect was seen): the SpMV on the bound layout runs at one of two speeds that
// follow the PHYSICAL memory the allocation received (profiles/r03_placement_probe.txt: 4.0 or 4.5 ms at 512^3, alternating between
// allocations).  The first solve on a workspace times two SpMVs, tries up to two more allocations (if memory allows; at most two alive) the
// same way and keeps the fastest (ws_trial_decide, solve_decide.h) -- the solve starts over on each candidate, like after a refused layout.  Once
// per workspace; the allocations themselves are what it costs (about 7 s at 512^3: hipMalloc / hipFree of 45 GB, twice).
// With a communicator (round 4: the same choice at N > 1 as at N = 1) the trial is rank-local -- its timing uses no collective -- but the START
// OVER is agreed: the set-up holds collectives, so all ranks repeat it together while any rank still has a candidate to try (two
// 1-scalar all-reduces per solve while the knob is on, none otherwise).
static int ws_trial(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  const bool in_trial = g_ws_trial && ctx->ws_try < 99 && R.total >= ((size_t)8 << 30) && !R.o->scale_in_place && R.layout_bytes > 0;
  bool any_trial = in_trial;
  int rc = MFEM_OK;
  if (g_ws_trial && ctx->comm) {
    rc = agree(ctx, in_trial, &any_trial);
    if (rc) return rc;
  }
  if (!any_trial) return MFEM_OK;
  bool restart = false;
  if (in_trial) {
    float ms = 0.f;
    rc = time_two_spmvs(R, &ms);
    if (rc) return rc;
    const int tried = ctx->ws_try;
    if (tried >= 0 && tried < 3) ctx->ws_log[tried] = ms;
    switch (ws_trial_decide(tried, ms, ctx->ws_try_ms)) {
      case WS_ALLOC_FIRST:
        ctx->ws_try_ms = ms;
        rc = mfem_ws_next_candidate(ctx);  // (the first stays alive as the alternative)
        if (rc) return rc;
        if (ctx->ws_try == 1) restart = true;
        else ctx->ws_try = 99;  // no memory for a second one: the first stays
        break;
      case WS_KEEP:
        rc = mfem_ws_decide(ctx, true);
        break;
      case WS_BACK:
        rc = mfem_ws_decide(ctx, false);
        restart = true;
        break;
      case WS_SWAP_ALLOC_NEXT: {
        void* t = ctx->ws; ctx->ws = ctx->ws_alt; ctx->ws_alt = t;
        t = ctx->ws_raw; ctx->ws_raw = ctx->ws_alt_raw; ctx->ws_alt_raw = t;
        ctx->ws_try_ms = ms;
      }
        [[fallthrough]];
      case WS_ALLOC_NEXT:
        rc = mfem_ws_next_candidate(ctx);
        if (rc) return rc;
        if (ctx->ws_try == tried) rc = mfem_ws_decide(ctx, true);  // (no memory: what is left stays)
        restart = true;
        break;
    }
    if (rc) return rc;
  }
  if (ctx->comm) {
    rc = agree(ctx, restart, &restart);
    if (rc) return rc;
  }
  if (restart) R.next = START_OVER;
  return MFEM_OK;
}

// return Pr(x) = x ./ d  (:75, 93-96)
static int unscale_to_x_out(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  const int64_t n = R.A->n;
  if (R.cg_scaled) {  // x = S^-1 x^
    hipLaunchKernelGGL(k_mul, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, R.V.x, R.dinv_buf, R.x_out);
    MFEM_CHECK_LAUNCH();
  } else if (R.jac && !R.is_cg) {
    hipLaunchKernelGGL(k_div, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, R.V.x, R.V.d, R.x_out);
    MFEM_CHECK_LAUNCH();
  } else {
    MFEM_CHECK_HIP(hipMemcpyAsync(R.x_out, R.V.x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return MFEM_OK;
}

// The symmetric lattice tiles store one triangle of a matrix that passed a symmetry GATE (LAT_SYM_GATE of the row's diagonal; a remainder, where one is
// carried, repairs the rows above it): a residual the caller is told -- and a residual that ENDS the passes -- must not come from that copy.  One
// product with the CSR kernel on the caller's own values: ||b - A x_out|| / sqrt(n), x_out = Pr(x) (one rank: x_out carries no ghost
// entries; not in benchmark mode, where bench.py does the same recomputation outside its timed region).  V.w[0] is free between passes.
static int csr_true_residual(SolveRun& R, int* spmvs, double* out) {
  mfem_context_s* ctx = R.ctx;
  const int64_t n = R.A->n;
  int rc = unscale_to_x_out(R);
  if (rc) return rc;
  {
    struct ForceCsr {  // (cleared on every way out, a C++ exception from a lazily made CSR plan included: ADVICE r5)
      mfem_context_s* c;
      explicit ForceCsr(mfem_context_s* c_) : c(c_) { c->force_csr = 1; }
      ~ForceCsr() { c->force_csr = 0; }
    } guard(ctx);
    rc = mfem_spmv_launch(ctx, R.A, R.vals, R.x_out, R.V.w[0], -1.0, 0.0, nullptr, nullptr, nullptr);
  }
  if (rc) return rc;
  ++*spmvs;
  const int grid = mfem_vec_grid(ctx, n);
  hipLaunchKernelGGL(k_resid_finish, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, n, (const d2_t*)R.V.b, (d2_t*)R.V.w[0], ctx->d_partials);  // (V.b: the aligned copy of b; unscaled on this path)
  MFEM_CHECK_LAUNCH();
  rc = mfem_sum_partials(ctx, ctx->d_partials, grid, ctx->d_scalars + S_RR);
  if (!rc) rc = mfem_read_scalars(ctx, S_RR, 1);
  if (rc) return rc;
  *out = sqrt(ctx->h_scalars[S_RR] * R.n_inv) * g_recheck_scale.load();  // (x 1 unless a test asks: mfem_debug_set_recheck_scale)
  return MFEM_OK;
}

// true residual between passes (:53-55) on the working matrix; with a left preconditioner, the tolerance factor of the next pass (:57-59)
static int residual_between_passes(SolveRun& R, double* res_out, double* tol_factor) {
  mfem_context_s* ctx = R.ctx;
  KrylovVecs& V = R.V;
  const int64_t n = R.A->n;
  int rc = mfem_true_residual(ctx, R.A, R.vals_work, V.b, V.x, V.w[0], ctx->d_scalars + S_RR);
  if (!rc) rc = mfem_read_scalars(ctx, S_RR, 1);
  if (rc) return rc;
  *res_out = sqrt(ctx->h_scalars[S_RR] * R.n_inv);
  if (!(R.left || R.cg_scaled)) return MFEM_OK;
  // w0 holds the row-scaled residual Pl(r) (scaled CG: S^-1 r): the one above is the preconditioned one; the true one is ||D_l w0|| (:57-59)
  const double pres = *res_out;
  hipLaunchKernelGGL(k_mul, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, V.w[0], R.cg_scaled ? V.d : R.dinv_buf, V.w[0]);
  MFEM_CHECK_LAUNCH();
  rc = mfem_dot_device(ctx, n, V.w[0], V.w[0], ctx->d_scalars + S_RR);
  if (rc) return rc;
  if (ctx->comm) {
    rc = mfem_comm_allreduce(ctx, ctx->d_scalars + S_RR, 1);
    if (rc) return rc;
  }
  rc = mfem_read_scalars(ctx, S_RR, 1);
  if (rc) return rc;
  const double res = *res_out = sqrt(ctx->h_scalars[S_RR] * R.n_inv);
  if (R.left) *tol_factor = res > 0.0 ? fmin(pres / res, 1.0) : 1.0;
  return MFEM_OK;
}

// 8. the passes, the residual between them, x_out and the statistics
static int run_passes(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  const mfem_solve_options* o = R.o;
  KrylovVecs& V = R.V;
  // initial residual for the report: b itself since x0 = 0 (:42-45)
  int rc = mfem_dot_device(ctx, A->n, R.b, R.b, ctx->d_scalars + S_TMP0);
  if (rc) return rc;
  if (ctx->comm) {
    rc = mfem_comm_allreduce(ctx, ctx->d_scalars + S_TMP0, 1);
    if (rc) return rc;
  }
  rc = mfem_read_scalars(ctx, S_TMP0, 1);
  if (rc) return rc;
  const double res0 = sqrt(ctx->h_scalars[S_TMP0] * R.n_inv);

  int pass = 1, total_iters = 0, spmvs = 0;
  V.x_zero = true;  // (the workspace was cleared in carve_workspace; nothing has written x since)
  double res = res0;
  double tol_factor = 1.0;  // only a left preconditioner moves it (:57-59); the scaled CG's kernels test the true residual themselves
  const bool csr_recheck = R.tiles_bound && !ctx->comm && !o->fixed_iterations;  // (csr_true_residual)
  bool res_from_csr = false;
  double prev_csr_res = -1.0;  // the caller's residual at the previous recheck that did not end the passes
  for (;;) {
    int it = 0;
    rc = R.method->pass(ctx, A, R.vals_work, V, o, R.s_param, tol_factor * o->converge_tol, R.n_global, &it, &spmvs);
    if (rc) return rc;
    V.x_zero = false;
    total_iters += it;
    rc = residual_between_passes(R, &res, &tol_factor);
    if (rc) return rc;
    ++spmvs;
    res_from_csr = false;
    if (csr_recheck && res < o->converge_tol) {  // the tiles' copy says converged: the caller's matrix decides (another pass runs if it disagrees)
      const double tile_res = res;
      rc = csr_true_residual(R, &spmvs, &res);
      if (rc) return rc;
      res_from_csr = true;
      // still above the tolerance: the next pass iterates to a tighter one, or the passes end here, not converged (solve_decide.h)
      const RecheckStep t = recheck_tighten(o->converge_tol, tile_res, res, prev_csr_res, tol_factor);
      if (t.stop) break;
      prev_csr_res = t.prev_csr_res;
      tol_factor = t.tol_factor;
    }
    if (o->fixed_iterations || res < o->converge_tol || pass >= o->max_pass) break;
    ++pass;
  }
  if (csr_recheck && !res_from_csr) {  // (x_out is written there)
    rc = csr_true_residual(R, &spmvs, &res);
    if (rc) return rc;
  } else if (!res_from_csr) {
    rc = unscale_to_x_out(R);
    if (rc) return rc;
  }
  MFEM_CHECK_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  MFEM_CHECK_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  MFEM_CHECK_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (R.stats) {
    R.stats->passes = pass;
    R.stats->iterations = total_iters;
    R.stats->final_res = res;
    R.stats->initial_res = res0;
    R.stats->solve_ms = ms;
    R.stats->converged = res < o->converge_tol ? 1 : 0;
    R.stats->spmv_count = spmvs;
  }
  return MFEM_OK;
}

// One attempt: the set-up, then the passes unless a stage asks to start over.  Whatever gets bound is released on every way out.
static int solve_attempt(SolveRun& R) {
  struct LayoutGuard { mfem_csr_s* A; ~LayoutGuard() { mfem_layout_unbind(A); } } layout_guard{R.A};
  R.next = GO_ON;
  int rc = plan_layouts(R);
  if (!rc) rc = carve_workspace(R);
  if (!rc) rc = bind_tiles(R);
  if (rc || R.next) return rc;
  rc = try_scaled_cg(R);
  if (!rc && R.jac && !R.cg_scaled) rc = right_jacobi(R);
  if (!rc) rc = left_precond(R);
  if (!rc) rc = bind_rows(R);
  if (!rc) rc = ws_trial(R);
  if (rc || R.next) return rc;
  return run_passes(R);
}

// The method and n_global are settled once: a start-over issues NO collective before the point it left (a refusal of the tiles is a rank-local
// verdict: the other ranks are already past it and on their way to the next collective of the schedule).
static int solve_inner(mfem_context ctx, mfem_csr A, double* vals, const double* b, double* x_out, const mfem_solve_options* o, mfem_solve_stats* stats) {
  SolveRun R{ctx, A, vals, b, x_out, o, stats};
  int rc = choose_method(R);
  if (rc || A->n == 0) return rc;
  R.allow_lat = true;
  do {
    rc = solve_attempt(R);
    if (R.next == START_OVER_NO_TILES) R.allow_lat = false;
  } while (!rc && R.next);
  return rc;
}

// Cycle graphs around a solve of n rows: not with a communicator (RCCL calls inside the cycle), not while per-launch SpMV timing is on (event
// records inside the cycle), not in benchmark mode on large systems.  The legacy null stream cannot be captured: the
// solve then runs on a private stream, ordered after / before the caller's stream work through events.
template <class Inner>
static int solve_with_graphs(mfem_context_s* ctx, int64_t n, Inner inner) {
  const bool graphs = g_graphs && (!ctx->comm || (graph_comm_wanted() && !mfem_graph_comm_broken && mfem_comm_capturable(ctx))) && !ctx->prof_on && n > 0 &&
                      n <= g_graph_max_n;
  if (!graphs) return inner();
  hipStream_t user = ctx->stream;
  if (user == nullptr) {
    if (!ctx->graph_stream) {
      MFEM_CHECK_HIP(hipStreamCreateWithFlags(&ctx->graph_stream, hipStreamNonBlocking));
      MFEM_CHECK_HIP(hipEventCreateWithFlags(&ctx->graph_ev, hipEventDisableTiming));
    }
    MFEM_CHECK_HIP(hipEventRecord(ctx->graph_ev, user));
    MFEM_CHECK_HIP(hipStreamWaitEvent(ctx->graph_stream, ctx->graph_ev, 0));
    ctx->stream = ctx->graph_stream;
  }
  // whatever way the solve is left -- a status or a C++ exception on its way to the entry point's handler (std::bad_alloc of a lazily made plan) -- the context
  // goes back to the caller's stream and out of capture mode: the header promises that handles stay usable after a non-zero return
  struct Restore {
    mfem_context_s* ctx;
    hipStream_t user;
    ~Restore() {
      ctx->graph_active = 0;
      if (user == nullptr && ctx->stream == ctx->graph_stream) {
        hipEventRecord(ctx->graph_ev, ctx->graph_stream);
        hipStreamWaitEvent(user, ctx->graph_ev, 0);
        ctx->stream = user;
      }
    }
  } restore{ctx, user};
  ctx->graph_active = 1;
  return inner();
}

extern "C" int mfem_solve(mfem_context ctx, mfem_csr A, double* vals, const double* b, double* x_out,
                          const mfem_solve_options* o, mfem_solve_stats* stats) try {
  MFEM_REQUIRE(ctx && A && o, "null argument");
  if (o->precond == MFEM_PRECOND_MULTIGRID) {  // (nothing is launched, nothing is written)
    mfem_set_error("mfem_solve: the multigrid preconditioner needs a hex-8 thermal brick operator (mfem_brick_operator_create), or a hex-8 elasticity one with a hierarchy of mfem_brick_multigrid_create_elasticity attached, and mfem_solve_operator: an assembled matrix has no lattice to coarsen");
    return MFEM_ERR_UNSUPPORTED;
  }
  return solve_with_graphs(ctx, A->n, [&]() { return solve_inner(ctx, A, vals, b, x_out, o, stats); });
} MFEM_API_CATCH("mfem_solve")

// ---- mfem_solve on a matrix-free operator (operator.h: mesh_operator.hip or brick_operator.hip) -------------------------------------------------
// The same driver with an operator attempt in place of solve_attempt: the workspace holds the vectors and the operator's scratch (the mesh operator's
// element vectors; the brick operator has none: mesh_operator_decide.h: mop_workspace) -- no layout, no copy of a matrix --, the Jacobi vector comes from the operator's diagonal kernel, and the
// bound operator serves every product of the unchanged run_passes.  The stages that read CSR values (bind_tiles, try_scaled_cg, left_precond,
// ws_trial, csr_true_residual) are never entered.  CG keeps K unscaled and takes 1 / d; the solvers on A D^-1 hand d to the product, which gathers
// x_j / d_j (the role dsc plays for the lattice tiles).
static int operator_attempt(SolveRun& R) {
  mfem_context_s* ctx = R.ctx;
  mfem_csr_s* A = R.A;
  KrylovVecs& V = R.V;
  const int64_t n = A->n;
  R.next = GO_ON;
  R.tiles_bound = R.rows_bound = R.cg_scaled = false;
  R.fused_scale = R.jac && !R.is_cg;
  R.need_copy = R.scaled_copy = R.gather_early = false;
  R.tplan = nullptr;
  R.lp = mfem_layout_plan_s{MFEM_LAYOUT_CSR, MFEM_LAYOUT_CSR, 0, 0};
  V = KrylovVecs{};
  V.n = n;
  const int64_t nv = V.nv = (int64_t)align_up((size_t)n, 32);
  cg_work_vectors(R.method, R.s_param, V, &R.nclear);
  const int nwork = V.nwork;
  const OpWorkspace W = mop_workspace(nv, nwork, R.opi->scratch_doubles(R.op),
                                      R.o->method == MFEM_SOLVER_GMRES ? mfem_gmres_workspace_bytes() : 0);
  R.vec_bytes = W.vec_bytes;
  R.csr_copy_bytes = R.layout_bytes = 0;
  R.gm_offset = W.gm_offset;
  R.total = W.total;
  int rc = mfem_ws_reserve(ctx, R.total);
  if (rc) return rc;
  char* base = (char*)ctx->ws;
  MFEM_CHECK_HIP(hipMemsetAsync(base, 0, R.vec_bytes * R.nclear, ctx->stream));
  V.x = (double*)(base);
  V.b = (double*)(base + R.vec_bytes);
  V.d = (double*)(base + 2 * R.vec_bytes);
  R.dinv_buf = (double*)(base + 3 * R.vec_bytes);
  for (int i = 0; i < nwork; ++i) V.w[i] = (double*)(base + (4 + i) * R.vec_bytes);
  if (R.o->method == MFEM_SOLVER_GMRES) V.gm = (double*)(base + R.gm_offset);
  double* scratch = (double*)(base + W.scratch_offset);
  R.vals_work = nullptr;
  R.vals_src = nullptr;
  R.lay = nullptr;
  MFEM_CHECK_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  MFEM_CHECK_HIP(hipMemcpyAsync(V.b, R.b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (R.jac) {  // Pr_Jacobi!: d = |diag K| under the guarded rule (a row without adjacency or with a zero diagonal keeps the preset 1)
    rc = mfem_fill(ctx, n, 1.0, V.d);
    if (!rc) rc = R.opi->jacobi(ctx, R.op, scratch, V.d);
    if (rc) return rc;
    if (R.is_cg) {
      hipLaunchKernelGGL(k_recip, dim3(mfem_vec_grid(ctx, n)), dim3(MFEM_BLOCK), 0, ctx->stream, n, V.d, R.dinv_buf);
      MFEM_CHECK_LAUNCH();
      V.dinv = R.dinv_buf;
    }
  }
  if (R.mg) {  // Pr_Multigrid: the setup of the attached hierarchy, always, where the Jacobi diagonal is computed -- inside solve_ms
    rc = mfem_mg_setup_attached(ctx, R.op);
    if (rc) return rc;
  }
  rc = R.opi->bind(R.op, scratch, R.fused_scale ? V.d : nullptr);
  if (rc) return rc;
  struct Unbind { SolveRun& R; ~Unbind() { R.opi->unbind(R.op); } } unbind{R};
  return run_passes(R);
}

extern "C" int mfem_solve_operator(mfem_context ctx, uint64_t handle, const double* b, double* x_out, const mfem_solve_options* o,
                                   mfem_solve_stats* stats) try {
  mfem_operator_head* op = (mfem_operator_head*)(uintptr_t)handle;
  MFEM_REQUIRE(ctx && op && o, "null argument");
  const mfem_operator_interface* opi = mfem_operator_interface_of(op);
  MFEM_REQUIRE(opi, "the handle is neither a mesh operator's nor a brick operator's");
  MFEM_REQUIRE(opi->ctx(op) == ctx, "the operator was created on another context");
  mfem_csr_s* A = opi->csr(op);
  MFEM_REQUIRE(!A->op, "the operator is bound to a running solve");
  MFEM_REQUIRE(A->n == 0 || (b && x_out), "null array");
  MFEM_REQUIRE(o->method >= MFEM_SOLVER_CG && o->method <= MFEM_SOLVER_LSQR, "unknown method");
  MFEM_REQUIRE(o->precond >= MFEM_PRECOND_NONE && o->precond <= MFEM_PRECOND_MULTIGRID, "unknown precond");
  MFEM_REQUIRE(o->left_precond >= MFEM_LEFT_NONE && o->left_precond <= MFEM_LEFT_JACOBI_ROWNORM, "unknown left_precond");
  const bool mg = o->precond == MFEM_PRECOND_MULTIGRID;
  if (mg) {  // the new value is gated in front of mop_solve_gate: what is missing is named, nothing is launched, nothing is written
    const int rcg = mfem_mg_solve_check(ctx, op, o);
    if (rcg) return rcg;
  }
  const char* why = "";
  const int gate = mop_solve_gate(o->method, o->precond, o->left_precond, o->scale_in_place, ctx->comm != nullptr, &why);
  if (gate) {
    mfem_set_error("mfem_solve_operator: %s", why);
    return gate;
  }
  auto run = [&]() -> int {
    SolveRun R{ctx, A, nullptr, b, x_out, o, stats};
    R.op = op;
    R.opi = opi;
    R.mg = mg;
    const int rc = choose_method(R);
    if (rc || A->n == 0) return rc;
    R.allow_lat = false;
    return operator_attempt(R);
  };
  if (mg) {  // a default hierarchy when none is attached (thermal; an elasticity operator passed the gate with its own attached): allocated here, before the workspace is taken; the pass captures no cycle graph
    MFEM_REQUIRE(o->maxiter >= 0 && o->max_pass >= 1, "maxiter >= 0 and max_pass >= 1 required");
    const int rca = mfem_mg_attach_default(ctx, op);
    if (rca) return rca;
    return run();
  }
  return solve_with_graphs(ctx, A->n, run);
} MFEM_API_CATCH("mfem_solve_operator")
