// Geometric multigrid V-cycle on hex-8 thermal and elasticity bricks and on hex-27 thermal bricks: the preconditioner behind MFEM_PRECOND_MULTIGRID (cg! on the matrix-free brick operator;
// the pass: krylov_cg_mg.hip).  The hierarchy of an (nx, ny, nz) brick is the bricks (nx/2, ny/2, nz/2), ...: library-owned mfem_bricks whose
// coordinates are injected from the next finer level at every setup, with a brick operator each (rediscretisation: the caller's parameters on the
// coarse brick).  Everything is made of that operator's product and diagonal and of the kernels below; no matrix, no pattern, no atomic.
//   A = s K, s = the sign of diag K (detected per setup: k_mg_dinv), dinv = 1 / |diag K|
//   k_mg_inject    coarse coordinates (i, j, k) <- fine (2 i, 2 j, 2 k)
//   k_mg_restrict  b_c = P' r: a thread per COARSE point adds its <= 27 fine neighbours in a fixed order, weights (1/2)^(number of odd offsets)
//   k_mg_prolong   a thread per FINE point: e = P z_c (its <= 8 coarse parents in a fixed order), z += e, d = e (for the product r -= A d that follows)
//   k_mg_cheb      one step of the Chebyshev smoother: d = c1 d + c2 dinv . r, z (+)= d -- and, on the first step from a zero start, r = b
//   k_mg_power_*   the estimate of lambda_max(D^-1 A): power steps v <- D^-1 A v / |.|, the Rayleigh quotient v . A v / v . D v of the last iterate
// The transfer kernels map lanes along k, the fastest lattice index (tiles: brick_multigrid_decide.h).  The residual of a level is carried by
// recurrence (r -= A d through the operator's own launch with alpha = -s, beta = 1) and never recomputed.  All sums have a fixed order: a cycle, a
// setup and a solve give the same bits on every run.
// Vector streams per cycle beside the products: mg_cycle_streams (12 nu + 2 on a level below the coarsest).
// An elasticity hierarchy (mfem_brick_multigrid_create_elasticity) carries three field-major fields per lattice point: a level vector holds
// fields x points entries, the transfers are the <NF = 3> instantiations (one launch, a thread per lattice point looping over the fields: P is
// I_3 (x) the scalar P), the coarse operators are mfem_brick_operator_create_elasticity's, and everything elementwise runs on n = fields x points.
// A hex-27 hierarchy (mfem_brick_multigrid_create_hex27) is p-coarsened once: level 0 is the caller's order-2 brick on the lattice 2 ne + 1, level 1 a
// hex-8 brick of the SAME elements on ne + 1 -- mf = 2 mc - 1 as between two hex-8 levels, so k_mg_inject (the corner nodes), k_mg_restrict<1> and
// k_mg_prolong<1> (the embedding Q1 in Q2) serve unchanged -- and the thermal h-hierarchy follows; level 0's signed diagonal is the plane sweep of
// brick_operator_hex27_diagonal.hip, its product bop27_launch through the operator interface.
// A nonsymmetric hierarchy (mfem_brick_multigrid_create_nonsymmetric) is the hex-8 thermal one with mfem_brick_multigrid_s.nonsym set: its setup
// takes an active Nitsche (fixed_faces) term -- every kernel above runs unchanged on the nonsymmetric K -- and gmres! takes its cycle as a right
// preconditioner (krylov_gmres_mg.hip).
#include <memory>
#include "brick_operator.h"
#include "brick_multigrid.h"
#include "brick_multigrid_decide.h"
#include "brick_operator_elasticity_hex27_decide.h"
#include "krylov.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

#define MFEM_MULTIGRID_KIND 0x4d47424du
enum { S_MG_LAMBDA = S_SOLVER + 100 };  // [ , + MG_MAX_LEVELS): the estimates of a setup, read back once (no solve runs during a setup)
static_assert(S_MG_LAMBDA + MG_MAX_LEVELS <= 240, "inside the solver-private block of the device scalars");
static_assert(MG_TILE_THREADS == MFEM_BLOCK, "a transfer tile is one workgroup");

struct MgLevel {
  int ne[3], m[3];
  int fields;            // 1 (thermal) or 3 (elasticity), field-major: field f of a level vector starts at f * points
  int64_t points;        // lattice points
  int64_t n, npad;       // fields * points; mg_padded(n): the vector is padded, not each field
  mfem_brick_s* brick;        // level 0: the caller's (borrowed); coarse levels: owned
  mfem_brick_operator_s* op;  // likewise
  double* slab;               // the level's vectors, one allocation
  double *dinv, *r, *d, *b, *z;  // (b, z: coarse levels only)
  double lambda_max;
  int64_t products;
};
struct mfem_brick_multigrid_s {
  uint32_t kind;
  mfem_context_s* ctx;
  mfem_brick_operator_s* fine;
  MgOptions opt;
  int nlev;
  MgLevel lev[MG_MAX_LEVELS];
  int32_t* d_flags;  // [4]: a positive, a negative, a zero diagonal entry seen (k_mg_dinv)
  int sign;
  bool ready;        // a setup has succeeded since creation
  bool nonsym;       // of mfem_brick_multigrid_create_nonsymmetric: a setup runs with a Nitsche term active too, gmres! takes the cycle
  int64_t bytes, cycles, setups, setup_products;
};

static mfem_brick_multigrid_s* mg_from_handle(uint64_t h) {
  mfem_brick_multigrid_s* mg = (mfem_brick_multigrid_s*)(uintptr_t)h;
  return mg && mg->kind == MFEM_MULTIGRID_KIND ? mg : nullptr;
}
static int mg_refuse(int tag, const char* why) {  // (tag: the physics the refusing party builds hierarchies for; its row has the name)
  mfem_set_error("multigrid on the %s brick operator: %s", bop_physics_row(tag)->name, why);
  return MFEM_ERR_UNSUPPORTED;
}
// Why create entry point `which` (BOP_MG_*) does not build the hierarchy of an operator with physics `tag` (BOP_PHYSICS_*); nullptr where it does.
static const char* mg_wrong_physics(int which, int tag) {
  static const char* const takes_create = "a hex-8 thermal operator's handle: it takes mfem_brick_multigrid_create";
  static const char* const not_covered = "elasticity and hex-27 operators are not covered (a hex-8 elasticity operator takes mfem_brick_multigrid_create_elasticity, a hex-27 "
                                         "thermal operator mfem_brick_multigrid_create_hex27)";
  static const char* const thermal_only = "mfem_brick_multigrid_create_nonsymmetric covers the hex-8 thermal operator only (the penalty faces of a hex-8 elasticity operator "
                                          "are symmetric: mfem_brick_multigrid_create_elasticity and cg!; a hex-27 thermal operator takes mfem_brick_multigrid_create_hex27 "
                                          "without a Nitsche term)";
  static const char* const why[BOP_MG_ENTRIES][BOP_PHYSICS_ROWS] = {  // [entry point][tag - 1]
      {nullptr, not_covered, not_covered, bop_e27_multigrid_refusal()},
      {nullptr, thermal_only, thermal_only, bop_e27_multigrid_refusal()},
      {takes_create, nullptr, "a hex-27 operator's handle: it takes mfem_brick_multigrid_create_hex27", bop_e27_multigrid_refusal()},
      {takes_create, "a hex-8 elasticity operator's handle: it takes mfem_brick_multigrid_create_elasticity", nullptr, bop_e27_multigrid_refusal()}};
  return why[which][tag - 1];
}
// which hierarchy an operator takes: its physics row names the entry point that builds it (brick_operator_physics.h)
static bool mg_is_elasticity(const mfem_brick_operator_s* op) { return bop_row(op).multigrid == BOP_MG_CREATE_ELASTICITY; }
static bool mg_is_hex27(const mfem_brick_operator_s* op) { return bop_row(op).multigrid == BOP_MG_CREATE_HEX27; }

// ---- kernels -------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mg_point(int m1, int m2, int& i, int& j, int& k) {
  i = (int)blockIdx.z;
  j = (int)blockIdx.y * MG_TILE_J + (int)threadIdx.x / MG_TILE_K;
  k = (int)blockIdx.x * MG_TILE_K + (int)threadIdx.x % MG_TILE_K;
  return j < m1 && k < m2;
}

__global__ __launch_bounds__(MG_TILE_THREADS) void k_mg_inject(int mc1, int mc2, int mf1, int mf2, const double* __restrict__ F0, const double* __restrict__ F1,
                                                                 const double* __restrict__ F2, double* __restrict__ C0, double* __restrict__ C1,
                                                                 double* __restrict__ C2) {
  int i, j, k;
  if (!mg_point(mc1, mc2, i, j, k)) return;
  const int64_t c = ((int64_t)i * mc1 + j) * mc2 + k;
  const int64_t f = ((int64_t)(2 * i) * mf1 + 2 * j) * mf2 + 2 * k;  // (mf = 2 mc - 1: 2 (mc - 1) is the last fine index)
  C0[c] = F0[f];
  C1[c] = F1[f];
  C2[c] = F2[f];
}

// NF fields, field-major: field f of rf starts at f * pf (fine points), of bc at f * pc (coarse points).  The neighbour's index and weight are
// computed once and serve every field; within a field the sum runs in the order of the one-field kernel (<1> is that kernel).
template <int NF>
__global__ __launch_bounds__(MG_TILE_THREADS) void k_mg_restrict(int mc1, int mc2, int mf0, int mf1, int mf2, int64_t pf, int64_t pc,
                                                                   const double* __restrict__ rf, double* __restrict__ bc) {
  int I, J, K;
  if (!mg_point(mc1, mc2, I, J, K)) return;
  double acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = 0.0;
#pragma unroll
  for (int di = -1; di <= 1; ++di) {
    const int fi = 2 * I + di;
    if (fi < 0 || fi >= mf0) continue;
    const double wi = di ? 0.5 : 1.0;
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      const int fj = 2 * J + dj;
      if (fj < 0 || fj >= mf1) continue;
      const double wij = dj ? 0.5 * wi : wi;
#pragma unroll
      for (int dk = -1; dk <= 1; ++dk) {
        const int fk = 2 * K + dk;
        if (fk < 0 || fk >= mf2) continue;
        const double w = dk ? 0.5 * wij : wij;
        const int64_t src = ((int64_t)fi * mf1 + fj) * mf2 + fk;
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] += w * rf[f * pf + src];
      }
    }
  }
  const int64_t dst = ((int64_t)I * mc1 + J) * mc2 + K;
#pragma unroll
  for (int f = 0; f < NF; ++f) bc[f * pc + dst] = acc[f];
}

// z may be null (the transfer alone).  NF fields as in k_mg_restrict: the parents and the weight once, the correction fused for every field.
template <int NF>
__global__ __launch_bounds__(MG_TILE_THREADS) void k_mg_prolong(int mf1, int mf2, int mc1, int mc2, int64_t pf, int64_t pc, const double* __restrict__ ec,
                                                                  double* __restrict__ z, double* __restrict__ d) {
  int i, j, k;
  if (!mg_point(mf1, mf2, i, j, k)) return;
  // an even index has the one parent i / 2 (weight 1), an odd one the parents (i - 1) / 2 and (i + 1) / 2 (1/2 each; the upper one exists: an odd
  // index is never the last of a lattice of 2 mc - 1 points)
  const int ni = 1 + (i & 1), nj = 1 + (j & 1), nk = 1 + (k & 1);
  const double w = ((i & 1) ? 0.5 : 1.0) * ((j & 1) ? 0.5 : 1.0) * ((k & 1) ? 0.5 : 1.0);
  double acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = 0.0;
  for (int a = 0; a < ni; ++a)
    for (int b = 0; b < nj; ++b)
      for (int c = 0; c < nk; ++c) {
        const int64_t src = ((int64_t)((i >> 1) + a) * mc1 + (j >> 1) + b) * mc2 + (k >> 1) + c;
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] += ec[f * pc + src];
      }
  const int64_t dst = ((int64_t)i * mf1 + j) * mf2 + k;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const double e = acc[f] * w;
    if (z) z[f * pf + dst] += e;
    d[f * pf + dst] = e;
  }
}

// d (holding the signed diagonal, preset 0) -> dinv = 1 / |d|; flags: every thread that sees a positive / negative / zero entry stores 1 to its flag
// (plain stores of one value: no atomic, no order)
__global__ __launch_bounds__(MFEM_BLOCK) void k_mg_dinv(int64_t n, const double* __restrict__ d, double* __restrict__ dinv, int32_t* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = d[i];
    if (v > 0.0) flags[0] = 1;
    else if (v < 0.0) flags[1] = 1;
    else flags[2] = 1;  // (zero, or not a number)
    dinv[i] = 1.0 / fabs(v);
  }
}

// One Chebyshev step on n entries: d = c1 d + c2 dinv . r, z = z + d.  FIRST: c1 = 0 and d is not read.  ZERO: z starts from zero and is not read, and
// rcopy (may be null) receives r -- the residual of a zero start is b itself, which the level must not change.
template <typename T, bool FIRST, bool ZERO>
__device__ __forceinline__ void mg_cheb_range(int64_t first, int64_t count, int64_t stride, double c1, double c2, const T* __restrict__ r,
                                              const T* __restrict__ dinv, T* __restrict__ d, T* __restrict__ z, T* __restrict__ rcopy) {
  for (int64_t i = first; i < count; i += stride) {
    const T rv = r[i];
    T dv = c2 * (dinv[i] * rv);
    if (!FIRST) dv += c1 * d[i];
    d[i] = dv;
    z[i] = ZERO ? dv : z[i] + dv;
    if (ZERO && rcopy) rcopy[i] = rv;
  }
}
template <bool FIRST, bool ZERO>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mg_cheb(int64_t n, double c1, double c2, const double* __restrict__ r, const double* __restrict__ dinv,
                                                          double* __restrict__ d, double* __restrict__ z, double* __restrict__ rcopy) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool al = ((((uintptr_t)r) | ((uintptr_t)dinv) | ((uintptr_t)d) | ((uintptr_t)z) | ((uintptr_t)rcopy)) & 15) == 0;
  if (al) {
    mg_cheb_range<d2_t, FIRST, ZERO>(tid, n >> 1, stride, c1, c2, (const d2_t*)r, (const d2_t*)dinv, (d2_t*)d, (d2_t*)z, (d2_t*)rcopy);
    if ((n & 1) && tid == 0) mg_cheb_range<double, FIRST, ZERO>(n - 1, n, 1, c1, c2, r, dinv, d, z, rcopy);
  } else {
    mg_cheb_range<double, FIRST, ZERO>(tid, n, stride, c1, c2, r, dinv, d, z, rcopy);
  }
}

// power step, part 1: w = A v is in; partial sums of v . w, v . D v and |D^-1 w|^2 at [0, G), [G, 2 G), [2 G, 3 G)
__global__ __launch_bounds__(MFEM_BLOCK) void k_mg_power_dots(int64_t n, const double* __restrict__ v, const double* __restrict__ w, const double* __restrict__ dinv,
                                                                double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double num = 0.0, den = 0.0, nrm = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const double vv = v[i], ww = w[i], di = dinv[i];
    num += vv * ww;
    den += vv * (vv / di);
    const double t = di * ww;
    nrm += t * t;
  }
  const double s0 = block_reduce_sum(num, red);
  const double s1 = block_reduce_sum(den, red);
  const double s2 = block_reduce_sum(nrm, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s0;
    partials[gridDim.x + blockIdx.x] = s1;
    partials[2 * gridDim.x + blockIdx.x] = s2;
  }
}
// part 2: v <- D^-1 w / |D^-1 w|; *lambda = v . A v / v . D v of the v that came in
__global__ __launch_bounds__(MFEM_BLOCK) void k_mg_power_next(int64_t n, double* __restrict__ v, const double* __restrict__ w, const double* __restrict__ dinv,
                                                                const double* __restrict__ partials, int np, double* __restrict__ lambda) {
  __shared__ double red[4];
  const double num = reduce_partials_bcast(partials, np, red);
  const double den = reduce_partials_bcast(partials + np, np, red);
  const double nrm = reduce_partials_bcast(partials + 2 * np, np, red);
  const double sc = 1.0 / sqrt(nrm);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) v[i] = sc * (dinv[i] * w[i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) *lambda = num / den;
}

// ---- host: products on a level ------------------------------------------------------------------------------------------------------------------------
// y = alpha K_l x + beta y through the level operator's own launch.  Level 0 inside a solve is bound by the driver (cg!: without a column scaling);
// everywhere else the operator is bound for this product alone (host only).
static int mg_product(mfem_brick_multigrid_s* mg, int l, const double* x, double* y, double alpha, double beta) {
  mfem_brick_operator_s* op = mg->lev[l].op;
  const mfem_operator_interface* I = mfem_brick_operator_interface();
  const bool mine = !op->csr.op;
  MFEM_REQUIRE(mine || op->csr.op_dsc == nullptr, "the level operator is bound with a column scaling");
  if (mine) {
    const int rc = I->bind(&op->head, nullptr, nullptr);
    if (rc) return rc;
  }
  const int rc = mfem_spmv_launch(mg->ctx, &op->csr, nullptr, x, y, alpha, beta, nullptr, nullptr, nullptr, nullptr);
  if (mine) I->unbind(&op->head);
  return rc;
}

static int mg_vec_grid(mfem_context_s* ctx, int64_t n) { return mfem_vec_grid(ctx, n); }

static int mg_cheb_step(mfem_context_s* ctx, const MgLevel& L, bool first, bool zero, double c1, double c2, const double* r, double* z, double* rcopy) {
  const dim3 g(mg_vec_grid(ctx, L.n)), b(MFEM_BLOCK);
  if (first && zero) hipLaunchKernelGGL((k_mg_cheb<true, true>), g, b, 0, ctx->stream, L.n, c1, c2, r, (const double*)L.dinv, L.d, z, rcopy);
  else if (first) hipLaunchKernelGGL((k_mg_cheb<true, false>), g, b, 0, ctx->stream, L.n, c1, c2, r, (const double*)L.dinv, L.d, z, (double*)nullptr);
  else hipLaunchKernelGGL((k_mg_cheb<false, false>), g, b, 0, ctx->stream, L.n, c1, c2, r, (const double*)L.dinv, L.d, z, (double*)nullptr);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// z = Cheb(A, dinv, b, nu, lo, hi, start): zero: z starts from zero and the residual is b, else z holds the start and L.r its residual.  The residual is
// carried in L.r; residual_after: it is brought up to date after the last step too (one more product).
static int mg_cheb(mfem_brick_multigrid_s* mg, int l, const double* b, double* z, bool zero, int nu, double lo, double hi, bool residual_after, int* products) {
  mfem_context_s* ctx = mg->ctx;
  MgLevel& L = mg->lev[l];
  double c1, c2;
  MgCheb C = mg_cheb_start(lo, hi, &c1, &c2);
  const bool need_r = nu > 1 || residual_after;
  int rc = mg_cheb_step(ctx, L, true, zero, c1, c2, zero ? b : L.r, z, (zero && need_r) ? L.r : nullptr);
  if (rc) return rc;
  for (int k = 1; k < nu; ++k) {
    rc = mg_product(mg, l, L.d, L.r, -(double)mg->sign, 1.0);  // r -= A d
    if (rc) return rc;
    ++*products;
    mg_cheb_next(&C, &c1, &c2);
    rc = mg_cheb_step(ctx, L, false, false, c1, c2, L.r, z, nullptr);
    if (rc) return rc;
  }
  if (residual_after) {
    rc = mg_product(mg, l, L.d, L.r, -(double)mg->sign, 1.0);
    if (rc) return rc;
    ++*products;
  }
  return MFEM_OK;
}

static int mg_restrict(mfem_context_s* ctx, const MgLevel& F, const MgLevel& Cc, const double* rf, double* bc) {
  const MgGrid g = mg_transfer_grid(Cc.m[0], Cc.m[1], Cc.m[2]);
  MFEM_REQUIRE(mg_grid_ok(g), "a lattice too large for the transfer kernels' grid");
  const auto kernel = F.fields == MG_ELASTICITY_FIELDS ? k_mg_restrict<MG_ELASTICITY_FIELDS> : k_mg_restrict<1>;
  hipLaunchKernelGGL(kernel, dim3(g.gx, g.gy, g.gz), dim3(MG_TILE_THREADS), 0, ctx->stream, Cc.m[1], Cc.m[2], F.m[0], F.m[1], F.m[2], F.points, Cc.points, rf,
                     bc);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
static int mg_prolong(mfem_context_s* ctx, const MgLevel& F, const MgLevel& Cc, const double* ec, double* z, double* d) {
  const MgGrid g = mg_transfer_grid(F.m[0], F.m[1], F.m[2]);
  MFEM_REQUIRE(mg_grid_ok(g), "a lattice too large for the transfer kernels' grid");
  const auto kernel = F.fields == MG_ELASTICITY_FIELDS ? k_mg_prolong<MG_ELASTICITY_FIELDS> : k_mg_prolong<1>;
  hipLaunchKernelGGL(kernel, dim3(g.gx, g.gy, g.gz), dim3(MG_TILE_THREADS), 0, ctx->stream, F.m[1], F.m[2], Cc.m[1], Cc.m[2], F.points, Cc.points, ec, z, d);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

static int mg_cycle_level(mfem_brick_multigrid_s* mg, int l, const double* b, double* z) {
  mfem_context_s* ctx = mg->ctx;
  MgLevel& L = mg->lev[l];
  const double hi = MG_EIG_SAFETY * L.lambda_max;
  int products = 0;
  int rc = MFEM_OK;
  if (l == mg->nlev - 1) {
    rc = mg_cheb(mg, l, b, z, true, mg->opt.nu_c, hi / mg->opt.range_c, hi, false, &products);
  } else {
    MgLevel& Cc = mg->lev[l + 1];
    rc = mg_cheb(mg, l, b, z, true, mg->opt.nu, hi / mg->opt.range_s, hi, true, &products);
    if (!rc) rc = mg_restrict(ctx, L, Cc, L.r, Cc.b);
    if (!rc) rc = mg_cycle_level(mg, l + 1, Cc.b, Cc.z);
    if (!rc) rc = mg_prolong(ctx, L, Cc, Cc.z, z, L.d);  // z += P e, d = P e
    if (!rc) {
      rc = mg_product(mg, l, L.d, L.r, -(double)mg->sign, 1.0);  // r -= A (P e)
      ++products;
    }
    if (!rc) rc = mg_cheb(mg, l, b, z, false, mg->opt.nu, hi / mg->opt.range_s, hi, false, &products);
  }
  L.products += products;
  return rc;
}

int mfem_mg_cycle(mfem_context_s* ctx, mfem_brick_multigrid_s* mg, const double* r, double* z) {
  MFEM_REQUIRE(mg && mg->ctx == ctx && mg->ready, "the multigrid hierarchy has had no successful setup");
  const int rc = mg_cycle_level(mg, 0, r, z);
  ++mg->cycles;
  return rc;
}

// ---- host: create, setup, release --------------------------------------------------------------------------------------------------------------------
void mfem_mg_release(mfem_brick_multigrid_s* mg) {
  if (!mg) return;
  const bool alive = mg->ctx && mfem_context_alive(mg->ctx);
  if (alive) (void)hipStreamSynchronize(mg->ctx->stream);
  for (int l = 0; l < mg->nlev; ++l) {
    MgLevel& L = mg->lev[l];
    if (l > 0) {
      if (L.op) (void)mfem_brick_operator_destroy((uint64_t)(uintptr_t)L.op);
      if (L.brick) (void)mfem_brick_destroy(L.brick);
    }
    if (L.slab) (void)hipFree(L.slab);
  }
  if (mg->d_flags) (void)hipFree(mg->d_flags);
  if (mg->fine && mg->fine->mg == mg) mg->fine->mg = nullptr;
  mg->kind = 0;
  delete mg;
}

static int mg_create(mfem_context_s* ctx, mfem_brick_operator_s* op, const MgOptions& opt, mfem_brick_multigrid_s** out) {
  const mfem_brick_s* fb = op->brick;
  const bool hex27 = mg_is_hex27(op);  // level 0 on the lattice 2 ne + 1, a hex-8 brick of the same elements below it (mg_plan_hex27)
  const MgPlan P = hex27 ? mg_plan_hex27(fb->ne[0], fb->ne[1], fb->ne[2], opt.max_levels) : mg_plan(fb->ne[0], fb->ne[1], fb->ne[2], opt.max_levels);
  const int fields = bop_row(op).fields;
  mfem_host_alloc_probe();
  mfem_brick_multigrid_s* mg = new mfem_brick_multigrid_s();
  memset(mg, 0, sizeof(*mg));
  mg->kind = MFEM_MULTIGRID_KIND;
  mg->ctx = ctx;
  mg->opt = opt;
  mg->nlev = P.nlev;
  auto build = [&]() -> int {
    MFEM_CHECK_HIP(hipMalloc((void**)&mg->d_flags, MG_FLAG_BYTES));
    for (int l = 0; l < P.nlev; ++l) {
      MgLevel& L = mg->lev[l];
      for (int d = 0; d < 3; ++d) {
        L.ne[d] = P.ne[l][d];
        L.m[d] = hex27 ? mg_lattice_hex27(l, P.ne[l][d]) : P.ne[l][d] + 1;
      }
      L.fields = fields;
      L.points = hex27 ? mg_points_hex27(l, L.ne) : mg_points(L.ne);
      L.n = (int64_t)fields * L.points;
      L.npad = mg_padded(L.n);
      if (l == 0) {
        L.brick = op->brick;
        L.op = op;
      } else {
        int rc = mfem_brick_create(ctx, L.ne[0], L.ne[1], L.ne[2], fb->len[0], fb->len[1], fb->len[2], 1, fb->itg_order, &L.brick);
        if (rc) return rc;
        uint64_t h = 0;
        rc = fields == 1 ? mfem_brick_operator_create(ctx, L.brick, &op->thermal, &h) : mfem_brick_operator_create_elasticity(ctx, L.brick, &op->elasticity, &h);
        if (rc) return rc;
        L.op = bop_from_handle(h);
      }
      const int nvec = mg_level_vectors(l);
      MFEM_CHECK_HIP(hipMalloc((void**)&L.slab, (size_t)nvec * L.npad * sizeof(double)));
      MFEM_CHECK_HIP(hipMemsetAsync(L.slab, 0, (size_t)nvec * L.npad * sizeof(double), ctx->stream));
      L.dinv = L.slab;
      L.r = L.slab + L.npad;
      L.d = L.slab + 2 * L.npad;
      L.b = l ? L.slab + 3 * L.npad : nullptr;
      L.z = l ? L.slab + 4 * L.npad : nullptr;
    }
    return MFEM_OK;
  };
  int rc = MFEM_OK;
  try {
    rc = build();
  } catch (...) {
    mfem_mg_release(mg);
    throw;
  }
  if (rc) {
    mfem_mg_release(mg);
    return rc;
  }
  mg->bytes = hex27 ? mg_bytes_hex27(P) : mg_bytes_fields(P, fields);
  mg->fine = op;
  op->mg = mg;
  *out = mg;
  return MFEM_OK;
}

static bool mg_nitsche(const mfem_brick_operator_s* op) { return bop_nitsche_on(op->thermal.k, op->thermal.h_penalty, op->thermal.fixed_faces); }

static int mg_setup(mfem_context_s* ctx, mfem_brick_multigrid_s* mg) {
  mfem_brick_operator_s* fine = mg->fine;
  mg->ready = false;
  const bool elasticity = mg_is_elasticity(fine);
  if (elasticity) {
    const char* why = mg_elasticity_refusal(fine->elasticity.tau, fine->elasticity.penalty_faces);
    if (why) return mg_refuse(fine->physics, why);
  } else if (mg_is_hex27(fine)) {
    const char* why = mg_hex27_refusal(fine->brick->ng, mg_nitsche(fine));
    if (why) return mg_refuse(fine->physics, why);
  } else if (mg_setup_refuses_nitsche(mg->nonsym, mg_nitsche(fine))) {
    return mg_refuse(fine->physics, "a Nitsche (fixed_faces) term is active: K is not symmetric");
  }
  const auto refuse = [fine](const char* why) { return mg_refuse(fine->physics, why); };
  for (int l = 0; l < mg->nlev; ++l) MFEM_REQUIRE(!mg->lev[l].op->csr.op, "a level's operator is bound to a running solve");
  const mfem_brick_s* fb = fine->brick;
  MFEM_REQUIRE(fb->ne[0] == mg->lev[0].ne[0] && fb->ne[1] == mg->lev[0].ne[1] && fb->ne[2] == mg->lev[0].ne[2] && fb->plo == 0 && fb->phi == fb->m[0],
               "the brick changed under the hierarchy");
  // 1. the fine operator's current parameters on every level; the coordinates, level by level
  for (int l = 1; l < mg->nlev; ++l) {
    MgLevel &F = mg->lev[l - 1], &L = mg->lev[l];
    L.op->thermal = fine->thermal;
    L.op->elasticity = fine->elasticity;
    ++L.op->csr.op_epoch;
    const MgGrid g = mg_transfer_grid(L.m[0], L.m[1], L.m[2]);
    MFEM_REQUIRE(mg_grid_ok(g), "a lattice too large for the transfer kernels' grid");
    hipLaunchKernelGGL(k_mg_inject, dim3(g.gx, g.gy, g.gz), dim3(MG_TILE_THREADS), 0, ctx->stream, L.m[1], L.m[2], F.m[1], F.m[2], (const double*)F.brick->coords[0],
                       (const double*)F.brick->coords[1], (const double*)F.brick->coords[2], L.brick->coords[0], L.brick->coords[1], L.brick->coords[2]);
    MFEM_CHECK_LAUNCH();
  }
  // 2. the diagonals and the sign
  MFEM_CHECK_HIP(hipMemsetAsync(mg->d_flags, 0, MG_FLAG_BYTES, ctx->stream));
  for (int l = 0; l < mg->nlev; ++l) {
    MgLevel& L = mg->lev[l];
    int rc = mfem_fill(ctx, L.n, 0.0, L.r);
    if (!rc) rc = bop_signed_diagonal(ctx, L.op, L.r);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mg_dinv, dim3(mg_vec_grid(ctx, L.n)), dim3(MFEM_BLOCK), 0, ctx->stream, L.n, (const double*)L.r, L.dinv, mg->d_flags);
    MFEM_CHECK_LAUNCH();
  }
  int32_t flags[4] = {0, 0, 0, 0};
  MFEM_CHECK_HIP(hipMemcpyAsync(flags, mg->d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  if (flags[2]) return refuse("diag K has a zero (or an entry that is not a number) on some level");
  if (flags[0] && flags[1]) return refuse("diag K has entries of both signs");
  mg->sign = flags[0] ? 1 : -1;
  // 3. lambda_max(D^-1 A) per level: eig_steps power steps from a fixed seeded start, the Rayleigh quotient of the last iterate
  const double s = (double)mg->sign;
  for (int l = 0; l < mg->nlev; ++l) {
    MgLevel& L = mg->lev[l];
    double *v = L.r, *w = L.d;
    int rc = mfem_rand(ctx, L.n, MG_EIG_SEED, (uint32_t)l, v);
    if (rc) return rc;
    const int G = mg_vec_grid(ctx, L.n);
    for (int k = 0; k < mg->opt.eig_steps; ++k) {
      rc = mg_product(mg, l, v, w, s, 0.0);
      if (rc) return rc;
      ++mg->setup_products;
      hipLaunchKernelGGL(k_mg_power_dots, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, L.n, (const double*)v, (const double*)w, (const double*)L.dinv, ctx->d_partials);
      MFEM_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_mg_power_next, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, L.n, v, (const double*)w, (const double*)L.dinv, (const double*)ctx->d_partials, G,
                         ctx->d_scalars + S_MG_LAMBDA + l);
      MFEM_CHECK_LAUNCH();
    }
  }
  int rc = mfem_read_scalars(ctx, S_MG_LAMBDA, mg->nlev);
  if (rc) return rc;
  for (int l = 0; l < mg->nlev; ++l) {
    const double lam = ctx->h_scalars[S_MG_LAMBDA + l];
    if (!(lam > 0.0) || !(lam < __builtin_huge_val())) return refuse("the estimate of lambda_max(D^-1 A) is not a positive number: K is not definite");
    mg->lev[l].lambda_max = lam;
  }
  ++mg->setups;
  mg->ready = true;
  return MFEM_OK;
}

// ---- what the solve driver calls (brick_multigrid.h) ---------------------------------------------------------------------------------------------------
int mfem_mg_solve_check(mfem_context_s* ctx, mfem_operator_head* head, const mfem_solve_options* o) {
  const bool brick = head->kind == MFEM_OPERATOR_BRICK;
  const mfem_brick_operator_s* op = brick ? (const mfem_brick_operator_s*)head : nullptr;
  if (op && bop_row(op).multigrid == BOP_MG_NONE) {  // (a physics without a hierarchy: every create entry point answers it alike)
    mfem_set_error("mfem_solve_operator: MFEM_PRECOND_MULTIGRID on %s", mg_wrong_physics(BOP_MG_CREATE, op->physics));
    return MFEM_ERR_UNSUPPORTED;
  }
  const bool thermal = op && bop_row(op).multigrid == BOP_MG_CREATE;
  const bool elasticity = op && mg_is_elasticity(op);
  const bool hex27 = op && mg_is_hex27(op);
  const char* why = mg_solve_refusal_nonsym(brick, thermal, elasticity, hex27, op && op->mg != nullptr, op && op->mg && op->mg->nonsym, o->method,
                                            o->left_precond, ctx->comm != nullptr, (thermal || hex27) && mg_nitsche(op));
  if (!why && hex27) {  // (the setup inside the solve would refuse it: answered here, before anything is launched)
    why = mg_hex27_refusal(op->brick->ng, false);
    if (why) return mg_refuse(op->physics, why);
  }
  if (!why && elasticity) {  // (the setup inside the solve would refuse it: answered here, before anything is launched)
    why = mg_elasticity_refusal(op->elasticity.tau, op->elasticity.penalty_faces);
    if (why) return mg_refuse(op->physics, why);
  }
  if (!why) return MFEM_OK;
  mfem_set_error("mfem_solve_operator: %s", why);
  return MFEM_ERR_UNSUPPORTED;
}
int mfem_mg_attach_default(mfem_context_s* ctx, mfem_operator_head* head) {
  mfem_brick_operator_s* op = (mfem_brick_operator_s*)head;
  if (op->mg) {
    MFEM_REQUIRE(op->mg->ctx == ctx, "the hierarchy was created on another context");
    return MFEM_OK;
  }
  MgOptions opt;
  (void)mg_options(nullptr, &opt);
  mfem_brick_multigrid_s* mg = nullptr;
  return mg_create(ctx, op, opt, &mg);
}
int mfem_mg_setup_attached(mfem_context_s* ctx, mfem_operator_head* head) {
  mfem_brick_operator_s* op = (mfem_brick_operator_s*)head;
  MFEM_REQUIRE(op->mg, "no multigrid hierarchy is attached");
  return mg_setup(ctx, op->mg);
}
int mfem_mg_level0_products(const mfem_brick_multigrid_s* mg) { return mg_cycle_products(0, mg->nlev, mg->opt.nu, mg->opt.nu_c); }
mfem_brick_multigrid_s* mfem_mg_of(const mfem_csr_s* A) {
  if (!A->op || A->op->kind != MFEM_OPERATOR_BRICK) return nullptr;
  return ((const mfem_brick_operator_s*)A->op)->mg;
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------------
// One body for the four create entry points.  `which` is BOP_MG_*: _CREATE builds the hierarchy of a hex-8 thermal operator; _CREATE_NONSYMMETRIC the
// same, marked nonsymmetric: created and set up with or without an active Nitsche term (the parameters are read live at every setup), and the opt-in of
// gmres! with the cycle (mg_solve_refusal_nonsym); _CREATE_ELASTICITY that of a hex-8 elasticity operator, three field-major fields per lattice point;
// _CREATE_HEX27 that of a hex-27 thermal operator: p-coarsening once onto a hex-8 brick of the same elements, then the thermal h-hierarchy.  The
// contract is the same for all: attached, one per operator, destroyed with it.
static int mg_create_entry(mfem_context ctx, uint64_t handle, const mfem_multigrid_options* opts, uint64_t* out, int which) {
  static const struct { const char* name; int tag; } entries[BOP_MG_ENTRIES] = {  // the entry point's name and the physics it builds hierarchies for
      {"mfem_brick_multigrid_create", BOP_PHYSICS_THERMAL}, {"mfem_brick_multigrid_create_nonsymmetric", BOP_PHYSICS_THERMAL},
      {"mfem_brick_multigrid_create_elasticity", BOP_PHYSICS_ELASTICITY}, {"mfem_brick_multigrid_create_hex27", BOP_PHYSICS_HEX27}};
  const auto& E = entries[which];
  MFEM_REQUIRE(out, "null out");
  *out = 0;
  mfem_operator_head* head = (mfem_operator_head*)(uintptr_t)handle;
  MFEM_REQUIRE(ctx && head, "null argument");
  if (head->kind == MFEM_OPERATOR_MESH) return mg_refuse(E.tag, "a mesh operator's handle: the hierarchy is built on the lattice of a brick");
  mfem_brick_operator_s* op = bop_from_handle(handle);
  MFEM_REQUIRE(op, "not an operator's handle");
  if (op->physics != E.tag) return mg_refuse(E.tag, mg_wrong_physics(which, op->physics));
  MFEM_REQUIRE(op->ctx == ctx, "the operator was created on another context");
  MFEM_REQUIRE(!op->mg, "the operator already has a hierarchy (one per operator: destroy it first)");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  const char* why = nullptr;  // the entry point's own refusal (the nonsymmetric one has none)
  if (which == BOP_MG_CREATE && mg_nitsche(op)) why = "a Nitsche (fixed_faces) term is active: K is not symmetric";
  if (which == BOP_MG_CREATE_ELASTICITY) why = mg_elasticity_refusal(op->elasticity.tau, op->elasticity.penalty_faces);
  if (which == BOP_MG_CREATE_HEX27) why = mg_hex27_refusal(op->brick->ng, mg_nitsche(op));
  if (why) return mg_refuse(E.tag, why);
  MgOptions opt;
  const char* bad = mg_options(opts, &opt);
  if (bad) {
    mfem_set_error("%s: %s", E.name, bad);
    return MFEM_ERR_INVALID;
  }
  mfem_brick_multigrid_s* mg = nullptr;
  const int rc = mg_create(ctx, op, opt, &mg);
  if (rc) return rc;
  mg->nonsym = which == BOP_MG_CREATE_NONSYMMETRIC;
  *out = (uint64_t)(uintptr_t)mg;
  return MFEM_OK;
}
extern "C" int mfem_brick_multigrid_create(mfem_context ctx, uint64_t handle, const mfem_multigrid_options* opts, uint64_t* out) try {
  return mg_create_entry(ctx, handle, opts, out, BOP_MG_CREATE);
} MFEM_API_CATCH("mfem_brick_multigrid_create")
extern "C" int mfem_brick_multigrid_create_nonsymmetric(mfem_context ctx, uint64_t handle, const mfem_multigrid_options* opts, uint64_t* out) try {
  return mg_create_entry(ctx, handle, opts, out, BOP_MG_CREATE_NONSYMMETRIC);
} MFEM_API_CATCH("mfem_brick_multigrid_create_nonsymmetric")
extern "C" int mfem_brick_multigrid_create_elasticity(mfem_context ctx, uint64_t handle, const mfem_multigrid_options* opts, uint64_t* out) try {
  return mg_create_entry(ctx, handle, opts, out, BOP_MG_CREATE_ELASTICITY);
} MFEM_API_CATCH("mfem_brick_multigrid_create_elasticity")
extern "C" int mfem_brick_multigrid_create_hex27(mfem_context ctx, uint64_t handle, const mfem_multigrid_options* opts, uint64_t* out) try {
  return mg_create_entry(ctx, handle, opts, out, BOP_MG_CREATE_HEX27);
} MFEM_API_CATCH("mfem_brick_multigrid_create_hex27")

// 1: a hierarchy of mfem_brick_multigrid_create_nonsymmetric, 0: any other; MFEM_ERR_INVALID: not a hierarchy's handle (mfem_multigrid_info keeps
// its layout: the flag is answered here)
extern "C" int mfem_brick_multigrid_nonsymmetric(uint64_t handle) try {
  mfem_brick_multigrid_s* mg = mg_from_handle(handle);
  MFEM_REQUIRE(mg, "not a multigrid hierarchy's handle");
  return mg->nonsym ? 1 : 0;
} MFEM_API_CATCH("mfem_brick_multigrid_nonsymmetric")

static int mg_target(mfem_context ctx, uint64_t handle, mfem_brick_multigrid_s** out) {
  mfem_brick_multigrid_s* mg = mg_from_handle(handle);
  MFEM_REQUIRE(ctx && mg, "null argument, or not a multigrid hierarchy's handle");
  MFEM_REQUIRE(mg->ctx == ctx, "the hierarchy was created on another context");
  MFEM_REQUIRE(!mg->fine->csr.op, "the operator is bound to a running solve");
  *out = mg;
  return MFEM_OK;
}

extern "C" int mfem_brick_multigrid_setup(mfem_context ctx, uint64_t handle) try {
  mfem_brick_multigrid_s* mg = nullptr;
  const int rc = mg_target(ctx, handle, &mg);
  if (rc) return rc;
  return mg_setup(ctx, mg);
} MFEM_API_CATCH("mfem_brick_multigrid_setup")

extern "C" int mfem_brick_multigrid_apply(mfem_context ctx, uint64_t handle, const double* r, double* z) try {
  mfem_brick_multigrid_s* mg = nullptr;
  const int rc = mg_target(ctx, handle, &mg);
  if (rc) return rc;
  MFEM_REQUIRE(r && z && r != z, "null vector, or z is r");
  MFEM_REQUIRE(mg->ready, "the hierarchy has had no successful setup (mfem_brick_multigrid_setup)");
  return mfem_mg_cycle(ctx, mg, r, z);
} MFEM_API_CATCH("mfem_brick_multigrid_apply")

extern "C" int mfem_brick_multigrid_info(uint64_t handle, mfem_multigrid_info* info) try {
  mfem_brick_multigrid_s* mg = mg_from_handle(handle);
  MFEM_REQUIRE(mg && info, "null argument, or not a multigrid hierarchy's handle");
  memset(info, 0, sizeof(*info));
  info->levels = mg->nlev;
  info->sign = mg->sign;
  for (int l = 0; l < mg->nlev; ++l) {
    info->nx[l] = mg->lev[l].ne[0];
    info->ny[l] = mg->lev[l].ne[1];
    info->nz[l] = mg->lev[l].ne[2];
    info->lambda_max[l] = mg->lev[l].lambda_max;
    info->products[l] = mg->lev[l].products;
  }
  info->setup_products = mg->setup_products;
  info->bytes = mg->bytes;
  info->cycles = mg->cycles;
  info->setups = mg->setups;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_brick_multigrid_info")

extern "C" int mfem_brick_multigrid_destroy(uint64_t handle) try {
  if (!handle) return MFEM_OK;
  mfem_brick_multigrid_s* mg = mg_from_handle(handle);
  MFEM_REQUIRE(mg, "not a multigrid hierarchy's handle");
  MFEM_REQUIRE(!mg->fine->csr.op, "the operator is bound to a running solve");
  mfem_mg_release(mg);
  return MFEM_OK;
} MFEM_API_CATCH("mfem_brick_multigrid_destroy")

extern "C" int mfem_debug_brick_multigrid_transfer(mfem_context ctx, uint64_t handle, int32_t level, int32_t restriction, const double* in, double* out) try {
  mfem_brick_multigrid_s* mg = nullptr;
  const int rc = mg_target(ctx, handle, &mg);
  if (rc) return rc;
  MFEM_REQUIRE(in && out && in != out, "null vector");
  MFEM_REQUIRE(level >= 0 && level + 1 < mg->nlev, "no level below this one");
  const MgLevel &F = mg->lev[level], &Cc = mg->lev[level + 1];
  return restriction ? mg_restrict(ctx, F, Cc, in, out) : mg_prolong(ctx, F, Cc, in, nullptr, out);
} MFEM_API_CATCH("mfem_debug_brick_multigrid_transfer")

extern "C" double* mfem_debug_brick_multigrid_coords(uint64_t handle, int32_t level, int32_t dim_id) {
  mfem_brick_multigrid_s* mg = mg_from_handle(handle);
  if (!mg || level < 0 || level >= mg->nlev || dim_id < 0 || dim_id > 2) return nullptr;
  return mg->lev[level].brick->coords[dim_id];
}
