// cg!: the two Jacobi-preconditioned CG passes behind mfem_solve (not in the reference, F5) with their kernels -- mfem_cg_pass, the classic recurrence
// (its z-carrying and scaled variants included), and mfem_cg_single_pass, one reduction group per iteration.  Which of the two a solve runs, and the
// scaled system of cg_variant 4, are decided and set up by the driver (krylov.hip); the lattice tiles' fused residual update restates k_cg_update's
// arithmetic in its own file (spmv_lat27_gather.hip: k_lat27_gather_cg).
//
// Vector streams of one iteration of mfem_cg_pass beside the SpMV (scaled CG, cg_variant 4; the other variants add the stream of 1 / d where they
// read it): k_cg_update reads A p and r and writes r (3); k_cg_pupdate reads r and p_it and writes p_(it+1) (3) -- 6 at the iterations that leave x
// alone.  x is written once per m iterations from the ring of the last m directions (cg_decide.h): a flush position adds the m - 1 earlier
// directions and the read and the write of x, 6 + (m - 1) + 2.  On average 6 + (m + 1) / m: 8 with m = 1 (x += alpha p every iteration), 7.125 with
// m = 8.  The pending updates are applied per element in iteration order, one fma per component each, as the per-iteration update applies them: x is
// the same bit for bit for every m, and nothing else in the iteration reads x.
#include "krylov.h"
#include "cg_decide.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------
// Jacobi-preconditioned CG (added solver; M = |diag K|).  Three kernels per iteration:
//   SpMV (+ p.Ap partials) | x,r update (+ r.z, r.r partials) | p update (+ scalar bookkeeping)
// ------------------------------------------------------------------------------------------
// Streaming hints of the two CG vector kernels (round 4; tools/ab_libs.sh with tools/cg_per_solve.py on one box): NT = 2, nontemporal LOADS, is worth
// 4.7 % of a CG iteration at 256^3 (0.758 -> 0.723 ms: the vectors of one iteration are within reach of the 256 MB Infinity Cache, plain stores keep p
// there for the SpMV that reads it next); NT = 1, nontemporal loads AND stores, 1 - 2 % at 512^3 (5.58 -> 5.45-5.54 ms; NT = 2 there: + 0.6 %).  Chosen by
// the vector length at the launch (cg_nt_mode); 0 = plain accesses (bit 0 of mfem_debug_set_cg_streaming off).
template <int NT>
__device__ __forceinline__ d2_t cg_ld(const d2_t* p, int64_t i) {
  if constexpr (NT >= 1) return __builtin_nontemporal_load(p + i);
  else return p[i];
}
template <int NT>
__device__ __forceinline__ void cg_st(d2_t* p, int64_t i, d2_t v) {
  if constexpr (NT == 1) __builtin_nontemporal_store(v, p + i);
  else p[i] = v;
}
#define CG_LD(p, i) cg_ld<NT>((p), (i))
#define CG_ST(p, i, v) cg_st<NT>((p), (i), (v))
static std::atomic<int> g_cg_streaming{1};
static std::atomic<int> g_cg_ring{0};  // depth of the ring of search directions: 0 = cg_ring_depth's own choice, 1 .. CG_RING_MAX forced
extern "C" int mfem_debug_set_cg_ring(int depth) try {
  ++mfem_debug_epoch;
  g_cg_ring = (depth >= 1 && depth <= CG_RING_MAX) ? depth : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_cg_ring")
static std::atomic<long long> g_cg_ring_passes{0};
extern "C" long long mfem_debug_cg_ring_count(void) { return g_cg_ring_passes; }
int mfem_cg_ring_depth(int64_t nv) { return cg_ring_depth(nv, g_cg_ring); }  // (krylov.hip: the work vectors of a cg! solve)
extern "C" int mfem_debug_set_cg_streaming(int on) try {
  ++mfem_debug_epoch;
  g_cg_streaming = on ? 1 : 0;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_cg_streaming")
enum { S_CG_RING_ALPHA = S_SOLVER + 8 };  // [ , + CG_RING_MAX): the step lengths of the iterations whose directions the ring holds (mfem_cg_pass)
struct CgArgs {
  int64_t n2;       // padded length / 2
  double n_inv;     // 1 / global n (for normalized_norm)
  double tol;
  int32_t maxiter;
  int32_t fixed;    // benchmark mode: never converge
  int64_t n_owned;  // entries in front of the ghost entries / padding (zrec: dinv counts as 0 behind them, whatever the array holds there)
  int32_t zrec;     // the `r` array carries z = r .* dinv (cg_variant 3): k_cg_pupdate then reads neither r nor dinv -- 9 vector
                    // streams per iteration instead of 10; r.z and r.r come from r = z ./ dinv in k_cg_update
  // scaled CG (cg_variant 4; sw = nullptr otherwise): the iteration runs on r^ = S^-1 r, the stop test wants |r|.  Far from convergence the
  // kernels store the bound smax^2 |r^|^2 >= |r|^2 (no extra stream, the test cannot fire wrongly); once that bound is within gate2 of the
  // tolerance they read S and store |S r^|^2 = |r|^2 itself -- the same stopping rule as the classic recurrence.
  const d2_t* sw;
  double smax2, gate2;
};

// z = r .* dinv ; p = z ; partials: [0,G) r.z  [G,2G) r.r
__global__ __launch_bounds__(MFEM_BLOCK) void k_cg_init(CgArgs a, d2_t* __restrict__ r, const d2_t* __restrict__ dinv,
                                                          d2_t* __restrict__ p, double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double rz = 0.0, rr = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
    const d2_t rv = r[i];
    const d2_t z = dinv ? rv * dinv[i] : rv;
    p[i] = z;
    if (a.zrec && dinv) r[i] = z;
    rz += rv.x * z.x + rv.y * z.y;
    rr += rv.x * rv.x + rv.y * rv.y;
  }
  const double s0 = block_reduce_sum(rz, red);
  const double s1 = block_reduce_sum(rr, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s0;
    partials[gridDim.x + blockIdx.x] = a.sw ? s1 * a.smax2 : s1;
  }
}

// Single workgroup: fold the init partials into S[RZ0], S[RR]; iteration counter = 0; DONE if already converged.
__global__ __launch_bounds__(MFEM_BLOCK) void k_cg_init_fin(CgArgs a, const double* __restrict__ partials, int np,
                                                              double* __restrict__ S, int32_t* __restrict__ flags) {
  __shared__ double red[4];
  const double rz = reduce_partials_bcast(partials, np, red);
  const double rr = reduce_partials_bcast(partials + np, np, red);
  if (threadIdx.x == 0) {
    S[S_RZ0] = rz;
    S[S_RR] = rr;
    flags[F_ITER] = 0;
    flags[F_DONE] = (!a.fixed && sqrt(rr * a.n_inv) <= a.tol) ? 1 : 0;
  }
}

__device__ __forceinline__ double recip_nr(double d) { return mfem_recip_nr(d); }  // (krylov.h)

// alpha = rz / p.Ap ; x += alpha p ; r -= alpha Ap ; partials2: [0,G) r.z  [G,2G) r.r   (z = r .* dinv)
template <int NT>
__global__ __launch_bounds__(MFEM_BLOCK) void k_cg_update(CgArgs a, int cur, const double* __restrict__ pap_partials,
                                                            int np, const d2_t* __restrict__ Ap,
                                                            const d2_t* __restrict__ dinv,
                                                            d2_t* __restrict__ r, const double* __restrict__ S,
                                                            const int32_t* __restrict__ flags,
                                                            double* __restrict__ partials2) {
  __shared__ double red[4];
  if (flags[F_DONE]) return;
  const double pap = np > 0 ? reduce_partials_bcast(pap_partials, np, red) : S[S_PAP];
  const double alpha = S[S_RZ0 + cur] / pap;
  const bool exact = a.sw && S[S_RR] * a.n_inv <= a.gate2;  // (S[RR]: what the previous iteration stored; uniform over the grid)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double rz = 0.0, rr = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
    const d2_t av = CG_LD(Ap, i);  // x += alpha p happens in k_cg_pupdate, which reads p anyway (one vector stream less per iteration)
    d2_t rv, z;
    if (a.zrec && dinv) {  // the array holds z: z -= alpha dinv .* Ap ; r = z ./ dinv for the two dot products only
      d2_t dv = dinv[i];
      if (2 * i >= a.n_owned) dv.x = 0.0;  // ghost entries (a neighbour's values, its dinv) and padding take no part
      if (2 * i + 1 >= a.n_owned) dv.y = 0.0;
      z = r[i] - alpha * (av * dv);
      r[i] = z;
      rv.x = dv.x != 0.0 ? z.x * recip_nr(dv.x) : 0.0;
      rv.y = dv.y != 0.0 ? z.y * recip_nr(dv.y) : 0.0;
    } else {
      rv = CG_LD(r, i) - alpha * av;
      CG_ST(r, i, rv);
      z = dinv ? rv * dinv[i] : rv;
    }
    rz += rv.x * z.x + rv.y * z.y;
    if (exact) {
      const d2_t t = a.sw[i] * rv;
      rr += t.x * t.x + t.y * t.y;
    } else {
      rr += rv.x * rv.x + rv.y * rv.y;
    }
  }
  const double s0 = block_reduce_sum(rz, red);
  const double s1 = block_reduce_sum(rr, red);
  if (threadIdx.x == 0) {
    partials2[blockIdx.x] = s0;
    partials2[gridDim.x + blockIdx.x] = (a.sw && !exact) ? s1 * a.smax2 : s1;
  }
}

// The ring of search directions as k_cg_pupdate and k_cg_xflush see it (cg_decide.h).  Slot 0 is the pass's p vector, slots 1 .. m - 1 lie n2 apart
// behind `ring`; alpha[k] is the step length of the iteration whose direction slot k holds.
struct CgRing {
  d2_t* p0;
  d2_t* ring;
  double* alpha;
  int32_t m;      // depth (a kernel instantiated for one depth uses its own constant)
  int32_t slot;   // of this iteration's p; the next one's goes to (slot + 1) % m
};
__device__ __forceinline__ d2_t* cg_ring_ptr(const CgRing& g, int64_t n2, int k) { return k == 0 ? g.p0 : g.ring + (int64_t)(k - 1) * n2; }
// x + alpha p as the iterate has always been updated: the compiler contracted `x + alpha * p` to one fma per component; spelled out, so that the
// deferred applications and the per-iteration one round alike whatever the contraction setting
__device__ __forceinline__ d2_t cg_axpy(double alpha, d2_t pv, d2_t xv) {
  d2_t o;
  o.x = __builtin_fma(alpha, pv.x, xv.x);
  o.y = __builtin_fma(alpha, pv.y, xv.y);
  return o;
}

// alpha (that of k_cg_update, recomputed from the same partials) ; beta = rz_new / rz_old ; p_(it+1) = z + beta p_it, read from slot it % m of the
// ring and written to slot (it + 1) % m ; workgroup 0 also advances the scalar state and stores alpha beside its direction.
// x: at a flush position ((it + 1) % m == 0, every iteration with m = 1) x += alpha_j p_j for the m - 1 earlier iterations of the ring, in iteration
// order, then this one's -- x[i] read once, written once.  The slot of the oldest of them is the slot p_(it+1) goes to: the same thread reads that
// element before it writes it (no __restrict__ on the ring).  Elsewhere x is not touched.  An iteration that turns out to be the last writes no
// direction; at a flush position x gets all m pending updates, elsewhere they are left to k_cg_xflush.
// MU: 1 = no ring (m = 1), 8 / 16 = that depth with the flush unrolled (all loads of an element in flight), 0 = the depth g.m.
template <int NT, int MU>
__global__ __launch_bounds__(MFEM_BLOCK) void k_cg_pupdate(CgArgs a, int cur, const double* __restrict__ pap_partials, int np1,
                                                             const double* __restrict__ partials2, int np,
                                                             const d2_t* __restrict__ r, const d2_t* __restrict__ dinv,
                                                             CgRing g, d2_t* __restrict__ x, double* __restrict__ S,
                                                             const int32_t* __restrict__ flags, int32_t* __restrict__ flags_next) {
  __shared__ double red[4];
  if (flags[F_DONE]) {  // the stop state moves on to the bank the next iteration reads
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      flags_next[F_DONE] = 1;
      flags_next[F_ITER] = flags[F_ITER];
    }
    return;
  }
  const double pap = np1 > 0 ? reduce_partials_bcast(pap_partials, np1, red) : S[S_PAP];
  const double alpha = S[S_RZ0 + cur] / pap;
  double rz_new, rr;
  if (np > 0) {
    rz_new = reduce_partials_bcast(partials2, np, red);
    rr = reduce_partials_bcast(partials2 + np, np, red);
  } else {
    rz_new = S[S_TMP0];
    rr = S[S_TMP1];
  }
  const double beta = rz_new / S[S_RZ0 + cur];
  const int iter = flags[F_ITER] + 1;
  const bool done = (!a.fixed && sqrt(rr * a.n_inv) <= a.tol) || iter >= a.maxiter;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int m = MU ? MU : g.m;
  const bool flush = MU == 1 || g.slot == m - 1;
  const d2_t* pc = cg_ring_ptr(g, a.n2, MU == 1 ? 0 : g.slot);
  d2_t* pn = cg_ring_ptr(g, a.n2, (MU == 1 || flush) ? 0 : g.slot + 1);
  constexpr int NE = MU > 1 ? MU - 1 : 1;  // earlier iterations of an unrolled flush
  double al[NE];
  if (MU > 1 && flush) {
#pragma unroll
    for (int k = 0; k < NE; ++k) al[k] = g.alpha[k];
  }
  // the pending updates of element i on top of xv, oldest first
  auto pending = [&](d2_t xv, int64_t i, d2_t pv) -> d2_t {
    if constexpr (MU > 1) {
      d2_t e[NE];
#pragma unroll
      for (int k = 0; k < NE; ++k) e[k] = CG_LD(cg_ring_ptr(g, a.n2, k), i);
#pragma unroll
      for (int k = 0; k < NE; ++k) xv = cg_axpy(al[k], e[k], xv);
    } else if constexpr (MU == 0) {
      for (int k = 0; k < m - 1; ++k) xv = cg_axpy(g.alpha[k], CG_LD(cg_ring_ptr(g, a.n2, k), i), xv);
    }
    return cg_axpy(alpha, pv, xv);
  };
  if (!done) {
    if (flush) {
      for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
        const d2_t rv = CG_LD(r, i), pv = CG_LD(pc, i);
        const d2_t xv = pending(CG_LD(x, i), i, pv);
        CG_ST(x, i, xv);
        const d2_t z = (dinv && !a.zrec) ? rv * dinv[i] : rv;
        CG_ST(pn, i, cg_axpy(beta, pv, z));
      }
    } else {
      for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
        const d2_t rv = CG_LD(r, i), pv = CG_LD(pc, i);
        const d2_t z = (dinv && !a.zrec) ? rv * dinv[i] : rv;
        CG_ST(pn, i, cg_axpy(beta, pv, z));
      }
    }
  } else if (flush) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) x[i] = pending(x[i], i, pc[i]);
  }
  // bookkeeping last: every workgroup has read flags/S before workgroup 0 can change them only if it
  // reads first -- workgroup 0 reads above, writes here; other workgroups read slots this write does
  // not touch (S[RZ0+cur], F_ITER is re-read only by the next kernel).
  // F_ITER / F_DONE of the NEXT iteration live in the other flag bank (iterations alternate between two banks, like the scalar
  // slots): no workgroup of this kernel reads what is written here, so a late workgroup still sees the flags its siblings saw --
  // and no separate 1-thread kernel per iteration is needed for it.
  // alpha[slot]: the flush of this ring reads the EARLIER slots only (this iteration's alpha it computes itself), k_cg_xflush runs after this kernel.
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    S[S_RZ0 + (cur ^ 1)] = rz_new;
    S[S_RR] = rr;
    if (MU != 1) g.alpha[g.slot] = alpha;
    flags_next[F_ITER] = iter;
    flags_next[F_DONE] = done ? 1 : 0;
  }
}

// End of a pass: the updates of x that the ring still holds -- F_ITER % m of them, slots 0 .. pending - 1 in order -- whichever way the pass ended
// (a tolerance stop inside a ring, maxiter, the end of a pass before a restart).  Nothing pending: returns at once.
__global__ __launch_bounds__(MFEM_BLOCK) void k_cg_xflush(int64_t n2, CgRing g, d2_t* __restrict__ x, const int32_t* __restrict__ flags) {
  const int pending = cg_ring_pending(flags[F_ITER], g.m);
  if (pending == 0) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += stride) {
    d2_t xv = x[i];
    for (int k = 0; k < pending; ++k) xv = cg_axpy(g.alpha[k], cg_ring_ptr(g, n2, k)[i], xv);
    x[i] = xv;
  }
}

int mfem_cg_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int, double tol, int64_t n_global,
                 int* iters_out, int* spmv_out) {
  // V.x (current iterate), V.b ; work: r, p (slot 0 of the ring of directions), Ap, slots 1 .. m - 1 of the ring ; dinv
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  double* r = V.w[0];
  double* p = V.w[1];
  double* Ap = V.w[2];
  const int m = V.cg_ring > 1 ? V.cg_ring : 1;  // (cg_decide.h; the driver has carved w[3 .. m + 1] one vector apart)
  CgRing ring{(d2_t*)p, m > 1 ? (d2_t*)V.w[3] : nullptr, S + S_CG_RING_ALPHA, m, 0};
  auto slot_ptr = [&](int k) -> double* { return k == 0 ? p : V.w[3] + (int64_t)(k - 1) * V.nv; };
  const double* dinv = V.dinv;
  const int64_t nv = V.nv;
  CgArgs a;
  a.n2 = nv / 2;
  a.n_inv = 1.0 / (double)n_global;
  a.tol = tol;
  a.maxiter = o->maxiter;
  a.fixed = o->fixed_iterations;
  a.zrec = (dinv && (o->cg_variant == 3 || (o->cg_variant == 0 && mfem_comm_world(ctx) <= 1))) ? 1 : 0;
  a.n_owned = V.n;
  a.sw = (const d2_t*)V.cg_s;
  a.smax2 = V.cg_smax * V.cg_smax;
  {
    const double ratio = V.cg_smin > 0.0 ? V.cg_smax / V.cg_smin : __builtin_huge_val();
    a.gate2 = 16.0 * tol * tol * ratio * ratio;
  }
  double* part1 = ctx->d_partials;                          // SpMV p.Ap partials
  double* part2 = ctx->d_partials + MFEM_MAX_PARTIALS;       // 2 x G
  int rc = mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out);
  if (rc) return rc;
  const int G = mfem_vec_grid(ctx, nv);
  hipLaunchKernelGGL(k_cg_init, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, (d2_t*)r, (const d2_t*)dinv, (d2_t*)p,
                     part2);
  MFEM_CHECK_LAUNCH();
  if (ctx->comm) {
    rc = mfem_fold_list(ctx, FoldList{{part2, part2 + G}, {G, G}, 2}, S + S_TMP0);
    if (rc) return rc;
    rc = mfem_comm_allreduce(ctx, S + S_TMP0, 2);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cg_init_fin, dim3(1), dim3(MFEM_BLOCK), 0, ctx->stream, a, S + S_TMP0, 1, S, F);
  } else {
    hipLaunchKernelGGL(k_cg_init_fin, dim3(1), dim3(MFEM_BLOCK), 0, ctx->stream, a, part2, G, S, F);
  }
  MFEM_CHECK_LAUNCH();
  const int check = o->check_every > 0 ? o->check_every : 32;
  const int nt = !g_cg_streaming ? 0 : (nv >= 40000000 ? 1 : 2);  // (see cg_ld / cg_st: loads only while a vector is within reach of the Infinity Cache)
  uint64_t key = mfem_pass_key(MFEM_SOLVER_CG, A, vals, V, tol, n_global, o);
  key = mfem_hash(key, dinv); key = mfem_hash(key, a.zrec); key = mfem_hash(key, V.cg_s); key = mfem_hash(key, a.smax2); key = mfem_hash(key, a.gate2);
  const bool lat_fused = mfem_lat27_cg_fused(ctx, A, vals);  // (lattice tiles of the hex-27 matrix, one rank: pass 2 inside the residual update)
  key = mfem_hash(key, (int)lat_fused); key = mfem_hash(key, m);
  const int unit = cg_ring_unit(m);
  if (m > 1) ++g_cg_ring_passes;
  int it = 0;
  // flag banks: iteration `it` reads bank it & 1 (k_cg_init_fin fills bank 0) and leaves the next state in the other one
  for (;;) {
    if (!o->fixed_iterations || it == 0) {
      rc = mfem_read_flags(ctx);
      if (rc) return rc;
      if (ctx->h_flags[4 * (it & 1) + F_DONE]) break;
    }
    const int burst = (o->maxiter - it) < check ? (o->maxiter - it) : check;
    if (burst <= 0) break;
    // k_cg_pupdate by streaming mode and ring depth (MU: 1 no ring, 8 / 16 unrolled, 0 any other depth)
#define CG_PUPDATE_NM(NT_, MU_, PAP_, NP1_, NP2_) hipLaunchKernelGGL((k_cg_pupdate<NT_, MU_>), dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, cur, PAP_, NP1_, part2, \
                                                                     NP2_, (const d2_t*)r, (const d2_t*)dinv, g, (d2_t*)V.x, S, F, Fn)
#define CG_PUPDATE_N(NT_, PAP_, NP1_, NP2_)                                      \
  do {                                                                           \
    if (m == 1) CG_PUPDATE_NM(NT_, 1, PAP_, NP1_, NP2_);                         \
    else if (m == 8) CG_PUPDATE_NM(NT_, 8, PAP_, NP1_, NP2_);                    \
    else if (m == 16) CG_PUPDATE_NM(NT_, 16, PAP_, NP1_, NP2_);                  \
    else CG_PUPDATE_NM(NT_, 0, PAP_, NP1_, NP2_);                                \
  } while (0)
#define CG_PUPDATE(PAP_, NP1_, NP2_)                                             \
  do {                                                                           \
    if (nt == 1) CG_PUPDATE_N(1, PAP_, NP1_, NP2_);                              \
    else if (nt == 2) CG_PUPDATE_N(2, PAP_, NP1_, NP2_);                         \
    else CG_PUPDATE_N(0, PAP_, NP1_, NP2_);                                      \
  } while (0)
    auto iteration = [&](int it_) -> int {
      const int cur = it_ & 1;
      int32_t* F = ctx->d_flags + 4 * cur;          // this iteration's bank
      int32_t* Fn = ctx->d_flags + 4 * (cur ^ 1);   // the next one's
      CgRing g = ring;
      g.slot = cg_ring_slot(it_, m);
      double* p = slot_ptr(g.slot);  // this iteration's direction
      int np1 = 0;
      // with a communicator: the exchange of p's boundary planes runs beside the rows that need no ghost entry, and every
      // reduction group is one fold kernel + one all-reduce
      if (lat_fused) {
        // lattice tiles, one rank: pass 1 (its blocks stay in the dump, p . A p comes as one partial per tile), the fold of the partials, then pass 2 and
        // the residual update in one kernel (spmv_lat27_gather.hip: k_lat27_gather_cg) -- A p itself is never stored
        int rc = mfem_spmv_halo(ctx, A, vals, p, nullptr, 1.0, 0.0, p, part1, &np1, F);
        if (rc) return rc;
        int npt = 0;
        const double* tp = mfem_lat27_dot_partials(A, &npt);  // (one per tile; both kernels below fold them themselves, like the partials of any other SpMV)
        const LatCgUpdate U{a.zrec, cur, (const double*)a.sw, a.smax2, a.gate2, a.n_inv, dinv, r, S, F, part2, tp, npt};
        rc = mfem_lat27_gather_cg_update(ctx, A, U, G);
        if (rc) return rc;
        CG_PUPDATE(tp, npt, G);
        MFEM_CHECK_LAUNCH();
        return MFEM_OK;
      }
      int rc = mfem_spmv_halo(ctx, A, vals, p, Ap, 1.0, 0.0, p, part1, &np1, F);
      if (rc) return rc;
      int np2 = G;
      if (ctx->comm) {
        rc = mfem_fold_list(ctx, FoldList{{part1}, {np1}, 1}, S + S_PAP, F);
        if (rc) return rc;
        rc = mfem_comm_allreduce(ctx, S + S_PAP, 1);
        if (rc) return rc;
        np1 = 0;
      }
#define CG_UPDATE(NT_) hipLaunchKernelGGL(k_cg_update<NT_>, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, cur, part1, np1, \
                                          (const d2_t*)Ap, (const d2_t*)dinv, (d2_t*)r, S, F, part2)
      if (nt == 1) CG_UPDATE(1); else if (nt == 2) CG_UPDATE(2); else CG_UPDATE(0);
#undef CG_UPDATE
      MFEM_CHECK_LAUNCH();
      if (ctx->comm) {
        rc = mfem_fold_list(ctx, FoldList{{part2, part2 + G}, {G, G}, 2}, S + S_TMP0, F);
        if (rc) return rc;
        rc = mfem_comm_allreduce(ctx, S + S_TMP0, 2);
        if (rc) return rc;
        np2 = 0;
      }
      CG_PUPDATE(part1, np1, np2);
      MFEM_CHECK_LAUNCH();
      return MFEM_OK;
    };
#undef CG_PUPDATE
#undef CG_PUPDATE_N
#undef CG_PUPDATE_NM
    // iterations alternate between two scalar slots (cur = it & 1) and walk the m slots of the ring: `unit` of them (cg_ring_unit; the even/odd PAIR
    // with m = 1) have constant arguments and are what is captured and replayed (mfem_cycle_run), starting at it % unit == 0; iterations after whole
    // units -- and, with a ring, those of a burst in front of them -- are launched directly with their own bank, slot and position
    int k = 0;
    if (m > 1)
      for (; k < burst && it % unit != 0; ++k, ++it) {
        rc = iteration(it);
        if (rc) return rc;
      }
    for (; k + unit <= burst && it % unit == 0; k += unit, it += unit) {
      rc = mfem_cycle_run(ctx, key, [&]() -> int {
        int r2 = MFEM_OK;
        for (int j = 0; j < unit && !r2; ++j) r2 = iteration(j);
        return r2;
      });
      if (rc) return rc;
    }
    for (; k < burst; ++k, ++it) {
      rc = iteration(it);
      if (rc) return rc;
    }
  }
  if (m > 1) {  // (m = 1: nothing is ever pending)
    hipLaunchKernelGGL(k_cg_xflush, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a.n2, ring, (d2_t*)V.x, (const int32_t*)(ctx->d_flags + 4 * (it & 1)));
    MFEM_CHECK_LAUNCH();
  }
  rc = mfem_read_flags(ctx);
  if (rc) return rc;
  // every iteration that runs (k_cg_pupdate: F_ITER + 1 unless DONE) has one product, A p; converged at k_cg_init_fin: 0 iterations, 0 products
  *iters_out = ctx->h_flags[4 * (it & 1) + F_ITER];
  *spmv_out += *iters_out;
  return MFEM_OK;
}

// ------------------------------------------------------------------------------------------
// Jacobi-PCG with ONE reduction group per iteration (Chronopoulos & Gear 1989; the form used by pipelined Krylov solvers).
// The classic recurrence needs p.Ap before it can update r and then (r.z, r.r) before it can update p: two dependent
// all-reduces per iteration on several GPUs.  Carrying s = A p by recurrence (s = w + beta s with w = A u, u = M^-1 r) makes
// all three scalars of an iteration -- gamma = r.u, delta = w.u, r.r -- available at the same point, right after the SpMV:
//     p = u + beta p ; s = w + beta s ; x += alpha p ; u -= alpha s ./ d  (r = u .* d for the dot products only)    one pass, 10 vector streams
//     w = A u  (+ delta partials)                                                       halo of u overlapped, as above
//     all-reduce(gamma, r.r, delta) ; beta' = gamma'/gamma ; alpha' = gamma'/(delta' - beta' gamma'/alpha)
// Same iterates as the classic CG in exact arithmetic (and the same stop rule, evaluated every iteration); in floating point
// they differ at round-off level.  Default with a communicator of more than one rank; mfem_solve_options.cg_variant selects.
// ------------------------------------------------------------------------------------------
enum { S_CG_GAMMA = S_SOLVER + 0, S_CG_ALPHA = S_SOLVER + 1, S_CG_BETA = S_SOLVER + 2 };

// u = r .* dinv ; partials: [0,G) r.u  [G,2G) r.r
__global__ __launch_bounds__(MFEM_BLOCK) void k_cgcg_init(CgArgs a, const d2_t* __restrict__ r, const d2_t* __restrict__ dinv,
                                                            d2_t* __restrict__ u, double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double ru = 0.0, rr = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
    const d2_t rv = r[i];
    const d2_t z = dinv ? rv * dinv[i] : rv;
    u[i] = z;
    ru += rv.x * z.x + rv.y * z.y;
    rr += rv.x * rv.x + rv.y * rv.y;
  }
  const double s0 = block_reduce_sum(ru, red);
  const double s1 = block_reduce_sum(rr, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s0;
    partials[gridDim.x + blockIdx.x] = a.sw ? s1 * a.smax2 : s1;  // (scaled CG: the bound, see CgArgs)
  }
}

// Single workgroup: the scalar step.  L.m == 3: fold the local partial sums (gamma', r.r, delta') here; L.m == 0: they are in
// T[0..2] already (folded and all-reduced).  init != 0: first step (beta = 0, alpha = gamma / delta, iteration counter 0).
__global__ __launch_bounds__(MFEM_BLOCK) void k_cgcg_scal(CgArgs a, FoldList L, const double* __restrict__ T, int init,
                                                            double* __restrict__ S, int32_t* __restrict__ flags) {
  __shared__ double red[4];
  if (!init && flags[F_DONE]) return;
  double g, rr, dl;
  if (L.m == 3) {
    g = reduce_partials_bcast(L.src[0], L.cnt[0], red);
    rr = reduce_partials_bcast(L.src[1], L.cnt[1], red);
    dl = reduce_partials_bcast(L.src[2], L.cnt[2], red);
  } else {
    g = T[0];
    rr = T[1];
    dl = T[2];
  }
  if (threadIdx.x != 0) return;
  S[S_RR] = rr;
  if (init) {
    S[S_CG_GAMMA] = g;
    S[S_CG_ALPHA] = g / dl;
    S[S_CG_BETA] = 0.0;
    flags[F_ITER] = 0;
    flags[F_DONE] = (!a.fixed && sqrt(rr * a.n_inv) <= a.tol) ? 1 : 0;
    return;
  }
  const int iter = flags[F_ITER] + 1;
  flags[F_ITER] = iter;
  if ((!a.fixed && sqrt(rr * a.n_inv) <= a.tol) || iter >= a.maxiter) {
    flags[F_DONE] = 1;
    return;
  }
  const double beta = g / S[S_CG_GAMMA];
  const double alpha = g / (dl - beta * g / S[S_CG_ALPHA]);
  S[S_CG_GAMMA] = g;
  S[S_CG_ALPHA] = alpha;
  S[S_CG_BETA] = beta;
}

// p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s ; u = r .* dinv ; partials: [0,G) r.u  [G,2G) r.r
__global__ __launch_bounds__(MFEM_BLOCK) void k_cgcg_update(CgArgs a, const d2_t* __restrict__ w, const d2_t* __restrict__ dinv,
                                                              d2_t* __restrict__ u, d2_t* __restrict__ p, d2_t* __restrict__ sv,
                                                              d2_t* __restrict__ x, d2_t* __restrict__ r,
                                                              const double* __restrict__ S, const int32_t* __restrict__ flags,
                                                              double* __restrict__ partials) {
  __shared__ double red[4];
  if (flags[F_DONE]) return;
  const double alpha = S[S_CG_ALPHA], beta = S[S_CG_BETA];
  const bool first = beta == 0.0;  // p and s hold nothing yet (or leftovers of an earlier pass)
  const bool exact = a.sw && S[S_RR] * a.n_inv <= a.gate2;  // scaled CG: |r| itself instead of its bound (a rank's own gate: the sum over
                                                            // ranks of bounds and exact parts is still a bound)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double ru = 0.0, rr = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n2; i += stride) {
    // (streaming loads: every vector is read once per iteration here -- see cg_ld)
    const d2_t uv = __builtin_nontemporal_load(u + i), wv = __builtin_nontemporal_load(w + i);
    const d2_t pv = first ? uv : uv + beta * __builtin_nontemporal_load(p + i);
    const d2_t sn = first ? wv : wv + beta * __builtin_nontemporal_load(sv + i);
    p[i] = pv;
    sv[i] = sn;
    x[i] = __builtin_nontemporal_load(x + i) + alpha * pv;
    d2_t rv, z;
    if (a.zrec && dinv) {  // u carries the recurrence (u -= alpha dinv .* s); r = u ./ dinv for the dot products only: r is neither read nor written
      d2_t dv = dinv[i];
      if (2 * i >= a.n_owned) dv.x = 0.0;  // ghost entries (u holds the neighbours' values there, dinv may hold theirs) and padding take no part
      if (2 * i + 1 >= a.n_owned) dv.y = 0.0;
      z = uv - alpha * (sn * dv);
      rv.x = dv.x != 0.0 ? z.x * recip_nr(dv.x) : 0.0;
      rv.y = dv.y != 0.0 ? z.y * recip_nr(dv.y) : 0.0;
    } else if (a.zrec) {  // no preconditioner (scaled CG, Identity): u IS r -- 9 vector streams, r neither read nor written
      z = uv - alpha * sn;
      rv = z;
      if (2 * i >= a.n_owned) rv.x = 0.0;  // (ghost entries and padding take no part in the sums)
      if (2 * i + 1 >= a.n_owned) rv.y = 0.0;
    } else {
      rv = r[i] - alpha * sn;
      r[i] = rv;
      z = dinv ? rv * dinv[i] : rv;
    }
    u[i] = z;
    // ghost entries of u may hold anything (a neighbour's values; NaN while an exchange is in flight in the test transport): their
    // r is 0 by the mask above, but 0 * NaN is NaN -- keep them out of the sums explicitly
    if (2 * i < a.n_owned) ru += rv.x * z.x;
    if (2 * i + 1 < a.n_owned) ru += rv.y * z.y;
    if (exact) {
      const d2_t sc = a.sw[i];
      if (2 * i < a.n_owned) rr += (sc.x * rv.x) * (sc.x * rv.x);
      if (2 * i + 1 < a.n_owned) rr += (sc.y * rv.y) * (sc.y * rv.y);
    } else {
      rr += rv.x * rv.x + rv.y * rv.y;
    }
  }
  const double s0 = block_reduce_sum(ru, red);
  const double s1 = block_reduce_sum(rr, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s0;
    partials[gridDim.x + blockIdx.x] = (a.sw && !exact) ? s1 * a.smax2 : s1;
  }
}

int mfem_cg_single_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int, double tol,
                        int64_t n_global, int* iters_out, int* spmv_out) {
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  double *r = V.w[0], *p = V.w[1], *sv = V.w[2], *u = V.w[3], *w = V.w[4];
  const double* dinv = V.dinv;
  const int64_t nv = V.nv;
  CgArgs a;
  a.n2 = nv / 2;
  a.n_inv = 1.0 / (double)n_global;
  a.tol = tol;
  a.maxiter = o->maxiter;
  a.fixed = o->fixed_iterations;
  a.zrec = 1;  // 10 vector streams in k_cgcg_update instead of 12 (9 without a preconditioner: u is r)
  a.n_owned = V.n;
  a.sw = (const d2_t*)V.cg_s;
  a.smax2 = V.cg_smax * V.cg_smax;
  {
    const double ratio = V.cg_smin > 0.0 ? V.cg_smax / V.cg_smin : __builtin_huge_val();
    a.gate2 = 16.0 * tol * tol * ratio * ratio;
  }
  double* part1 = ctx->d_partials;                      // SpMV w.u partials
  double* part2 = ctx->d_partials + MFEM_MAX_PARTIALS;   // 2 x G: r.u, r.r
  double* T = S + S_TMP0;
  int rc = mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out);
  if (rc) return rc;
  const int G = mfem_vec_grid(ctx, nv);
  // the scalar step after an SpMV: fold (+ all-reduce) gamma', r.r, delta' and advance alpha / beta / the stop flags
  auto scalars = [&](int np1, int init) -> int {
    const FoldList L{{part2, part2 + G, part1}, {G, G, np1}, 3};
    if (ctx->comm) {
      int rc = mfem_fold_list(ctx, L, T, init ? nullptr : F);
      if (rc) return rc;
      rc = mfem_comm_allreduce(ctx, T, 3);
      if (rc) return rc;
      hipLaunchKernelGGL(k_cgcg_scal, dim3(1), dim3(MFEM_BLOCK), 0, ctx->stream, a, FoldList{{nullptr}, {0}, 0}, T, init, S, F);
    } else {
      hipLaunchKernelGGL(k_cgcg_scal, dim3(1), dim3(MFEM_BLOCK), 0, ctx->stream, a, L, T, init, S, F);
    }
    MFEM_CHECK_LAUNCH();
    return MFEM_OK;
  };
  hipLaunchKernelGGL(k_cgcg_init, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, (const d2_t*)r, (const d2_t*)dinv, (d2_t*)u, part2);
  MFEM_CHECK_LAUNCH();
  int np1 = 0;
  rc = mfem_spmv_halo(ctx, A, vals, u, w, 1.0, 0.0, u, part1, &np1, nullptr);
  if (rc) return rc;
  rc = scalars(np1, 1);
  if (rc) return rc;
  const int check = o->check_every > 0 ? o->check_every : 32;
  uint64_t key = mfem_pass_key(MFEM_SOLVER_CG + 64, A, vals, V, tol, n_global, o);
  key = mfem_hash(key, dinv); key = mfem_hash(key, V.cg_s); key = mfem_hash(key, a.smax2); key = mfem_hash(key, a.gate2);
  auto iteration = [&]() -> int {
    hipLaunchKernelGGL(k_cgcg_update, dim3(G), dim3(MFEM_BLOCK), 0, ctx->stream, a, (const d2_t*)w, (const d2_t*)dinv, (d2_t*)u,
                       (d2_t*)p, (d2_t*)sv, (d2_t*)V.x, (d2_t*)r, S, F, part2);
    MFEM_CHECK_LAUNCH();
    int np = 0;
    int rc = mfem_spmv_halo(ctx, A, vals, u, w, 1.0, 0.0, u, part1, &np, F);
    if (rc) return rc;
    return scalars(np, 0);
  };
  int it = 0;
  for (;;) {
    if (!o->fixed_iterations || it == 0) {
      rc = mfem_read_flags(ctx);
      if (rc) return rc;
      if (ctx->h_flags[F_DONE]) break;
    }
    const int burst = (o->maxiter - it) < check ? (o->maxiter - it) : check;
    if (burst <= 0) break;
    for (int k = 0; k < burst; ++k, ++it) {
      rc = mfem_cycle_run(ctx, key, iteration);  // every iteration has the same kernel arguments: one captured cycle
      if (rc) return rc;
    }
  }
  rc = mfem_read_flags(ctx);
  if (rc) return rc;
  // the initial A u runs whatever the start finds (unguarded), then every iteration that runs (k_cgcg_scal: F_ITER + 1 unless DONE) has one, A u
  *iters_out = ctx->h_flags[F_ITER];
  *spmv_out += 1 + *iters_out;
  return MFEM_OK;
}
