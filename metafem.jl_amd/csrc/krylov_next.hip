// cgs!, tfqmr! and lsqr!  -- reference linear_solver/07_CGS.jl:13-52, 08_QMR.jl:3-74 and 06_LSQR.jl:10-70, statement for statement.
// cgs! is the alternative line to cgs2! in examples/incompressible_flow/lid_driven_cavity_flow/2D_Script.jl:98, the docs pick tfqmr! for
// incompressible flow (07_CGS.jl:6-7) and call lsqr! the most robust of the set.  As in the other solvers every scalar stays on the device,
// the kernels are guarded by the DONE flag and one iteration is captured and replayed as a graph (kk_drive); the host only polls the flag,
// and the products are counted on the device.
// One rank only (mfem_solve refuses a communicator): the vector kernels below sum their dot products over the whole (zero-padded) vector.
#include "krylov_kernels.h"

enum { F_NX_SKIP = F_AUX };  // lsqr!: the beta == 0 branch (or DONE) -- the done flag of the A' u product

// r = Pl(b - A x) is in place and S[S_RR] = r.r: iter = 1, or 0 iterations if normalized_norm(r) <= tol.  `init_products` run after
// this kernel unless the pass ends here (tfqmr!: A p, lsqr!: A' u).
__device__ void nx_init(const KrylovArgs& a, const double* __restrict__ S, int32_t* __restrict__ F, int init_products) {
  const bool conv = kk_converged(a, S[S_RR]);
  kk_start(conv, F);
  F[F_SPMV] = conv ? 0 : init_products;
  F[F_NX_SKIP] = conv ? 1 : 0;
}

// partial of x . y over the first n entries, written by thread 0 of every workgroup (the vector kernels that fuse an update with its norm)
__device__ __forceinline__ void nx_partial(double acc, double* __restrict__ part, double* red) {
  const double s = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

#define NX_LOOP(n2) \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, _st = (int64_t)gridDim.x * blockDim.x; i < (n2); i += _st)
// the two entries of pair i that belong to the first n (the rest of a vector is padding)
#define NX_DOT2(a, b) ((2 * i < n ? (a).x * (b).x : 0.0) + (2 * i + 1 < n ? (a).y * (b).y : 0.0))

// =====================================================================================================================================
// cgs!  (07_CGS.jl:13-52)
enum { CS_RHO = S_SOLVER + 0, CS_ALPHA, CS_BETA, CS_DOT = S_SOLVER + 8 };

__global__ void kcs_init(KrylovArgs a, double* __restrict__ S, int32_t* __restrict__ F) {
  nx_init(a, S, F, 0);
  S[CS_RHO] = S[CS_ALPHA] = S[CS_BETA] = 1.0;  // :24
}
// rhobar = rho ; rho = dot(r, r0) ; beta = rho / rhobar  (:31-33)
__global__ void kcs_beta(FoldArg fa, double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x != 0) return;
  const double rhobar = S[CS_RHO];
  S[CS_RHO] = S[CS_DOT];
  S[CS_BETA] = S[CS_RHO] / rhobar;
}
// s = r + beta p ; u = s + beta (p + beta u)  (:35-36)
__global__ __launch_bounds__(MFEM_BLOCK) void kcs_su(int64_t n2, const d2_t* __restrict__ r, const d2_t* __restrict__ p, d2_t* __restrict__ s,
                                                     d2_t* __restrict__ u, const double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const double beta = S[CS_BETA];
  NX_LOOP(n2) {
    const d2_t pi = p[i];
    const d2_t si = r[i] + beta * pi;
    s[i] = si;
    u[i] = si + beta * (pi + beta * u[i]);
  }
}
// alpha = rho / dot(v, r0)  (:40)
__global__ void kcs_alpha(FoldArg fa, double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x == 0) S[CS_ALPHA] = S[CS_RHO] / S[CS_DOT];
}
// p = s - alpha v ; x += alpha (p + s)  (:42-43)
__global__ __launch_bounds__(MFEM_BLOCK) void kcs_px(int64_t n2, const d2_t* __restrict__ s, const d2_t* __restrict__ v, d2_t* __restrict__ p,
                                                     d2_t* __restrict__ x, const double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const double alpha = S[CS_ALPHA];
  NX_LOOP(n2) {
    const d2_t si = s[i];
    const d2_t pi = si - alpha * v[i];
    p[i] = pi;
    x[i] = x[i] + alpha * (pi + si);
  }
}
// iter += 1 ; stop if normalized_norm(r) <= tol || iter > maxiter  (:49-50); A u and the true residual ran
__global__ void kcs_end(KrylovArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const int iter = F[F_ITER] + 1;
  F[F_ITER] = iter;
  F[F_SPMV] += 2;
  if (kk_converged(a, S[S_RR]) || iter > a.maxiter) F[F_DONE] = 1;
}

// =====================================================================================================================================
// tfqmr!  (08_QMR.jl:3-74)
enum { TQ_ALPHA = S_SOLVER + 0, TQ_BETA, TQ_RHO, TQ_RNORM, TQ_TAU, TQ_THETA, TQ_ETA, TQ_C1, TQ_E1, TQ_C2, TQ_E2, TQ_DOT = S_SOLVER + 16 };

// r_norm = tau = norm(r) ; rho = dot(r, r) ; theta = eta = 0  (:28-30)
__global__ void ktq_init(KrylovArgs a, double* __restrict__ S, int32_t* __restrict__ F) {
  nx_init(a, S, F, 1);
  S[TQ_ALPHA] = S[TQ_BETA] = 1.0;
  S[TQ_RNORM] = S[TQ_TAU] = sqrt(S[S_RR]);
  S[TQ_RHO] = S[S_RR];
  S[TQ_THETA] = S[TQ_ETA] = 0.0;
}
// alpha = rho / dot(v, r0)  (:33)
__global__ void ktq_alpha(FoldArg fa, double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x == 0) S[TQ_ALPHA] = S[TQ_RHO] / S[TQ_DOT];
}
// q = u - alpha v ; v = u + q  (:34-35)
__global__ __launch_bounds__(MFEM_BLOCK) void ktq_qv(int64_t n2, const d2_t* __restrict__ u, d2_t* __restrict__ v, d2_t* __restrict__ q,
                                                     const double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const double alpha = S[TQ_ALPHA];
  NX_LOOP(n2) {
    const d2_t ui = u[i];
    const d2_t qi = ui - alpha * v[i];
    q[i] = qi;
    v[i] = ui + qi;
  }
}
// r_cgs -= alpha tmp  (:38), and the partials of norm(r_cgs)^2 (:41) and dot(r_cgs, r0) (:58) in the same pass: [0, G) and [G, 2 G)
__global__ __launch_bounds__(MFEM_BLOCK) void ktq_rcgs(int64_t n, int64_t n2, const d2_t* __restrict__ tmp, const d2_t* __restrict__ r0,
                                                       d2_t* __restrict__ rc, double* __restrict__ part, const double* __restrict__ S,
                                                       const int32_t* __restrict__ F) {
  __shared__ double red[MFEM_BLOCK / MFEM_WAVE];
  if (F[F_DONE]) return;
  const double alpha = S[TQ_ALPHA];
  double arr = 0.0, ar0 = 0.0;
  NX_LOOP(n2) {
    const d2_t ri = rc[i] - alpha * tmp[i];
    rc[i] = ri;
    arr += NX_DOT2(ri, ri);
    ar0 += NX_DOT2(ri, r0[i]);
  }
  nx_partial(arr, part, red);
  nx_partial(ar0, part + gridDim.x, red);
}
// every scalar of the two half-steps and of the next direction (:40-59) -- none of them depends on d or x, so one kernel computes them
// all and a single vector pass applies them
__global__ void ktq_scalars(FoldArg fa, double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x != 0) return;
  const double alpha = S[TQ_ALPHA];
  const double r_norm_old = S[TQ_RNORM];
  const double r_norm = sqrt(S[TQ_DOT]);
  double theta = S[TQ_THETA], eta = S[TQ_ETA], tau = S[TQ_TAU];
  S[TQ_C1] = theta * theta * eta / alpha;  // d = u + (theta^2 eta / alpha) d  (:43)
  theta = r_norm_old / tau;
  double c = 1.0 / sqrt(1.0 + theta * theta);
  tau *= theta * c;
  eta = c * c * alpha;
  S[TQ_E1] = eta;                          // x += eta d  (:48)
  S[TQ_C2] = theta * theta * eta / alpha;  // d = q + (theta^2 eta / alpha) d  (:50)
  theta = sqrt(r_norm * r_norm_old) / tau;
  c = 1.0 / sqrt(1.0 + theta * theta);
  tau *= theta * c;
  eta = c * c * alpha;
  S[TQ_E2] = eta;                          // x += eta d  (:55)
  S[TQ_THETA] = theta;
  S[TQ_ETA] = eta;
  S[TQ_TAU] = tau;
  S[TQ_RNORM] = r_norm;
  const double rhobar = S[TQ_RHO];         // rhobar = rho ; rho = dot(r_cgs, r0) ; beta = rho / rhobar  (:57-59)
  S[TQ_RHO] = S[TQ_DOT + 1];
  S[TQ_BETA] = S[TQ_RHO] / rhobar;
}
// d = u + c1 d ; x += e1 d ; d = q + c2 d ; x += e2 d ; u = r_cgs + beta q ; p = u + beta (q + beta p)  (:43-61), one pass
__global__ __launch_bounds__(MFEM_BLOCK) void ktq_update(int64_t n2, const d2_t* __restrict__ rc, const d2_t* __restrict__ q, d2_t* __restrict__ u,
                                                         d2_t* __restrict__ d, d2_t* __restrict__ p, d2_t* __restrict__ x, const double* __restrict__ S,
                                                         const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const double c1 = S[TQ_C1], e1 = S[TQ_E1], c2 = S[TQ_C2], e2 = S[TQ_E2], beta = S[TQ_BETA];
  NX_LOOP(n2) {
    const d2_t qi = q[i], ui = u[i];
    d2_t di = ui + c1 * d[i];
    d2_t xi = x[i] + e1 * di;
    di = qi + c2 * di;
    x[i] = xi + e2 * di;
    d[i] = di;
    const d2_t un = rc[i] + beta * qi;
    u[i] = un;
    p[i] = un + beta * (qi + beta * p[i]);
  }
}
// iter += 1 ; iter > maxiter ends the pass (:65-66); A v and A p ran
__global__ void ktq_end(KrylovArgs a, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const int iter = F[F_ITER] + 1;
  F[F_ITER] = iter;
  F[F_SPMV] += 2;
  if (iter > a.maxiter) F[F_DONE] = 1;
}
// iter % checkiter == 0: the true residual r = Pl(b - A x) just ran (:67-71)
__global__ void ktq_check(KrylovArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  F[F_SPMV] += 1;
  if (sqrt(S[S_RR] * a.n_inv) <= a.tol) F[F_DONE] = 1;
}

// =====================================================================================================================================
// lsqr!  (06_LSQR.jl:10-70).  A' u is the product with the transposed working matrix (spmv_t.hip, built by mfem_solve): row i of it
// is Pl(A_r')'s row, p_i c_i a(j, i), what the reference's Pl(tmul!(A, u)) computes (:23-24, 42-43).
enum { LQ_ALPHA = S_SOLVER + 0, LQ_BETA, LQ_PHIBAR, LQ_RHOBAR, LQ_PHIR, LQ_THETAR, LQ_VDIV, LQ_DOT = S_SOLVER + 8 };

// beta = norm(u) (u = r: :18-19)
__global__ void klq_init(KrylovArgs a, double* __restrict__ S, int32_t* __restrict__ F) {
  nx_init(a, S, F, 1);
  S[LQ_BETA] = sqrt(S[S_RR]);
}
// u = r / beta  (:18-20), and every later u ./= beta (:41)
__global__ __launch_bounds__(MFEM_BLOCK) void klq_uscale(int64_t n2, const d2_t* src, d2_t* u, const double* __restrict__ S,
                                                         const int32_t* __restrict__ F, int flag) {
  if (F[flag]) return;
  const double beta = S[LQ_BETA];
  NX_LOOP(n2) u[i] = src[i] / beta;
}
// alpha = norm(v) ; v ./= alpha if alpha != 0 ; w = v ; phibar = beta ; rhobar = alpha  (:25-32): the scalars
__global__ void klq_start(FoldArg fa, double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x != 0) return;
  const double alpha = sqrt(S[LQ_DOT]);
  S[LQ_ALPHA] = alpha;
  S[LQ_VDIV] = alpha != 0.0 ? 1.0 : 0.0;
  S[LQ_PHIBAR] = S[LQ_BETA];
  S[LQ_RHOBAR] = alpha;
}
// ... the vectors
__global__ __launch_bounds__(MFEM_BLOCK) void klq_vw(int64_t n2, d2_t* __restrict__ v, d2_t* __restrict__ w, const double* __restrict__ S,
                                                     const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const bool div = S[LQ_VDIV] != 0.0;
  const double alpha = S[LQ_ALPHA];
  NX_LOOP(n2) {
    const d2_t vi = div ? v[i] / alpha : v[i];
    v[i] = vi;
    w[i] = vi;
  }
}
// out = Pl(tmp) - c out (u with c = alpha, :37; v with c = beta, :43) and the partials of norm(out)^2 (:39, :45)
__global__ __launch_bounds__(MFEM_BLOCK) void klq_lin_norm(int64_t n, int64_t n2, const d2_t* __restrict__ tmp, d2_t* __restrict__ out, double* __restrict__ part,
                                                           int slot, const double* __restrict__ S, const int32_t* __restrict__ F, int flag) {
  __shared__ double red[MFEM_BLOCK / MFEM_WAVE];
  if (F[flag]) return;
  const double c = S[slot];
  double acc = 0.0;
  NX_LOOP(n2) {
    const d2_t o = tmp[i] - c * out[i];
    out[i] = o;
    acc += NX_DOT2(o, o);
  }
  nx_partial(acc, part, red);
}
// beta = norm(u); the branch `beta != 0` (:40-49) runs while F_NX_SKIP is clear
__global__ void klq_beta(FoldArg fa, double* __restrict__ S, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x != 0) return;
  const double beta = sqrt(S[LQ_DOT]);
  S[LQ_BETA] = beta;
  F[F_NX_SKIP] = beta != 0.0 ? 0 : 1;
}
// alpha = norm(v) (inside the branch), then the plane rotation (:51-57) and its two coefficients phi / rho, theta / rho (:59-60)
__global__ void klq_rot(FoldArg fa, double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  kk_fold_dev(fa, S);
  if (threadIdx.x != 0) return;
  const bool branch = F[F_NX_SKIP] == 0;
  double alpha = S[LQ_ALPHA];
  if (branch) alpha = sqrt(S[LQ_DOT]);
  S[LQ_VDIV] = branch && alpha != 0.0 ? 1.0 : 0.0;  // v ./= alpha (:45-47)
  const double beta = S[LQ_BETA], rhobar = S[LQ_RHOBAR], phibar = S[LQ_PHIBAR];
  const double rho = sqrt(rhobar * rhobar + beta * beta);
  const double c = rhobar / rho, s = beta / rho;
  const double theta = s * alpha;
  S[LQ_RHOBAR] = -c * alpha;
  const double phi = c * phibar;
  S[LQ_PHIBAR] = s * phibar;
  S[LQ_ALPHA] = alpha;
  S[LQ_PHIR] = phi / rho;
  S[LQ_THETAR] = theta / rho;
}
// v ./= alpha (when the rotation kernel says so) ; x += (phi / rho) w ; w = v - (theta / rho) w  (:45-47, 59-60)
__global__ __launch_bounds__(MFEM_BLOCK) void klq_xw(int64_t n2, d2_t* __restrict__ v, d2_t* __restrict__ w, d2_t* __restrict__ x,
                                                     const double* __restrict__ S, const int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const bool div = S[LQ_VDIV] != 0.0;
  const double alpha = S[LQ_ALPHA], phir = S[LQ_PHIR], thetar = S[LQ_THETAR];
  NX_LOOP(n2) {
    d2_t vi = v[i];
    if (div) {
      vi = vi / alpha;
      v[i] = vi;
    }
    const d2_t wi = w[i];
    x[i] = x[i] + phir * wi;
    w[i] = vi - thetar * wi;
  }
}
// iter += 1 ; the true residual just ran ; stop if normalized_norm(r) <= tol || iter > maxiter  (:62-67)
__global__ void klq_end(KrylovArgs a, const double* __restrict__ S, int32_t* __restrict__ F) {
  if (F[F_DONE]) return;
  const int iter = F[F_ITER] + 1;
  F[F_ITER] = iter;
  F[F_SPMV] += F[F_NX_SKIP] ? 2 : 3;
  if (kk_converged(a, S[S_RR]) || iter > a.maxiter) {
    F[F_DONE] = 1;
    F[F_NX_SKIP] = 1;  // (the A' u product of a replay after DONE is skipped too)
  }
}

// =====================================================================================================================================
// (all three: the stop rule iter > maxiter fires by host iteration maxiter + 1)
int mfem_cgs_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int, double tol,
                  int64_t n_global, int* iters_out, int* spmv_out) {
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  const int64_t nv = V.nv;
  double *r = V.w[0], *r0 = V.w[1], *u = V.w[2], *p = V.w[3], *s = V.w[4], *v = V.w[5];
  KK k{ctx, nv, V.n, mfem_vec_grid(ctx, nv), S, F, ctx->stream};
  const KrylovArgs a = kk_args(tol, n_global, o);
  RC(mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out));  // :14-17
  K1(kcs_init, a, S, F);
  MFEM_CHECK_HIP(hipMemcpyAsync(r0, r, sizeof(double) * nv, hipMemcpyDeviceToDevice, ctx->stream));  // r0 = copy(r)
  for (double* z : {u, p, s, v}) MFEM_CHECK_HIP(hipMemsetAsync(z, 0, sizeof(double) * nv, ctx->stream));
  auto step = [&](int) -> int {
    FoldArg fa;
    RC(k.dot1_partials(r, r0, CS_DOT, &fa));
    K1F(kcs_beta, fa, S, F);
    KV(kcs_su, nv / 2, (const d2_t*)r, (const d2_t*)p, (d2_t*)s, (d2_t*)u, S, F);
    RC(k.spmv(A, vals, u, v));
    RC(k.dot1_partials(v, r0, CS_DOT, &fa));
    K1F(kcs_alpha, fa, S, F);
    KV(kcs_px, nv / 2, (const d2_t*)s, (const d2_t*)v, (d2_t*)p, (d2_t*)V.x, S, F);
    // r = b - A x (:45-47); not DONE-guarded, harmless: once DONE is set x no longer changes
    RC(mfem_true_residual(ctx, A, vals, V.b, V.x, r, S + S_RR));
    K1(kcs_end, a, S, F);
    return MFEM_OK;
  };
  return kk_drive(ctx, o, mfem_pass_key(MFEM_SOLVER_CGS, A, vals, V, tol, n_global, o), 1, (int64_t)o->maxiter + 1, step, kc_main, iters_out,
                  spmv_out);
}

int mfem_tfqmr_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int checkiter,
                    double tol, int64_t n_global, int* iters_out, int* spmv_out) {
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  const int64_t nv = V.nv;
  double *r = V.w[0], *r0 = V.w[1], *rc = V.w[2], *p = V.w[3], *q = V.w[4], *u = V.w[5], *v = V.w[6], *d = V.w[7], *tmp = V.w[8];
  KK k{ctx, nv, V.n, mfem_vec_grid(ctx, nv), S, F, ctx->stream};
  const KrylovArgs a = kk_args(tol, n_global, o);
  RC(mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out));  // :4-7
  K1(ktq_init, a, S, F);
  for (double* z : {r0, rc, p, u}) MFEM_CHECK_HIP(hipMemcpyAsync(z, r, sizeof(double) * nv, hipMemcpyDeviceToDevice, ctx->stream));  // :22-25
  for (double* z : {q, d, tmp}) MFEM_CHECK_HIP(hipMemsetAsync(z, 0, sizeof(double) * nv, ctx->stream));
  RC(k.spmv(A, vals, p, v));  // v = Pl(A p)  (:26-27)
  auto step = [&](int form) -> int {
    FoldArg fa;
    RC(k.dot1_partials(v, r0, TQ_DOT, &fa));
    K1F(ktq_alpha, fa, S, F);
    KV(ktq_qv, nv / 2, (const d2_t*)u, (d2_t*)v, (d2_t*)q, S, F);
    RC(k.spmv(A, vals, v, tmp));
    KV(ktq_rcgs, V.n, nv / 2, (const d2_t*)tmp, (const d2_t*)r0, (d2_t*)rc, ctx->d_partials, S, F);
    K1F(ktq_scalars, FoldArg{ctx->d_partials, k.G, 2, TQ_DOT}, S, F);
    KV(ktq_update, nv / 2, (const d2_t*)rc, (const d2_t*)q, (d2_t*)u, (d2_t*)d, (d2_t*)p, (d2_t*)V.x, S, F);
    RC(k.spmv(A, vals, p, v));
    K1(ktq_end, a, F);
    if (form == KC_ALT) {  // (iter % checkiter == 0: the only iterations that compute a residual)
      RC(mfem_true_residual(ctx, A, vals, V.b, V.x, r, S + S_RR));
      K1(ktq_check, a, S, F);
    }
    return MFEM_OK;
  };
  uint64_t key = mfem_pass_key(MFEM_SOLVER_TFQMR, A, vals, V, tol, n_global, o);
  key = mfem_hash(key, checkiter);
  const bool fixed = o->fixed_iterations != 0;
  auto variant = [&](int, int64_t iter) { return !fixed && iter % checkiter == 0 ? KC_ALT : KC_MAIN; };
  return kk_drive(ctx, o, key, 1, (int64_t)o->maxiter + 1, step, variant, iters_out, spmv_out);
}

int mfem_lsqr_pass(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, KrylovVecs& V, const mfem_solve_options* o, int, double tol,
                   int64_t n_global, int* iters_out, int* spmv_out) {
  MFEM_REQUIRE(V.AT && (V.valsT || V.AT->nnz == 0), "lsqr!: the transposed working matrix is missing");
  double* S = ctx->d_scalars;
  int32_t* F = ctx->d_flags;
  const int64_t nv = V.nv;
  double *r = V.w[0], *u = V.w[1], *v = V.w[2], *w = V.w[3], *tmp = V.w[4];
  KK k{ctx, nv, V.n, mfem_vec_grid(ctx, nv), S, F, ctx->stream};
  const KrylovArgs a = kk_args(tol, n_global, o);
  RC(mfem_pass_residual(ctx, A, vals, V, r, S + S_RR, spmv_out));  // :11-14
  K1(klq_init, a, S, F);
  for (double* z : {u, v, w, tmp}) MFEM_CHECK_HIP(hipMemsetAsync(z, 0, sizeof(double) * nv, ctx->stream));
  // u = r / beta ; v = Pl(A' u) ; alpha = norm(v) ; v ./= alpha ; w = v ; phibar = beta ; rhobar = alpha  (:18-32)
  KV(klq_uscale, nv / 2, (const d2_t*)r, (d2_t*)u, S, F, (int)F_DONE);
  RC(mfem_spmv_launch(ctx, V.AT, V.valsT, u, v, 1.0, 0.0, nullptr, nullptr, nullptr, F));
  FoldArg fa0;
  RC(k.dot1_partials(v, v, LQ_DOT, &fa0));
  K1F(klq_start, fa0, S, F);
  KV(klq_vw, nv / 2, (d2_t*)v, (d2_t*)w, S, F);
  const FoldArg fa{ctx->d_partials, k.G, 1, LQ_DOT};
  auto step = [&](int) -> int {
    RC(k.spmv(A, vals, v, tmp));                                                        // tmp = A v
    KV(klq_lin_norm, V.n, nv / 2, (const d2_t*)tmp, (d2_t*)u, ctx->d_partials, (int)LQ_ALPHA, S, F, (int)F_DONE);  // u = Pl(tmp) - alpha u
    K1F(klq_beta, fa, S, F);                                                                         // beta = norm(u)
    KV(klq_uscale, nv / 2, (const d2_t*)u, (d2_t*)u, S, F, (int)F_NX_SKIP);                         // u ./= beta
    RC(mfem_spmv_launch(ctx, V.AT, V.valsT, u, tmp, 1.0, 0.0, nullptr, nullptr, nullptr, F + F_NX_SKIP));  // tmp = A' u
    KV(klq_lin_norm, V.n, nv / 2, (const d2_t*)tmp, (d2_t*)v, ctx->d_partials, (int)LQ_BETA, S, F, (int)F_NX_SKIP);  // v = Pl(tmp) - beta v
    K1F(klq_rot, fa, S, F);
    KV(klq_xw, nv / 2, (d2_t*)v, (d2_t*)w, (d2_t*)V.x, S, F);
    RC(mfem_true_residual(ctx, A, vals, V.b, V.x, r, S + S_RR));                                 // r = Pl(b - A x)  (:64-66)
    K1(klq_end, a, S, F);
    return MFEM_OK;
  };
  uint64_t key = mfem_pass_key(MFEM_SOLVER_LSQR, A, vals, V, tol, n_global, o);
  key = mfem_csr_graph_key(key, V.AT); key = mfem_hash(key, V.valsT);
  return kk_drive(ctx, o, key, 1, (int64_t)o->maxiter + 1, step, kc_main, iters_out, spmv_out);
}
