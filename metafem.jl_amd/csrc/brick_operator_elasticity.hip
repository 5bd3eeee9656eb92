// The matrix-free hex-8 brick operator on three-field linear elasticity: y = alpha K x~ + beta y and |diag K| for the K of
// mfem_brick_assemble_elasticity -- the volume term -int sigma_ij(u) d_jN_a and the penalty faces -tau N_a N_b delta_fg -- straight from the brick's
// coordinates.  K x is the fused residual (hex8_elasticity.hip) with the traction dropped and x as the displacement; traction_faces and sig contribute
// nothing to K and are never read.  Unknowns are field-major (brick_xindex), n = 3 n_owned; x~_j = x_j / dsc_j when a solve on A D^-1 binds its
// column scaling, x otherwise.  The handle, the entry points and the contract of a launch: brick_operator.hip; what both files share: brick_operator.h.
//   volume  k_bop_elasticity_sweep (2-point rule): the plane sweep of k_elasticity_residual_sweep<2> -- same 15 x 15 tile, same segments, same
//           request() prefetch, same summation order; k_bop_elasticity_points (1-, 3- and 4-point rules): the per-control-point form of
//           k_elasticity_residual on the immutable tables of bop_tables.  Every unknown is written once, by its owner: y = alpha r + beta y
//           (beta == 0: y is not read).  With partial sums the work items are folded onto <= BOP_VOLUME_PARTIALS workgroups (brick_operator_decide.h).
//   faces   k_bop_elasticity_faces: a thread strides over the boundary control points and adds alpha times its own penalty rows.
//   diagonal k_bop_elasticity_diagonal: a thread per control point, for f = 0..2
//           K_(f,a),(f,a) = -sum_el sum_q w det [lam g_f^2 + mu (|g|^2 + g_f^2)] - tau sum_faces sum_q w^s N_a^2; a zero sum keeps the preset.
// No atomics; the same bits on every run.
#include "hex8_device.h"
#include "hex8_sumfac.h"
#include "blas1.h"
#include "brick_operator.h"

// =================================================================================================
// Volume, sweep form.  The body is k_elasticity_residual_sweep<2>'s (read its comments first: the prefetch discipline of request() is kept word for
// word -- every thread requests on every step, from clamped positions, and the scaling's division happens where the requested plane is CONSUMED, never
// in request(), which would wait for the loads at once).  DSC and DOT are template parameters: the unscaled product carries no scaling registers,
// and the product that leaves no partial sums (one workgroup per item) neither the fold's loop nor the dot's accumulator -- the arithmetic on y is
// the same in all four instantiations, so are the bits.
// =================================================================================================
template <bool DSC, bool DOT>
__global__ __launch_bounds__(SW_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_bop_elasticity_sweep(
    BrickView B, int L, int64_t items, double lam, double mu, const double* __restrict__ x, const double* __restrict__ dsc, double* __restrict__ y,
    double alpha, double beta, const double* __restrict__ dotw, double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  __shared__ double Fe[SW_THREADS * ESW_STRIDE];
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  const int tid = threadIdx.x, ek = tid % SW_E, ej = tid / SW_E;
  double dot_acc = 0.0;
  int64_t w = blockIdx.x;
  do {  // (workgroup-uniform; DOT: the items w, w + grid, ...; otherwise the one item of this workgroup)
    const SweepTile T = h8_sweep_tile((unsigned)w, B.m1, B.m2, B.plo, B.phi, L, SW_N, SW_N);
    const int J = T.tj0 - 1 + ej, K = T.tk0 - 1 + ek;  // phase A: this thread's element column
    const bool el_ok = J >= 0 && J < B.ne1 && K >= 0 && K < B.ne2;
    const int j = T.tj0 + ej, k = T.tk0 + ek;          // phase B: this thread's control point column
    const bool nd_ok = ej < SW_N && ek < SW_N && j < B.m1 && k < B.m2;
    double Xn[3][4], Un[3][4], Dn[3][4];  // the plane requested last (consumed at the top of the next step)
    const int Jc = min(max(J, 0), B.ne1 - 1), Kc = min(max(K, 0), B.ne2 - 1);
    auto request = [&](int ip) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t ci = brick_cindex(B, ip, Jc + (c & 1), Kc + (c >> 1));
        Xn[0][c] = B.X0[ci];
        Xn[1][c] = B.X1[ci];
        Xn[2][c] = B.X2[ci];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          const int64_t xi = brick_xindex(B, f, ip, Jc + (c & 1), Kc + (c >> 1));
          Un[f][c] = x[xi];
          if constexpr (DSC) Dn[f][c] = dsc[xi];
        }
      }
    };
    double X[3][2][4], U[3][2][4];
    const int Ifirst = max(T.i0 - 1, 0), Ilast = min(T.i1 - 1, B.ne0 - 1);  // element planes of this segment
    {
      request(Ifirst);
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          X[d][1][c] = Xn[d][c];
          U[d][1][c] = DSC ? Un[d][c] / Dn[d][c] : Un[d][c];
        }
      request(Ifirst + 1);
    }
    double carry[3] = {0.0, 0.0, 0.0};
    for (int I = T.i0 - 1; I < T.i1; ++I) {
      const bool plane = I >= 0 && I < B.ne0;  // workgroup-uniform
      if (plane && el_ok) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
          for (int c = 0; c < 4; ++c) {  // last step's upper nodes are this step's lower ones; the requested plane arrives
            X[d][0][c] = X[d][1][c];
            U[d][0][c] = U[d][1][c];
            X[d][1][c] = Xn[d][c];
            U[d][1][c] = DSC ? Un[d][c] / Dn[d][c] : Un[d][c];
          }
        double fe[3][2][4];
        sf_elasticity_fe<2>(X, U, lam, mu, fe);
#pragma unroll
        for (int f = 0; f < 3; ++f)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            Fe[tid * ESW_STRIDE + f * 8 + 2 * c] = fe[f][0][c];
            Fe[tid * ESW_STRIDE + f * 8 + 2 * c + 1] = fe[f][1][c];
          }
      }
      request(min(max(I + 2, Ifirst), Ilast + 1));  // in flight during the rest of this plane's step
      mfem_lds_barrier();
      if (nd_ok) {
        double lo[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 0.0, 0.0};
        if (plane) {
#pragma unroll
          for (int ez = 0; ez < 2; ++ez)
#pragma unroll
            for (int ey = 0; ey < 2; ++ey) {
              const int Jn = j - 1 + ey, Kn = k - 1 + ez;
              if (Jn < 0 || Jn >= B.ne1 || Kn < 0 || Kn >= B.ne2) continue;
              const double* fp = Fe + ((ej + ey) * SW_E + ek + ez) * ESW_STRIDE + 2 * ((1 - ey) + 2 * (1 - ez));
#pragma unroll
              for (int f = 0; f < 3; ++f) {
                lo[f] += fp[f * 8];
                up[f] += fp[f * 8 + 1];
              }
            }
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          if (I >= T.i0) {
            const int64_t row = (int64_t)f * B.n_owned + (int64_t)(I - B.plo) * B.plane_len + (int64_t)j * B.m2 + k;
            double yv = alpha * (carry[f] + lo[f]);
            if (beta != 0.0) yv += beta * y[row];
            y[row] = yv;
            if (DOT && dotw) dot_acc += yv * dotw[row];
          }
          carry[f] = up[f];
        }
      }
      mfem_lds_barrier();
    }
  } while (DOT && (w += gridDim.x) < items);
  if constexpr (DOT) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Volume, per-control-point form (1-, 3- and 4-point rules): the arithmetic of k_elasticity_residual without its face terms, on the tables of
// bop_tables.  Work item w = the H8_BLOCK control points from w H8_BLOCK on (bop_point_range).
// =================================================================================================
__global__ __launch_bounds__(MFEM_BLOCK) void k_bop_elasticity_points(BrickView B, const H8Tables* __restrict__ T8, int64_t items, double lam, double mu,
                                                                        const double* __restrict__ x, const double* __restrict__ dsc, double* __restrict__ y,
                                                                        double alpha, double beta, const double* __restrict__ dotw,
                                                                        double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int nq = B.ng * B.ng * B.ng;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {  // (workgroup-uniform)
    const int64_t node = w * MFEM_BLOCK + threadIdx.x;
    if (node >= B.n_owned) continue;
    int i, j, k;
    node_ijk(B, node, i, j, k);
    double r[3] = {0.0, 0.0, 0.0};
    for (int e = 0; e < 8; ++e) {
      const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
      const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
      if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
      const int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
      double X[8][3], u[8][3];
      hex8_load_coords(B, I, J, K, X);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int ni = I + (b & 1), nj = J + ((b >> 1) & 1), nk = K + (b >> 2);
#pragma unroll
        for (int f = 0; f < 3; ++f) u[b][f] = bop_scaled(x, dsc, brick_xindex(B, f, ni, nj, nk));
      }
      for (int q = 0; q < nq; ++q) {
        double g[8][3];
        const double wd = bop_geom(T8, X, q, g);
        double du[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // du[i][j] = d_j u_i
        double ga[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 8; ++b) {
#pragma unroll
          for (int fi = 0; fi < 3; ++fi)
#pragma unroll
            for (int fj = 0; fj < 3; ++fj) du[fi][fj] += u[b][fi] * g[b][fj];
          const bool me = (b == a);
          ga[0] = me ? g[b][0] : ga[0];
          ga[1] = me ? g[b][1] : ga[1];
          ga[2] = me ? g[b][2] : ga[2];
        }
        const double tr = du[0][0] + du[1][1] + du[2][2];
#pragma unroll
        for (int fi = 0; fi < 3; ++fi) {
          double acc = 0.0;
#pragma unroll
          for (int fj = 0; fj < 3; ++fj) {
            double sg = mu * (du[fi][fj] + du[fj][fi]);
            if (fi == fj) sg += lam * tr;
            acc += sg * ga[fj];
          }
          r[fi] -= wd * acc;
        }
      }
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const int64_t row = (int64_t)f * B.n_owned + node;
      double yv = alpha * r[f];
      if (beta != 0.0) yv += beta * y[row];
      y[row] = yv;
      if (dotw) dot_acc += yv * dotw[row];
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Penalty faces of the rows of control point (i, j, k) (elasticity_face_residual with dw = 0 and no traction).
//   DIAG = false: r[f] = sum_faces sum_q w^s N_a (-tau) sum_b N_b x~_(f,b); DIAG = true: r[0] = -tau sum_faces sum_q w^s N_a^2 (the same for every field)
// =================================================================================================
template <bool DIAG>
__device__ __forceinline__ void bop_penalty_rows(const BrickView& B, const H8Tables* __restrict__ T8, double tau, uint32_t penalty, int i, int j, int k,
                                                 const double* __restrict__ x, const double* __restrict__ dsc, double (&r)[3]) {
  visit_boundary_faces(B, i, j, k, penalty, [&](int nd, int side, int ca, const int (&fn)[4][3], const double (&Xf)[4][3]) {
    double uf[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int f = 0; f < 3; ++f) uf[c][f] = DIAG ? 0.0 : bop_scaled(x, dsc, brick_xindex(B, f, fn[c][0], fn[c][1], fn[c][2]));
    for (int q = 0; q < B.ng * B.ng; ++q) {
      const double ws = bop_face_weight(T8, Xf, q, side == 0);
      double na = 0.0, uq[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        na = (c == ca) ? T8->fN[q][c] : na;
#pragma unroll
        for (int f = 0; f < 3; ++f) uq[f] += T8->fN[q][c] * uf[c][f];
      }
      if (DIAG) {
        r[0] += ws * na * (-tau * na);
      } else {
#pragma unroll
        for (int f = 0; f < 3; ++f) r[f] += ws * na * (tau * (0.0 - uq[f]));
      }
    }
  });
}

// a thread strides over the boundary control points; after the volume kernel (y holds alpha K_vol x~ + beta y): y += alpha (penalty rows . x~), and
// the increments' partial sums of dotw . y over the three fields
__global__ __launch_bounds__(MFEM_BLOCK) void k_bop_elasticity_faces(BrickView B, const H8Tables* __restrict__ T8, double tau, uint32_t penalty, int64_t count,
                                                                       const double* __restrict__ x, const double* __restrict__ dsc, double* __restrict__ y,
                                                                       double alpha, const double* __restrict__ dotw, double* __restrict__ partials,
                                                                       const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x; t < count; t += (int64_t)gridDim.x * MFEM_BLOCK) {
    int i, j, k;
    if (!h8_boundary_point(t, B.plo, B.phi, B.ne0, B.ne1, B.ne2, B.plane_len, B.m1, B.m2, i, j, k)) continue;
    const int64_t node = (int64_t)(i - B.plo) * B.plane_len + (int64_t)j * B.m2 + k;
    double r[3] = {0.0, 0.0, 0.0};
    bop_penalty_rows<false>(B, T8, tau, penalty, i, j, k, x, dsc, r);
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const int64_t row = (int64_t)f * B.n_owned + node;
      const double inc = alpha * r[f];
      y[row] += inc;
      if (dotw) dot_acc += inc * dotw[row];
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Diagonal: d_(f,a) <- |K_(f,a),(f,a)| where it is not zero (else d keeps its preset: the guarded rule of jacobi.hip).  A thread per control point sums,
// over its <= 8 adjacent elements, -sum_q w det [lam g_f^2 + mu (|g|^2 + g_f^2)] with g = grad N_a (table form), then its own penalty term.
// Nothing is stored per element.  Runs once per solve.
// =================================================================================================
template <bool SIGNED>  // (SIGNED: K_(f,a),(f,a) itself, for the multigrid setup, which reads the sign of K from it)
__global__ __launch_bounds__(MFEM_BLOCK) void k_bop_elasticity_diagonal(BrickView B, const H8Tables* __restrict__ T8, double lam, double mu, double tau,
                                                                          uint32_t penalty, int face_terms, double* __restrict__ d) {
  const int64_t node = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x;
  if (node >= B.n_owned) return;
  int i, j, k;
  node_ijk(B, node, i, j, k);
  double sum[3] = {0.0, 0.0, 0.0};
  const int nq = B.ng * B.ng * B.ng;
  if (lam != 0.0 || mu != 0.0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
      const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
      if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
      const int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
      double X[8][3];
      hex8_load_coords(B, I, J, K, X);
      double acc[3] = {0.0, 0.0, 0.0};
      for (int q = 0; q < nq; ++q) {
        double g[8][3];
        const double wd = bop_geom(T8, X, q, g);
        const double g2 = g[a][0] * g[a][0] + g[a][1] * g[a][1] + g[a][2] * g[a][2];
#pragma unroll
        for (int f = 0; f < 3; ++f) acc[f] -= wd * (lam * (g[a][f] * g[a][f]) + mu * (g2 + g[a][f] * g[a][f]));
      }
#pragma unroll
      for (int f = 0; f < 3; ++f) sum[f] += acc[f];
    }
  }
  if (face_terms && (i == 0 || i == B.ne0 || j == 0 || j == B.ne1 || k == 0 || k == B.ne2)) {
    double r[3] = {0.0, 0.0, 0.0};
    bop_penalty_rows<true>(B, T8, tau, penalty, i, j, k, nullptr, nullptr, r);
#pragma unroll
    for (int f = 0; f < 3; ++f) sum[f] += r[0];
  }
#pragma unroll
  for (int f = 0; f < 3; ++f)
    if (sum[f] != 0.0) d[(int64_t)f * B.n_owned + node] = SIGNED ? sum[f] : fabs(sum[f]);
}

// ---- host side (called from brick_operator.hip: bop_launch, bop_jacobi) -----------------------------------------------------------------------------
int bop_elasticity_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                          double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  const mfem_brick_s* m = op->brick;
  const mfem_elasticity_params& p = op->elasticity;
  const BopVolume V = bop_elasticity_volume(m->ng, m->m[0], m->m[1], m->m[2]);
  const int64_t vgrid = bop_volume_grid(V, partials != nullptr);  // (folded onto the partial sums only when some are asked for)
  MFEM_REQUIRE(vgrid < ((int64_t)1 << 31), "too many work items for one launch");
  if (V.kernel == BOP_SWEEP) {
    const auto kernel = partials ? (dsc ? k_bop_elasticity_sweep<true, true> : k_bop_elasticity_sweep<false, true>)
                                 : (dsc ? k_bop_elasticity_sweep<true, false> : k_bop_elasticity_sweep<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)vgrid), dim3(SW_THREADS), 0, ctx->stream, B, V.L, V.items, p.lambda, p.mu, x, dsc, y, alpha, beta, dotw,
                       partials, done_flag);
  } else {
    hipLaunchKernelGGL(k_bop_elasticity_points, dim3((unsigned)vgrid), dim3(MFEM_BLOCK), 0, ctx->stream, B, op->tables, V.items, p.lambda, p.mu, x, dsc, y,
                       alpha, beta, dotw, partials, done_flag);
  }
  MFEM_CHECK_LAUNCH();
  int np = partials ? V.grid : 0;
  if (bop_elasticity_face_launch(p.tau, p.penalty_faces)) {
    const int64_t count = bop_boundary_count(m->m[0], m->m[1], m->m[2]);
    const int grid = bop_face_grid(count);
    hipLaunchKernelGGL(k_bop_elasticity_faces, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, op->tables, p.tau, p.penalty_faces, count, x, dsc,
                       y, alpha, dotw, partials ? partials + np : nullptr, done_flag);
    MFEM_CHECK_LAUNCH();
    if (partials) np += grid;
  }
  if (n_partials) *n_partials = np;
  return MFEM_OK;
}

template <bool SIGNED>
static int bop_elasticity_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) {
  const mfem_elasticity_params& p = op->elasticity;
  const int64_t grid = bop_diagonal_grid(B.n_owned);
  MFEM_REQUIRE(grid < ((int64_t)1 << 31), "too many control points for one launch");
  hipLaunchKernelGGL(k_bop_elasticity_diagonal<SIGNED>, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, op->tables, p.lambda, p.mu, p.tau, p.penalty_faces,
                     bop_elasticity_face_launch(p.tau, p.penalty_faces) ? 1 : 0, d);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
int bop_elasticity_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) { return bop_elasticity_diagonal<false>(ctx, op, B, d); }
int bop_elasticity_signed_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) {
  return bop_elasticity_diagonal<true>(ctx, op, B, d);
}
