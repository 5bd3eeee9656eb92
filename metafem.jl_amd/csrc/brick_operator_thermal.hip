// The hex-8 thermal physics of the matrix-free brick operator (BOP_PHYSICS_THERMAL): y = alpha K x~ + beta y and diag K for the K of
// mfem_brick_assemble_thermal -- the volume term -k grad N_a . grad N_b, the Robin faces -h N_a N_b and the weakly imposed (Nitsche) Dirichlet faces
// N_a (-h_penalty N_b + k n . grad N_b), which make K nonsymmetric -- straight from the brick's coordinates: no pattern, no values, no element
// matrices, no scratch.  K x is the fused residual (hex8_thermal.hip) with s = 0, Tenv = 0, Tw = 0; x~_j = x_j / dsc_j when a solve on A D^-1 binds its
// column scaling, x otherwise.
//   volume  k_brick_product_sweep (2- and 3-point rules): the plane sweep of k_thermal_residual_sweep -- same 15 x 15 tile, same segments, same
//           request() prefetch, same affine shortcut, no source stream; k_brick_product_tiles (1- and 4-point rules): the 4 x 4 x 8 tiles of
//           k_thermal_residual.  Every control point is written once, by its owner: y = alpha r + beta y (beta == 0: y is not read).
//   faces   k_brick_product_faces: a thread per boundary control point (row-owner, like k_thermal_residual_robin) adds alpha times its own Robin and
//           Nitsche terms, computed from x~ of the host elements: one launch in place of the residual's Robin kernel and the 24 coloured launches of
//           mfem_brick_nitsche_faces.  A product is two launches, one without face terms.
//   diagonal k_brick_diagonal: a thread per control point sums the diagonal entries of its <= 8 adjacent Ke and its own face terms; a zero sum keeps
//           the preset (the guarded rule of jacobi.hip).
// The handle, the entry points, the bind and the contract of a launch are brick_operator.hip's, whose ops table hands an operator of this physics over to
// the three launchers at the end of this file, as it hands the other three physics over to theirs; what the files share is in brick_operator.h.
#include "hex8_device.h"
#include "hex8_sumfac.h"
#include "blas1.h"
#include "brick_operator.h"

// what the kernels take of the weak form (thermal; the elasticity block and its kernels: brick_operator_elasticity.hip)
struct BopThermal {
  double k, h, hp;
  uint32_t robin, fixed;
  int ng;
  double gp[4], gw[4];  // 1-D Gauss points / weights on [0, 1] (the Nitsche terms evaluate the host element's basis on the face)
  const H8Tables* T;    // the reference-cell tables of the brick's rule: bop_tables
};

// =================================================================================================
// Volume, sweep form.  The body is k_thermal_residual_sweep's (read its comments first: the prefetch discipline of request() is kept word for word --
// every thread requests on every step, from clamped positions, and the scaling's division happens where the requested plane is CONSUMED, never in
// request(), which would wait for the loads at once).
// =================================================================================================
template <int NG>
__global__ __launch_bounds__(SW_THREADS) __attribute__((amdgpu_waves_per_eu(NG == 2 ? 2 : 1))) void k_brick_product_sweep(
    BrickView B, int L, int64_t items, double kcond, const double* __restrict__ x, const double* __restrict__ dsc, double* __restrict__ y, double alpha,
    double beta, int affine_fast, const double* __restrict__ dotw, double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  __shared__ double Fe[SW_THREADS * 9];
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  const int tid = threadIdx.x, ek = tid % SW_E, ej = tid / SW_E;
  const bool has_dsc = dsc != nullptr;
  double dot_acc = 0.0;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {  // (workgroup-uniform)
    const SweepTile T = h8_sweep_tile((unsigned)w, B.m1, B.m2, B.plo, B.phi, L, SW_N, SW_N);
    const int J = T.tj0 - 1 + ej, K = T.tk0 - 1 + ek;  // phase A: this thread's element column
    const bool el_ok = J >= 0 && J < B.ne1 && K >= 0 && K < B.ne2;
    const int j = T.tj0 + ej, k = T.tk0 + ek;          // phase B: this thread's control point column
    const bool nd_ok = ej < SW_N && ek < SW_N && j < B.m1 && k < B.m2;
    double Xn[3][4], Tq[4], Dq[4];  // the plane requested last (consumed at the top of the next step)
#pragma unroll
    for (int c = 0; c < 4; ++c) Dq[c] = 1.0;
    const int Jc = min(max(J, 0), B.ne1 - 1), Kc = min(max(K, 0), B.ne2 - 1);
    auto request = [&](int ip) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t ci = brick_cindex(B, ip, Jc + (c & 1), Kc + (c >> 1));
        Xn[0][c] = B.X0[ci];
        Xn[1][c] = B.X1[ci];
        Xn[2][c] = B.X2[ci];
        const int64_t xi = brick_xindex(B, 0, ip, Jc + (c & 1), Kc + (c >> 1));
        Tq[c] = x[xi];
        if (has_dsc) Dq[c] = dsc[xi];
      }
    };
    double X[3][2][4], Tn[2][4], Sn[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) Sn[0][c] = Sn[1][c] = 0.0;
    const int Ifirst = max(T.i0 - 1, 0), Ilast = min(T.i1 - 1, B.ne0 - 1);  // element planes of this segment
    {
      request(Ifirst);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        X[0][1][c] = Xn[0][c]; X[1][1][c] = Xn[1][c]; X[2][1][c] = Xn[2][c];
        Tn[1][c] = has_dsc ? Tq[c] / Dq[c] : Tq[c];
      }
      request(Ifirst + 1);
    }
    double carry = 0.0;
    for (int I = T.i0 - 1; I < T.i1; ++I) {
      const bool plane = I >= 0 && I < B.ne0;  // workgroup-uniform
      if (plane && el_ok) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // last step's upper nodes are this step's lower ones; the requested plane arrives
          X[0][0][c] = X[0][1][c]; X[1][0][c] = X[1][1][c]; X[2][0][c] = X[2][1][c];
          Tn[0][c] = Tn[1][c];
          X[0][1][c] = Xn[0][c]; X[1][1][c] = Xn[1][c]; X[2][1][c] = Xn[2][c];
          Tn[1][c] = has_dsc ? Tq[c] / Dq[c] : Tq[c];
        }
        double fe[2][4];
        if (affine_fast && sf_is_affine(X)) sf_thermal_fe<NG, true>(X, Tn, Sn, false, kcond, fe);
        else sf_thermal_fe<NG, false>(X, Tn, Sn, false, kcond, fe);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          Fe[tid * 9 + 2 * c] = fe[0][c];
          Fe[tid * 9 + 2 * c + 1] = fe[1][c];
        }
      }
      request(min(max(I + 2, Ifirst), Ilast + 1));  // in flight during the rest of this plane's step
      mfem_lds_barrier();
      if (nd_ok) {
        double lo = 0.0, up = 0.0;
        if (plane) {
#pragma unroll
          for (int ez = 0; ez < 2; ++ez)
#pragma unroll
            for (int ey = 0; ey < 2; ++ey) {
              const int Jn = j - 1 + ey, Kn = k - 1 + ez;
              if (Jn < 0 || Jn >= B.ne1 || Kn < 0 || Kn >= B.ne2) continue;
              const double* f = Fe + ((ej + ey) * SW_E + ek + ez) * 9 + 2 * ((1 - ey) + 2 * (1 - ez));
              lo += f[0];
              up += f[1];
            }
        }
        if (I >= T.i0) {
          const int64_t node = (int64_t)(I - B.plo) * B.plane_len + (int64_t)j * B.m2 + k;
          double yv = alpha * (carry + lo);
          if (beta != 0.0) yv += beta * y[node];
          y[node] = yv;
          if (dotw) dot_acc += yv * dotw[node];
        }
        carry = up;
      }
      mfem_lds_barrier();
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Volume, tile form (1- and 4-point rules): k_thermal_residual without its source and Robin terms.
// =================================================================================================
__global__ __launch_bounds__(TT_THREADS) void k_brick_product_tiles(BrickView B, const H8Tables* __restrict__ T8, int64_t items, double kcond, const double* __restrict__ x,
                                                                      const double* __restrict__ dsc, double* __restrict__ y, double alpha, double beta,
                                                                      const double* __restrict__ dotw, double* __restrict__ partials,
                                                                      const int32_t* __restrict__ done_flag) {
  __shared__ double Fe[TT_NEL * 9];
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  const int tid = threadIdx.x;
  double dot_acc = 0.0;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {  // (workgroup-uniform)
    const H8TileOrigin T = h8_tile_origin(w, B.m1, B.m2, B.plo);
    for (int e = tid; e < TT_NEL; e += TT_THREADS) {
      const int ek = e % TT_EK, ej = (e / TT_EK) % TT_EJ, ei = e / (TT_EK * TT_EJ);
      const int I = T.ti - 1 + ei, J = T.tj - 1 + ej, K = T.tk - 1 + ek;
      if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
      double X[8][3], Tn[8], fe[8];
      hex8_load_coords(B, I, J, K, X);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        Tn[b] = bop_scaled(x, dsc, brick_xindex(B, 0, I + (b & 1), J + ((b >> 1) & 1), K + (b >> 2)));
        fe[b] = 0.0;
      }
      const int nq = B.ng * B.ng * B.ng;
      for (int q = 0; q < nq; ++q) {
        double g[8][3];
        const double wd = bop_geom(T8, X, q, g);
        double gT0 = 0.0, gT1 = 0.0, gT2 = 0.0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          gT0 += g[b][0] * Tn[b];
          gT1 += g[b][1] * Tn[b];
          gT2 += g[b][2] * Tn[b];
        }
        const double c = -kcond * wd;
#pragma unroll
        for (int a = 0; a < 8; ++a) fe[a] += c * (g[a][0] * gT0 + g[a][1] * gT1 + g[a][2] * gT2);
      }
#pragma unroll
      for (int a = 0; a < 8; ++a) Fe[e * 9 + a] = fe[a];
    }
    __syncthreads();
    const int lk = tid % TT_NK, lj = (tid / TT_NK) % TT_NJ, li = tid / (TT_NK * TT_NJ);
    const int i = T.ti + li, j = T.tj + lj, k = T.tk + lk;
    if (i < B.phi && j < B.m1 && k < B.m2) {
      const int64_t node = (int64_t)(i - B.plo) * B.plane_len + (int64_t)j * B.m2 + k;
      double r = 0.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
        if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
        const int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
        r += Fe[((li + ex) * (TT_EJ * TT_EK) + (lj + ey) * TT_EK + (lk + ez)) * 9 + a];
      }
      double yv = alpha * r;
      if (beta != 0.0) yv += beta * y[node];
      y[node] = yv;
      if (dotw) dot_acc += yv * dotw[node];
    }
    __syncthreads();  // (the next work item overwrites Fe)
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Face terms of row (i, j, k).  DIAG = false: sum_b K^face_ab x~_b; DIAG = true: K^face_aa.
//   Robin    sum_q w^s N_a (-h) N_b                                   (k_thermal_matrix_robin)
//   Nitsche  sum_q w^s N_a (-h_penalty N_b + k n . grad N_b)           (k_brick_nitsche: the basis of ALL eight nodes of the host element on the face)
// =================================================================================================
template <bool DIAG>
__device__ __forceinline__ double bop_robin_row(const BrickView& B, const BopThermal& P, int i, int j, int k, const double* __restrict__ x,
                                                const double* __restrict__ dsc) {
  double r = 0.0;
  visit_boundary_faces(B, i, j, k, P.robin, [&](int nd, int side, int ca, const int (&fn)[4][3], const double (&Xf)[4][3]) {
    double Tf[4] = {0.0, 0.0, 0.0, 0.0};
    if (!DIAG) {
#pragma unroll
      for (int c = 0; c < 4; ++c) Tf[c] = bop_scaled(x, dsc, brick_xindex(B, 0, fn[c][0], fn[c][1], fn[c][2]));
    }
    for (int q = 0; q < B.ng * B.ng; ++q) {
      const double ws = bop_face_weight(P.T, Xf, q, side == 0);
      double na = 0.0, Tq = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        na = (c == ca) ? P.T->fN[q][c] : na;
        Tq += P.T->fN[q][c] * Tf[c];
      }
      r += (-P.h * ws) * (na * (DIAG ? na : Tq));
    }
  });
  return r;
}

template <bool DIAG>
__device__ __forceinline__ double bop_nitsche_row(const BrickView& B, const BopThermal& P, int i, int j, int k, const double* __restrict__ x,
                                                  const double* __restrict__ dsc) {
  double r = 0.0;
  const int idx[3] = {i, j, k};
  const int ne[3] = {B.ne0, B.ne1, B.ne2};
  for (int nd = 0; nd < 3; ++nd) {
    for (int side = 0; side < 2; ++side) {
      const bool on = side == 0 ? (idx[nd] == 0) : (idx[nd] == ne[nd]);
      if (!on || !(P.fixed & face_bit(nd, side))) continue;
      const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
      for (int q4 = 0; q4 < 4; ++q4) {  // the <= 4 face elements that contain the point
        const int f1 = q4 & 1, f2 = q4 >> 1;
        int E[3], la[3];
        E[nd] = side ? ne[nd] - 1 : 0;
        E[t1] = idx[t1] - 1 + f1;
        E[t2] = idx[t2] - 1 + f2;
        if (E[t1] < 0 || E[t1] >= ne[t1] || E[t2] < 0 || E[t2] >= ne[t2]) continue;
        la[nd] = side;
        la[t1] = 1 - f1;
        la[t2] = 1 - f2;
        double X[8][3], Tn[8];
        hex8_load_coords(B, E[0], E[1], E[2], X);  // node b = b0 + 2 b1 + 4 b2
#pragma unroll
        for (int b = 0; b < 8; ++b)
          Tn[b] = DIAG ? 0.0 : bop_scaled(x, dsc, brick_xindex(B, 0, E[0] + (b & 1), E[1] + ((b >> 1) & 1), E[2] + (b >> 2)));
        for (int q = 0; q < P.ng * P.ng; ++q) {
          const int q1 = q % P.ng, q2 = q / P.ng;  // first in-face coordinate fastest
          double xi[3];
          xi[nd] = side ? 1.0 : 0.0;
          xi[t1] = P.gp[q1];
          xi[t2] = P.gp[q2];
          double Lb[3][2];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            Lb[d][0] = 1.0 - xi[d];
            Lb[d][1] = xi[d];
          }
          double Nb[8], dN[8][3];
          double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const int b0 = b & 1, b1 = (b >> 1) & 1, b2 = b >> 2;
            const double s0 = b0 ? 1.0 : -1.0, s1 = b1 ? 1.0 : -1.0, s2 = b2 ? 1.0 : -1.0;
            Nb[b] = Lb[0][b0] * Lb[1][b1] * Lb[2][b2];
            dN[b][0] = s0 * Lb[1][b1] * Lb[2][b2];
            dN[b][1] = Lb[0][b0] * s1 * Lb[2][b2];
            dN[b][2] = Lb[0][b0] * Lb[1][b1] * s2;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              J[c][0] += dN[b][0] * X[b][c];
              J[c][1] += dN[b][1] * X[b][c];
              J[c][2] += dN[b][2] * X[b][c];
            }
          }
          const double det = J[0][0] * J[1][1] * J[2][2] - J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] + J[0][1] * J[1][2] * J[2][0] +
                             J[0][2] * J[1][0] * J[2][1] - J[0][2] * J[1][1] * J[2][0];
          const double id = 1.0 / det;
          double Iv[3][3];
          Iv[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
          Iv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
          Iv[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) * id;
          Iv[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) * id;
          Iv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
          Iv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
          Iv[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
          Iv[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) * id;
          Iv[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) * id;
          double ta[3], tb[3];  // tangents, the first negated on the low face: ta x tb points outward
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double jt1 = t1 == 0 ? J[c][0] : t1 == 1 ? J[c][1] : J[c][2];
            const double jt2 = t2 == 0 ? J[c][0] : t2 == 1 ? J[c][1] : J[c][2];
            ta[c] = side ? jt1 : -jt1;
            tb[c] = jt2;
          }
          const double r0 = ta[1] * tb[2] - ta[2] * tb[1], r1 = -ta[0] * tb[2] + ta[2] * tb[0], r2 = ta[0] * tb[1] - ta[1] * tb[0];
          const double ld = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
          const double nrm[3] = {r0 / ld, r1 / ld, r2 / ld};
          const double ws = P.gw[q1] * P.gw[q2] * ld;
          double v[3];  // n . grad N_b = sum_m dN_b/dxi_m v[m]
#pragma unroll
          for (int m = 0; m < 3; ++m) v[m] = Iv[m][0] * nrm[0] + Iv[m][1] * nrm[1] + Iv[m][2] * nrm[2];
          const int a = la[0] + 2 * la[1] + 4 * la[2];
          double Na = 0.0, ga = 0.0, Tq = 0.0, dTn = 0.0;
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const double gb = dN[b][0] * v[0] + dN[b][1] * v[1] + dN[b][2] * v[2];
            Na = b == a ? Nb[b] : Na;
            ga = b == a ? gb : ga;
            Tq += Nb[b] * Tn[b];
            dTn += gb * Tn[b];
          }
          r += DIAG ? ws * Na * (-P.hp * Na + P.k * ga) : ws * Na * (-P.hp * Tq + P.k * dTn);
        }
      }
    }
  }
  return r;
}

template <bool DIAG>
__device__ __forceinline__ double bop_face_row(const BrickView& B, const BopThermal& P, int i, int j, int k, const double* __restrict__ x,
                                               const double* __restrict__ dsc) {
  double r = 0.0;
  if (h8_robin_launch(P.h, P.robin)) r += bop_robin_row<DIAG>(B, P, i, j, k, x, dsc);
  if (bop_nitsche_on(P.k, P.hp, P.fixed)) r += bop_nitsche_row<DIAG>(B, P, i, j, k, x, dsc);
  return r;
}

// a thread strides over the boundary control points; after the volume kernel (y holds alpha K_vol x~ + beta y): y += alpha (face row . x~), and the
// increments' partial sums of dotw . y
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick_product_faces(BrickView B, BopThermal P, int64_t count, const double* __restrict__ x,
                                                                      const double* __restrict__ dsc, double* __restrict__ y, double alpha,
                                                                      const double* __restrict__ dotw, double* __restrict__ partials,
                                                                      const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x; t < count; t += (int64_t)gridDim.x * MFEM_BLOCK) {
    int i, j, k;
    if (!h8_boundary_point(t, B.plo, B.phi, B.ne0, B.ne1, B.ne2, B.plane_len, B.m1, B.m2, i, j, k)) continue;
    const int64_t node = (int64_t)(i - B.plo) * B.plane_len + (int64_t)j * B.m2 + k;
    const double inc = alpha * bop_face_row<false>(B, P, i, j, k, x, dsc);
    y[node] += inc;
    if (dotw) dot_acc += inc * dotw[node];
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Diagonal: d_i <- |K_ii| where K_ii != 0 (else d_i keeps its preset).  A thread per control point: the (a, a) entry of each adjacent element's
// Ke = sum_q w det (-k) |grad N_a|^2 (table form, hex8_geom), then the point's own face terms.  Nothing is stored.  Runs once per solve.
// =================================================================================================
template <bool SIGNED>  // (SIGNED: K_ii itself, for the multigrid setup, which reads the sign of K from it)
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick_diagonal(BrickView B, BopThermal P, double* __restrict__ d) {
  const int64_t node = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x;
  if (node >= B.n_owned) return;
  int i, j, k;
  node_ijk(B, node, i, j, k);
  double sum = 0.0;
  const int nq = B.ng * B.ng * B.ng;
  if (P.k != 0.0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
      const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
      if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
      const int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
      double X[8][3];
      hex8_load_coords(B, I, J, K, X);
      double acc = 0.0;
      for (int q = 0; q < nq; ++q) {
        double g[8][3];
        const double wd = bop_geom(P.T, X, q, g);
        acc += (-P.k * wd) * (g[a][0] * g[a][0] + g[a][1] * g[a][1] + g[a][2] * g[a][2]);
      }
      sum += acc;
    }
  }
  if (i == 0 || i == B.ne0 || j == 0 || j == B.ne1 || k == 0 || k == B.ne2) sum += bop_face_row<true>(B, P, i, j, k, nullptr, nullptr);
  if (sum != 0.0) d[node] = SIGNED ? sum : fabs(sum);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
static BopThermal bop_thermal(const mfem_brick_operator_s* op) {
  BopThermal P;
  memset(&P, 0, sizeof(P));
  const mfem_thermal_params& p = op->thermal;
  P.k = p.k; P.h = p.h; P.hp = p.h_penalty;
  P.robin = p.robin_faces; P.fixed = p.fixed_faces;
  P.ng = op->brick->ng;
  P.T = op->tables;
  for (int q = 0; q < P.ng; ++q) {
    P.gp[q] = H8_GP[P.ng - 1][q] / 2.0 + 0.5;
    P.gw[q] = H8_GW[P.ng - 1][q] / 2.0;
  }
  return P;
}

// the product on the view its caller verified (bop_view); the launch contract is bop_launch's
int bop_thermal_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                       double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  const mfem_brick_s* m = op->brick;
  const BopThermal P = bop_thermal(op);
  const BopVolume V = bop_volume(m->ng, m->m[0], m->m[1], m->m[2]);
  const int64_t vgrid = bop_volume_grid(V, partials != nullptr);  // (folded onto the partial sums only when some are asked for)
  MFEM_REQUIRE(vgrid < ((int64_t)1 << 31), "too many work items for one launch");
  if (V.kernel == BOP_SWEEP) {
    const auto kernel = m->ng == 2 ? k_brick_product_sweep<2> : k_brick_product_sweep<3>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)vgrid), dim3(SW_THREADS), 0, ctx->stream, B, V.L, V.items, P.k, x, dsc, y, alpha, beta, 1, dotw, partials,
                       done_flag);
  } else {
    hipLaunchKernelGGL(k_brick_product_tiles, dim3((unsigned)vgrid), dim3(TT_THREADS), 0, ctx->stream, B, op->tables, V.items, P.k, x, dsc, y, alpha, beta,
                       dotw, partials, done_flag);
  }
  MFEM_CHECK_LAUNCH();
  int np = partials ? V.grid : 0;
  if (bop_face_launch(P.k, P.h, P.robin, P.hp, P.fixed)) {
    const int64_t count = bop_boundary_count(m->m[0], m->m[1], m->m[2]);
    const int grid = bop_face_grid(count);
    hipLaunchKernelGGL(k_brick_product_faces, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, P, count, x, dsc, y, alpha, dotw,
                       partials ? partials + np : nullptr, done_flag);
    MFEM_CHECK_LAUNCH();
    if (partials) np += grid;
  }
  if (n_partials) *n_partials = np;
  return MFEM_OK;
}

static int bop_thermal_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d, bool with_sign) {
  const int64_t grid = bop_diagonal_grid(B.n_owned);
  MFEM_REQUIRE(grid < ((int64_t)1 << 31), "too many control points for one launch");
  hipLaunchKernelGGL(with_sign ? k_brick_diagonal<true> : k_brick_diagonal<false>, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, bop_thermal(op), d);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
int bop_thermal_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) { return bop_thermal_diagonal(ctx, op, B, d, false); }
int bop_thermal_signed_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) { return bop_thermal_diagonal(ctx, op, B, d, true); }
