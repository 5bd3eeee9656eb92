// Fused hex-8 assembly: geometry update + element operators + scatter in ONE pass per quantity.
// Replaces, for the constant-coefficient thermal / elasticity weak forms:
//   update_BasicElements_3D + inv_Jac_3D + update_Basic_itgval_1_3D   mesh/unstructured_mesh/4_Update_Integrator.jl:2-33,90-154
//   update_BasicBoundary_3D + tangents/normals                        :35-75,173-226
//   _Var_Basic / _Kval_Basic / _Res_Basic                             solver/06_FEM_Kernel.jl:1-13,28-45,65-79
//   the generated K_linear / K_nonlinear bodies                        solver/05_CodeGenerator.jl:52-154
// The reference stores 4 KB of physical-space basis tables per element and launches one
// thread-per-element kernel PER bilinear term with FP64 atomics into hash-ordered slots.  Here nothing
// per-element is stored: a row-owner thread (one per control point) recomputes J, det, J^-1 and the
// pushed-forward gradients of its <= 8 adjacent elements from nodal coordinates, accumulates its own
// matrix row and writes it once -- race-free without atomics or colours, CSR order, nnz*8 B written
// exactly once (the algorithmic minimum).  Thermal rows are staged in LDS and leave the CU as one
// contiguous, fully coalesced stream per workgroup.
// This file: the thermal kernels and entry points.  hex8_elasticity.hip: elasticity.  hex8_device.h: what both share on the device.
// hex8_decide.h: every host decision (knobs, kernel choice, grids) and the tile constants.
#include "hex8_device.h"
#include "hex8_sumfac.h"

// =================================================================================================
// Thermal K:  vals = sum_el sum_q w (-k) grad N_a . grad N_b  +  sum_facets sum_q w^s (-h) N_a N_b
// Row-owner with element sharing: a workgroup owns a 4 x 4 x 8 tile of control points (128 threads).
//   phase A: the 5 x 5 x 9 elements touching the tile are integrated ONCE each (one thread per element: J, det,
//            J^-1, gradients at every Gauss point -> the 36 unique entries of the symmetric 8 x 8 Ke) into LDS;
//   phase B: every control point gathers its row from the <= 8 adjacent Ke (64 statically indexed adds) and
//            writes its <= 27 CSR values once -- no atomics, no colours, nnz*8 B written exactly once.
// Geometry is evaluated 225/128 = 1.76x per element instead of 8x in the plain row-owner form.
// =================================================================================================
__device__ __forceinline__ constexpr int sym36(int a, int b) {  // upper-triangular packing of a symmetric 8 x 8
  return a <= b ? a * 8 - (a * (a - 1)) / 2 + (b - a) : b * 8 - (b * (b - 1)) / 2 + (a - b);
}

typedef H8TileOrigin TileGeom;  // first control point of the tile (global lattice ids)
__device__ __forceinline__ TileGeom tile_origin(const BrickView& B, int64_t tile) { return h8_tile_origin(tile, B.m1, B.m2, B.plo); }

__global__ __launch_bounds__(TT_THREADS) void k_thermal_matrix(BrickView B, double kcond, double* __restrict__ vals) {
  __shared__ double Ke[TT_NEL * TT_KSTRIDE];
  const int tid = threadIdx.x;
  const TileGeom T = tile_origin(B, blockIdx.x);
  // ---- phase A: one thread per element of the halo'd tile
  for (int e = tid; e < TT_NEL; e += TT_THREADS) {
    const int ek = e % TT_EK, ej = (e / TT_EK) % TT_EJ, ei = e / (TT_EK * TT_EJ);
    const int I = T.ti - 1 + ei, J = T.tj - 1 + ej, K = T.tk - 1 + ek;
    // elements needed by owned rows only: I in [plo-1, phi-1]
    if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2 || I < B.plo - 1 || I > B.phi - 1) continue;
    double X[8][3];
    hex8_load_coords(B, I, J, K, X);
    double k36[36];
#pragma unroll
    for (int t = 0; t < 36; ++t) k36[t] = 0.0;
    const int nq = B.ng * B.ng * B.ng;
    for (int q = 0; q < nq; ++q) {
      double g[8][3];
      const double c = -kcond * hex8_geom(X, q, g);
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = a; b < 8; ++b) k36[sym36(a, b)] += c * (g[a][0] * g[b][0] + g[a][1] * g[b][1] + g[a][2] * g[b][2]);
    }
#pragma unroll
    for (int t = 0; t < 36; ++t) Ke[e * TT_KSTRIDE + t] = k36[t];
  }
  __syncthreads();
  // ---- phase B: one thread per control point
  const int lk = tid % TT_NK, lj = (tid / TT_NK) % TT_NJ, li = tid / (TT_NK * TT_NJ);
  const int i = T.ti + li, j = T.tj + lj, k = T.tk + lk;
  if (i >= B.phi || j >= B.m1 || k >= B.m2) return;
  double acc[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) acc[t] = 0.0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
    const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
    if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
    const int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
    const double* ke = Ke + ((li + ex) * (TT_EJ * TT_EK) + (lj + ey) * TT_EK + (lk + ez)) * TT_KSTRIDE;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int di = ex + (b & 1), dj = ey + ((b >> 1) & 1), dk = ez + (b >> 2);  // 0..2 = neighbour offset + 1
      acc[(di * 3 + dj) * 3 + dk] += ke[sym36(a, b)];
    }
  }
  const int li0 = B.lo0[i], lj0 = B.lo1[j], lk0 = B.lo2[k];
  const int cj = B.c1[j], ck = B.c2[k];
  double* row = vals + brick_prefix(B, i, j, k);
#pragma unroll
  for (int di = 0; di < 3; ++di)
#pragma unroll
    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
      for (int dk = 0; dk < 3; ++dk) {
        const int ni = i - 1 + di, nj = j - 1 + dj, nk = k - 1 + dk;
        if (ni < 0 || ni >= B.m0 || nj < 0 || nj >= B.m1 || nk < 0 || nk >= B.m2) continue;
        row[((ni - li0) * cj + (nj - lj0)) * ck + (nk - lk0)] = acc[(di * 3 + dj) * 3 + dk];
      }
}

// Robin faces: h*Bilinear(T, Tenv - T) contributes -h N_a N_b (3D_Script.jl:31).  One thread per BOUNDARY control point, which
// read-modify-writes its OWN row (row owner => race-free), after the matrix kernel.
__global__ __launch_bounds__(MFEM_BLOCK) void k_thermal_matrix_robin(BrickView B, double h, uint32_t robin,
                                                                       double* __restrict__ vals) {
  int i, j, k;
  if (!boundary_point(B, i, j, k)) return;
  const int li = i > 0 ? i - 1 : 0, lj = j > 0 ? j - 1 : 0, lk = k > 0 ? k - 1 : 0;  // (the row box from closed forms: no table loads in front of the face loads)
  const int cj = sw1_cnt(j, B.m1), ck = sw1_cnt(k, B.m2);
  double* row = vals + sw1_prefix(B, i, j, k);
  visit_boundary_faces(B, i, j, k, robin, [&](int nd, int side, int ca, const int (&fn)[4][3], const double (&Xf)[4][3]) {
    double mab[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < B.ng * B.ng; ++q) {
      const double ws = face_geom(Xf, q, side == 0, nullptr);
      double na = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) na = (c == ca) ? c_fN[q][c] : na;
#pragma unroll
      for (int c = 0; c < 4; ++c) mab[c] += (-h * ws) * (na * c_fN[q][c]);  // N_a N_c first: entry (a, c) == entry (c, a) bitwise
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) row[((fn[c][0] - li) * cj + (fn[c][1] - lj)) * ck + (fn[c][2] - lk)] += mab[c];
  });
}

// Robin face terms of the residual at an owned control point: sum_q w^s N_a h (Tenv - T)
__device__ __forceinline__ double thermal_robin_residual(const BrickView& B, int i, int j, int k, double h, double Tenv,
                                                         uint32_t robin, const double* __restrict__ x) {
  double r = 0.0;
  const int idx[3] = {i, j, k};
  const int ne[3] = {B.ne0, B.ne1, B.ne2};
  for (int nd = 0; nd < 3; ++nd) {
    for (int side = 0; side < 2; ++side) {
      const bool on = side == 0 ? (idx[nd] == 0) : (idx[nd] == ne[nd]);
      if (!on || !(robin & face_bit(nd, side))) continue;
      const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
      for (int f = 0; f < 4; ++f) {
        const int f1 = f & 1, f2 = f >> 1;
        int E1 = idx[t1] - 1 + f1, E2 = idx[t2] - 1 + f2;
        if (E1 < 0 || E1 >= ne[t1] || E2 < 0 || E2 >= ne[t2]) continue;
        const int ca = (1 - f1) + 2 * (1 - f2);
        double Xf[4][3], Tf[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int fn[3];
          fn[nd] = idx[nd];
          fn[t1] = E1 + (c & 1);
          fn[t2] = E2 + (c >> 1);
          const int64_t ci = brick_cindex(B, fn[0], fn[1], fn[2]);
          Xf[c][0] = B.X0[ci];
          Xf[c][1] = B.X1[ci];
          Xf[c][2] = B.X2[ci];
          Tf[c] = x[brick_xindex(B, 0, fn[0], fn[1], fn[2])];
        }
        for (int q = 0; q < B.ng * B.ng; ++q) {
          const double ws = face_geom(Xf, q, side == 0, nullptr);
          double na = 0.0, Tq = 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            na = (c == ca) ? c_fN[q][c] : na;
            Tq += c_fN[q][c] * Tf[c];
          }
          r += ws * na * h * (Tenv - Tq);
        }
      }
    }
  }
  return r;
}

// the same terms as a kernel of their own over the boundary control points (after the sweep residual kernel)
__global__ __launch_bounds__(MFEM_BLOCK) void k_thermal_residual_robin(BrickView B, double h, double Tenv, uint32_t robin,
                                                                         const double* __restrict__ x, double* __restrict__ res) {
  int i, j, k;
  if (!boundary_point(B, i, j, k)) return;
  res[(int64_t)(i - B.plo) * B.plane_len + (int64_t)j * B.m2 + k] += thermal_robin_residual(B, i, j, k, h, Tenv, robin, x);
}

// =================================================================================================
// Thermal residual (matrix-free, at x_star):
//   R[a] = sum_q w (-k grad N_a . grad T + N_a s) + sum_q w^s N_a h (Tenv - T)
// Same tiling as k_thermal_matrix: the element load vectors fe[8] of the 5 x 5 x 9 elements touching a 4 x 4 x 8
// tile of control points are integrated once each into LDS, then every control point sums its <= 8 entries and adds
// its own Robin face terms.
// =================================================================================================
__global__ __launch_bounds__(TT_THREADS) void k_thermal_residual(BrickView B, double kcond, double h, double Tenv,
                                                                   uint32_t robin, const double* __restrict__ x,
                                                                   const double* __restrict__ src,
                                                                   double* __restrict__ res) {
  __shared__ double Fe[TT_NEL * 9];
  const int tid = threadIdx.x;
  const TileGeom T = tile_origin(B, blockIdx.x);
  for (int e = tid; e < TT_NEL; e += TT_THREADS) {
    const int ek = e % TT_EK, ej = (e / TT_EK) % TT_EJ, ei = e / (TT_EK * TT_EJ);
    const int I = T.ti - 1 + ei, J = T.tj - 1 + ej, K = T.tk - 1 + ek;
    if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2 || I < B.plo - 1 || I > B.phi - 1) continue;
    double X[8][3], Tn[8], Sn[8], fe[8];
    hex8_load_coords(B, I, J, K, X);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int64_t xi = brick_xindex(B, 0, I + (b & 1), J + ((b >> 1) & 1), K + (b >> 2));
      Tn[b] = x[xi];
      Sn[b] = src ? src[xi] : 0.0;
      fe[b] = 0.0;
    }
    const int nq = B.ng * B.ng * B.ng;
    for (int q = 0; q < nq; ++q) {
      double g[8][3];
      const double wd = hex8_geom(X, q, g);
      double gT0 = 0.0, gT1 = 0.0, gT2 = 0.0, sq = 0.0;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        gT0 += g[b][0] * Tn[b];
        gT1 += g[b][1] * Tn[b];
        gT2 += g[b][2] * Tn[b];
        sq += c_N[q][b] * Sn[b];
      }
      const double c = -kcond * wd;
#pragma unroll
      for (int a = 0; a < 8; ++a) fe[a] += c * (g[a][0] * gT0 + g[a][1] * gT1 + g[a][2] * gT2) + wd * c_N[q][a] * sq;
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) Fe[e * 9 + a] = fe[a];
  }
  __syncthreads();
  const int lk = tid % TT_NK, lj = (tid / TT_NK) % TT_NJ, li = tid / (TT_NK * TT_NJ);
  const int i = T.ti + li, j = T.tj + lj, k = T.tk + lk;
  if (i >= B.phi || j >= B.m1 || k >= B.m2) return;
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
  if (h != 0.0 && robin != 0u) r += thermal_robin_residual(B, i, j, k, h, Tenv, robin, x);
  res[node] = r;
}


// =================================================================================================
// Sweep form of the two thermal kernels (default for 2- and 3-point Gauss rules).
// A workgroup of 256 threads owns a 15 x 15 tile of control points in (j, k) and sweeps it through a segment of lattice
// planes along i.  Per element plane I (the elements between node planes I and I + 1):
//   phase A  thread <-> element of the 16 x 16 element tile: the element's upper four nodes are loaded (the lower four are
//            last step's upper ones, kept in registers), the element is integrated with the sum-factorised routines of
//            hex8_sumfac.h and its fe[8] / 36 unique Ke entries go to LDS;
//   phase B  thread <-> control point: the point of node plane I adds the four elements above it to what it carried over
//            from the four elements below (element plane I - 1) and writes its residual entry / its <= 27 CSR values once;
//            the same four elements' contributions to the point above it (node plane I + 1) become the next carry.
// Element evaluations per control point: 256 / 225 x (L + 1) / L = 1.17 (L = 32 planes per segment) against 1.76 for the
// 4 x 4 x 8 tiles, each at ~40 % of the table form's arithmetic.  Row-owner as before: no atomics, no colours, every value
// written once; the sums over the shared elements of a mirrored pair of entries run in the same order, so the matrix stays
// bitwise symmetric (the symmetric-sweep SpMV depends on that).
// =================================================================================================
template <int NG>
__global__ __launch_bounds__(SW_THREADS) __attribute__((amdgpu_waves_per_eu(NG == 2 ? 2 : 1))) void k_thermal_residual_sweep(BrickView B, int L, double kcond, const double* __restrict__ x,
                                                                         const double* __restrict__ src,
                                                                         double* __restrict__ res, int affine_fast) {
  __shared__ double Fe[SW_THREADS * 9];
  const int tid = threadIdx.x, ek = tid % SW_E, ej = tid / SW_E;
  const SweepTile T = sweep_tile(B, L);
  if (T.i0 >= T.i1) return;
  const int J = T.tj0 - 1 + ej, K = T.tk0 - 1 + ek;  // phase A: this thread's element column
  const bool el_ok = J >= 0 && J < B.ne1 && K >= 0 && K < B.ne2;
  const int j = T.tj0 + ej, k = T.tk0 + ek;          // phase B: this thread's control point column
  const bool nd_ok = ej < SW_N && ek < SW_N && j < B.m1 && k < B.m2;
  const bool has_src = src != nullptr;
  // nodal data of lattice plane ip at the element's four (j, k) corners
  double Xn[3][4], Tq[4], Sq[4];  // the plane requested last (consumed at the top of the next step)
#pragma unroll
  for (int c = 0; c < 4; ++c) Sq[c] = 0.0;
  const int Jc = min(max(J, 0), B.ne1 - 1), Kc = min(max(K, 0), B.ne2 - 1);  // (threads without an element column load what a neighbour loads)
  // (every thread requests on every step, from clamped positions: behind a condition the requested registers meet their old values in a phi, and the copies that resolves into wait for the loads AT ONCE -- the prefetch then costs a memory round trip per plane instead of hiding one: round 5, found in the ISA)
  auto request = [&](int ip) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t ci = brick_cindex(B, ip, Jc + (c & 1), Kc + (c >> 1));
      Xn[0][c] = B.X0[ci];
      Xn[1][c] = B.X1[ci];
      Xn[2][c] = B.X2[ci];
      const int64_t xi = brick_xindex(B, 0, ip, Jc + (c & 1), Kc + (c >> 1));
      Tq[c] = x[xi];
      if (has_src) Sq[c] = src[xi];
    }
  };
  double X[3][2][4], Tn[2][4], Sn[2][4];
  const int Ifirst = max(T.i0 - 1, 0), Ilast = min(T.i1 - 1, B.ne0 - 1);  // element planes of this segment
  {
    request(Ifirst);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      X[0][1][c] = Xn[0][c]; X[1][1][c] = Xn[1][c]; X[2][1][c] = Xn[2][c];
      Tn[1][c] = Tq[c]; Sn[1][c] = Sq[c];
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
        Tn[0][c] = Tn[1][c]; Sn[0][c] = Sn[1][c];
        X[0][1][c] = Xn[0][c]; X[1][1][c] = Xn[1][c]; X[2][1][c] = Xn[2][c];
        Tn[1][c] = Tq[c]; Sn[1][c] = Sq[c];
      }
      double fe[2][4];
      if (affine_fast && sf_is_affine(X)) sf_thermal_fe<NG, true>(X, Tn, Sn, has_src, kcond, fe);  // (one adjugate for a parallelepiped: see k_thermal_matrix_sweep)
      else sf_thermal_fe<NG, false>(X, Tn, Sn, has_src, kcond, fe);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        Fe[tid * 9 + 2 * c] = fe[0][c];
        Fe[tid * 9 + 2 * c + 1] = fe[1][c];
      }
    }
    request(min(max(I + 2, Ifirst), Ilast + 1));  // in flight during the rest of this plane's step: gather, write-out, barriers (mfem_lds_barrier does not wait for it)
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
      if (I >= T.i0) res[(int64_t)(I - B.plo) * B.plane_len + (int64_t)j * B.m2 + k] = carry + lo;
      carry = up;
    }
    mfem_lds_barrier();
  }
}

// The matrix sweep on its own, smaller tile (round 6): 8 x 16 elements, 128 threads, 38 KB of LDS -- FOUR workgroups per CU instead of two (the waves per
// CU stay 8: 250 VGPRs), so that the load / integrate / gather / write-out phases of more independent workgroups overlap (ablation: the phases of two did not).
template <int NG>
__global__ __launch_bounds__(MS_THREADS) __attribute__((amdgpu_waves_per_eu(NG == 2 ? 2 : 1))) void k_thermal_matrix_sweep(BrickView B, int L, double kcond, double* __restrict__ vals, int stage_rows) {
  __shared__ double Ke[MS_THREADS * SW_KSTRIDE];
  const int tid = threadIdx.x, ek = tid % MS_EK, ej = tid / MS_EK;
  const SweepTile T = sweep_tile_m(B, L);
  if (T.i0 >= T.i1) return;
  const int J = T.tj0 - 1 + ej, K = T.tk0 - 1 + ek;
  const bool el_ok = J >= 0 && J < B.ne1 && K >= 0 && K < B.ne2;
  const int j = T.tj0 + ej, k = T.tk0 + ek;
  const bool nd_ok = ej < MS_NJ && ek < MS_NK && j < B.m1 && k < B.m2;
  int lj0 = 0, lk0 = 0, cj = 1, ck = 1;
  if (nd_ok) {
    lj0 = B.lo1[j];
    lk0 = B.lo2[k];
    cj = B.c1[j];
    ck = B.c2[k];
  }
  const bool jk_inner = nd_ok && j > 0 && j < B.ne1 && k > 0 && k < B.ne2;  // all nine in-plane neighbours exist
  const bool staged = (stage_rows & 1) != 0;  // (kernel argument, uniform: the per-thread write-out is kept behind bit 1 of the "hex8_thermal" knob; the flag word: h8_thermal_stage_rows)
  double Xn[3][4];
  const int Jc = min(max(J, 0), B.ne1 - 1), Kc = min(max(K, 0), B.ne2 - 1);  // (threads without an element column load what a neighbour loads)
  // (every thread requests on every step, from clamped positions: behind a condition the requested registers meet their old values in a phi, and the copies that resolves into wait for the loads AT ONCE -- the prefetch then costs a memory round trip per plane instead of hiding one: round 5, found in the ISA)
  auto request = [&](int ip) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t ci = brick_cindex(B, ip, Jc + (c & 1), Kc + (c >> 1));
      Xn[0][c] = B.X0[ci];
      Xn[1][c] = B.X1[ci];
      Xn[2][c] = B.X2[ci];
    }
  };
  double X[3][2][4];
  const int Ifirst = max(T.i0 - 1, 0), Ilast = min(T.i1 - 1, B.ne0 - 1);
  {
    request(Ifirst);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      X[0][1][c] = Xn[0][c]; X[1][1][c] = Xn[1][c]; X[2][1][c] = Xn[2][c];
    }
    request(Ifirst + 1);
  }
  double carry[18];
#pragma unroll
  for (int t = 0; t < 18; ++t) carry[t] = 0.0;
  for (int I = T.i0 - 1; I < T.i1; ++I) {
    const bool plane = I >= 0 && I < B.ne0;
    if (plane && el_ok) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        X[0][0][c] = X[0][1][c]; X[1][0][c] = X[1][1][c]; X[2][0][c] = X[2][1][c];
        X[0][1][c] = Xn[0][c]; X[1][1][c] = Xn[1][c]; X[2][1][c] = Xn[2][c];
      }
      double k36[36];
      // affine elements (unless bit 2 of the "hex8_thermal" knob is set): one adjugate instead of NG^3 -- the FP64 work is what this kernel's time follows (a table of
      // reference integrals, ke = sum_t g0[t] K6[t], was measured too: 216 constant loads per element made the kernel 1.7x SLOWER)
      if (stage_rows & 4) {
#pragma unroll
        for (int t = 0; t < 36; ++t) k36[t] = 0.0;
      } else if ((stage_rows & 2) && sf_is_affine(X)) sf_thermal_ke<NG, true>(X, kcond, k36);
      else sf_thermal_ke<NG, false>(X, kcond, k36);
#pragma unroll
      for (int t = 0; t < 36; ++t) Ke[tid * SW_KSTRIDE + t] = k36[t];
    }
    request(min(max(I + 2, Ifirst), Ilast + 1));  // in flight during the rest of this plane's step: gather, write-out, barriers (mfem_lds_barrier does not wait for it)
    mfem_lds_barrier();
    // now[bx * 9 + dj * 3 + dk]: entries of this plane's point towards node plane I + bx; up[...]: entries of the point above it
    // (node plane I + 1) towards node plane I + bx
    double now[18], up[18];
#pragma unroll
    for (int t = 0; t < 18; ++t) now[t] = up[t] = 0.0;
    if (nd_ok && plane && !(stage_rows & 8)) {
#pragma unroll
      for (int ez = 0; ez < 2; ++ez)
#pragma unroll
        for (int ey = 0; ey < 2; ++ey) {
          const int Jn = j - 1 + ey, Kn = k - 1 + ez;
          if (Jn < 0 || Jn >= B.ne1 || Kn < 0 || Kn >= B.ne2) continue;
          const double* ke = Ke + ((ej + ey) * MS_EK + ek + ez) * SW_KSTRIDE;
          const int a0 = 2 * (1 - ey) + 4 * (1 - ez);
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const int slot = (b & 1) * 9 + (ey + ((b >> 1) & 1)) * 3 + ez + (b >> 2);
            now[slot] += ke[sym36(a0, b)];
            up[slot] += ke[sym36(a0 + 1, b)];
          }
        }
    }
    // Write-out.  A point away from the lattice boundary has its full 27-entry row, one contiguous run in (di, dj, dk) order -- and the rows of the
    // points of one tile line are contiguous in CSR too.  Writing row[t] per thread puts 64 lanes 216 bytes apart: 27 x 64 eight-byte requests per
    // wave and plane, and at 4.6e8 requests per assembly (256^3) the L2's request rate, not its bytes, set the kernel's time (round 4).  The rows now go
    // through LDS (the element matrices of this plane are dead once every point has gathered them) and leave as contiguous streams: a wave per tile line.
    // (Every barrier below is reached by ALL threads of the workgroup: `staged` is a kernel argument, nothing here sits inside a per-thread branch.)
    const bool full_row = nd_ok && jk_inner && I > 0 && I < B.ne0 && I >= T.i0;
    if (staged) {
      mfem_lds_barrier();  // every point has gathered from Ke
      if (full_row) {
        double* st = Ke + tid * 27;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          st[t] = carry[t];
          st[9 + t] = carry[9 + t] + now[t];
          st[18 + t] = now[9 + t];
        }
      }
    }
    if (nd_ok) {
      if (I >= T.i0 && !(staged && full_row)) {
        double* row = vals + brick_prefix(B, I, j, k);
        if (jk_inner && I > 0 && I < B.ne0) {  // the full 27-entry row is one contiguous run in (di, dj, dk) order
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            row[t] = carry[t];
            row[9 + t] = carry[9 + t] + now[t];
            row[18 + t] = now[9 + t];
          }
        } else {
          const int li0 = B.lo0[I];
#pragma unroll
          for (int di = 0; di < 3; ++di)
#pragma unroll
            for (int dj = 0; dj < 3; ++dj)
#pragma unroll
              for (int dk = 0; dk < 3; ++dk) {
                const int ni = I - 1 + di, nj = j - 1 + dj, nk = k - 1 + dk;
                if (ni < 0 || ni >= B.m0 || nj < 0 || nj >= B.m1 || nk < 0 || nk >= B.m2) continue;
                const int t = dj * 3 + dk;
                const double v = di == 0 ? carry[t] : di == 1 ? carry[9 + t] + now[t] : now[9 + t];
                row[((ni - li0) * cj + (nj - lj0)) * ck + (nk - lk0)] = v;
              }
        }
      }
#pragma unroll
      for (int t = 0; t < 18; ++t) carry[t] = up[t];
    }
    if (staged) {
      mfem_lds_barrier();  // the staged rows are complete
      if (I >= T.i0 && I > 0 && I < B.ne0) {
        const int k0 = max(T.tk0, 1), k1 = min(min(T.tk0 + MS_NK, B.ne2), B.m2);  // points of a tile line with a full row: k in [k0, k1)
        const int cnt = (k1 - k0) * 27;
        for (int line = tid >> 6; line < MS_NJ; line += MS_THREADS / 64) {
          const int jl = T.tj0 + line;
          if (jl < 1 || jl >= B.ne1 || jl >= B.m1 || cnt <= 0 || (stage_rows & 16)) continue;
          double* dst = vals + sw1_prefix(B, I, jl, k0);
          const double* src = Ke + (line * MS_EK + (k0 - T.tk0)) * 27;
          // 16 bytes per lane from the destination's first 16-byte boundary on (round 6: a wave's store instruction covers 1 KB of the run instead of 512 bytes)
          const int head = (int)(((uintptr_t)dst >> 3) & 1), np = (cnt - head) >> 1, ln = tid & 63;
          typedef double sw_d2 __attribute__((ext_vector_type(2)));
          for (int m = ln; m < np; m += 64) {
            const int idx = head + 2 * m;
            __builtin_nontemporal_store(sw_d2{src[idx], src[idx + 1]}, reinterpret_cast<sw_d2*>(dst + idx));
          }
          if (ln == 0 && head) __builtin_nontemporal_store(src[0], dst);
          if (ln == 1 && ((cnt - head) & 1)) __builtin_nontemporal_store(src[cnt - 1], dst + cnt - 1);
        }
      }
    }
    mfem_lds_barrier();
  }
}

// ---- host: knobs, the sweeps' instantiations, entry points (every decision: hex8_decide.h) -----------------------------------------------------------
static std::atomic<H8ThermalKnobs> g_thermal_knobs{h8_thermal_knobs(0)};
static_assert(std::atomic<H8ThermalKnobs>::is_always_lock_free, "the knobs are read and set without a lock");
extern "C" int mfem_debug_set_hex8_thermal(int variant) try {
  ++mfem_debug_epoch;
  g_thermal_knobs = h8_thermal_knobs(variant);
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_hex8_thermal")

static void launch_matrix_sweep(mfem_context_s* ctx, const BrickView& B, int ng, const H8Sweep& S, double kcond, double* vals, int stage_rows) {
  const auto kernel = ng == 2 ? k_thermal_matrix_sweep<2> : k_thermal_matrix_sweep<3>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)S.grid), dim3(MS_THREADS), 0, ctx->stream, B, S.L, kcond, vals, stage_rows);
}
static void launch_residual_sweep(mfem_context_s* ctx, const BrickView& B, int ng, const H8Sweep& S, double kcond, const double* x, const double* src,
                                  double* res, int affine_fast) {
  const auto kernel = ng == 2 ? k_thermal_residual_sweep<2> : k_thermal_residual_sweep<3>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)S.grid), dim3(SW_THREADS), 0, ctx->stream, B, S.L, kcond, x, src, res, affine_fast);
}

int mfem_hex27_assemble_thermal(mfem_context_s* ctx, mfem_brick_s* m, mfem_csr_s* A, const mfem_thermal_params* p, double* vals);
int mfem_hex27_residual_thermal(mfem_context_s* ctx, mfem_brick_s* m, const mfem_thermal_params* p, const double* x_star, const double* s,
                                double* residue);
int mfem_brick_nitsche_faces(mfem_context_s* ctx, mfem_brick_s* m, bool matrix, const mfem_thermal_params* p, const double* xstar, double* out);

extern "C" int mfem_brick_assemble_thermal(mfem_context ctx, mfem_brick m, mfem_csr A, const mfem_thermal_params* p,
                                           double* vals) try {
  MFEM_REQUIRE(ctx && m && A && p && vals, "null argument");
  MFEM_REQUIRE(A->n == m->n_owned, "pattern was not built for 1 field on this brick");
  if (m->p == 2) {  // FP64 MFMA Ke = B^T D B path
    const int rc27 = mfem_hex27_assemble_thermal(ctx, m, A, p, vals);
    return rc27 ? rc27 : mfem_brick_nitsche_faces(ctx, m, true, p, nullptr, vals);
  }
  int rc = mfem_hex8_upload_tables(m->ng);
  if (rc) return rc;
  BrickView B = mfem_brick_view(m, 1);
  const H8ThermalKnobs K = g_thermal_knobs.load();
  if (h8_thermal_kernel(K, m->ng) == H8_THERMAL_SWEEP)
    launch_matrix_sweep(ctx, B, m->ng, h8_matrix_sweep(m->m[1], m->m[2], m->phi - m->plo), p->k, vals, h8_thermal_stage_rows(K));
  else
    hipLaunchKernelGGL(k_thermal_matrix, dim3((unsigned)h8_tile_grid(m->phi - m->plo, m->m[1], m->m[2])), dim3(TT_THREADS), 0, ctx->stream, B, p->k, vals);
  MFEM_CHECK_LAUNCH();
  if (h8_robin_launch(p->h, p->robin_faces)) {
    hipLaunchKernelGGL(k_thermal_matrix_robin, boundary_grid(m), dim3(MFEM_BLOCK), 0, ctx->stream, B, p->h, p->robin_faces, vals);
    MFEM_CHECK_LAUNCH();
  }
  return mfem_brick_nitsche_faces(ctx, m, true, p, nullptr, vals);
} MFEM_API_CATCH("mfem_brick_assemble_thermal")

extern "C" int mfem_brick_residual_thermal(mfem_context ctx, mfem_brick m, const mfem_thermal_params* p,
                                           const double* x_star, const double* s, double* residue) try {
  MFEM_REQUIRE(ctx && m && p && x_star && residue, "null argument");
  if (m->p == 2) {
    const int rc27 = mfem_hex27_residual_thermal(ctx, m, p, x_star, s, residue);
    return rc27 ? rc27 : mfem_brick_nitsche_faces(ctx, m, false, p, x_star, residue);
  }
  int rc = mfem_hex8_upload_tables(m->ng);
  if (rc) return rc;
  BrickView B = mfem_brick_view(m, 1);
  const H8ThermalKnobs K = g_thermal_knobs.load();
  if (h8_thermal_kernel(K, m->ng) == H8_THERMAL_SWEEP) {  // the sweep leaves the Robin terms to a kernel over the boundary control points
    launch_residual_sweep(ctx, B, m->ng, h8_residual_sweep(m->m[1], m->m[2], m->phi - m->plo), p->k, x_star, s, residue, h8_thermal_affine_fast(K));
    if (h8_robin_launch(p->h, p->robin_faces)) {
      MFEM_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_thermal_residual_robin, boundary_grid(m), dim3(MFEM_BLOCK), 0, ctx->stream, B, p->h, p->Tenv, p->robin_faces,
                         x_star, residue);
    }
  } else {
    hipLaunchKernelGGL(k_thermal_residual, dim3((unsigned)h8_tile_grid(m->phi - m->plo, m->m[1], m->m[2])), dim3(TT_THREADS), 0, ctx->stream, B, p->k, p->h,
                       p->Tenv, p->robin_faces, x_star, s, residue);
  }
  MFEM_CHECK_LAUNCH();
  return mfem_brick_nitsche_faces(ctx, m, false, p, x_star, residue);
} MFEM_API_CATCH("mfem_brick_residual_thermal")

