// The SIGNED diagonal of the matrix-free hex-27 thermal brick operator as a plane sweep: d_i = K_ii for the K of brick_operator_hex27.hip -- what the
// multigrid setup reads the sign of K and the smoother's D from (bop_signed_diagonal).  mfem_brick_operator_diagonal and Pr_Jacobi_ keep
// k_brick27_diagonal (|K_ii|, a thread per control point) in brick_operator_hex27.hip, which this file leaves alone: the product's register allocation is
// sensitive to what shares its translation unit.
//   volume  k_brick27_diagonal_sweep: the product's skeleton (brick_operator_hex27_decide.h: b27_volume, b27_item, the 8 x 8 column tile, segments of
//           <= 32 element planes, the low-side halo).  A wave integrates an element: the geometry stage is the product's (sum-factorised J at the
//           Gauss points, the affine shortcut, the next element's nodes prefetched; no T component), then, in place of the two apply stages,
//           Ke_aa = sum_q sum_(d <= e) H_de(q) dN_a/dxi_d dN_a/dxi_e with H_de = (-k w det)(2 - [d == e]) (Jinv Jinv^T)_de: per pair (d, e) the factor
//           of direction r is a 3 x ng table of products of 1-D values (l^2, l l', l'^2), so the sum over q runs in three short stages over q2, q1
//           and q0, spread over the 64 lanes.  The 27 entries go to the workgroup's LDS block; after the plane's barrier the owner of a
//           control-point column adds the <= 4 that meet in it in a fixed order and writes the two finished planes, carrying the third.  Every
//           control point is written once -- a zero diagonal as 0: no atomics, no memset, the same bits on every run.
//   faces   k_brick27_diagonal_faces: a thread per boundary control point adds its own Robin and Nitsche entries K^face_aa (the terms of
//           b27_face_row<true, true> of brick_operator_hex27.hip, restated here for the diagonal alone).
#include "hex8_device.h"
#include "hex27.h"
#include "brick_operator.h"
#include "brick_operator_hex27_decide.h"

struct Bop27Diag {
  double k, h, hp;
  uint32_t robin, fixed;
  int ng;
  double gp[4], gw[4];  // 1-D Gauss points / weights on [0, 1]
  const Hex27Tables* T;
};

#define D_X 0
#define D_T1 (27 * NI)
#define D_J 0
#define D_T2 b27_w_t2(ng)
#define D_H D_T2
#define D_VA 0
#define D_WB b27d_w_wb(ng)
#define D_D b27_w_d(ng)

// __launch_bounds__(B27_THREADS, 4): two workgroups of 8 waves fit a CU (<= 128 VGPRs per lane), the product's rule.
__global__ __launch_bounds__(B27_THREADS, 4) void k_brick27_diagonal_sweep(BrickView B, const Hex27Tables* __restrict__ tab, B27Volume V, double kcond,
                                                                            double* __restrict__ dg, int affine_fast) {
  extern __shared__ double lds[];
  constexpr int NI = B27_NI;
  const int ng = B.ng, nq = ng * ng * ng, ngg = ng * ng;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* s_w = lds;
  double* s_tab1 = lds + b27d_off_tab1(ng);
  double* s_tabp = lds + b27d_off_tabp(ng);
  int32_t* s_dec = reinterpret_cast<int32_t*>(lds + b27d_off_dec(ng));
  double* Fe = lds + b27d_off_fe(ng);
  double* W = lds + b27d_off_waves(ng) + (size_t)wv * b27_w_size(ng);
  const int n1 = b27_n1(ng), n2 = b27_n2(ng), n3 = b27d_n3(ng), nA = b27d_na(ng), nB = b27d_nb(ng);
  for (int i = tid; i < nq; i += B27_THREADS) s_w[i] = tab->w[i];
  for (int i = tid; i < 8 * ng; i += B27_THREADS) s_tab1[i] = tab->tab1[i / (4 * ng)][(i >> 2) % ng][i & 3];
  for (int i = tid; i < 12 * ng; i += B27_THREADS) {  // tabp[kind][q][a]: l^2, l l', l'^2
    const int a = i & 3, q = (i >> 2) % ng, kind = i / (4 * ng);
    const double l = tab->tab1[0][q][a], dl = tab->tab1[1][q][a];
    s_tabp[i] = kind == 0 ? l * l : (kind == 1 ? l * dl : dl * dl);
  }
  // decode words of the geometry stages: the product's (k_brick27_product), word for word
  for (int t = tid; t < n1; t += B27_THREADS) {
    const int i = t % NI, a12 = (t / NI) % 9, kq = t / (9 * NI);
    s_dec[t] = (3 * a12 * NI + i) | ((4 * kq) << 16);
  }
  for (int t = tid; t < n2; t += B27_THREADS) {
    const int i = t % NI, a2 = (t / NI) % 3, q1 = (t / (3 * NI)) % ng, q0 = (t / (3 * NI * ng)) % ng, kk = t / (3 * NI * ng * ng);
    const int k = kk == 0 ? 1 : 0, kt = kk == 1 ? 1 : 0;
    s_dec[n1 + t] = (((k * ng + q0) * 9 + 3 * a2) * NI + i) | ((4 * (kt * ng + q1)) << 16);
  }
  for (int t = tid; t < n3; t += B27_THREADS) {  // J[q][i][m]
    const int m = t % 3, i = (t / 3) % 3, q = t / 9;
    const int q0 = q % ng, q1 = (q / ng) % ng, q2 = q / (ng * ng);
    const int kt = m == 2 ? 1 : 0;
    s_dec[n1 + n2 + t] = ((((m * ng + q0) * ng + q1) * 3) * NI + i) | ((4 * (kt * ng + q2)) << 16);
  }
  // the diagonal's stages: low 12 bits = offset of the first operand, bits 12-13 = the node index along the direction summed, bits 14-15 = the
  // factor's kind along it
  for (int t = tid; t < nA; t += B27_THREADS) {  // VA[p][q0][q1][a2] = sum_q2 tabp[kind_2(p)][q2][a2] H[p][q0 + ng q1 + ng^2 q2]
    const int a2 = t % 3, q1 = (t / 3) % ng, q0 = (t / (3 * ng)) % ng, p = t / (3 * ng * ng);
    s_dec[n1 + n2 + n3 + t] = (p * nq + q0 + ng * q1) | (a2 << 12) | (b27d_kind(p, 2) << 14);
  }
  for (int t = tid; t < nB; t += B27_THREADS) {  // WB[p][q0][a1 + 3 a2] = sum_q1 tabp[kind_1(p)][q1][a1] VA[p][q0][q1][a2]
    const int a12 = t % 9, a1 = a12 % 3, a2 = a12 / 3, q0 = (t / 9) % ng, p = t / (9 * ng);
    s_dec[n1 + n2 + n3 + nA + t] = (((p * ng + q0) * ng) * 3 + a2) | (a1 << 12) | (b27d_kind(p, 1) << 14);
  }
  __syncthreads();
  const int oA = n1 + n2 + n3, oB = oA + nA;

  struct NodePre {
    double x0, x1, x2;
  };
  const int ln = lane < 27 ? lane : 26;
  const int64_t lane_off = (int64_t)(ln % 3) * B.plane_len + (int64_t)((ln / 3) % 3) * B.m2 + ln / 9;
  auto fetch_nodes = [&](int I, int J, int K) -> NodePre {
    NodePre n;
    const int64_t c = ((int64_t)(2 * I) * B.plane_len + (int64_t)(2 * J) * B.m2 + 2 * K) + lane_off;
    n.x0 = B.X0[c];
    n.x1 = B.X1[c];
    n.x2 = B.X2[c];
    return n;
  };

  for (int64_t w = blockIdx.x; w < V.items; w += gridDim.x) {  // (workgroup-uniform)
    const B27Item it = b27_item(V, w, B.ne0, B.ne1, B.ne2);
    const int nEK = it.K1 - it.K0;
    // phase B: this thread's control-point column
    const int lj = tid / B27_NP, lk = tid % B27_NP;
    const int j = it.j0 + lj, k = it.k0 + lk;
    const bool nd_ok = tid < B27_NP * B27_NP && j < it.j1 && k < it.k1;
    int Ej[2], cj[2], Ek[2], ck[2];
    const int nj = b27_face_elements(nd_ok ? j : 0, B.ne1, Ej, cj), nk = b27_face_elements(nd_ok ? k : 0, B.ne2, Ek, ck);
    double carry = 0.0;
    // phase A: the wave's walk over (plane, element column), B27_WAVES columns apart; it always holds the node data of its next element
    const int nEJ = it.J1 - it.J0;
    int ej0 = 0, ek0 = wv;
    while (ek0 >= nEK && ej0 < nEJ) { ek0 -= nEK; ++ej0; }
    const bool wave_has = ej0 < nEJ;
    NodePre cur = fetch_nodes(it.I0, it.J0 + (wave_has ? ej0 : 0), it.K0 + (wave_has ? ek0 : 0));
    for (int I = it.I0; I < it.I1; ++I) {
      for (int ej = ej0, ek = ek0; ej < nEJ;) {
        const int J = it.J0 + ej, K = it.K0 + ek;
        // ---- 1. nodes
        if (lane < 27) {
          W[D_X + NI * lane + 0] = cur.x0;
          W[D_X + NI * lane + 1] = cur.x1;
          W[D_X + NI * lane + 2] = cur.x2;
        }
        {  // the next element of this wave: its loads are in flight during this element's stages
          ek += B27_WAVES;
          while (ek >= nEK && ej < nEJ) { ek -= nEK; ++ej; }
          const bool more = ej < nEJ;
          const int In = more ? I : (I + 1 < it.I1 ? I + 1 : I);
          cur = fetch_nodes(In, it.J0 + (more ? ej : ej0), it.K0 + (more ? ek : ek0));
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 2'. affine elements: J is one matrix (the product's test, word for word)
        bool affine = false;
        if (affine_fast) {
          const double x0 = W[D_X + 0], y0 = W[D_X + 1], z0 = W[D_X + 2];
          const double ex0 = W[D_X + NI * 2 + 0] - x0, ey0 = W[D_X + NI * 2 + 1] - y0, ez0 = W[D_X + NI * 2 + 2] - z0;
          const double ex1 = W[D_X + NI * 6 + 0] - x0, ey1 = W[D_X + NI * 6 + 1] - y0, ez1 = W[D_X + NI * 6 + 2] - z0;
          const double ex2 = W[D_X + NI * 18 + 0] - x0, ey2 = W[D_X + NI * 18 + 1] - y0, ez2 = W[D_X + NI * 18 + 2] - z0;
          bool mine = true;
          if (lane < 27) {
            const double a0 = 0.5 * (lane % 3), a1 = 0.5 * ((lane / 3) % 3), a2 = 0.5 * (lane / 9);
            const double px = x0 + a0 * ex0 + a1 * ex1 + a2 * ex2, py = y0 + a0 * ey0 + a1 * ey1 + a2 * ey2, pz = z0 + a0 * ez0 + a1 * ez1 + a2 * ez2;
            const double mx = W[D_X + NI * lane + 0], my = W[D_X + NI * lane + 1], mz = W[D_X + NI * lane + 2];
            const double tol = 3.6e-15;
            mine = fabs(mx - px) <= tol * (fabs(x0) + fabs(ex0) + fabs(ex1) + fabs(ex2)) &&
                   fabs(my - py) <= tol * (fabs(y0) + fabs(ey0) + fabs(ey1) + fabs(ey2)) &&
                   fabs(mz - pz) <= tol * (fabs(z0) + fabs(ez0) + fabs(ez1) + fabs(ez2));
          }
          affine = __all(mine);
          if (affine) {
            const double j00 = ex0, j01 = ex1, j02 = ex2, j10 = ey0, j11 = ey1, j12 = ey2, j20 = ez0, j21 = ez1, j22 = ez2;
            const double det = j00 * j11 * j22 - j00 * j12 * j21 - j01 * j10 * j22 + j01 * j12 * j20 + j02 * j10 * j21 - j02 * j11 * j20;
            const double id = 1.0 / det;
            const double i0 = (j11 * j22 - j12 * j21) * id, i1 = (j02 * j21 - j01 * j22) * id, i2 = (j01 * j12 - j11 * j02) * id;
            const double i3 = (j12 * j20 - j22 * j10) * id, i4 = (j00 * j22 - j02 * j20) * id, i5 = (j02 * j10 - j00 * j12) * id;
            const double i6 = (j10 * j21 - j11 * j20) * id, i7 = (j01 * j20 - j21 * j00) * id, i8 = (j00 * j11 - j10 * j01) * id;
            __builtin_amdgcn_wave_barrier();  // (every lane has read X: J goes over it)
            for (int q = lane; q < nq; q += 64) {
              double* Jm = W + D_J + q * 9;
              Jm[0] = i0; Jm[1] = i1; Jm[2] = i2; Jm[3] = i3; Jm[4] = i4; Jm[5] = i5; Jm[6] = i6; Jm[7] = i7; Jm[8] = i8;
              W[D_D + q] = s_w[q] * det;
            }
          }
        }
        if (!affine) {
          // ---- 2a. J at the Gauss points, sum-factorised (the three coordinate components of the product's stages)
          for (int u = lane; u < (n1 / NI) * 3; u += 64) {
            const int t = (u / 3) * NI + u % 3;
            const int d = s_dec[t];
            const double* xs = W + D_X + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[D_T1 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          for (int u = lane; u < (n2 / NI) * 3; u += 64) {
            const int t = (u / 3) * NI + u % 3;
            const int d = s_dec[n1 + t];
            const double* xs = W + D_T1 + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[D_T2 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          for (int t = lane; t < n3; t += 64) {
            const int d = s_dec[n1 + n2 + t];
            const double* xs = W + D_T2 + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[D_J + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          // ---- 2b. det, inverse (adjugate), w det; Jinv overwrites J as [m][s]
          for (int q = lane; q < nq; q += 64) {
            double* Jm = W + D_J + q * 9;
            const double j00 = Jm[0], j01 = Jm[1], j02 = Jm[2], j10 = Jm[3], j11 = Jm[4], j12 = Jm[5], j20 = Jm[6], j21 = Jm[7], j22 = Jm[8];
            const double det = j00 * j11 * j22 - j00 * j12 * j21 - j01 * j10 * j22 + j01 * j12 * j20 + j02 * j10 * j21 - j02 * j11 * j20;
            const double id = 1.0 / det;
            Jm[0] = (j11 * j22 - j12 * j21) * id;
            Jm[1] = (j02 * j21 - j01 * j22) * id;
            Jm[2] = (j01 * j12 - j11 * j02) * id;
            Jm[3] = (j12 * j20 - j22 * j10) * id;
            Jm[4] = (j00 * j22 - j02 * j20) * id;
            Jm[5] = (j02 * j10 - j00 * j12) * id;
            Jm[6] = (j10 * j21 - j11 * j20) * id;
            Jm[7] = (j01 * j20 - j21 * j00) * id;
            Jm[8] = (j00 * j11 - j10 * j01) * id;
            W[D_D + q] = s_w[q] * det;
          }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 3. H[p][q] = (-k w det)(2 - [d == e]) sum_s Jinv[d][s] Jinv[e][s]  (T2 is dead: H overlays it)
        for (int q = lane; q < nq; q += 64) {
          const double* Ji = W + D_J + q * 9;
          const double sc = -kcond * W[D_D + q], sc2 = 2.0 * sc;
          W[D_H + 0 * nq + q] = sc * (Ji[0] * Ji[0] + Ji[1] * Ji[1] + Ji[2] * Ji[2]);
          W[D_H + 1 * nq + q] = sc * (Ji[3] * Ji[3] + Ji[4] * Ji[4] + Ji[5] * Ji[5]);
          W[D_H + 2 * nq + q] = sc * (Ji[6] * Ji[6] + Ji[7] * Ji[7] + Ji[8] * Ji[8]);
          W[D_H + 3 * nq + q] = sc2 * (Ji[0] * Ji[3] + Ji[1] * Ji[4] + Ji[2] * Ji[5]);
          W[D_H + 4 * nq + q] = sc2 * (Ji[0] * Ji[6] + Ji[1] * Ji[7] + Ji[2] * Ji[8]);
          W[D_H + 5 * nq + q] = sc2 * (Ji[3] * Ji[6] + Ji[4] * Ji[7] + Ji[5] * Ji[8]);
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 4. the three stages over q2, q1, q0 (J is dead: VA | WB overlay it)
        for (int t = lane; t < nA; t += 64) {
          const int d = s_dec[oA + t];
          const double* tp = s_tabp + ((d >> 14) & 3) * 4 * ng + ((d >> 12) & 3);
          const double* hp = W + D_H + (d & 0xfff);
          double acc = 0.0;
          for (int q2 = 0; q2 < ng; ++q2) acc += tp[4 * q2] * hp[ngg * q2];
          W[D_VA + t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < nB; t += 64) {
          const int d = s_dec[oB + t];
          const double* tp = s_tabp + ((d >> 14) & 3) * 4 * ng + ((d >> 12) & 3);
          const double* va = W + D_VA + (d & 0xfff);
          double acc = 0.0;
          for (int q1 = 0; q1 < ng; ++q1) acc += tp[4 * q1] * va[3 * q1];
          W[D_WB + t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        {  // lane a + 27 h sums the pairs 3 h .. 3 h + 2 of node a (the squares, then the mixed ones); lane a adds the two halves
          const int a = lane < 54 ? lane % 27 : 0, half = lane < 27 ? 0 : 1;
          const int a0 = a % 3, a12 = a / 3;
          double part = 0.0;
          if (lane < 54) {
            for (int pp = 0; pp < 3; ++pp) {
              const int p = 3 * half + pp;
              const double* tp = s_tabp + b27d_kind(p, 0) * 4 * ng + a0;
              const double* wb = W + D_WB + p * ng * 9 + a12;
              for (int q0 = 0; q0 < ng; ++q0) part += tp[4 * q0] * wb[9 * q0];
            }
          }
          const double other = __shfl(part, (lane + 27) & 63);
          if (lane < 27) Fe[((J - it.Jb) * B27_EH + (K - it.Kb)) * 27 + lane] = part + other;
        }
        __builtin_amdgcn_wave_barrier();
      }
      __syncthreads();
      // ---- phase B: the column's three planes of this element plane, the <= 4 element entries in a fixed order (j low to high, then k)
      if (nd_ok) {
        double lo = 0.0, mid = 0.0, up = 0.0;
        for (int a = 0; a < nj; ++a)
          for (int b = 0; b < nk; ++b) {
            const double* f = Fe + ((Ej[a] - it.Jb) * B27_EH + (Ek[b] - it.Kb)) * 27 + 3 * cj[a] + 9 * ck[b];
            lo += f[0];
            mid += f[1];
            up += f[2];
          }
        if (I >= it.Iown) {
          const int64_t node = (int64_t)(2 * I) * B.plane_len + (int64_t)j * B.m2 + k;
          dg[node] = carry + lo;
          dg[node + B.plane_len] = mid;
        }
        carry = up;
      }
      __syncthreads();  // (the next plane overwrites Fe)
    }
    if (nd_ok && it.last_seg) dg[(int64_t)(2 * B.ne0) * B.plane_len + (int64_t)j * B.m2 + k] = carry;  // the brick's last plane has no element above it
  }
}

// =================================================================================================
// Face entries K^face_aa of control point (i, j, k): the DIAG = true terms of b27_face_row (brick_operator_hex27.hip)
//   Robin    sum_q w^s N_a (-h) N_a                          (the 9 face nodes)
//   Nitsche  sum_q w^s N_a (-h_penalty N_a + k n . grad N_a)  (the basis of the host element's 27 nodes on the face)
// =================================================================================================
__device__ __forceinline__ void b27d_lag2(double x, double (&L)[3], double (&dL)[3]) {
  L[0] = 2.0 * (x - 0.5) * (x - 1.0);
  L[1] = -4.0 * x * (x - 1.0);
  L[2] = 2.0 * x * (x - 0.5);
  dL[0] = 4.0 * x - 3.0;
  dL[1] = -8.0 * x + 4.0;
  dL[2] = 4.0 * x - 1.0;
}

// NITSCHE = false leaves the host element's 27 nodes out of the code (the multigrid's launch: it refuses an active Nitsche term)
template <bool NITSCHE>
__device__ __forceinline__ double b27d_face_diag(const BrickView& B, const Bop27Diag& P, int i, int j, int k) {
  const bool robin_on = h8_robin_launch(P.h, P.robin), nitsche_on = NITSCHE && bop_nitsche_on(P.k, P.hp, P.fixed);
  double r = 0.0;
  const int idx[3] = {i, j, k};
  const int ne[3] = {B.ne0, B.ne1, B.ne2};
  for (int nd = 0; nd < 3; ++nd) {
    for (int side = 0; side < 2; ++side) {
      const bool on = side == 0 ? (idx[nd] == 0) : (idx[nd] == 2 * ne[nd]);
      if (!on) continue;
      const bool robin = robin_on && (P.robin & face_bit(nd, side)), nitsche = nitsche_on && (P.fixed & face_bit(nd, side));
      if (!robin && !nitsche) continue;
      const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
      int E1[2], c1[2], E2[2], c2[2];
      const int n1 = b27_face_elements(idx[t1], ne[t1], E1, c1), n2 = b27_face_elements(idx[t2], ne[t2], E2, c2);
      for (int f2 = 0; f2 < n2; ++f2)
        for (int f1 = 0; f1 < n1; ++f1) {
          if (robin) {
            const int a = c1[f1] + 3 * c2[f2];
            double Xf[9][3];
#pragma unroll
            for (int c = 0; c < 9; ++c) {
              int g[3];
              g[nd] = idx[nd];
              g[t1] = 2 * E1[f1] + c % 3;
              g[t2] = 2 * E2[f2] + c / 3;
              const int64_t ci = brick_cindex(B, g[0], g[1], g[2]);
              Xf[c][0] = B.X0[ci];
              Xf[c][1] = B.X1[ci];
              Xf[c][2] = B.X2[ci];
            }
            for (int q = 0; q < P.ng * P.ng; ++q) {
              double ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0};
#pragma unroll
              for (int c = 0; c < 9; ++c)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                  ta[d] += P.T->fdN[q][c][0] * Xf[c][d];
                  tb[d] += P.T->fdN[q][c][1] * Xf[c][d];
                }
              const double r0 = ta[1] * tb[2] - ta[2] * tb[1], r1 = -ta[0] * tb[2] + ta[2] * tb[0], r2 = ta[0] * tb[1] - ta[1] * tb[0];
              const double ws = P.T->fw[q] * sqrt(r0 * r0 + r1 * r1 + r2 * r2);
              const double na = P.T->fN[q][a];
              r += (-P.h * ws) * (na * na);
            }
          }
          if (NITSCHE && nitsche) {
            int E[3], la[3];
            E[nd] = side ? ne[nd] - 1 : 0;
            E[t1] = E1[f1];
            E[t2] = E2[f2];
            la[nd] = side ? 2 : 0;
            la[t1] = c1[f1];
            la[t2] = c2[f2];
            double X[27][3];
            for (int b = 0; b < 27; ++b) {
              const int64_t ci = brick_cindex(B, 2 * E[0] + b % 3, 2 * E[1] + (b / 3) % 3, 2 * E[2] + b / 9);
              X[b][0] = B.X0[ci];
              X[b][1] = B.X1[ci];
              X[b][2] = B.X2[ci];
            }
            for (int q = 0; q < P.ng * P.ng; ++q) {
              const int q1 = q % P.ng, q2 = q / P.ng;  // first in-face coordinate fastest
              double xi[3];
              xi[nd] = side ? 1.0 : 0.0;
              xi[t1] = P.gp[q1];
              xi[t2] = P.gp[q2];
              double L[3][3], dL[3][3];
              for (int d = 0; d < 3; ++d) b27d_lag2(xi[d], L[d], dL[d]);
              double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
              for (int b = 0; b < 27; ++b) {
                const int b0 = b % 3, b1 = (b / 3) % 3, b2 = b / 9;
                const double d0 = dL[0][b0] * L[1][b1] * L[2][b2], d1 = L[0][b0] * dL[1][b1] * L[2][b2], d2 = L[0][b0] * L[1][b1] * dL[2][b2];
                for (int c = 0; c < 3; ++c) {
                  J[c][0] += d0 * X[b][c];
                  J[c][1] += d1 * X[b][c];
                  J[c][2] += d2 * X[b][c];
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
              for (int c = 0; c < 3; ++c) {
                ta[c] = side ? J[c][t1] : -J[c][t1];
                tb[c] = J[c][t2];
              }
              const double r0 = ta[1] * tb[2] - ta[2] * tb[1], r1 = -ta[0] * tb[2] + ta[2] * tb[0], r2 = ta[0] * tb[1] - ta[1] * tb[0];
              const double ld = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
              const double nrm[3] = {r0 / ld, r1 / ld, r2 / ld};
              const double ws = P.gw[q1] * P.gw[q2] * ld;
              double v[3];  // n . grad N_b = sum_m dN_b/dxi_m v[m]
              for (int m = 0; m < 3; ++m) v[m] = Iv[m][0] * nrm[0] + Iv[m][1] * nrm[1] + Iv[m][2] * nrm[2];
              const double Na = L[0][la[0]] * L[1][la[1]] * L[2][la[2]];
              const double ga = dL[0][la[0]] * L[1][la[1]] * L[2][la[2]] * v[0] + L[0][la[0]] * dL[1][la[1]] * L[2][la[2]] * v[1] +
                                L[0][la[0]] * L[1][la[1]] * dL[2][la[2]] * v[2];
              r += ws * Na * (-P.hp * Na + P.k * ga);
            }
          }
        }
    }
  }
  return r;
}

// a thread strides over the boundary control points, after the sweep: d += K^face_aa (the only writer of its point)
template <bool NITSCHE>
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick27_diagonal_faces(BrickView B, Bop27Diag P, int64_t count, double* __restrict__ dg) {
  for (int64_t t = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x; t < count; t += (int64_t)gridDim.x * MFEM_BLOCK) {
    int i, j, k;
    if (!h8_boundary_point(t, 0, B.m0, B.m0 - 1, B.m1 - 1, B.m2 - 1, B.plane_len, B.m1, B.m2, i, j, k)) continue;
    const int64_t node = (int64_t)i * B.plane_len + (int64_t)j * B.m2 + k;
    dg[node] += b27d_face_diag<NITSCHE>(B, P, i, j, k);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
static const double B27D_GP[4][4] = {{0.0, 0, 0, 0},
                                     {-0.57735026918962576451, 0.57735026918962576451, 0, 0},
                                     {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                     {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double B27D_GW[4][4] = {{2.0, 0, 0, 0},
                                     {1.0, 1.0, 0, 0},
                                     {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                     {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};

// d_i <- K_ii for every control point (a zero diagonal is written as 0: the sweep owns every point)
int bop27_signed_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) {
  const mfem_brick_s* m = op->brick;
  const mfem_thermal_params& p = op->thermal;
  Bop27Diag P;
  memset(&P, 0, sizeof(P));
  P.k = p.k; P.h = p.h; P.hp = p.h_penalty;
  P.robin = p.robin_faces; P.fixed = p.fixed_faces;
  P.ng = m->ng;
  P.T = op->tables27;
  for (int q = 0; q < P.ng; ++q) {
    P.gp[q] = B27D_GP[P.ng - 1][q] / 2.0 + 0.5;
    P.gw[q] = B27D_GW[P.ng - 1][q] / 2.0;
  }
  const B27Volume V = b27_volume(m->ne[0], m->ne[1], m->ne[2]);
  MFEM_REQUIRE(V.items < ((int64_t)1 << 31), "too many work items for one launch");
  MFEM_REQUIRE(B.plo == 0 && B.clo == 0 && B.phi == B.m0, "the hex-27 operator runs on the whole lattice");
  const size_t lds = b27d_lds_bytes(m->ng);
  MFEM_REQUIRE(lds <= B27_LDS_LIMIT, "the diagonal sweep's LDS block exceeds a CU's");
  hipLaunchKernelGGL(k_brick27_diagonal_sweep, dim3((unsigned)V.items), dim3(B27_THREADS), lds, ctx->stream, B, op->tables27, V, P.k, d, 1);
  MFEM_CHECK_LAUNCH();
  if (bop_face_launch(P.k, P.h, P.robin, P.hp, P.fixed)) {
    const int64_t count = bop_boundary_count(m->m[0], m->m[1], m->m[2]);
    const auto kernel = bop_nitsche_on(P.k, P.hp, P.fixed) ? k_brick27_diagonal_faces<true> : k_brick27_diagonal_faces<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)bop_face_grid(count)), dim3(MFEM_BLOCK), 0, ctx->stream, B, P, count, d);
    MFEM_CHECK_LAUNCH();
  }
  return MFEM_OK;
}

// once per operator, beside bop27_prepare: the sweep's dynamic LDS goes beyond the default 64 KB
int bop27_diagonal_prepare(int ng) {
  MFEM_REQUIRE(ng >= 1 && ng <= BRICK_MAX_NG && b27d_lds_bytes(ng) <= B27_LDS_LIMIT, "the diagonal sweep's LDS block exceeds a CU's");
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_brick27_diagonal_sweep), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)b27d_lds_bytes(BRICK_MAX_NG)));
  return MFEM_OK;
}
