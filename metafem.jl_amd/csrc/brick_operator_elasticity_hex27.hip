// The kernels of the matrix-free operator on a hex-27 (Lagrange order 2) brick with three-field linear elasticity and their launchers:
// y = alpha K x~ + beta y, |diag K| and the residual K x* + f for the K of the reference's cantilever form on the order-2 lattice -- the volume term
// -int sigma_ij(u) d_jN_a with sigma = lambda tr(eps) I + 2 mu eps, and -tau N_a N_b delta_fg on penalty_faces -- straight from the coordinates.
// Unknowns are field-major (brick_xindex), n = 3 x control points.  The handle, the entry points and the bind are brick_operator.hip's (bop_launch and
// bop_jacobi hand an operator with physics == BOP_PHYSICS_ELASTICITY_HEX27 over to bop_e27_launch / bop_e27_jacobi); every host decision is in
// brick_operator_elasticity_hex27_decide.h, the ownership and the work items in brick_operator_hex27_decide.h.
//   volume  k_brick27e_product: the row-owner plane sweep of k_brick27_product (brick_operator_hex27.hip: read its comments first) with three fields.
//           A wave per element pushes SIX components (x1..x3, u1..u3) through the sum-factorised interpolation stages, forms per Gauss point
//           grad u = (grad_xi u) Jinv, the stress and the nine flux components -w det sigma_fj Jinv_mj, runs the transposed stages per field and leaves
//           the 81-entry element vector [f][a] in the workgroup's LDS block; after the plane's barrier the owner of a control-point column adds the
//           <= 4 element vectors that meet in it IN A FIXED ORDER and writes y = alpha r + beta y for its three unknowns (beta == 0: y is not read).
//           The affine shortcut, the next-element node prefetch, the dsc column scaling, the dotw partial sums and the fold are the thermal kernel's.
//           The number of waves is the launch's (e27_waves(ng)): elements are walked blockDim / 64 apart.
//   faces   k_brick27e_faces: a thread per boundary control point adds alpha times its own penalty rows (the Robin mass term of k_hex27_faces per
//           field, tau for h); RESID = true (mfem_brick_operator_residual_elasticity) adds the traction rows sum_q w^s N_a sig_fj n_j as well.
//   diagonal k_brick27e_diagonal: a thread per control point, for f = 0..2 K_(f,a),(f,a) = -sum_el sum_q w det [mu |g|^2 + (lambda + mu) g_f^2]
//           - tau sum_faces sum_q w^s N_a^2 with g = Jinv^T grad_xi N_a; nothing is stored, a zero sum keeps the preset.  (The pair-form plane sweep of
//           k_brick27_diagonal_sweep with three H tables is not built yet: this is the per-control-point form.)
// No atomics, no colours; the same bits on every run and on every grid.  The reference tables are bop27_tables' immutable copies.
#include <atomic>
#include "hex8_device.h"
#include "hex27.h"
#include "blas1.h"
#include "brick_operator.h"
#include "brick_operator_elasticity_hex27_decide.h"

// mfem_debug_set("elasticity_hex27", word): bit 0 = every element takes the general branch (no affine shortcut); bit 1 = TIMING ONLY (wrong values):
// the stress stage and the transposed stages run for one field; bits 8-11 = waves per workgroup (0 = e27_waves(ng); clamped to what fits)
static std::atomic<int> g_e27_word{0};
extern "C" int mfem_debug_set_elasticity_hex27(int word) {
  g_e27_word = word;
  return MFEM_OK;
}
static int e27_launch_waves(int ng, int word) {
  const int most = e27_waves(ng), ask = (word >> 8) & 15;
  return ask == 0 ? most : ask < E27_WAVES_MIN ? E27_WAVES_MIN : ask > most ? most : ask;
}

struct BopE27 {
  double lam, mu, tau;
  uint32_t penalty, traction;
  double sg[3][3];
  int ng;
  const Hex27Tables* T;
};

// the per-wave carve-up (brick_operator_elasticity_hex27_decide.h), over the kernel's own ng and nq
#define EW_X 0
#define EW_T1 (27 * NI)
#define EW_J 0
#define EW_GU (9 * nq)
#define EW_VA 0
#define EW_WB e27_w_wb(ng)
#define EW_T2 e27_w_t2(ng)
#define EW_G EW_T2
#define EW_D e27_w_d(ng)

// =================================================================================================
// Volume
// =================================================================================================
// __launch_bounds__(E27_THREADS_MAX): one workgroup of 12 waves per CU, 3 per SIMD: <= 168 VGPRs per lane
__global__ __launch_bounds__(E27_THREADS_MAX) void k_brick27e_product(BrickView B, const Hex27Tables* __restrict__ tab, B27Volume V, double lam, double mu,
                                                                      const double* __restrict__ x, const double* __restrict__ dsc, double* __restrict__ y,
                                                                      double alpha, double beta, int affine_fast, int one_field,
                                                                      const double* __restrict__ dotw, double* __restrict__ partials,
                                                                      const int32_t* __restrict__ done_flag) {
  extern __shared__ double lds[];
  __shared__ double red[16];
  static_assert(sizeof(red) == E27_LDS_STATIC, "the decide header counts the static LDS");
  if (done_flag && done_flag[0]) return;
  constexpr int NI = E27_NI;
  const int ng = B.ng, nq = ng * ng * ng;
  const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
  const int nwv = nthr >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: the element walk below runs on the scalar unit)
  double* s_w = lds;
  double* s_tab1 = lds + e27_off_tab1(ng);
  int32_t* s_dec = reinterpret_cast<int32_t*>(lds + e27_off_dec(ng));
  double* Fe = lds + e27_off_fe(ng);
  double* W = lds + e27_off_waves(ng) + (size_t)wv * e27_w_size(ng);
  const int ngg = ng * ng;
  const int n1 = e27_n1(ng), n2 = e27_n2(ng), n3 = e27_n3(ng), nA1 = 9 * ngg, nB1 = 18 * ng, nA = e27_na(ng), nB = e27_nb(ng);
  for (int i = tid; i < nq; i += nthr) s_w[i] = tab->w[i];
  for (int i = tid; i < 8 * ng; i += nthr) s_tab1[i] = tab->tab1[i / (4 * ng)][(i >> 2) % ng][i & 3];
  // decode words of the stages (k_brick27_product): low half = offset of the first of the 3 operands (stride NI), high half = offset of the 1-D table row
  for (int t = tid; t < n1; t += nthr) {  // T1[k][q0][a12][i] = sum_a0 tab1[k][q0][a0] X[a0 + 3 a12][i]
    const int i = t % NI, a12 = (t / NI) % 9, kq = t / (9 * NI);
    s_dec[t] = (3 * a12 * NI + i) | ((4 * kq) << 16);
  }
  for (int t = tid; t < n2; t += nthr) {  // T2[kk][q0][q1][a2][i] = sum_a1 tab1[kt][q1][a1] T1[k][q0][a1 + 3 a2][i]
    const int i = t % NI, a2 = (t / NI) % 3, q1 = (t / (3 * NI)) % ng, q0 = (t / (3 * NI * ng)) % ng, kk = t / (3 * NI * ng * ng);
    const int k = kk == 0 ? 1 : 0, kt = kk == 1 ? 1 : 0;  // kk = 0: d/dxi0, 1: d/dxi1, 2: values in both
    s_dec[n1 + t] = (((k * ng + q0) * 9 + 3 * a2) * NI + i) | ((4 * (kt * ng + q1)) << 16);
  }
  for (int t = tid; t < n3; t += nthr) {  // t < 9 nq: J[q][i][m]; then 9 nq: grad_xi u [q][f][m]
    const int tt = t < 9 * nq ? t : t - 9 * nq;
    const int m = tt % 3, i = (tt / 3) % 3 + (t < 9 * nq ? 0 : 3), q = tt / 9;
    const int q0 = q % ng, q1 = (q / ng) % ng, q2 = q / ngg;
    const int kt = m == 2 ? 1 : 0;
    s_dec[n1 + n2 + t] = ((((m * ng + q0) * ng + q1) * 3) * NI + i) | ((4 * (kt * ng + q2)) << 16);
  }
  for (int t = tid; t < nA; t += nthr) {  // VA[f][v][q0][q1][a2] = sum_q2 tab[q2][a2] h_f,v[q]  (v = 2: the derivative row)
    const int f = t / nA1, tt = t % nA1;
    const int a2 = tt % 3, q1 = (tt / 3) % ng, q0 = (tt / (3 * ng)) % ng, v = tt / (3 * ngg);
    const int qb = q0 + ng * q1;
    s_dec[n1 + n2 + n3 + t] = (f * 3 * nq + 3 * qb + v) | (a2 << 12) | ((v == 2 ? 1 : 0) << 14);
  }
  for (int t = tid; t < nB; t += nthr) {  // WB[f][w][q0][a12] = sum_q1 tab[q1][a1] VA[f][..]  (w = 1: D VA_1 + L VA_2)
    const int f = t / nB1, tt = t % nB1;
    const int a12 = tt % 9, a1 = a12 % 3, a2 = a12 / 3, q0 = (tt / 9) % ng, w = tt / (9 * ng);
    s_dec[n1 + n2 + n3 + nA + t] = (f * nA1 + ((w * ng + q0) * ng) * 3 + a2) | (a1 << 12) | (w << 14);
  }
  __syncthreads();
  const bool has_dsc = dsc != nullptr;
  const int oA = n1 + n2 + n3, oB = oA + nA;
  const int nAr = one_field ? nA1 : nA, nBr = one_field ? nB1 : nB;  // (one_field: a timing ablation)

  // node data of an element: lane a < 27 loads node a (lanes 27 .. 63 repeat node 26); issued for the NEXT element while this one is integrated.  The
  // brick is whole (bop_view refuses a slab: plo == clo == 0), so a control point has ONE index into the coordinates and, plus f n_owned, into x, dsc
  // and y: the element's first node (wave-uniform, scalar arithmetic) plus the lane's offset within the element.
  struct NodePre {
    double x0, x1, x2, u0, u1, u2, d0, d1, d2;
  };
  const int ln = lane < 27 ? lane : 26;
  const int64_t lane_off = (int64_t)(ln % 3) * B.plane_len + (int64_t)((ln / 3) % 3) * B.m2 + ln / 9;
  const int64_t NO = B.n_owned;
  auto fetch_nodes = [&](int I, int J, int K) -> NodePre {
    NodePre n;
    const int64_t c = ((int64_t)(2 * I) * B.plane_len + (int64_t)(2 * J) * B.m2 + 2 * K) + lane_off;
    n.x0 = B.X0[c];
    n.x1 = B.X1[c];
    n.x2 = B.X2[c];
    n.u0 = x[c];
    n.u1 = x[c + NO];
    n.u2 = x[c + 2 * NO];
    n.d0 = has_dsc ? dsc[c] : 1.0;
    n.d1 = has_dsc ? dsc[c + NO] : 1.0;
    n.d2 = has_dsc ? dsc[c + 2 * NO] : 1.0;
    return n;
  };

  double dot_acc = 0.0;
  for (int64_t w = blockIdx.x; w < V.items; w += gridDim.x) {  // (workgroup-uniform)
    const B27Item it = b27_item(V, w, B.ne0, B.ne1, B.ne2);
    const int nEK = it.K1 - it.K0;
    // phase B: this thread's control-point column
    const int lj = tid / B27_NP, lk = tid % B27_NP;
    const int j = it.j0 + lj, k = it.k0 + lk;
    const bool nd_ok = tid < B27_NP * B27_NP && j < it.j1 && k < it.k1;
    int Ej[2], cj[2], Ek[2], ck[2];
    const int nj = b27_face_elements(nd_ok ? j : 0, B.ne1, Ej, cj), nk = b27_face_elements(nd_ok ? k : 0, B.ne2, Ek, ck);
    double carry[3] = {0.0, 0.0, 0.0};
    // phase A: the wave's walk over (plane, element column), nwv columns apart; it always holds the node data of its next element
    const int nEJ = it.J1 - it.J0;
    int ej0 = 0, ek0 = wv;  // the wave's first column of a plane
    while (ek0 >= nEK && ej0 < nEJ) { ek0 -= nEK; ++ej0; }
    const bool wave_has = ej0 < nEJ;
    NodePre cur = fetch_nodes(it.I0, it.J0 + (wave_has ? ej0 : 0), it.K0 + (wave_has ? ek0 : 0));
    for (int I = it.I0; I < it.I1; ++I) {
      for (int ej = ej0, ek = ek0; ej < nEJ;) {
        const int J = it.J0 + ej, K = it.K0 + ek;
        // ---- 1. nodes
        if (lane < 27) {
          W[EW_X + NI * lane + 0] = cur.x0;
          W[EW_X + NI * lane + 1] = cur.x1;
          W[EW_X + NI * lane + 2] = cur.x2;
          W[EW_X + NI * lane + 3] = has_dsc ? cur.u0 / cur.d0 : cur.u0;
          W[EW_X + NI * lane + 4] = has_dsc ? cur.u1 / cur.d1 : cur.u1;
          W[EW_X + NI * lane + 5] = has_dsc ? cur.u2 / cur.d2 : cur.u2;
        }
        {  // the next element of this wave: its loads are in flight during this element's stages
          ek += nwv;
          while (ek >= nEK && ej < nEJ) { ek -= nEK; ++ej; }
          const bool more = ej < nEJ;
          const int In = more ? I : (I + 1 < it.I1 ? I + 1 : I);
          cur = fetch_nodes(In, it.J0 + (more ? ej : ej0), it.K0 + (more ? ek : ek0));
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 2'. affine elements: J is one matrix, only u goes through the stages (k_brick27_product's test, word for word)
        bool affine = false;
        if (affine_fast) {
          const double x0 = W[EW_X + 0], y0 = W[EW_X + 1], z0 = W[EW_X + 2];
          const double ex0 = W[EW_X + NI * 2 + 0] - x0, ey0 = W[EW_X + NI * 2 + 1] - y0, ez0 = W[EW_X + NI * 2 + 2] - z0;
          const double ex1 = W[EW_X + NI * 6 + 0] - x0, ey1 = W[EW_X + NI * 6 + 1] - y0, ez1 = W[EW_X + NI * 6 + 2] - z0;
          const double ex2 = W[EW_X + NI * 18 + 0] - x0, ey2 = W[EW_X + NI * 18 + 1] - y0, ez2 = W[EW_X + NI * 18 + 2] - z0;
          bool mine = true;
          if (lane < 27) {
            const double a0 = 0.5 * (lane % 3), a1 = 0.5 * ((lane / 3) % 3), a2 = 0.5 * (lane / 9);
            const double px = x0 + a0 * ex0 + a1 * ex1 + a2 * ex2, py = y0 + a0 * ey0 + a1 * ey1 + a2 * ey2, pz = z0 + a0 * ez0 + a1 * ez1 + a2 * ez2;
            const double mx = W[EW_X + NI * lane + 0], my = W[EW_X + NI * lane + 1], mz = W[EW_X + NI * lane + 2];
            const double tol = 3.6e-15;  // 16 ulp of the largest coordinate magnitude the element spans, per component
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
            for (int u = lane; u < n1 / 2; u += 64) {  // (components 3 .. 5 of every entry)
              const int t = (u / 3) * NI + 3 + u % 3;
              const int d = s_dec[t];
              const double* xs = W + EW_X + (d & 0xffff);
              const double* tb = s_tab1 + (d >> 16);
              W[EW_T1 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
            }
            __builtin_amdgcn_wave_barrier();
            for (int u = lane; u < n2 / 2; u += 64) {
              const int t = (u / 3) * NI + 3 + u % 3;
              const int d = s_dec[n1 + t];
              const double* xs = W + EW_T1 + (d & 0xffff);
              const double* tb = s_tab1 + (d >> 16);
              W[EW_T2 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
            }
            __builtin_amdgcn_wave_barrier();
            for (int t = 9 * nq + lane; t < n3; t += 64) {  // grad_xi u at the Gauss points
              const int d = s_dec[n1 + n2 + t];
              const double* xs = W + EW_T2 + (d & 0xffff);
              const double* tb = s_tab1 + (d >> 16);
              W[EW_J + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
            }
            for (int q = lane; q < nq; q += 64) {  // (rows 0 .. 9 nq: X and T1 are dead, the outputs above sit behind them)
              double* Jm = W + EW_J + q * 9;
              Jm[0] = i0; Jm[1] = i1; Jm[2] = i2; Jm[3] = i3; Jm[4] = i4; Jm[5] = i5; Jm[6] = i6; Jm[7] = i7; Jm[8] = i8;
              W[EW_D + q] = s_w[q] * det;
            }
          }
        }
        if (!affine) {
          // ---- 2a. J and grad_xi u at the Gauss points, sum-factorised
          for (int t = lane; t < n1; t += 64) {
            const int d = s_dec[t];
            const double* xs = W + EW_X + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[EW_T1 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          for (int t = lane; t < n2; t += 64) {
            const int d = s_dec[n1 + t];
            const double* xs = W + EW_T1 + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[EW_T2 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          for (int t = lane; t < n3; t += 64) {
            const int d = s_dec[n1 + n2 + t];
            const double* xs = W + EW_T2 + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[EW_J + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          // ---- 2b. det, inverse (adjugate), w det; Jinv overwrites J as [m][s]
          for (int q = lane; q < nq; q += 64) {
            double* Jm = W + EW_J + q * 9;
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
            W[EW_D + q] = s_w[q] * det;
          }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 3. fe[f][a] = -sum_q w det sigma_fj(u) d_jN_a:  grad u = (grad_xi u) Jinv, the stress, the flux h[f][m] = -w det sigma_fj Jinv_mj,
        //         then the transposed stages over q2, q1, q0 per field
        for (int q = lane; q < nq; q += 64) {
          const double* Ji = W + EW_J + q * 9;
          const double* G = W + EW_GU + q * 9;
          double du[3][3];  // du[f][s] = d u_f / d x_s
#pragma unroll
          for (int f = 0; f < 3; ++f)
#pragma unroll
            for (int s = 0; s < 3; ++s) du[f][s] = G[3 * f] * Ji[s] + G[3 * f + 1] * Ji[3 + s] + G[3 * f + 2] * Ji[6 + s];
          const double ltr = lam * (du[0][0] + du[1][1] + du[2][2]);
          const double sc = -W[EW_D + q];
#pragma unroll
          for (int f = 0; f < 3; ++f) {
            if (one_field && f > 0) break;
            double sg[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) sg[s] = mu * (du[f][s] + du[s][f]) + (f == s ? ltr : 0.0);
#pragma unroll
            for (int m = 0; m < 3; ++m) W[EW_G + f * 3 * nq + 3 * q + m] = sc * (sg[0] * Ji[3 * m] + sg[1] * Ji[3 * m + 1] + sg[2] * Ji[3 * m + 2]);
          }
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < nAr; t += 64) {
          const int d = s_dec[oA + t];
          const int a2 = (d >> 12) & 3, v2 = (d >> 14) & 1;
          const double* hp = W + EW_G + (d & 0xfff);
          double acc = 0.0;
          for (int q2 = 0; q2 < ng; ++q2) acc += s_tab1[((v2 ? ng : 0) + q2) * 4 + a2] * hp[3 * ngg * q2];
          W[EW_VA + t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < nBr; t += 64) {
          const int d = s_dec[oB + t];
          const int a1 = (d >> 12) & 3, wb = (d >> 14) & 1;
          const double* va = W + EW_VA + (d & 0xfff);
          double acc = 0.0;
          for (int q1 = 0; q1 < ng; ++q1) {
            const double L = s_tab1[q1 * 4 + a1], D = s_tab1[(ng + q1) * 4 + a1];
            acc += (wb ? D : L) * va[3 * q1];
            if (wb) acc += L * va[3 * ngg + 3 * q1];
          }
          W[EW_WB + t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        for (int l = lane; l < E27_NV; l += 64) {
          const int f = l / 27, a = l - 27 * f;
          const int a0 = a % 3, a12 = a / 3;
          double fe = 0.0;
          if (!(one_field && f > 0)) {
            const double* wbp = W + EW_WB + f * nB1;
            for (int q0 = 0; q0 < ng; ++q0) fe += s_tab1[(ng + q0) * 4 + a0] * wbp[q0 * 9 + a12] + s_tab1[q0 * 4 + a0] * wbp[(ng + q0) * 9 + a12];
          }
          Fe[((J - it.Jb) * B27_EH + (K - it.Kb)) * E27_NV + l] = fe;
        }
        __builtin_amdgcn_wave_barrier();
      }
      __syncthreads();
      // ---- phase B: the column's three planes of this element plane, the <= 4 element vectors in a fixed order (j low to high, then k), per field
      if (nd_ok) {
        double lo[3] = {0.0, 0.0, 0.0}, mid[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 0.0, 0.0};
        for (int a = 0; a < nj; ++a)
          for (int b = 0; b < nk; ++b) {
            const double* fp = Fe + ((Ej[a] - it.Jb) * B27_EH + (Ek[b] - it.Kb)) * E27_NV + 3 * cj[a] + 9 * ck[b];
#pragma unroll
            for (int f = 0; f < 3; ++f) {
              lo[f] += fp[27 * f];
              mid[f] += fp[27 * f + 1];
              up[f] += fp[27 * f + 2];
            }
          }
        const int64_t node = (int64_t)(2 * I) * B.plane_len + (int64_t)j * B.m2 + k;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          if (I >= it.Iown) {
            const int64_t row = (int64_t)f * NO + node;
            double y0 = alpha * (carry[f] + lo[f]), y1 = alpha * mid[f];
            if (beta != 0.0) {
              y0 += beta * y[row];
              y1 += beta * y[row + B.plane_len];
            }
            y[row] = y0;
            y[row + B.plane_len] = y1;
            if (dotw) dot_acc += y0 * dotw[row] + y1 * dotw[row + B.plane_len];
          }
          carry[f] = up[f];
        }
      }
      __syncthreads();  // (the next plane overwrites Fe)
    }
    if (nd_ok && it.last_seg) {  // the brick's last plane has no element above it
      const int64_t node = (int64_t)(2 * B.ne0) * B.plane_len + (int64_t)j * B.m2 + k;
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const int64_t row = (int64_t)f * NO + node;
        double yv = alpha * carry[f];
        if (beta != 0.0) yv += beta * y[row];
        y[row] = yv;
        if (dotw) dot_acc += yv * dotw[row];
      }
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Face terms of the rows of control point (i, j, k), summed over the <= 4 face elements per face the point lies on (the nine face nodes each).
//   DIAG = false: r[f] = sum_q w^s N_a (-tau) sum_b N_b x~_(f,b) on penalty faces  (+ RESID: sum_q w^s N_a sig_fj n_j on traction faces, n outward)
//   DIAG = true:  r[0] = -tau sum_q w^s N_a^2 (the same for every field)
// =================================================================================================
template <bool DIAG, bool RESID>
__device__ __forceinline__ void e27_face_rows(const BrickView& B, const BopE27& P, int i, int j, int k, const double* __restrict__ x,
                                              const double* __restrict__ dsc, double (&r)[3]) {
  const int idx[3] = {i, j, k};
  const int ne[3] = {B.ne0, B.ne1, B.ne2};
  for (int nd = 0; nd < 3; ++nd) {
    for (int side = 0; side < 2; ++side) {
      const bool on = side == 0 ? (idx[nd] == 0) : (idx[nd] == 2 * ne[nd]);
      if (!on) continue;
      const bool pen = P.tau != 0.0 && (P.penalty & face_bit(nd, side)), tra = RESID && (P.traction & face_bit(nd, side));
      if (!pen && !tra) continue;
      const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
      int E1[2], c1[2], E2[2], c2[2];
      const int n1 = b27_face_elements(idx[t1], ne[t1], E1, c1), n2 = b27_face_elements(idx[t2], ne[t2], E2, c2);
      for (int f2 = 0; f2 < n2; ++f2)
        for (int f1 = 0; f1 < n1; ++f1) {
          const int a = c1[f1] + 3 * c2[f2];
          double Xf[9][3], Uf[9][3];
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
#pragma unroll
            for (int f = 0; f < 3; ++f) Uf[c][f] = (DIAG || !pen) ? 0.0 : bop_scaled(x, dsc, brick_xindex(B, f, g[0], g[1], g[2]));
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
            // ta x tb points along +nd: outward on the high face, inward on the low one
            const double r0 = ta[1] * tb[2] - ta[2] * tb[1], r1 = -ta[0] * tb[2] + ta[2] * tb[0], r2 = ta[0] * tb[1] - ta[1] * tb[0];
            const double ld = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
            const double ws = P.T->fw[q] * ld;
            const double na = P.T->fN[q][a];
            if (DIAG) {
              r[0] += ws * na * (-P.tau * na);
            } else {
              double uq[3] = {0.0, 0.0, 0.0};
#pragma unroll
              for (int c = 0; c < 9; ++c)
#pragma unroll
                for (int f = 0; f < 3; ++f) uq[f] += P.T->fN[q][c] * Uf[c][f];
              const double sn = side ? 1.0 : -1.0;
              const double nrm[3] = {sn * r0 / ld, sn * r1 / ld, sn * r2 / ld};
#pragma unroll
              for (int f = 0; f < 3; ++f) {
                double v = 0.0;
                if (pen) v += P.tau * (0.0 - uq[f]);
                if (RESID && tra) v += P.sg[f][0] * nrm[0] + P.sg[f][1] * nrm[1] + P.sg[f][2] * nrm[2];
                r[f] += ws * na * v;
              }
            }
          }
        }
    }
  }
}

// a thread strides over the boundary control points; after the volume kernel: y += alpha (face rows), and the increments' partial sums of dotw . y
template <bool RESID>
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick27e_faces(BrickView B, BopE27 P, int64_t count, const double* __restrict__ x, const double* __restrict__ dsc,
                                                               double* __restrict__ y, double alpha, const double* __restrict__ dotw,
                                                               double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x; t < count; t += (int64_t)gridDim.x * MFEM_BLOCK) {
    int i, j, k;
    if (!h8_boundary_point(t, 0, B.m0, B.m0 - 1, B.m1 - 1, B.m2 - 1, B.plane_len, B.m1, B.m2, i, j, k)) continue;
    const int64_t node = (int64_t)i * B.plane_len + (int64_t)j * B.m2 + k;
    double r[3] = {0.0, 0.0, 0.0};
    e27_face_rows<false, RESID>(B, P, i, j, k, x, dsc, r);
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
// Diagonal: d_(f,a) <- |K_(f,a),(f,a)| where it is not zero (else d keeps its preset).  A thread per control point: over its <= 8 adjacent elements
// -sum_q w det [mu |g|^2 + (lambda + mu) g_f^2] with g = Jinv^T grad_xi N_a and J from the element's 27 nodes, then its own penalty term.  Runs once
// per solve.
// =================================================================================================
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick27e_diagonal(BrickView B, BopE27 P, int face_terms, double* __restrict__ d) {
  const int64_t node = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x;
  if (node >= B.n_owned) return;
  int i, j, k;
  node_ijk(B, node, i, j, k);
  double sum[3] = {0.0, 0.0, 0.0};
  const int nq = P.ng * P.ng * P.ng;
  if (P.lam != 0.0 || P.mu != 0.0) {
    int Ei[2], ci[2], Ej[2], cj[2], Ek[2], ck[2];
    const int ni = b27_face_elements(i, B.ne0, Ei, ci), nj = b27_face_elements(j, B.ne1, Ej, cj), nk = b27_face_elements(k, B.ne2, Ek, ck);
    for (int e0 = 0; e0 < ni; ++e0)
      for (int e1 = 0; e1 < nj; ++e1)
        for (int e2 = 0; e2 < nk; ++e2) {
          const int a = ci[e0] + 3 * cj[e1] + 9 * ck[e2];
          double X[27][3];
#pragma unroll
          for (int b = 0; b < 27; ++b) {
            const int64_t c = brick_cindex(B, 2 * Ei[e0] + b % 3, 2 * Ej[e1] + (b / 3) % 3, 2 * Ek[e2] + b / 9);
            X[b][0] = B.X0[c];
            X[b][1] = B.X1[c];
            X[b][2] = B.X2[c];
          }
          double acc[3] = {0.0, 0.0, 0.0};
          for (int q = 0; q < nq; ++q) {
            double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
            for (int b = 0; b < 27; ++b)
#pragma unroll
              for (int m = 0; m < 3; ++m) {
                const double dn = P.T->dN[q][m][b];
                J[0][m] += dn * X[b][0];
                J[1][m] += dn * X[b][1];
                J[2][m] += dn * X[b][2];
              }
            const double det = J[0][0] * J[1][1] * J[2][2] - J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] + J[0][1] * J[1][2] * J[2][0] +
                               J[0][2] * J[1][0] * J[2][1] - J[0][2] * J[1][1] * J[2][0];
            const double id = 1.0 / det;
            double Iv[3][3];  // Iv[m][s] = dxi_m / dx_s
            Iv[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
            Iv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
            Iv[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) * id;
            Iv[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) * id;
            Iv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
            Iv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
            Iv[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
            Iv[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) * id;
            Iv[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) * id;
            const double d0 = P.T->dN[q][0][a], d1 = P.T->dN[q][1][a], d2 = P.T->dN[q][2][a];
            const double g[3] = {d0 * Iv[0][0] + d1 * Iv[1][0] + d2 * Iv[2][0], d0 * Iv[0][1] + d1 * Iv[1][1] + d2 * Iv[2][1],
                                 d0 * Iv[0][2] + d1 * Iv[1][2] + d2 * Iv[2][2]};
            const double wd = P.T->w[q] * det, g2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
#pragma unroll
            for (int f = 0; f < 3; ++f) acc[f] -= wd * (P.mu * g2 + (P.lam + P.mu) * (g[f] * g[f]));
          }
#pragma unroll
          for (int f = 0; f < 3; ++f) sum[f] += acc[f];
        }
  }
  if (face_terms && (i == 0 || i == B.m0 - 1 || j == 0 || j == B.m1 - 1 || k == 0 || k == B.m2 - 1)) {
    double r[3] = {0.0, 0.0, 0.0};
    e27_face_rows<true, false>(B, P, i, j, k, nullptr, nullptr, r);
#pragma unroll
    for (int f = 0; f < 3; ++f) sum[f] += r[0];
  }
#pragma unroll
  for (int f = 0; f < 3; ++f)
    if (sum[f] != 0.0) d[(int64_t)f * B.n_owned + node] = fabs(sum[f]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
static BopE27 e27_params(const mfem_brick_operator_s* op) {
  BopE27 P;
  memset(&P, 0, sizeof(P));
  const mfem_elasticity_params& p = op->elasticity;
  P.lam = p.lambda; P.mu = p.mu; P.tau = p.tau;
  P.penalty = p.penalty_faces; P.traction = p.traction_faces;
  const double s11 = p.sig[0], s22 = p.sig[1], s33 = p.sig[2], s23 = p.sig[3], s13 = p.sig[4], s12 = p.sig[5];
  const double sg[3][3] = {{s11, s12, s13}, {s12, s22, s23}, {s13, s23, s33}};
  memcpy(P.sg, sg, sizeof(sg));
  P.ng = op->brick->ng;
  P.T = op->tables27;
  return P;
}

template <bool RESID>
static int e27_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                      double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  const mfem_brick_s* m = op->brick;
  const BopE27 P = e27_params(op);
  const B27Volume V = b27_volume(m->ne[0], m->ne[1], m->ne[2]);
  const int64_t vgrid = b27_volume_grid(V, partials != nullptr);  // (folded onto the partial sums only when some are asked for)
  MFEM_REQUIRE(vgrid < ((int64_t)1 << 31), "too many work items for one launch");
  MFEM_REQUIRE(B.plo == 0 && B.clo == 0 && B.phi == B.m0, "the hex-27 operator runs on the whole lattice");  // (the kernels index x, y and the coordinates alike)
  MFEM_REQUIRE(e27_rule_served(m->ng), "the volume kernel's LDS block exceeds a CU's");
  const int word = g_e27_word;  // (read once per launch)
  const int waves = e27_launch_waves(m->ng, word);
  const size_t lds = e27_lds_bytes(m->ng, waves);
  MFEM_REQUIRE(waves >= E27_WAVES_MIN && lds + E27_LDS_STATIC <= E27_LDS_LIMIT, "the volume kernel's LDS block exceeds a CU's");
  hipLaunchKernelGGL(k_brick27e_product, dim3((unsigned)vgrid), dim3(64 * waves), lds, ctx->stream, B, op->tables27, V, P.lam, P.mu, x, dsc, y, alpha, beta,
                     (word & 1) ? 0 : 1, (word & 2) ? 1 : 0, dotw, partials, done_flag);
  MFEM_CHECK_LAUNCH();
  int np = partials ? V.grid : 0;
  if (bop_e27_face_launch(P.tau, P.penalty, P.traction, RESID)) {
    const int64_t count = bop_boundary_count(m->m[0], m->m[1], m->m[2]);
    const int grid = bop_face_grid(count);
    hipLaunchKernelGGL(k_brick27e_faces<RESID>, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, P, count, x, dsc, y, alpha, dotw,
                       partials ? partials + np : nullptr, done_flag);
    MFEM_CHECK_LAUNCH();
    if (partials) np += grid;
  }
  if (n_partials) *n_partials = np;
  return MFEM_OK;
}

int bop_e27_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                   double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  return e27_launch<false>(ctx, op, B, x, dsc, y, alpha, beta, dotw, partials, n_partials, done_flag);
}

int bop_e27_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) {
  const int64_t grid = bop_diagonal_grid(B.n_owned);
  MFEM_REQUIRE(grid < ((int64_t)1 << 31), "too many control points for one launch");
  const BopE27 P = e27_params(op);
  hipLaunchKernelGGL(k_brick27e_diagonal, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, P, bop_e27_face_launch(P.tau, P.penalty, 0u, false) ? 1 : 0, d);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// once per operator (never at a launch, which may sit inside a stream capture): the volume kernel's dynamic LDS goes beyond the default 64 KB
int bop_e27_prepare(int ng) {
  MFEM_REQUIRE(e27_rule_served(ng), "the volume kernel's LDS block exceeds a CU's");
  size_t most = 0;
  for (int g = 1; g <= 4; ++g)
    if (e27_rule_served(g) && e27_lds_bytes(g, e27_waves(g)) > most) most = e27_lds_bytes(g, e27_waves(g));
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_brick27e_product), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
  return MFEM_OK;
}

// K_nonlinear_func of the form: residue = K x* + f, f_(f,a) = sum_traction faces sum_q w^s N_a sig_fj n_j from the operator's current parameters
extern "C" int mfem_brick_operator_residual_elasticity(mfem_context ctx, uint64_t handle, const double* x_star, double* residue) try {
  mfem_operator_head* head = (mfem_operator_head*)(uintptr_t)handle;
  MFEM_REQUIRE(ctx && head, "null argument");
  mfem_brick_operator_s* op = bop_from_handle(handle);
  if (!op && head->kind == MFEM_OPERATOR_MESH) {  // (every operator handle starts with its kind tag)
    mfem_set_error("matrix-free brick operator: mfem_brick_operator_residual_elasticity takes a hex-27 elasticity operator (mfem_brick_operator_create_elasticity_hex27) only, not a mesh operator");
    return MFEM_ERR_UNSUPPORTED;
  }
  MFEM_REQUIRE(op, "not an operator's handle");
  MFEM_REQUIRE(op->ctx == ctx, "the operator was created on another context");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  if (op->physics != BOP_PHYSICS_ELASTICITY_HEX27) {
    mfem_set_error("matrix-free brick operator: mfem_brick_operator_residual_elasticity takes a hex-27 elasticity operator (mfem_brick_operator_create_elasticity_hex27) only");
    return MFEM_ERR_UNSUPPORTED;
  }
  MFEM_REQUIRE(x_star && residue, "null vector");
  BrickView B;  // (the refusal, the size and the rule: the handle's own checks)
  const int rc = bop_view(op, &B);
  if (rc) return rc;
  return e27_launch<true>(ctx, op, B, x_star, nullptr, residue, 1.0, 0.0, nullptr, nullptr, nullptr, nullptr);
} MFEM_API_CATCH("mfem_brick_operator_residual_elasticity")
