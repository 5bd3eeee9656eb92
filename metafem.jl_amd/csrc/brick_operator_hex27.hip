// The kernels of the matrix-free operator on a hex-27 (Lagrange order 2) thermal brick and their launchers: y = alpha K x~ + beta y and |diag K| for
// the K of mfem_brick_assemble_thermal on an order-2 brick -- volume term, Robin faces, Nitsche fixed_faces -- straight from the coordinates.  The
// handle, the entry points and the bind are brick_operator.hip's (bop_launch and bop_jacobi hand an operator with physics == BOP_PHYSICS_HEX27 over to
// bop27_launch / bop27_jacobi); every host decision is in brick_operator_hex27_decide.h.
//   volume  k_brick27_product: a workgroup sweeps the element planes of its segment along i over a tile of 8 x 8 element columns plus the low-side
//           halo.  A wave integrates an element with the sum-factorised stages of k_hex27<false> (assemble_hex27.hip: same decode words, same affine
//           shortcut, same prefetch of the next element's nodes; no source component) and leaves the element vector in the workgroup's LDS block; after
//           the plane's barrier the owner of a control-point column adds the <= 4 element vectors that meet in it IN A FIXED ORDER and writes the two
//           finished planes, k fastest, carrying the third into the next step.  Every control point is written once: y = alpha r + beta y (beta == 0:
//           y is not read).  No atomics, no colours: the bits do not depend on the grid, so the folded and the unfolded launch agree.
//   faces   k_brick27_product_faces: a thread per boundary control point adds alpha times its own Robin (k_hex27_faces) and Nitsche
//           (k_brick_nitsche<2>) rows, summed over the <= 4 face elements per face the point lies on.
//   diagonal k_brick27_diagonal: a thread per control point, K_ii from the <= 8 adjacent elements plus its own face terms; nothing is stored.
// The reference tables are immutable device copies per (device, rule) (bop27_tables), made when an operator is created: nothing is uploaded at a launch
// and the mutable tables of the assembly (hex27_tables()) are never read.
#include <memory>
#include "hex8_device.h"
#include "hex27.h"
#include "blas1.h"
#include "brick_operator.h"
#include "brick_operator_hex27_decide.h"

int bop27_tables(int device, int ng, const Hex27Tables** out) {
  static std::mutex mu;
  static Hex27Tables* tables[64][BRICK_MAX_NG];
  MFEM_REQUIRE(device >= 0 && device < 64 && ng >= 1 && ng <= BRICK_MAX_NG, "device or Gauss rule out of range");
  std::lock_guard<std::mutex> lk(mu);
  if (!tables[device][ng - 1]) {
    mfem_host_alloc_probe();
    std::unique_ptr<Hex27Tables> host(new Hex27Tables());
    hex27_fill_tables(ng, host.get());
    DevBuf<Hex27Tables> buf;
    MFEM_CHECK_HIP(buf.alloc(1));
    MFEM_CHECK_HIP(hipMemcpy(buf, host.get(), sizeof(Hex27Tables), hipMemcpyHostToDevice));
    tables[device][ng - 1] = buf.release();
  }
  *out = tables[device][ng - 1];
  return MFEM_OK;
}

struct Bop27 {
  double k, h, hp;
  uint32_t robin, fixed;
  int ng;
  double gp[4], gw[4];  // 1-D Gauss points / weights on [0, 1] (the Nitsche terms evaluate the host element's basis on the face)
  const Hex27Tables* T;
};

// the per-wave carve-up (brick_operator_hex27_decide.h), over the kernel's own ng and nq
#define V_X 0
#define V_T1 (27 * NI)
#define V_J 0
#define V_GX (9 * nq)
#define V_VA 0
#define V_WB b27_pad(9 * ng * ng)
#define V_T2 b27_w_t2(ng)
#define V_G V_T2
#define V_D b27_w_d(ng)

// =================================================================================================
// Volume
// =================================================================================================
// __launch_bounds__(B27_THREADS, 4): two workgroups of 8 waves must fit a CU (16 waves, 4 per SIMD: <= 128 VGPRs per lane), as for k_hex27.
__global__ __launch_bounds__(B27_THREADS, 4) void k_brick27_product(BrickView B, const Hex27Tables* __restrict__ tab, B27Volume V, double kcond,
                                                                 const double* __restrict__ x, const double* __restrict__ dsc, double* __restrict__ y,
                                                                 double alpha, double beta, int affine_fast, const double* __restrict__ dotw,
                                                                 double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  extern __shared__ double lds[];
  __shared__ double red[16];
  if (done_flag && done_flag[0]) return;
  constexpr int NI = B27_NI;
  const int ng = B.ng, nq = ng * ng * ng;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: the element walk below runs on the scalar unit)
  double* s_w = lds;
  double* s_tab1 = lds + b27_off_tab1(ng);
  int32_t* s_dec = reinterpret_cast<int32_t*>(lds + b27_off_dec(ng));
  double* Fe = lds + b27_off_fe(ng);
  double* W = lds + b27_off_waves(ng) + (size_t)wv * b27_w_size(ng);
  const int n1 = b27_n1(ng), n2 = b27_n2(ng), n3 = b27_n3(ng), nA = b27_na(ng), nB = b27_nb(ng);
  for (int i = tid; i < nq; i += B27_THREADS) s_w[i] = tab->w[i];
  for (int i = tid; i < 8 * ng; i += B27_THREADS) s_tab1[i] = tab->tab1[i / (4 * ng)][(i >> 2) % ng][i & 3];
  // decode words of the stages (k_hex27): low half = offset of the first of the 3 operands (stride NI), high half = offset of the 1-D table row
  for (int t = tid; t < n1; t += B27_THREADS) {  // T1[k][q0][a12][i] = sum_a0 tab1[k][q0][a0] X[a0 + 3 a12][i]
    const int i = t % NI, a12 = (t / NI) % 9, kq = t / (9 * NI);
    s_dec[t] = (3 * a12 * NI + i) | ((4 * kq) << 16);
  }
  for (int t = tid; t < n2; t += B27_THREADS) {  // T2[kk][q0][q1][a2][i] = sum_a1 tab1[kt][q1][a1] T1[k][q0][a1 + 3 a2][i]
    const int i = t % NI, a2 = (t / NI) % 3, q1 = (t / (3 * NI)) % ng, q0 = (t / (3 * NI * ng)) % ng, kk = t / (3 * NI * ng * ng);
    const int k = kk == 0 ? 1 : 0, kt = kk == 1 ? 1 : 0;  // kk = 0: d/dxi0, 1: d/dxi1, 2: values in both
    s_dec[n1 + t] = (((k * ng + q0) * 9 + 3 * a2) * NI + i) | ((4 * (kt * ng + q1)) << 16);
  }
  for (int t = tid; t < n3; t += B27_THREADS) {  // t < 9 nq: J[q][i][m]; then 3 nq: grad_xi T[q][m]
    int m, i, q;
    if (t < 9 * nq) {
      m = t % 3; i = (t / 3) % 3; q = t / 9;
    } else {
      m = (t - 9 * nq) % 3; i = 3; q = (t - 9 * nq) / 3;
    }
    const int q0 = q % ng, q1 = (q / ng) % ng, q2 = q / (ng * ng);
    const int kt = m == 2 ? 1 : 0;
    s_dec[n1 + n2 + t] = ((((m * ng + q0) * ng + q1) * 3) * NI + i) | ((4 * (kt * ng + q2)) << 16);
  }
  for (int t = tid; t < nA; t += B27_THREADS) {  // VA[v][q0][q1][a2] = sum_q2 tab[q2][a2] h_v[q]  (v = 2: the derivative row)
    const int a2 = t % 3, q1 = (t / 3) % ng, q0 = (t / (3 * ng)) % ng, v = t / (3 * ng * ng);
    const int qb = q0 + ng * q1;
    s_dec[n1 + n2 + n3 + t] = (3 * qb + v) | (a2 << 12) | ((v == 2 ? 1 : 0) << 14);
  }
  for (int t = tid; t < nB; t += B27_THREADS) {  // WB[w][q0][a12] = sum_q1 tab[q1][a1] VA[..]  (w = 1: D VA_1 + L VA_2)
    const int a12 = t % 9, a1 = a12 % 3, a2 = a12 / 3, q0 = (t / 9) % ng, w = t / (9 * ng);
    s_dec[n1 + n2 + n3 + nA + t] = (((w * ng + q0) * ng) * 3 + a2) | (a1 << 12) | (w << 14);
  }
  __syncthreads();
  const bool has_dsc = dsc != nullptr;
  const int ngg = ng * ng, oA = n1 + n2 + n3, oB = oA + nA;

  // node data of an element: lane a < 27 loads node a (lanes 27 .. 63 repeat node 26); issued for the NEXT element while this one is integrated.  The
  // brick is whole (bop_view refuses a slab: plo == clo == 0), so a control point has ONE index into the coordinates, x, dsc and y: the element's
  // first node (wave-uniform, scalar arithmetic) plus the lane's offset within the element.
  struct NodePre {
    double x0, x1, x2, t, d;
  };
  const int ln = lane < 27 ? lane : 26;
  const int64_t lane_off = (int64_t)(ln % 3) * B.plane_len + (int64_t)((ln / 3) % 3) * B.m2 + ln / 9;
  auto fetch_nodes = [&](int I, int J, int K) -> NodePre {
    NodePre n;
    const int64_t c = ((int64_t)(2 * I) * B.plane_len + (int64_t)(2 * J) * B.m2 + 2 * K) + lane_off;
    n.x0 = B.X0[c];
    n.x1 = B.X1[c];
    n.x2 = B.X2[c];
    n.t = x[c];
    n.d = has_dsc ? dsc[c] : 1.0;
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
    double carry = 0.0;
    // phase A: the wave's walk over (plane, element column), B27_WAVES columns apart (no division: a few scalar adds); it always holds the node data
    // of its next element
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
          W[V_X + NI * lane + 0] = cur.x0;
          W[V_X + NI * lane + 1] = cur.x1;
          W[V_X + NI * lane + 2] = cur.x2;
          W[V_X + NI * lane + 3] = has_dsc ? cur.t / cur.d : cur.t;
        }
        {  // the next element of this wave: its loads are in flight during this element's stages
          ek += B27_WAVES;
          while (ek >= nEK && ej < nEJ) { ek -= nEK; ++ej; }
          const bool more = ej < nEJ;
          const int In = more ? I : (I + 1 < it.I1 ? I + 1 : I);
          cur = fetch_nodes(In, it.J0 + (more ? ej : ej0), it.K0 + (more ? ek : ek0));
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 2'. affine elements: J is one matrix, only T goes through the stages (k_hex27's test, word for word)
        bool affine = false;
        if (affine_fast) {
          const double x0 = W[V_X + 0], y0 = W[V_X + 1], z0 = W[V_X + 2];
          const double ex0 = W[V_X + NI * 2 + 0] - x0, ey0 = W[V_X + NI * 2 + 1] - y0, ez0 = W[V_X + NI * 2 + 2] - z0;
          const double ex1 = W[V_X + NI * 6 + 0] - x0, ey1 = W[V_X + NI * 6 + 1] - y0, ez1 = W[V_X + NI * 6 + 2] - z0;
          const double ex2 = W[V_X + NI * 18 + 0] - x0, ey2 = W[V_X + NI * 18 + 1] - y0, ez2 = W[V_X + NI * 18 + 2] - z0;
          bool mine = true;
          if (lane < 27) {
            const double a0 = 0.5 * (lane % 3), a1 = 0.5 * ((lane / 3) % 3), a2 = 0.5 * (lane / 9);
            const double px = x0 + a0 * ex0 + a1 * ex1 + a2 * ex2, py = y0 + a0 * ey0 + a1 * ey1 + a2 * ey2, pz = z0 + a0 * ez0 + a1 * ez1 + a2 * ez2;
            const double mx = W[V_X + NI * lane + 0], my = W[V_X + NI * lane + 1], mz = W[V_X + NI * lane + 2];
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
            for (int u = lane; u < n1 / NI; u += 64) {
              const int t = u * NI + 3;
              const int d = s_dec[t];
              const double* xs = W + V_X + (d & 0xffff);
              const double* tb = s_tab1 + (d >> 16);
              W[V_T1 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
            }
            __builtin_amdgcn_wave_barrier();
            for (int u = lane; u < n2 / NI; u += 64) {
              const int t = u * NI + 3;
              const int d = s_dec[n1 + t];
              const double* xs = W + V_T1 + (d & 0xffff);
              const double* tb = s_tab1 + (d >> 16);
              W[V_T2 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
            }
            __builtin_amdgcn_wave_barrier();
            for (int t = 9 * nq + lane; t < n3; t += 64) {  // grad_xi T at the Gauss points
              const int d = s_dec[n1 + n2 + t];
              const double* xs = W + V_T2 + (d & 0xffff);
              const double* tb = s_tab1 + (d >> 16);
              W[V_J + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
            }
            for (int q = lane; q < nq; q += 64) {  // (rows 0 .. 9 nq: X and T1 are dead, the outputs above sit behind them)
              double* Jm = W + V_J + q * 9;
              Jm[0] = i0; Jm[1] = i1; Jm[2] = i2; Jm[3] = i3; Jm[4] = i4; Jm[5] = i5; Jm[6] = i6; Jm[7] = i7; Jm[8] = i8;
              W[V_D + q] = s_w[q] * det;
            }
          }
        }
        if (!affine) {
          // ---- 2a. J and grad_xi T at the Gauss points, sum-factorised
          for (int t = lane; t < n1; t += 64) {
            const int d = s_dec[t];
            const double* xs = W + V_X + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[V_T1 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          for (int t = lane; t < n2; t += 64) {
            const int d = s_dec[n1 + t];
            const double* xs = W + V_T1 + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[V_T2 + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          for (int t = lane; t < n3; t += 64) {
            const int d = s_dec[n1 + n2 + t];
            const double* xs = W + V_T2 + (d & 0xffff);
            const double* tb = s_tab1 + (d >> 16);
            W[V_J + t] = tb[0] * xs[0] + tb[1] * xs[NI] + tb[2] * xs[2 * NI];
          }
          __builtin_amdgcn_wave_barrier();
          // ---- 2b. det, inverse (adjugate), w det; Jinv overwrites J as [m][s]
          for (int q = lane; q < nq; q += 64) {
            double* Jm = W + V_J + q * 9;
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
            W[V_D + q] = s_w[q] * det;
          }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 3. fe[a] = sum_q w det (-k) gradN_a . gradT:  h = -k w det Jinv (Jinv^T gxi), then the transposed stages over q2, q1, q0
        for (int q = lane; q < nq; q += 64) {
          const double* Ji = W + V_J + q * 9;
          const double g0 = W[V_GX + 3 * q], g1 = W[V_GX + 3 * q + 1], g2 = W[V_GX + 3 * q + 2];
          const double t0 = g0 * Ji[0] + g1 * Ji[3] + g2 * Ji[6];
          const double t1 = g0 * Ji[1] + g1 * Ji[4] + g2 * Ji[7];
          const double t2 = g0 * Ji[2] + g1 * Ji[5] + g2 * Ji[8];
          const double sc = -kcond * W[V_D + q];
          W[V_G + 3 * q + 0] = sc * (Ji[0] * t0 + Ji[1] * t1 + Ji[2] * t2);
          W[V_G + 3 * q + 1] = sc * (Ji[3] * t0 + Ji[4] * t1 + Ji[5] * t2);
          W[V_G + 3 * q + 2] = sc * (Ji[6] * t0 + Ji[7] * t1 + Ji[8] * t2);
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < nA; t += 64) {
          const int d = s_dec[oA + t];
          const int a2 = (d >> 12) & 3, v2 = (d >> 14) & 1;
          const double* hp = W + V_G + (d & 0xfff);
          double acc = 0.0;
          for (int q2 = 0; q2 < ng; ++q2) acc += s_tab1[((v2 ? ng : 0) + q2) * 4 + a2] * hp[3 * ngg * q2];
          W[V_VA + t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < nB; t += 64) {
          const int d = s_dec[oB + t];
          const int a1 = (d >> 12) & 3, wb = (d >> 14) & 1;
          const double* va = W + V_VA + (d & 0xfff);
          double acc = 0.0;
          for (int q1 = 0; q1 < ng; ++q1) {
            const double L = s_tab1[q1 * 4 + a1], D = s_tab1[(ng + q1) * 4 + a1];
            acc += (wb ? D : L) * va[3 * q1];
            if (wb) acc += L * va[3 * ngg + 3 * q1];
          }
          W[V_WB + t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < 27) {
          const int a0 = lane % 3, a12 = lane / 3;
          double fe = 0.0;
          for (int q0 = 0; q0 < ng; ++q0)
            fe += s_tab1[(ng + q0) * 4 + a0] * W[V_WB + q0 * 9 + a12] + s_tab1[q0 * 4 + a0] * W[V_WB + (ng + q0) * 9 + a12];
          Fe[((J - it.Jb) * B27_EH + (K - it.Kb)) * 27 + lane] = fe;
        }
        __builtin_amdgcn_wave_barrier();
      }
      __syncthreads();
      // ---- phase B: the column's three planes of this element plane, the <= 4 element vectors in a fixed order (j low to high, then k)
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
          double y0 = alpha * (carry + lo), y1 = alpha * mid;
          if (beta != 0.0) {
            y0 += beta * y[node];
            y1 += beta * y[node + B.plane_len];
          }
          y[node] = y0;
          y[node + B.plane_len] = y1;
          if (dotw) dot_acc += y0 * dotw[node] + y1 * dotw[node + B.plane_len];
        }
        carry = up;
      }
      __syncthreads();  // (the next plane overwrites Fe)
    }
    if (nd_ok && it.last_seg) {  // the brick's last plane has no element above it
      const int64_t node = (int64_t)(2 * B.ne0) * B.plane_len + (int64_t)j * B.m2 + k;
      double yv = alpha * carry;
      if (beta != 0.0) yv += beta * y[node];
      y[node] = yv;
      if (dotw) dot_acc += yv * dotw[node];
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// =================================================================================================
// Face terms of row (i, j, k).  DIAG = false: sum_b K^face_ab x~_b; DIAG = true: K^face_aa.
//   Robin    sum_q w^s N_a (-h) N_b                          (k_hex27_faces: the 9 face nodes)
//   Nitsche  sum_q w^s N_a (-h_penalty N_b + k n . grad N_b)  (k_brick_nitsche<2>: the basis of ALL 27 nodes of the host element on the face)
// =================================================================================================
__device__ __forceinline__ void b27_lag2(double x, double (&L)[3], double (&dL)[3]) {
  L[0] = 2.0 * (x - 0.5) * (x - 1.0);
  L[1] = -4.0 * x * (x - 1.0);
  L[2] = 2.0 * x * (x - 0.5);
  dL[0] = 4.0 * x - 3.0;
  dL[1] = -8.0 * x + 4.0;
  dL[2] = 4.0 * x - 1.0;
}

// NITSCHE = false leaves the host element's 27 nodes out of the code: the Robin-only launch (the flagship's) keeps its nine face nodes in registers
template <bool DIAG, bool NITSCHE>
__device__ __forceinline__ double b27_face_row(const BrickView& B, const Bop27& P, int i, int j, int k, const double* __restrict__ x, const double* __restrict__ dsc) {
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
            double Xf[9][3], Tf[9];
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
              Tf[c] = DIAG ? 0.0 : bop_scaled(x, dsc, brick_xindex(B, 0, g[0], g[1], g[2]));
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
              double Tq = 0.0;
#pragma unroll
              for (int c = 0; c < 9; ++c) Tq += P.T->fN[q][c] * Tf[c];
              r += (-P.h * ws) * (na * (DIAG ? na : Tq));
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
            double X[27][3], Tn[27];
            for (int b = 0; b < 27; ++b) {
              const int gi = 2 * E[0] + b % 3, gj = 2 * E[1] + (b / 3) % 3, gk = 2 * E[2] + b / 9;
              const int64_t ci = brick_cindex(B, gi, gj, gk);
              X[b][0] = B.X0[ci];
              X[b][1] = B.X1[ci];
              X[b][2] = B.X2[ci];
              Tn[b] = DIAG ? 0.0 : bop_scaled(x, dsc, brick_xindex(B, 0, gi, gj, gk));
            }
            for (int q = 0; q < P.ng * P.ng; ++q) {
              const int q1 = q % P.ng, q2 = q / P.ng;  // first in-face coordinate fastest
              double xi[3];
              xi[nd] = side ? 1.0 : 0.0;
              xi[t1] = P.gp[q1];
              xi[t2] = P.gp[q2];
              double L[3][3], dL[3][3];
              for (int d = 0; d < 3; ++d) b27_lag2(xi[d], L[d], dL[d]);
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
              if (DIAG) {
                const double ga = dL[0][la[0]] * L[1][la[1]] * L[2][la[2]] * v[0] + L[0][la[0]] * dL[1][la[1]] * L[2][la[2]] * v[1] +
                                  L[0][la[0]] * L[1][la[1]] * dL[2][la[2]] * v[2];
                r += ws * Na * (-P.hp * Na + P.k * ga);
              } else {
                double Tq = 0.0, dTn = 0.0;
                for (int b = 0; b < 27; ++b) {
                  const int b0 = b % 3, b1 = (b / 3) % 3, b2 = b / 9;
                  const double Nb = L[0][b0] * L[1][b1] * L[2][b2];
                  const double gb = dL[0][b0] * L[1][b1] * L[2][b2] * v[0] + L[0][b0] * dL[1][b1] * L[2][b2] * v[1] + L[0][b0] * L[1][b1] * dL[2][b2] * v[2];
                  Tq += Nb * Tn[b];
                  dTn += gb * Tn[b];
                }
                r += ws * Na * (-P.hp * Tq + P.k * dTn);
              }
            }
          }
        }
    }
  }
  return r;
}

// a thread strides over the boundary control points; after the volume kernel: y += alpha (face row . x~), and the increments' partial sums of dotw . y
template <bool NITSCHE>
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick27_product_faces(BrickView B, Bop27 P, int64_t count, const double* __restrict__ x,
                                                                       const double* __restrict__ dsc, double* __restrict__ y, double alpha,
                                                                       const double* __restrict__ dotw, double* __restrict__ partials,
                                                                       const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x; t < count; t += (int64_t)gridDim.x * MFEM_BLOCK) {
    int i, j, k;
    if (!h8_boundary_point(t, 0, B.m0, B.m0 - 1, B.m1 - 1, B.m2 - 1, B.plane_len, B.m1, B.m2, i, j, k)) continue;
    const int64_t node = (int64_t)i * B.plane_len + (int64_t)j * B.m2 + k;
    const double inc = alpha * b27_face_row<false, NITSCHE>(B, P, i, j, k, x, dsc);
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
// Ke = sum_q w det (-k) |Jinv^T dN_a|^2 with J from the element's 27 nodes, then the point's own face terms.  Runs once per solve.
// =================================================================================================
__global__ __launch_bounds__(MFEM_BLOCK) void k_brick27_diagonal(BrickView B, Bop27 P, double* __restrict__ d) {
  const int64_t node = (int64_t)blockIdx.x * MFEM_BLOCK + threadIdx.x;
  if (node >= B.n_owned) return;
  int i, j, k;
  node_ijk(B, node, i, j, k);
  double sum = 0.0;
  const int nq = P.ng * P.ng * P.ng;
  if (P.k != 0.0) {
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
          double acc = 0.0;
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
            const double g0 = d0 * Iv[0][0] + d1 * Iv[1][0] + d2 * Iv[2][0];
            const double g1 = d0 * Iv[0][1] + d1 * Iv[1][1] + d2 * Iv[2][1];
            const double g2 = d0 * Iv[0][2] + d1 * Iv[1][2] + d2 * Iv[2][2];
            acc += (-P.k * P.T->w[q] * det) * (g0 * g0 + g1 * g1 + g2 * g2);
          }
          sum += acc;
        }
  }
  if (i == 0 || i == B.m0 - 1 || j == 0 || j == B.m1 - 1 || k == 0 || k == B.m2 - 1) sum += b27_face_row<true, true>(B, P, i, j, k, nullptr, nullptr);
  if (sum != 0.0) d[node] = fabs(sum);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
static const double B27_GP[4][4] = {{0.0, 0, 0, 0},
                                    {-0.57735026918962576451, 0.57735026918962576451, 0, 0},
                                    {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                    {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double B27_GW[4][4] = {{2.0, 0, 0, 0},
                                    {1.0, 1.0, 0, 0},
                                    {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                    {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};

static Bop27 bop27_params(const mfem_brick_operator_s* op) {
  Bop27 P;
  memset(&P, 0, sizeof(P));
  const mfem_thermal_params& p = op->thermal;
  P.k = p.k; P.h = p.h; P.hp = p.h_penalty;
  P.robin = p.robin_faces; P.fixed = p.fixed_faces;
  P.ng = op->brick->ng;
  P.T = op->tables27;
  for (int q = 0; q < P.ng; ++q) {
    P.gp[q] = B27_GP[P.ng - 1][q] / 2.0 + 0.5;
    P.gw[q] = B27_GW[P.ng - 1][q] / 2.0;
  }
  return P;
}

int bop27_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                 double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  const mfem_brick_s* m = op->brick;
  const Bop27 P = bop27_params(op);
  const B27Volume V = b27_volume(m->ne[0], m->ne[1], m->ne[2]);
  const int64_t vgrid = b27_volume_grid(V, partials != nullptr);  // (folded onto the partial sums only when some are asked for)
  MFEM_REQUIRE(vgrid < ((int64_t)1 << 31), "too many work items for one launch");
  MFEM_REQUIRE(B.plo == 0 && B.clo == 0 && B.phi == B.m0, "the hex-27 operator runs on the whole lattice");  // (the kernels index x, y and the coordinates alike)
  const size_t lds = b27_lds_bytes(m->ng);
  MFEM_REQUIRE(lds <= B27_LDS_LIMIT, "the volume kernel's LDS block exceeds a CU's");
  hipLaunchKernelGGL(k_brick27_product, dim3((unsigned)vgrid), dim3(B27_THREADS), lds, ctx->stream, B, op->tables27, V, P.k, x, dsc, y, alpha, beta, 1, dotw,
                     partials, done_flag);
  MFEM_CHECK_LAUNCH();
  int np = partials ? V.grid : 0;
  if (bop_face_launch(P.k, P.h, P.robin, P.hp, P.fixed)) {
    const int64_t count = bop_boundary_count(m->m[0], m->m[1], m->m[2]);
    const int grid = bop_face_grid(count);
    const auto kernel = bop_nitsche_on(P.k, P.hp, P.fixed) ? k_brick27_product_faces<true> : k_brick27_product_faces<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, P, count, x, dsc, y, alpha, dotw,
                       partials ? partials + np : nullptr, done_flag);
    MFEM_CHECK_LAUNCH();
    if (partials) np += grid;
  }
  if (n_partials) *n_partials = np;
  return MFEM_OK;
}

int bop27_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d) {
  const int64_t grid = bop_diagonal_grid(B.n_owned);
  MFEM_REQUIRE(grid < ((int64_t)1 << 31), "too many control points for one launch");
  hipLaunchKernelGGL(k_brick27_diagonal, dim3((unsigned)grid), dim3(MFEM_BLOCK), 0, ctx->stream, B, bop27_params(op), d);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// once per operator (never at a launch, which may sit inside a stream capture): the volume kernel's dynamic LDS goes beyond the default 64 KB
int bop27_prepare(int ng) {
  MFEM_REQUIRE(ng >= 1 && ng <= BRICK_MAX_NG && b27_lds_bytes(ng) <= B27_LDS_LIMIT, "the volume kernel's LDS block exceeds a CU's");
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_brick27_product), hipFuncAttributeMaxDynamicSharedMemorySize, (int)b27_lds_bytes(BRICK_MAX_NG)));
  return MFEM_OK;
}
