// Fused hex-8 assembly, linear elasticity: the matrix and residual kernels and their entry points (the scheme: hex8_thermal.hip; what both physics share
// on the device: hex8_device.h; every host decision and the tile constants: hex8_decide.h).
#include "hex8_device.h"
#include "hex8_sumfac.h"

// =================================================================================================
// Linear elasticity (examples/linear_elasticity/cantilever/3D_Script.jl:52-63), 3 fields, field-major:
//   K[(i,a),(k,b)] = -sum_q w [ lam d_iN_a d_kN_b + mu d_kN_a d_iN_b + mu delta_ik gradN_a.gradN_b ]
//                    - tau sum_q w^s N_a N_b delta_ik   on penalty faces
// i.e. the 21 _Kval_Basic launches of the reference in one pass.  Row-owner: a thread
// owns the 3 rows of its control point and accumulates them in place (exclusive => no atomics); `vals`
// must be zero on entry (the launcher memsets it).
// =================================================================================================
__global__ __launch_bounds__(MFEM_BLOCK) void k_elasticity_matrix(BrickView B, double lam, double mu, double tau,
                                                                    uint32_t penalty, int64_t T,
                                                                    double* __restrict__ vals) {
  const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= B.n_owned) return;
  int i, j, k;
  node_ijk(B, node, i, j, k);
  const int li = B.lo0[i], lj = B.lo1[j], lk = B.lo2[k];
  const int cj = B.c1[j], ck = B.c2[k];
  const int64_t cn = (int64_t)B.c0[i] * cj * ck;
  const int64_t pre = brick_prefix(B, i, j, k);
  // row (f,node) starts at f*3*T + 3*pre; block g at + g*cn
  double* row[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) row[f] = vals + (int64_t)f * 3 * T + 3 * pre;
  for (int e = 0; e < 8; ++e) {
    const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
    const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
    if (I < 0 || I >= B.ne0 || J < 0 || J >= B.ne1 || K < 0 || K >= B.ne2) continue;
    const int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
    double X[8][3];
    hex8_load_coords(B, I, J, K, X);
    // G[b][s][t] = sum_q w d_sN_a d_tN_b
    double G[8][3][3];
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int t = 0; t < 3; ++t) G[b][s][t] = 0.0;
    const int nq = B.ng * B.ng * B.ng;
    for (int q = 0; q < nq; ++q) {
      double g[8][3];
      const double wd = hex8_geom(X, q, g);
      double ga[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool me = (b == a);
        ga[0] = me ? g[b][0] : ga[0];
        ga[1] = me ? g[b][1] : ga[1];
        ga[2] = me ? g[b][2] : ga[2];
      }
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int t = 0; t < 3; ++t) G[b][s][t] += wd * ga[s] * g[b][t];
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int ni = I + (b & 1), nj = J + ((b >> 1) & 1), nk = K + (b >> 2);
      const int slot = ((ni - li) * cj + (nj - lj)) * ck + (nk - lk);
      const double tr = G[b][0][0] + G[b][1][1] + G[b][2][2];
#pragma unroll
      for (int fi = 0; fi < 3; ++fi)
#pragma unroll
        for (int fk = 0; fk < 3; ++fk) {
          double v = lam * G[b][fi][fk] + mu * G[b][fk][fi];
          if (fi == fk) v += mu * tr;
          row[fi][fk * cn + slot] -= v;
        }
    }
  }
  if (tau != 0.0 && penalty != 0u) {
    visit_boundary_faces(B, i, j, k, penalty, [&](int nd, int side, int ca, const int (&fn)[4][3], const double (&Xf)[4][3]) {
      double mab[4] = {0.0, 0.0, 0.0, 0.0};
      for (int q = 0; q < B.ng * B.ng; ++q) {
        const double ws = face_geom(Xf, q, side == 0, nullptr);
        double na = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) na = (c == ca) ? c_fN[q][c] : na;
#pragma unroll
        for (int c = 0; c < 4; ++c) mab[c] += ws * na * c_fN[q][c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int slot = ((fn[c][0] - li) * cj + (fn[c][1] - lj)) * ck + (fn[c][2] - lk);
#pragma unroll
        for (int fi = 0; fi < 3; ++fi) row[fi][fi * cn + slot] -= tau * mab[c];
      }
    });
  }
}

// Same operator, one thread per (control point, adjacent element): a workgroup owns 32 consecutive control points, its
// 256 threads integrate the 8 adjacent elements of each of them concurrently (the row-owner kernel above walks them one after
// the other and read-modify-writes global memory 576 times per thread).  The three rows of a control point are accumulated
// in LDS in eight conflict-free steps (see below; fixed summation order: a second assembly gives the same bits, the row-owner kernel's
// order is the reverse, equal to round-off) and leave as contiguous runs, every CSR value written exactly once -- no memset, no atomics,
// no colours.  128^3: 1.80 ms (profiles/r03_elasticity_matrix_steps.txt).
// G[b][s][t] = sum_q w det d_sN_a d_tN_b for the row node a = AH + 1 - ex of the thread's element
template <int AH>
__device__ __forceinline__ void el2_integrate(const double (&C)[7][3], int nq, int ex, double (&G)[8][3][3]) {
  double A[8][3][3];  // the loop's own accumulators, handed over once after the loop (accumulating into G itself makes the register allocator
                      // rotate the 72 sums through ~140 copies per pass)
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t) A[b][s][t] = 0.0;
  for (int q = 0; q < nq; ++q) {
    double g[8][3];
    const double wd = hex8_geom_trilinear(C, q, g);
    double ga[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) ga[s] = wd * (ex ? g[AH][s] : g[AH + 1][s]);
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int t = 0; t < 3; ++t) A[b][s][t] += ga[s] * g[b][t];
  }
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t) G[b][s][t] = A[b][s][t];
}
// The same sums on an AFFINE element (a parallelepiped: the bilinear and trilinear coefficients of its map vanish -- every element of make_Brick until a caller
// moves coordinates): the Jacobian is one matrix, so G[b][s][t] = det sum_mn Jinv[m][s] Jinv[n][t] M[a][b][m][n] with the reference integrals M of the
// quadrature in constant memory: 54 multiply-adds per neighbour b instead of 8 Gauss points x (148 of geometry + 75): 0.55 k against 1.8 k FP64 instructions per thread.
template <int AH>
__device__ __forceinline__ void el2_affine(const double (&C)[7][3], int ex, double (&G)[8][3][3]) {
  double J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    J[i][0] = C[0][i];
    J[i][1] = C[1][i];
    J[i][2] = C[3][i];
  }
  const double det = J[0][0] * J[1][1] * J[2][2] - J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] +
                     J[0][1] * J[1][2] * J[2][0] + J[0][2] * J[1][0] * J[2][1] - J[0][2] * J[1][1] * J[2][0];
  const double id = 1.0 / det;
  double I[3][3];
  I[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
  I[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
  I[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) * id;
  I[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) * id;
  I[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
  I[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
  I[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
  I[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) * id;
  I[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) * id;
  double Id[3][3];  // det * Jinv: the left factor
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int s = 0; s < 3; ++s) Id[m][s] = det * I[m][s];
  const double (*Ma)[3][3] = c_M[ex ? AH : AH + 1];
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    double T[3][3];  // T[s][n] = sum_m Id[m][s] M[a][b][m][n]
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int n = 0; n < 3; ++n) T[s][n] = Id[0][s] * Ma[b][0][n] + Id[1][s] * Ma[b][1][n] + Id[2][s] * Ma[b][2][n];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t) G[b][s][t] = T[s][0] * I[0][t] + T[s][1] * I[1][t] + T[s][2] * I[2][t];
  }
}
__global__ __launch_bounds__(MFEM_BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_elasticity_matrix_lds(BrickView B, double lam, double mu, double tau,
                                                                        uint32_t penalty, int64_t T, double* __restrict__ vals, int abl) {
  __shared__ double rows[3 * EL2_CH];
  __shared__ int64_t s_pre[EL2_NODES];
  __shared__ int32_t s_cn[EL2_NODES];
  // lane <-> control point, half-wave <-> adjacent element (two elements that differ in dimension 0 per wave): neighbouring lanes load
  // neighbouring elements' coordinates, and the row node of a thread inside its element is known per wave up to one bit
  const int tid = threadIdx.x, nl = tid & (EL2_NODES - 1), e = tid / EL2_NODES;
  const int64_t node = (int64_t)blockIdx.x * EL2_NODES + nl;
  const bool live = node < B.n_owned;
  for (int t = tid; t < 3 * EL2_CH; t += MFEM_BLOCK) rows[t] = 0.0;
  int i = 0, j = 0, k = 0, li = 0, lj = 0, lk = 0, cj = 1, ck = 1, cn = 0;
  if (live) {
    node_ijk(B, node, i, j, k);
    li = i > 0 ? i - 1 : 0; lj = j > 0 ? j - 1 : 0; lk = k > 0 ? k - 1 : 0;  // (closed forms of the order-1 row boxes instead of table loads: sw1_prefix, hex8_device.h)
    cj = sw1_cnt(j, B.m1); ck = sw1_cnt(k, B.m2);
    cn = sw1_cnt(i, B.m0) * cj * ck;
    if (e == 0) {
      s_pre[nl] = sw1_prefix(B, i, j, k);
      s_cn[nl] = cn;
    }
  } else if (e == 0) {
    s_pre[nl] = 0;
    s_cn[nl] = 0;
  }
  const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
  const int I = i - 1 + ex, J = j - 1 + ey, K = k - 1 + ez;
  const bool valid = live && I >= 0 && I < B.ne0 && J >= 0 && J < B.ne1 && K >= 0 && K < B.ne2;
  double G[8][3][3];
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t) G[b][s][t] = 0.0;
  if (valid) {
    double C[7][3];
    bool affine;
    {
      double X[8][3];
      hex8_load_coords_pairs(B, I, J, K, X);
      hex8_trilinear(X, C);
      affine = !(abl & 8) && hex8_is_affine(X, C);  // (bit 5 of mfem_debug_set_elasticity: every element takes the general path)
    }
    // the row node a = (1 - ex) + 2 (1 - ey) + 4 (1 - ez) of this thread in its element: (ey, ez) is the wave's, ex the half-wave's -- the
    // loop is instantiated per wave with the node pair as a constant, so its gradient is one select instead of a search through all eight
    const int nq = (abl & 4) ? 0 : B.ng * B.ng * B.ng;
    if (affine && nq > 0) {
      switch (e >> 1) {
        case 0: el2_affine<6>(C, ex, G); break;
        case 1: el2_affine<4>(C, ex, G); break;
        case 2: el2_affine<2>(C, ex, G); break;
        default: el2_affine<0>(C, ex, G); break;
      }
    } else {
    switch (e >> 1) {
      case 0: el2_integrate<6>(C, nq, ex, G); break;
      case 1: el2_integrate<4>(C, nq, ex, G); break;
      case 2: el2_integrate<2>(C, nq, ex, G); break;
      default: el2_integrate<0>(C, nq, ex, G); break;
    }
    }
  }
  __syncthreads();
  // (round 6) the LDS copy is laid out IN MEMORY ORDER -- per row field one chunk holding the nodes' rows back to back, 3 cn values each (a node's row
  // sits at 3 (pre(node) - pre(first node)), as in the value array) -- so that the write-out below is a plain linear copy with unit-stride lanes.  The old
  // layout (a fixed 243-double block per node, a half-wave per row at the write-out: 256-byte pieces, 8 bytes per lane) spent 0.54 - 0.77 of the
  // kernel's 1.50 ms issuing stores.
  const int relp = 3 * (int)(s_pre[nl] - s_pre[0]);
  double* R = rows + relp;  // + fi * EL2_CH: [block fk * cn + slot]
  // Accumulation without conflicts: in step b EVERY thread adds its element's block towards the element's node b.  The eight threads of a
  // control point sit in eight different elements (offsets e), so in one step they touch the eight different neighbours e + b -- all 256
  // threads work in every step, and a barrier orders the steps (an entry's contributions arrive by decreasing e: a fixed order, the same
  // for the two mirrored entries of a pair of control points).
  if (!(abl & 1)) {
    const int slot0 = ((I - li) * cj + (J - lj)) * ck + (K - lk);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (valid) {
        const int slot = slot0 + ((b & 1) * cj + ((b >> 1) & 1)) * ck + (b >> 2);
        double cur[3][3];
#pragma unroll
        for (int fi = 0; fi < 3; ++fi)
#pragma unroll
          for (int fk = 0; fk < 3; ++fk) cur[fi][fk] = R[fi * EL2_CH + fk * cn + slot];
        const double tr = G[b][0][0] + G[b][1][1] + G[b][2][2];
#pragma unroll
        for (int fi = 0; fi < 3; ++fi)
#pragma unroll
          for (int fk = 0; fk < 3; ++fk) {
            double v = lam * G[b][fi][fk] + mu * G[b][fk][fi];
            if (fi == fk) v += mu * tr;
            R[fi * EL2_CH + fk * cn + slot] = cur[fi][fk] - v;
          }
      }
      // steps b and b + 1 (b even) meet only in neighbours e + b == e' + b + 1, i.e. between the two threads of a control point whose
      // elements differ in dimension 0 alone: the two halves of ONE wave, whose LDS instructions execute in program order -- no barrier
      if (b & 1) __syncthreads();
      else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"), __builtin_amdgcn_wave_barrier();
    }
  }
  if (live && e == 0 && tau != 0.0 && penalty != 0u) {
    visit_boundary_faces(B, i, j, k, penalty, [&](int nd, int side, int ca, const int (&fn)[4][3], const double (&Xf)[4][3]) {
      double mab[4] = {0.0, 0.0, 0.0, 0.0};
      for (int q = 0; q < B.ng * B.ng; ++q) {
        const double ws = face_geom(Xf, q, side == 0, nullptr);
        double na = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) na = (c == ca) ? c_fN[q][c] : na;
#pragma unroll
        for (int c = 0; c < 4; ++c) mab[c] += ws * na * c_fN[q][c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int slot = ((fn[c][0] - li) * cj + (fn[c][1] - lj)) * ck + (fn[c][2] - lk);
#pragma unroll
        for (int fi = 0; fi < 3; ++fi) R[fi * EL2_CH + fi * cn + slot] -= tau * mab[c];
      }
    });
  }
  __syncthreads();
  // write-out: per row field f the chunk [3 pre(first node), 3 (pre(last) + cn(last))) of the value array = the LDS chunk f, copied with unit-stride lanes
  if (!(abl & 2)) {
    // 3 x the couplings of the block's live nodes (the nodes behind the mesh's last one carry pre = 0, cn = 0)
    const int64_t nlive = B.n_owned - (int64_t)blockIdx.x * EL2_NODES;
    const int lastlive = nlive < EL2_NODES ? (int)nlive - 1 : EL2_NODES - 1;
    const int L3 = 3 * (int)(s_pre[lastlive] + s_cn[lastlive] - s_pre[0]);
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      double* dst = vals + (int64_t)f * 3 * T + 3 * s_pre[0];
      const double* src = rows + f * EL2_CH;
      // 16 bytes per lane from the first 16-byte boundary of the destination on (a wave's store = 1 KB of one run); the odd ends by single lanes
      const int head = L3 > 0 ? (int)(((uintptr_t)dst >> 3) & 1) : 0;
      const int np = (L3 - head) >> 1;
      typedef double el2_d2 __attribute__((ext_vector_type(2)));
      for (int m = tid; m < np; m += MFEM_BLOCK) {
        const int idx = head + 2 * m;
        __builtin_nontemporal_store(el2_d2{src[idx], src[idx + 1]}, reinterpret_cast<el2_d2*>(dst + idx));
      }
      if (tid == 0 && head) __builtin_nontemporal_store(src[0], dst);
      if (tid == 64 && ((L3 - head) & 1)) __builtin_nontemporal_store(src[L3 - 1], dst + L3 - 1);
    }
  }
}

// Surface terms of the elasticity residual at control point (i, j, k): tau (0 - u_i) on penalty faces, sig_ij n_j on traction faces
// (cantilever/3D_Script.jl:60-61), added to r[3].
__device__ __forceinline__ void elasticity_face_residual(const BrickView& B, int i, int j, int k, double tau, uint32_t penalty, uint32_t traction,
                                                         double s11, double s22, double s33, double s23, double s13, double s12,
                                                         const double* __restrict__ x, double (&r)[3]) {
  const uint32_t both = penalty | traction;
  if (both != 0u) {
    const double sg[3][3] = {{s11, s12, s13}, {s12, s22, s23}, {s13, s23, s33}};
    visit_boundary_faces(B, i, j, k, both, [&](int nd, int side, int ca, const int (&fn)[4][3], const double (&Xf)[4][3]) {
      const bool pen = (penalty & face_bit(nd, side)) != 0u && tau != 0.0;
      const bool tra = (traction & face_bit(nd, side)) != 0u;
      double uf[4][3];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int f = 0; f < 3; ++f) uf[c][f] = x[brick_xindex(B, f, fn[c][0], fn[c][1], fn[c][2])];
      for (int q = 0; q < B.ng * B.ng; ++q) {
        double nrm[3];
        const double ws = face_geom(Xf, q, side == 0, nrm);
        double na = 0.0, uq[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          na = (c == ca) ? c_fN[q][c] : na;
#pragma unroll
          for (int f = 0; f < 3; ++f) uq[f] += c_fN[q][c] * uf[c][f];
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          double v = 0.0;
          if (pen) v += tau * (0.0 - uq[f]);
          if (tra) v += sg[f][0] * nrm[0] + sg[f][1] * nrm[1] + sg[f][2] * nrm[2];
          r[f] += ws * na * v;
        }
      }
    });
  }
}

// Residual at x_star (matrix-free):
//   R[(i,a)] = -sum_q w sigma_ij(u) d_jN_a + sum_q w^s N_a [ tau (0 - u_i) |penalty faces + sig_ij n_j |traction faces ]
__global__ __launch_bounds__(MFEM_BLOCK) void k_elasticity_residual(BrickView B, double lam, double mu, double tau,
                                                                      uint32_t penalty, uint32_t traction,
                                                                      double s11, double s22, double s33, double s23,
                                                                      double s13, double s12,
                                                                      const double* __restrict__ x,
                                                                      double* __restrict__ res) {
  const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= B.n_owned) return;
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
      for (int f = 0; f < 3; ++f) u[b][f] = x[brick_xindex(B, f, ni, nj, nk)];
    }
    const int nq = B.ng * B.ng * B.ng;
    for (int q = 0; q < nq; ++q) {
      double g[8][3];
      const double wd = hex8_geom(X, q, g);
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
  elasticity_face_residual(B, i, j, k, tau, penalty, traction, s11, s22, s33, s23, s13, s12, x, r);
#pragma unroll
  for (int f = 0; f < 3; ++f) res[(int64_t)f * B.n_owned + node] = r[f];
}

// The same residual in the plane-sweep form of the thermal kernels (k_thermal_residual_sweep): a workgroup owns a 15 x 15 tile of
// control points in (j, k) and sweeps it through a segment of lattice planes; per element plane, phase A: thread <-> element of the
// 16 x 16 element tile -- ONE sum-factorised integration per element (sf_elasticity_fe; the kernel above integrates an element once
// per adjacent control point: 8 x the geometry), fe[3][8] to LDS; phase B: thread <-> control point adds the four elements above
// it to what it carried over from the four below.  Fixed summation order (elements (ey, ez) ascending, lower plane first), so a slab
// computes bitwise what the global mesh computes.  Surface terms: k_elasticity_residual_faces, one thread per boundary control point.
template <int NG>
__global__ __launch_bounds__(SW_THREADS) __attribute__((amdgpu_waves_per_eu(NG == 2 ? 2 : 1))) void k_elasticity_residual_sweep(BrickView B, int L, double lam, double mu,
                                                                                                                 const double* __restrict__ x,
                                                                                                                 double* __restrict__ res) {
  __shared__ double Fe[SW_THREADS * ESW_STRIDE];
  const int tid = threadIdx.x, ek = tid % SW_E, ej = tid / SW_E;
  const SweepTile T = sweep_tile(B, L);
  if (T.i0 >= T.i1) return;
  const int J = T.tj0 - 1 + ej, K = T.tk0 - 1 + ek;  // phase A: this thread's element column
  const bool el_ok = J >= 0 && J < B.ne1 && K >= 0 && K < B.ne2;
  const int j = T.tj0 + ej, k = T.tk0 + ek;          // phase B: this thread's control point column
  const bool nd_ok = ej < SW_N && ek < SW_N && j < B.m1 && k < B.m2;
  double Xn[3][4], Un[3][4];  // the plane requested last (consumed at the top of the next step)
  const int Jc = min(max(J, 0), B.ne1 - 1), Kc = min(max(K, 0), B.ne2 - 1);  // (threads without an element column load what a neighbour loads)
  // (every thread requests on every step, from clamped positions: behind a condition the requested registers meet their old values in a phi, and the copies that resolves into wait for the loads AT ONCE -- the prefetch then costs a memory round trip per plane instead of hiding one: round 5, found in the ISA)
  auto request = [&](int ip) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t ci = brick_cindex(B, ip, Jc + (c & 1), Kc + (c >> 1));
      Xn[0][c] = B.X0[ci];
      Xn[1][c] = B.X1[ci];
      Xn[2][c] = B.X2[ci];
#pragma unroll
      for (int f = 0; f < 3; ++f) Un[f][c] = x[brick_xindex(B, f, ip, Jc + (c & 1), Kc + (c >> 1))];
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
        U[d][1][c] = Un[d][c];
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
          U[d][1][c] = Un[d][c];
        }
      double fe[3][2][4];
      sf_elasticity_fe<NG>(X, U, lam, mu, fe);
#pragma unroll
      for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          Fe[tid * ESW_STRIDE + f * 8 + 2 * c] = fe[f][0][c];
          Fe[tid * ESW_STRIDE + f * 8 + 2 * c + 1] = fe[f][1][c];
        }
    }
    request(min(max(I + 2, Ifirst), Ilast + 1));  // in flight during the rest of this plane's step: gather, write-out, barriers (mfem_lds_barrier does not wait for it)
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
        if (I >= T.i0) res[(int64_t)f * B.n_owned + (int64_t)(I - B.plo) * B.plane_len + (int64_t)j * B.m2 + k] = carry[f] + lo[f];
        carry[f] = up[f];
      }
    }
    mfem_lds_barrier();
  }
}

__global__ __launch_bounds__(MFEM_BLOCK) void k_elasticity_residual_faces(BrickView B, double tau, uint32_t penalty, uint32_t traction,
                                                                            double s11, double s22, double s33, double s23, double s13,
                                                                            double s12, const double* __restrict__ x, double* __restrict__ res) {
  int i, j, k;
  if (!boundary_point(B, i, j, k)) return;
  double r[3] = {0.0, 0.0, 0.0};
  elasticity_face_residual(B, i, j, k, tau, penalty, traction, s11, s22, s33, s23, s13, s12, x, r);
  const int64_t node = (int64_t)(i - B.plo) * B.plane_len + (int64_t)j * B.m2 + k;
#pragma unroll
  for (int f = 0; f < 3; ++f) res[(int64_t)f * B.n_owned + node] += r[f];
}

// ---- host: knobs and entry points (every decision: hex8_decide.h) ------------------------------------------------------------------------------------
static std::atomic<H8ElasticityKnobs> g_elasticity_knobs{h8_elasticity_knobs(0)};
static_assert(std::atomic<H8ElasticityKnobs>::is_always_lock_free, "the knobs are read and set without a lock");
extern "C" int mfem_debug_set_elasticity(int variant) try {
  ++mfem_debug_epoch;
  g_elasticity_knobs = h8_elasticity_knobs(variant);
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_elasticity")

extern "C" int mfem_brick_assemble_elasticity(mfem_context ctx, mfem_brick m, mfem_csr A, const mfem_elasticity_params* p,
                                              double* vals) try {
  MFEM_REQUIRE(ctx && m && A && p && vals, "null argument");
  MFEM_REQUIRE(m->p == 1, "fused elasticity assembly is implemented for hex-8 (itp_order 1)");
  MFEM_REQUIRE(A->n == 3 * m->n_owned, "pattern was not built for 3 fields on this brick");
  int rc = mfem_hex8_upload_tables(m->ng);
  if (rc) return rc;
  BrickView B = mfem_brick_view(m, 3);
  const int64_t T = A->nnz / 9;
  const H8ElasticityKnobs K = g_elasticity_knobs.load();
  if (h8_elasticity_matrix_kernel(K) == H8_EL_MATRIX_LDS) {  // one thread per (control point, element), rows accumulated in LDS, written once
    hipLaunchKernelGGL(k_elasticity_matrix_lds, dim3(h8_el2_grid(m->n_owned)), dim3(MFEM_BLOCK), 0, ctx->stream, B, p->lambda, p->mu, p->tau,
                       p->penalty_faces, T, vals, h8_elasticity_abl(K));
  } else {
    MFEM_CHECK_HIP(hipMemsetAsync(vals, 0, sizeof(double) * (size_t)A->nnz, ctx->stream));
    hipLaunchKernelGGL(k_elasticity_matrix, dim3(h8_point_grid(m->n_owned)), dim3(MFEM_BLOCK), 0, ctx->stream, B, p->lambda, p->mu, p->tau,
                       p->penalty_faces, T, vals);
  }
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
} MFEM_API_CATCH("mfem_brick_assemble_elasticity")

extern "C" int mfem_brick_residual_elasticity(mfem_context ctx, mfem_brick m, const mfem_elasticity_params* p,
                                              const double* x_star, double* residue) try {
  MFEM_REQUIRE(ctx && m && p && x_star && residue, "null argument");
  MFEM_REQUIRE(m->p == 1, "fused elasticity residual is implemented for hex-8 (itp_order 1)");
  int rc = mfem_hex8_upload_tables(m->ng);
  if (rc) return rc;
  BrickView B = mfem_brick_view(m, 3);
  if (h8_elasticity_residual_kernel(g_elasticity_knobs.load(), m->ng) == H8_EL_RESIDUAL_SWEEP) {  // one integration per element; faces by a kernel of their own
    const H8Sweep S = h8_residual_sweep(m->m[1], m->m[2], m->phi - m->plo);
    hipLaunchKernelGGL(k_elasticity_residual_sweep<2>, dim3((unsigned)S.grid), dim3(SW_THREADS), 0, ctx->stream, B, S.L, p->lambda, p->mu, x_star, residue);
    MFEM_CHECK_LAUNCH();
    if (h8_elasticity_faces_launch(p->tau, p->penalty_faces, p->traction_faces))
      hipLaunchKernelGGL(k_elasticity_residual_faces, boundary_grid(m), dim3(MFEM_BLOCK), 0, ctx->stream, B, p->tau, p->penalty_faces,
                         p->traction_faces, p->sig[0], p->sig[1], p->sig[2], p->sig[3], p->sig[4], p->sig[5], x_star, residue);
  } else {
    hipLaunchKernelGGL(k_elasticity_residual, dim3(h8_point_grid(m->n_owned)), dim3(MFEM_BLOCK), 0, ctx->stream, B, p->lambda, p->mu, p->tau,
                       p->penalty_faces, p->traction_faces, p->sig[0], p->sig[1], p->sig[2], p->sig[3], p->sig[4], p->sig[5],
                       x_star, residue);
  }
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
} MFEM_API_CATCH("mfem_brick_residual_elasticity")

