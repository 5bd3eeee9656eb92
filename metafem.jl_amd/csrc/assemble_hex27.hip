// hex-27 (Lagrange order 2) thermal assembly: the one place in this backend where the work is a dense GEMM,
//   Ke = B^T D B,   B[(q,s), a] = dN_a/dx_s (q)  (81 x 27),   D = diag(-k w_q det J_q),
// so it runs on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), one wave per element:
//   * the element's 27 nodal coordinates and its row descriptors are staged in per-wave LDS;
//   * the wave builds J at all quadrature points (one (q,i) row per lane), inverts it (adjugate, inv_Jac_3D),
//     and forms each MFMA fragment of B = dN/dxi * J^-1 on the fly from the reference table in LDS (3 FMAs per
//     fragment element) -- B itself is never materialised, which keeps the per-wave LDS footprint at ~9 KB
//     and lets 16 waves share a CU;
//   * Ke (27 x 27 padded to 32 x 32) = 2 x 2 accumulator tiles; the lower-left tile is the transpose of the
//     upper-right one and is not computed: 3 tiles x 21 k-steps = 63 MFMAs per element;
//   * scatter into the global CSR is race-free WITHOUT atomics through the parity colouring of the structured
//     element grid (8 colours: same-colour elements share no control point), one launch per colour -- the
//     colour-partitioned ordering BASELINE.json's north_star asks for.
// Replaces for this element type: update_BasicElements_3D (4_Update_Integrator.jl:2-33,90-154) + the three
// _Kval_Basic launches of the thermal form (06_FEM_Kernel.jl:28-45) + their 46.7 KB/element basis tables (F7).
// The matrix-free residual and the Robin faces use the same wave-per-element / thread-per-face structure with
// plain FP64 FMAs (matrix-vector work, not GEMM).
// This file: the reference tables, k_hex27, the Robin faces, the residual and the driver of the matrix paths (hex27_decide.h chooses among
// them); the other kernels: hex27_gather.hip, hex27_direct.hip, hex27_rows.hip.
#include <memory>
#include "hex27.h"

typedef double d4_t __attribute__((ext_vector_type(4)));

static Hex27Tables* g_tab = nullptr;  // (reached through hex27_tables())
static std::atomic<int> g_tab_ng{0};
const Hex27Tables* hex27_tables() { return g_tab; }

static const double GP27[4][4] = {{0.0, 0, 0, 0},
                                  {-0.57735026918962576451, 0.57735026918962576451, 0, 0},
                                  {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                  {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double GW27[4][4] = {{2.0, 0, 0, 0},
                                  {1.0, 1.0, 0, 0},
                                  {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                  {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};

static void lag2(double x, double* L, double* dL) {  // nodes 0, 1/2, 1 (102_Interpolations.jl:3-23)
  L[0] = 2.0 * (x - 0.5) * (x - 1.0);
  L[1] = -4.0 * x * (x - 1.0);
  L[2] = 2.0 * x * (x - 0.5);
  dL[0] = 4.0 * x - 3.0;
  dL[1] = -8.0 * x + 4.0;
  dL[2] = 4.0 * x - 1.0;
}

// the reference tables of ng Gauss points per direction, on the host (hex27.h: the matrix-free operator makes its own immutable copies from it)
void hex27_fill_tables(int ng, Hex27Tables* h) {
  memset(h, 0, sizeof(*h));
  double gp[4], gw[4];
  for (int i = 0; i < ng; ++i) {
    gp[i] = GP27[ng - 1][i] / 2.0 + 0.5;
    gw[i] = GW27[ng - 1][i] / 2.0;
  }
  for (int q1 = 0; q1 < ng; ++q1) lag2(gp[q1], h->tab1[0][q1], h->tab1[1][q1]);
  for (int qz = 0; qz < ng; ++qz)
    for (int qy = 0; qy < ng; ++qy)
      for (int qx = 0; qx < ng; ++qx) {
        const int q = qx + ng * (qy + ng * qz);
        double L[3][3], dL[3][3];
        lag2(gp[qx], L[0], dL[0]);
        lag2(gp[qy], L[1], dL[1]);
        lag2(gp[qz], L[2], dL[2]);
        h->w[q] = gw[qx] * gw[qy] * gw[qz];
        for (int a = 0; a < 27; ++a) {
          const int ax = a % 3, ay = (a / 3) % 3, az = a / 9;
          h->N[q][a] = L[0][ax] * L[1][ay] * L[2][az];
          h->dN[q][0][a] = dL[0][ax] * L[1][ay] * L[2][az];
          h->dN[q][1][a] = L[0][ax] * dL[1][ay] * L[2][az];
          h->dN[q][2][a] = L[0][ax] * L[1][ay] * dL[2][az];
        }
      }
  for (int q2 = 0; q2 < ng; ++q2)
    for (int q1 = 0; q1 < ng; ++q1) {
      const int q = q1 + ng * q2;
      double L1[3], d1[3], L2[3], d2[3];
      lag2(gp[q1], L1, d1);
      lag2(gp[q2], L2, d2);
      h->fw[q] = gw[q1] * gw[q2];
      for (int c = 0; c < 9; ++c) {
        const int c1 = c % 3, c2 = c / 3;
        h->fN[q][c] = L1[c1] * L2[c2];
        h->fdN[q][c][0] = d1[c1] * L2[c2];
        h->fdN[q][c][1] = L1[c1] * d2[c2];
      }
    }
  for (int a = 0; a < 3; ++a)  // 1-D integrals of the affine-element path, with THIS quadrature (what the general path sums on an element with a constant Jacobian)
    for (int b2 = 0; b2 < 3; ++b2) {
      double dd = 0.0, mm = 0.0, cc = 0.0, ct = 0.0;
      for (int q = 0; q < ng; ++q) {
        const double* L = h->tab1[0][q];
        const double* dL = h->tab1[1][q];
        dd += gw[q] * dL[a] * dL[b2];
        mm += gw[q] * L[a] * L[b2];
        cc += gw[q] * dL[a] * L[b2];
        ct += gw[q] * L[a] * dL[b2];
      }
      h->T1[0][a][b2] = dd; h->T1[1][a][b2] = mm; h->T1[2][a][b2] = cc; h->T1[3][a][b2] = ct;
    }
}

static int hex27_upload_tables(int ng) {
  static std::mutex mu;  // uploads from two host threads must not interleave (the tables themselves are process-wide: see the threading note in include/metafem_mi355x.h)
  std::lock_guard<std::mutex> lk(mu);
  if (g_tab && g_tab_ng == ng) return MFEM_OK;
  mfem_host_alloc_probe();
  std::unique_ptr<Hex27Tables> h(new Hex27Tables());
  hex27_fill_tables(ng, h.get());
  if (!g_tab) MFEM_CHECK_HIP(hipMalloc(&g_tab, sizeof(Hex27Tables)));
  MFEM_CHECK_HIP(hipMemcpy(g_tab, h.get(), sizeof(Hex27Tables), hipMemcpyHostToDevice));
  g_tab_ng = ng;
  return MFEM_OK;
}

// Walk of one wave over its elements: the elements of a launch form an n0 x n1 x n2 grid (one colour's sub-lattice, or the
// planes [e_lo, e_lo + e_cnt) of the whole mesh for the scratch path); the wave starts at running index e and advances by
// the number of waves.  The mixed-radix step is worked out once, so an advance is a few adds instead of three integer
// divisions per element.
struct ElemWalk {
  int ci, cj, ck;      // position in the launch's grid
  int si, sj, sk;      // mixed-radix digits of the stride
  int n0, n1, n2;
  int mul, o0, o1, o2; // element (I, J, K) = mul * (ci, cj, ck) + (o0, o1, o2)
  __device__ __forceinline__ void init(const BrickView& B, int colour, int e_lo, int e_cnt, int64_t e, int stride) {
    if (colour < 0) {
      n0 = e_cnt; n1 = B.ne1; n2 = B.ne2;
      mul = 1; o0 = e_lo; o1 = 0; o2 = 0;
    } else {
      o0 = e_lo + (((colour & 1) - e_lo) & 1);  // first plane of the range with the colour's parity
      o1 = (colour >> 1) & 1; o2 = colour >> 2;
      n0 = (e_lo + e_cnt - o0 + 1) >> 1; n1 = (B.ne1 - o1 + 1) >> 1; n2 = (B.ne2 - o2 + 1) >> 1;
      mul = 2;
    }
    if (n0 <= 0 || n1 <= 0 || n2 <= 0) {
      ci = 0; n0 = 0; cj = ck = si = sj = sk = 0;
      return;
    }
    const int64_t n12 = (int64_t)n1 * n2;
    ci = (int)(e / n12 < n0 ? e / n12 : n0);
    cj = (int)((e % n12) / n2);
    ck = (int)(e % n2);
    const int64_t sI = stride / n12;
    si = (int)(sI < n0 ? sI : n0);
    sj = (int)((stride % n12) / n2);
    sk = (int)(stride % n2);
  }
  __device__ __forceinline__ bool have() const { return ci < n0; }
  __device__ __forceinline__ void get(int& I, int& J, int& K) const {
    I = mul * ci + o0; J = mul * cj + o1; K = mul * ck + o2;
  }
  __device__ __forceinline__ void advance() {
    ck += sk;
    if (ck >= n2) { ck -= n2; cj += 1; }
    cj += sj;
    if (cj >= n1) { cj -= n1; ci += 1; }
    ci += si;
  }
};

// __launch_bounds__(512, 4) (second argument = waves per SIMD in HIP): two workgroups must fit a CU, i.e. <= 128 VGPRs per lane; without it the
// scatter epilogue pushed the kernel to 145 VGPRs and only ONE workgroup (2 waves per SIMD) was resident.
// SCRATCH: the two-pass variant (Ke -> element-major scratch) is its own instantiation, free of the scatter's registers.
template <bool MATRIX, bool SCRATCH = false>
__global__ __launch_bounds__(H27_THREADS, 4) void k_hex27(Hex27Args A, const double* __restrict__ xstar,
                                                        const double* __restrict__ src, double* __restrict__ out) {
  extern __shared__ double lds[];
  constexpr int NI = MATRIX ? 3 : 5;
  // workgroup-shared reference tables
  double* s_dN = lds;                           // [nqp + 1][3][27] (matrix only: MFMA operands; nqp = nq rounded up to the 4 Gauss points of a k-group,
                                                //  rows nq .. nqp zero: the k-rows past the last Gauss point and the columns past node 26 read zeros)
  double* s_w = s_dN + (MATRIX ? (H27_NQP(A.nq) + 1) * 81 : 0); // [nq]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nq = A.nq, ng = A.ng;
  double* s_tab1 = s_w + ((A.nq + 1) & ~1);     // [2][ng][4]
  int32_t* s_dec = reinterpret_cast<int32_t*>(s_tab1 + 8 * ng);
  double* wave_base = s_tab1 + 8 * ng + (h27_pad(H27_NDEC) >> 1);
  const int n1 = H27_N1, n2 = H27_N2, n3 = H27_N3;
  if (MATRIX)
    for (int i = tid; i < (H27_NQP(nq) + 1) * 81; i += H27_THREADS) s_dN[i] = i < nq * 81 ? (&A.tab->dN[0][0][0])[i] : 0.0;
  for (int i = tid; i < nq; i += H27_THREADS) s_w[i] = A.tab->w[i];
  for (int i = tid; i < 8 * ng; i += H27_THREADS) s_tab1[i] = A.tab->tab1[i / (4 * ng)][(i >> 2) % ng][i & 3];
  // decode words of the three sum-factorisation stages: low half = offset of the first of the 3 operands (stride NI),
  // high half = offset of the 1-D table row
  for (int t = tid; t < n1; t += H27_THREADS) {   // T1[k][q0][a12][i] = sum_a0 tab1[k][q0][a0] X[a0 + 3 a12][i]
    const int i = t % NI, a12 = (t / NI) % 9, kq = t / (9 * NI);
    s_dec[t] = (3 * a12 * NI + i) | ((4 * kq) << 16);
  }
  for (int t = tid; t < n2; t += H27_THREADS) {   // T2[kk][q0][q1][a2][i] = sum_a1 tab1[kt][q1][a1] T1[k][q0][a1 + 3 a2][i]
    const int i = t % NI, a2 = (t / NI) % 3, q1 = (t / (3 * NI)) % ng, q0 = (t / (3 * NI * ng)) % ng, kk = t / (3 * NI * ng * ng);
    const int k = kk == 0 ? 1 : 0, kt = kk == 1 ? 1 : 0;  // kk = 0: d/dxi0, 1: d/dxi1, 2: values in both (for d/dxi2 and values)
    s_dec[n1 + t] = (((k * ng + q0) * 9 + 3 * a2) * NI + i) | ((4 * (kt * ng + q1)) << 16);
  }
  for (int t = tid; t < n3; t += H27_THREADS) {
    // t < 9 nq:   J[q][i][m]     = sum_a2 tab1[m == 2][q2][a2] T2[m][q0][q1][a2][i]        (i < 3)
    // then 3 nq:  grad_xi T[q][m] = the same with component 3; then nq: s[q] = sum_a2 L[q2][a2] T2[2][q0][q1][a2][4]
    int m, i, q;
    if (t < 9 * nq) {
      m = t % 3; i = (t / 3) % 3; q = t / 9;
    } else if (t < 12 * nq) {
      m = (t - 9 * nq) % 3; i = 3; q = (t - 9 * nq) / 3;
    } else {
      m = 3; i = 4; q = t - 12 * nq;
    }
    const int q0 = q % ng, q1 = (q / ng) % ng, q2 = q / (ng * ng);
    const int kk = m == 3 ? 2 : m, kt = m == 2 ? 1 : 0;
    s_dec[n1 + n2 + t] = ((((kk * ng + q0) * ng + q1) * 3) * NI + i) | ((4 * (kt * ng + q2)) << 16);
  }
  if (!MATRIX) {
    // transposed stages of the residual: fe[a] = sum_q ( dN[q][a][m] h[q][m] + N[q][a] sq[q] )
    for (int t = tid; t < H27_NA; t += H27_THREADS) {  // VA[v][q0][q1][a2] = sum_q2 tab[q2][a2] h_v[q]  (v = 2: D h_2 + L sq)
      const int a2 = t % 3, q1 = (t / 3) % ng, q0 = (t / (3 * ng)) % ng, v = t / (3 * ng * ng);
      const int qb = q0 + ng * q1;
      s_dec[n1 + n2 + n3 + t] = (3 * qb + v) | (a2 << 12) | ((v == 2 ? 1 : 0) << 14) | (qb << 16);
    }
    for (int t = tid; t < H27_NB; t += H27_THREADS) {  // WB[w][q0][a12] = sum_q1 tab[q1][a1] VA[..]  (w = 1: D VA_1 + L VA_2)
      const int a12 = t % 9, a1 = a12 % 3, a2 = a12 / 3, q0 = (t / 9) % ng, w = t / (9 * ng);
      s_dec[n1 + n2 + n3 + H27_NA + t] = (((w * ng + q0) * ng) * 3 + a2) | (a1 << 12) | (w << 14);
    }
  }
  double* W = wave_base + (size_t)wv * W_SIZE(MATRIX && !SCRATCH);
  if (MATRIX)  // G rows of the padding Gauss points nq .. nqp - 1: multiplied by the table's zero rows, so they only have to be finite -- cleared once
    for (int t = lane; t < 9 * (H27_NQP(nq) - nq); t += 64) W[W_J + 9 * nq + t] = 0.0;  // (later writes to this space are stage-2 sums: finite)
  __syncthreads();
  const BrickView& B = A.B;
  int64_t* rowbase = reinterpret_cast<int64_t*>(W + W_INFO);
  int32_t* info = reinterpret_cast<int32_t*>(W + W_INFO + 27);
  const int nwaves = gridDim.x * H27_WAVES;

  // Node data of an element (lane a < 27: coordinates of node a and, for the scatter, its CSR row descriptor).  The loads
  // of element e + nwaves are issued while element e is still being integrated and land in registers; they are written
  // to the wave's LDS block at the top of the next iteration, so their latency (three dependent table lookups + the
  // coordinate loads) never sits on the wave's critical path.
  struct NodePre {
    double x0, x1, x2;
    int64_t rb;
    int32_t s1, c2;
  };
  // (every lane loads -- lanes 27 .. 63 repeat node 26 -- and the wave fetches on every step, the last one repeating its element: behind a condition the
  // loaded registers meet zeros / their old values in a phi, and the copies that resolves into wait for the loads at once -- the prefetch would hide nothing)
  auto fetch_nodes = [&](int I, int J, int K) -> NodePre {
    NodePre n{0.0, 0.0, 0.0, 0, 0, 0};
    {
      const int ln = lane < 27 ? lane : 26;
      const int gi = 2 * I + ln % 3, gj = 2 * J + (ln / 3) % 3, gk = 2 * K + ln / 9;
      const int64_t c = brick_cindex(B, gi, gj, gk);
      n.x0 = B.X0[c];
      n.x1 = B.X1[c];
      n.x2 = B.X2[c];
      if (MATRIX && !SCRATCH) {
        // slot(a, b) = rowbase[a] + gi_b * s1_a + gj_b * s2_a + gk_b   with the row's box origin folded into rowbase
        const int c1 = B.c1[gj];
        n.c2 = B.c2[gk];
        const int64_t s1 = (int64_t)c1 * n.c2;
        n.s1 = (int32_t)s1;
        n.rb = brick_prefix(B, gi, gj, gk) - ((int64_t)B.lo0[gi] * s1 + (int64_t)B.lo1[gj] * n.c2 + B.lo2[gk]);
      }
    }
    return n;
  };
  int I = 0, J = 0, K = 0;
  ElemWalk walk;
  walk.init(B, A.colour, A.e_lo, A.e_cnt, (int64_t)blockIdx.x * H27_WAVES + wv, nwaves);
  // list mode (mixed meshes): the wave walks the entries lk, lk + nwaves, ... of the element list instead of the launch's grid
  int64_t lk = (int64_t)blockIdx.x * H27_WAVES + wv, lk_cur = 0;
  auto list_get = [&](int64_t k, int& I_, int& J_, int& K_) {
    const uint32_t id = (uint32_t)A.elist[k], n2 = (uint32_t)B.ne2, n12 = (uint32_t)B.ne1 * n2;
    const uint32_t i = id / n12, rem = id - i * n12, j = rem / n2;
    I_ = A.e_lo + (int)i; J_ = (int)j; K_ = (int)(rem - j * n2);
  };
  bool have = A.elist ? lk < A.ecount : walk.have();  // wave-uniform
  if (have) {
    if (A.elist) list_get(lk, I, J, K); else walk.get(I, J, K);
  }
  NodePre cur = fetch_nodes(have ? I : A.e_lo, have ? J : 0, have ? K : 0);  // (a wave without an element loads the first one of the launch's planes: inside the slab's coordinates)
  while (have) {
    // ---- 1. nodes: coordinates + row descriptors (matrix) / nodal values (residual)
    if (lane < 27) {
      W[W_X + NI * lane + 0] = cur.x0;
      W[W_X + NI * lane + 1] = cur.x1;
      W[W_X + NI * lane + 2] = cur.x2;
      const int gi = 2 * I + lane % 3, gj = 2 * J + (lane / 3) % 3, gk = 2 * K + lane / 9;
      if (MATRIX && SCRATCH) {
        // two-pass path: no row descriptors needed
      } else if (MATRIX) {
        rowbase[lane] = cur.rb;
        int32_t* in = info + 8 * lane;
        in[0] = cur.s1; in[1] = cur.c2;
        in[5] = gi; in[6] = gj; in[7] = gk;
      } else {
        const int64_t xi = brick_xindex(B, 0, gi, gj, gk);
        W[W_X + NI * lane + 3] = xstar[xi];
        W[W_X + NI * lane + (NI - 1)] = src ? src[xi] : 0.0;
      }
    }
    // next element of this wave: issue its node loads now
    const int Ic = I, Jc = J, Kc = K;
    lk_cur = lk;
    if (A.elist) {
      lk += nwaves;
      have = lk < A.ecount;
      if (have) list_get(lk, I, J, K);
    } else {
      walk.advance();
      have = walk.have();
      if (have) walk.get(I, J, K);
    }
    cur = fetch_nodes(I, J, K);  // (I, J, K keep the last element when the walk is over)
    __builtin_amdgcn_wave_barrier();
    // ---- 2'. AFFINE elements (round 4).  The counters say pass 1 is bound by the ONE pipe FP64 VALU and FP64 MFMA share (MFMA busy 53 % + FP64 /
    //      integer VALU 33 % of the SIMD cycles: profiles/r04_hex27_wave_counters.txt), and ~45 % of an element's 560 VALU instructions are the
    //      sum-factorised Jacobian, its adjugate and det at 27 Gauss points.  When the element's 27 nodes are an affine image of the reference
    //      nodes -- every element of make_Brick until a caller moves coordinates (mfem_brick_coords) -- J is one matrix: G_q = w_q G0 with
    //      G0 = -k adj(J) adj(J)^T / det, 6 numbers computed once.  The test is made per element on the coordinates themselves (lane a against
    //      x(0) + a0 e0 / 2 + a1 e1 / 2 + a2 e2 / 2 with the edge vectors e_m = x(corner m) - x(0)), to 16 ulp of the coordinates' magnitude:
    //      what J's own cancellation error is made of.  Anything else takes the general path below; both give G to round-off of each other.
    bool affine = false;
    if (A.affine_fast) {
      const double x0 = W[W_X + 0], y0 = W[W_X + 1], z0 = W[W_X + 2];
      const double ex0 = W[W_X + NI * 2 + 0] - x0, ey0 = W[W_X + NI * 2 + 1] - y0, ez0 = W[W_X + NI * 2 + 2] - z0;     // node (2,0,0): d x / d xi0
      const double ex1 = W[W_X + NI * 6 + 0] - x0, ey1 = W[W_X + NI * 6 + 1] - y0, ez1 = W[W_X + NI * 6 + 2] - z0;     // node (0,2,0): d x / d xi1
      const double ex2 = W[W_X + NI * 18 + 0] - x0, ey2 = W[W_X + NI * 18 + 1] - y0, ez2 = W[W_X + NI * 18 + 2] - z0;  // node (0,0,2): d x / d xi2
      bool mine = true;
      if (lane < 27) {
        const double a0 = 0.5 * (lane % 3), a1 = 0.5 * ((lane / 3) % 3), a2 = 0.5 * (lane / 9);
        const double px = x0 + a0 * ex0 + a1 * ex1 + a2 * ex2, py = y0 + a0 * ey0 + a1 * ey1 + a2 * ey2, pz = z0 + a0 * ez0 + a1 * ez1 + a2 * ez2;
        const double mx = W[W_X + NI * lane + 0], my = W[W_X + NI * lane + 1], mz = W[W_X + NI * lane + 2];
        const double tol = 3.6e-15;  // 16 ulp of the largest coordinate magnitude the element spans, per component
        mine = fabs(mx - px) <= tol * (fabs(x0) + fabs(ex0) + fabs(ex1) + fabs(ex2)) &&
               fabs(my - py) <= tol * (fabs(y0) + fabs(ey0) + fabs(ey1) + fabs(ey2)) &&
               fabs(mz - pz) <= tol * (fabs(z0) + fabs(ez0) + fabs(ez1) + fabs(ez2));
      }
      affine = __all(mine);
      if (affine && MATRIX) {
        // J[i][m] = e_m[i]; adjugate rows c_m (as in 2b), G0 = -k / det * C C^T
        const double j00 = ex0, j01 = ex1, j02 = ex2, j10 = ey0, j11 = ey1, j12 = ey2, j20 = ez0, j21 = ez1, j22 = ez2;
        const double det = j00 * j11 * j22 - j00 * j12 * j21 - j01 * j10 * j22 + j01 * j12 * j20 + j02 * j10 * j21 - j02 * j11 * j20;
        const double c00 = j11 * j22 - j12 * j21, c01 = j02 * j21 - j01 * j22, c02 = j01 * j12 - j11 * j02;
        const double c10 = j12 * j20 - j22 * j10, c11 = j00 * j22 - j02 * j20, c12 = j02 * j10 - j00 * j12;
        const double c20 = j10 * j21 - j11 * j20, c21 = j01 * j20 - j21 * j00, c22 = j00 * j11 - j10 * j01;
        const double sc0 = -A.kcond / det;
        const double g0 = sc0 * (c00 * c00 + c01 * c01 + c02 * c02), g1 = sc0 * (c00 * c10 + c01 * c11 + c02 * c12),
                     g2 = sc0 * (c00 * c20 + c01 * c21 + c02 * c22), g3 = sc0 * (c10 * c10 + c11 * c11 + c12 * c12),
                     g4 = sc0 * (c10 * c20 + c11 * c21 + c12 * c22), g5 = sc0 * (c20 * c20 + c21 * c21 + c22 * c22);
        __builtin_amdgcn_wave_barrier();  // (the reads of W_X above are done: W_J overlays it)
        for (int q = lane; q < nq; q += 64) {
          double* Jm = W + W_J + q * 9;
          const double wq = s_w[q];
          Jm[0] = wq * g0; Jm[1] = wq * g1; Jm[2] = wq * g2; Jm[3] = wq * g3; Jm[4] = wq * g4; Jm[5] = wq * g5;
        }
      }
      if (affine && !MATRIX) {
        // Residual on an affine element: only T and s (components 3, 4 of the 5 interleaved ones) go through the three sum-factorised stages -- the
        // same decode words, walked over the compact index u -> t = (u / 2) NI + 3 + (u & 1): 2 + 3 + 2 trips of 64 lanes instead of 5 + 7 + 6 --, and the
        // inverse Jacobian is one matrix, written to every Gauss point's row for the flux stage below (the general path computes 27 of them).
        const double j00 = ex0, j01 = ex1, j02 = ex2, j10 = ey0, j11 = ey1, j12 = ey2, j20 = ez0, j21 = ez1, j22 = ez2;
        const double det = j00 * j11 * j22 - j00 * j12 * j21 - j01 * j10 * j22 + j01 * j12 * j20 + j02 * j10 * j21 - j02 * j11 * j20;
        const double id = 1.0 / det;
        const double i0 = (j11 * j22 - j12 * j21) * id, i1 = (j02 * j21 - j01 * j22) * id, i2 = (j01 * j12 - j11 * j02) * id;
        const double i3 = (j12 * j20 - j22 * j10) * id, i4 = (j00 * j22 - j02 * j20) * id, i5 = (j02 * j10 - j00 * j12) * id;
        const double i6 = (j10 * j21 - j11 * j20) * id, i7 = (j01 * j20 - j21 * j00) * id, i8 = (j00 * j11 - j10 * j01) * id;
        for (int u = lane; u < 2 * (n1 / NI); u += 64) {
          const int t = (u >> 1) * NI + 3 + (u & 1);
          const int d = s_dec[t];
          const double* x = W + W_X + (d & 0xffff);
          const double* tb = s_tab1 + (d >> 16);
          W[W_T1 + t] = tb[0] * x[0] + tb[1] * x[NI] + tb[2] * x[2 * NI];
        }
        __builtin_amdgcn_wave_barrier();
        for (int u = lane; u < 2 * (n2 / NI); u += 64) {
          const int t = (u >> 1) * NI + 3 + (u & 1);
          const int d = s_dec[n1 + t];
          const double* x = W + W_T1 + (d & 0xffff);
          const double* tb = s_tab1 + (d >> 16);
          W[W_T2 + t] = tb[0] * x[0] + tb[1] * x[NI] + tb[2] * x[2 * NI];
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = 9 * nq + lane; t < n3; t += 64) {  // grad_xi T and s at the Gauss points (the J entries in front of them are not needed)
          const int d = s_dec[n1 + n2 + t];
          const double* x = W + W_T2 + (d & 0xffff);
          const double* tb = s_tab1 + (d >> 16);
          W[W_J + t] = tb[0] * x[0] + tb[1] * x[NI] + tb[2] * x[2 * NI];
        }
        for (int q = lane; q < nq; q += 64) {  // (rows 0 .. 9 nq of this space: X and T1 are dead, the outputs above sit behind them)
          double* Jm = W + W_J + q * 9;
          Jm[0] = i0; Jm[1] = i1; Jm[2] = i2; Jm[3] = i3; Jm[4] = i4; Jm[5] = i5; Jm[6] = i6; Jm[7] = i7; Jm[8] = i8;
          W[W_D + q] = s_w[q] * det;
        }
      }
    }
    if (!affine) {
    // ---- 2a. J[q][i][m] = sum_a dN[q][a][m] X[a][i], sum-factorised over the tensor-product basis
    //      (dN[q][a][0] = D(q0,a0) L(q1,a1) L(q2,a2), ...): three stages of 3-term sums through the wave's LDS block,
    //      ~2000 multiply-adds per element instead of 6561 -- FP64 VALU work runs on the same pipe as the FP64 MFMAs
    //      on this chip (the phase ablation is additive), so every VALU instruction saved here is matrix-core time.
    {
      for (int t = lane; t < n1; t += 64) {
        const int d = s_dec[t];
        const double* x = W + W_X + (d & 0xffff);
        const double* tb = s_tab1 + (d >> 16);
        W[W_T1 + t] = tb[0] * x[0] + tb[1] * x[NI] + tb[2] * x[2 * NI];
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = lane; t < n2; t += 64) {
        const int d = s_dec[n1 + t];
        const double* x = W + W_T1 + (d & 0xffff);
        const double* tb = s_tab1 + (d >> 16);
        W[W_T2 + t] = tb[0] * x[0] + tb[1] * x[NI] + tb[2] * x[2 * NI];
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = lane; t < n3; t += 64) {
        const int d = s_dec[n1 + n2 + t];
        const double* x = W + W_T2 + (d & 0xffff);
        const double* tb = s_tab1 + (d >> 16);
        W[W_J + t] = tb[0] * x[0] + tb[1] * x[NI] + tb[2] * x[2 * NI];
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- 2b. det, inverse (adjugate, inv_Jac_3D), w det ; Jinv overwrites J as [m][s]
    for (int q = lane; q < nq; q += 64) {
      double* Jm = W + W_J + q * 9;
      const double j00 = Jm[0], j01 = Jm[1], j02 = Jm[2], j10 = Jm[3], j11 = Jm[4], j12 = Jm[5], j20 = Jm[6], j21 = Jm[7],
                   j22 = Jm[8];
      const double det = j00 * j11 * j22 - j00 * j12 * j21 - j01 * j10 * j22 + j01 * j12 * j20 + j02 * j10 * j21 - j02 * j11 * j20;
      if (MATRIX) {
        // matrix: only G = -k w det Jinv Jinv^T (symmetric 3 x 3) is needed: Ke = sum_q dN_q G_q dN_q^T
        const double c00 = j11 * j22 - j12 * j21, c01 = j02 * j21 - j01 * j22, c02 = j01 * j12 - j11 * j02;
        const double c10 = j12 * j20 - j22 * j10, c11 = j00 * j22 - j02 * j20, c12 = j02 * j10 - j00 * j12;
        const double c20 = j10 * j21 - j11 * j20, c21 = j01 * j20 - j21 * j00, c22 = j00 * j11 - j10 * j01;
        const double sc = -A.kcond * s_w[q] / det;
        Jm[0] = sc * (c00 * c00 + c01 * c01 + c02 * c02);
        Jm[1] = sc * (c00 * c10 + c01 * c11 + c02 * c12);
        Jm[2] = sc * (c00 * c20 + c01 * c21 + c02 * c22);
        Jm[3] = sc * (c10 * c10 + c11 * c11 + c12 * c12);
        Jm[4] = sc * (c10 * c20 + c11 * c21 + c12 * c22);
        Jm[5] = sc * (c20 * c20 + c21 * c21 + c22 * c22);
        continue;
      }
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
      W[W_D + q] = s_w[q] * det;
    }
    }  // !affine
    __builtin_amdgcn_wave_barrier();
    if (MATRIX) {
      // ---- 3. Ke = B^T D B on the matrix cores.  MFMA fragments are formed on the fly:
      //      lane (k = lane>>4, c = lane&15) of k-step ks holds row r = 4 ks + k of B at columns c and c + 16,
      //      B[(q,s)][a] = sum_m dN[q][a][m] Jinv[q][m][s]; the A operand is the same row scaled by -k w det.
      d4_t C00 = {0, 0, 0, 0}, C01 = {0, 0, 0, 0}, C11 = {0, 0, 0, 0};
      const int c = lane & 15, kl = lane >> 4;
      const bool hi_ok = (c + 16) < 27;
      // Ke = sum_q dN_q G_q dN_q^T: k-row (q, n) has the B operand dN[q][b][n] straight from the table and the A operand
      // sum_m dN[q][a][m] G_q[m][n] (3 FMAs).  The order of the 3 nq rows along k is free: k-steps 3 g + n (n = 0..2) carry
      // the rows (q = 4 g + kl, n), so a lane keeps one Gauss point for three steps and reads its six table entries and the
      // six entries of G once per group (12 LDS words per group; the first version read 30).
      // Branch-free k-groups (round 4): the k-rows past the last Gauss point read zero rows of the table (and the finite filler behind G), the
      // lanes whose second column block lies past node 26 read the table's zero row with stride 0 -- no per-group zeroing of 24 registers, no
      // exec-mask regions between the LDS reads and the MFMAs.
      const int ngroups = H27_NQP(nq) >> 2;
      const double* dn0 = s_dN + kl * 81 + c;
      const double* dn1 = hi_ok ? dn0 + 16 : s_dN + H27_NQP(nq) * 81;
      const int st1 = hi_ok ? 4 * 81 : 0;
      const double* Gq = W + W_J + kl * 9;
      for (int g = 0; g < ngroups; ++g) {
        const double d0[3] = {dn0[0], dn0[27], dn0[54]};
        const double d1[3] = {dn1[0], dn1[27], dn1[54]};
        const double G[3][3] = {{Gq[0], Gq[1], Gq[2]}, {Gq[1], Gq[3], Gq[4]}, {Gq[2], Gq[4], Gq[5]}};
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          const double a0 = d0[0] * G[0][n] + d0[1] * G[1][n] + d0[2] * G[2][n];
          const double a1 = d1[0] * G[0][n] + d1[1] * G[1][n] + d1[2] * G[2][n];
          C00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, d0[n], C00, 0, 0, 0);
          C01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, d1[n], C01, 0, 0, 0);
          C11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, d1[n], C11, 0, 0, 0);
        }
        dn0 += 4 * 81;
        dn1 += st1;
        Gq += 36;
      }
      if (SCRATCH) {
        // ---- 4'. two-pass assembly: Ke goes to the element-major scratch [e][a][b] (written once, no RMW); the
        //      row-owner gather (hex27_gather.hip) turns it into CSR rows.
        double* ke = A.elist ? out + lk_cur * 729 : out + (((int64_t)(Ic % A.ring) * B.ne1 + Jc) * B.ne2 + Kc) * 729;
        const int rc_hi = scratch_row(16 + c > 26 ? 26 : 16 + c);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int ra = kl + 4 * reg;
          if (ra < 27) {
            const int r0 = scratch_row(ra);
            ke[r0 * 27 + c] = C00[reg];
            if (hi_ok) {
              ke[r0 * 27 + 16 + c] = C01[reg];
              ke[rc_hi * 27 + ra] = C01[reg];
            }
          }
          if (16 + ra < 27 && hi_ok) ke[scratch_row(16 + ra) * 27 + 16 + c] = C11[reg];
        }
        __builtin_amdgcn_wave_barrier();
        continue;
      }
      // ---- 4. colour-safe scatter: 16 entries per lane in two batches of 8 (register budget: 128 VGPRs = 4 waves per
      //      SIMD); all slots of one element are distinct, so a batch's loads are issued together, then its stores
      //      (plain read-modify-write, no atomics).
      const int rq = kl;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        int64_t slot[8];
        double val[8];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int reg = 2 * half + rr;
          const int ra = rq + 4 * reg;  // f64 MFMA C/D map: row = (lane>>4) + 4*reg, col = lane & 15
          const int aa[4] = {ra, ra, 16 + c, 16 + ra};
          const int bb[4] = {c, 16 + c, ra, 16 + c};  // tiles (0,0), (0,1), (1,0) = transpose of (0,1), (1,1)
          const double vv[4] = {C00[reg], C01[reg], C01[reg], C11[reg]};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int _a = aa[t], _b = bb[t];
            int64_t sl = -1;
            if (_a < 27 && _b < 27) {
              const int32_t* ia = info + 8 * _a;
              const int32_t* ib = info + 8 * _b;
              sl = rowbase[_a] + (int64_t)ib[5] * ia[0] + (int64_t)ib[6] * ia[1] + ib[7];
            }
            slot[4 * rr + t] = sl;
            val[4 * rr + t] = vv[t];
          }
        }
        if (A.colour == -2) {
          // atomics variant (what the reference's _Kval_Basic does, 06_FEM_Kernel.jl:41): all elements in one launch,
          // FP64 adds resolved in L2, nothing returns to the wave; summation order (and so the last bit) is not fixed
#pragma unroll
          for (int t = 0; t < 8; ++t)
            if (slot[t] >= 0) unsafeAtomicAdd(out + slot[t], val[t]);
          continue;
        }
        double old[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) old[t] = slot[t] >= 0 ? out[slot[t]] : 0.0;
#pragma unroll
        for (int t = 0; t < 8; ++t)
          if (slot[t] >= 0) out[slot[t]] = old[t] + val[t];
      }
    } else {
      // ---- 3'. residual: fe[a] = sum_q w det ( -k gradN_a . gradT + N_a s_q )
      //      gradN_a . gradT = sum_m dN[q][a][m] h[q][m],  h = Jinv (Jinv^T gxi),  gxi[m] = sum_b dN[q][b][m] T_b.
      //      gxi and s at the Gauss points came out of the sum-factorised stages above (components 3 and 4).
      for (int q = lane; q < nq; q += 64) {  // lanes q: gradT = Jinv^T gxi ; h = -k w det * Jinv gradT ; source
        const double* Ji = W + W_J + q * 9;
        const double g0 = W[W_GX + 3 * q], g1 = W[W_GX + 3 * q + 1], g2 = W[W_GX + 3 * q + 2];
        const double t0 = g0 * Ji[0] + g1 * Ji[3] + g2 * Ji[6];
        const double t1 = g0 * Ji[1] + g1 * Ji[4] + g2 * Ji[7];
        const double t2 = g0 * Ji[2] + g1 * Ji[5] + g2 * Ji[8];
        const double wd = W[W_D + q], sc = -A.kcond * wd;
        W[W_G + 3 * q + 0] = sc * (Ji[0] * t0 + Ji[1] * t1 + Ji[2] * t2);
        W[W_G + 3 * q + 1] = sc * (Ji[3] * t0 + Ji[4] * t1 + Ji[5] * t2);
        W[W_G + 3 * q + 2] = sc * (Ji[6] * t0 + Ji[7] * t1 + Ji[8] * t2);
        W[W_G + 3 * h27_pad(nq) + q] = W[W_SV + q] * wd;
      }
      __builtin_amdgcn_wave_barrier();
      // the contraction with dN / N, transposed sum factorisation: over q2, then q1, then q0
      const int oA = n1 + n2 + n3, oB = oA + H27_NA, ngg = ng * ng;
      for (int t = lane; t < H27_NA; t += 64) {
        const int d = s_dec[oA + t];
        const int a2 = (d >> 12) & 3, v2 = (d >> 14) & 1;
        const double* hp = W + W_G + (d & 0xfff);
        const double* sp = W + W_G + 3 * h27_pad(nq) + (d >> 16);
        double acc = 0.0;
        for (int q2 = 0; q2 < ng; ++q2) {
          const double L = s_tab1[q2 * 4 + a2], D = s_tab1[(ng + q2) * 4 + a2];
          acc += (v2 ? D : L) * hp[3 * ngg * q2];
          if (v2) acc += L * sp[ngg * q2];
        }
        W[W_VA + t] = acc;
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = lane; t < H27_NB; t += 64) {
        const int d = s_dec[oB + t];
        const int a1 = (d >> 12) & 3, w = (d >> 14) & 1;
        const double* va = W + W_VA + (d & 0xfff);
        double acc = 0.0;
        for (int q1 = 0; q1 < ng; ++q1) {
          const double L = s_tab1[q1 * 4 + a1], D = s_tab1[(ng + q1) * 4 + a1];
          acc += (w ? D : L) * va[3 * q1];
          if (w) acc += L * va[3 * ngg + 3 * q1];
        }
        W[W_WB + t] = acc;
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < 27) {
        const int a0 = lane % 3, a12 = lane / 3;
        double fe = 0.0;
        for (int q0 = 0; q0 < ng; ++q0)
          fe += s_tab1[(ng + q0) * 4 + a0] * W[W_WB + q0 * 9 + a12] + s_tab1[q0 * 4 + a0] * W[W_WB + (ng + q0) * 9 + a12];
        const int gi = 2 * Ic + lane % 3, gj = 2 * Jc + (lane / 3) % 3, gk = 2 * Kc + lane / 9;
        if (gi >= B.plo && gi < B.phi) out[(int64_t)(gi - B.plo) * B.plane_len + (int64_t)gj * B.m2 + gk] += fe;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- Robin faces (hex-27): one thread per (boundary face element, face node a) = one row of the 9 x 9 face matrix;
// 9 face nodes, ng x ng Gauss points.  colour = parity of the face element in its two tangential directions; the two
// opposite faces of a direction share no node and go into the same launch (side = -1): 4 launches per direction.

template <bool MATRIX>
__global__ __launch_bounds__(MFEM_BLOCK) void k_hex27_faces(Face27Args A, const double* __restrict__ xstar,
                                                              double* __restrict__ out) {
  const BrickView& B = A.B;
  const int ne[3] = {B.ne0, B.ne1, B.ne2};
  const int t1 = (A.nd + 1) % 3, t2 = (A.nd + 2) % 3;
  const int c1 = A.colour & 1, c2 = A.colour >> 1;
  const int n1 = (ne[t1] - c1 + 1) >> 1, n2 = (ne[t2] - c2 + 1) >> 1;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int a = (int)(tid % 9);
  int64_t f = tid / 9;
  int side = A.side;
  if (side < 0) {
    side = (int)(f & 1);
    f >>= 1;
  }
  if (n1 <= 0 || n2 <= 0 || f >= (int64_t)n1 * n2) return;
  int E[3];
  E[A.nd] = side ? ne[A.nd] - 1 : 0;
  E[t1] = 2 * (int)(f % n1) + c1;
  E[t2] = 2 * (int)(f / n1) + c2;
  if (A.nd == 0) {  // slab: the face lies in one control-point plane, the tangential faces span three
    const int gp = side ? 2 * ne[0] : 0;
    if (gp < B.plo || gp >= B.phi) return;
  } else if (2 * E[0] + 2 < B.plo || 2 * E[0] >= B.phi) {
    return;
  }
  int g[9][3];
  double Xf[9][3], Tf[9];
  for (int c = 0; c < 9; ++c) {
    g[c][A.nd] = side ? 2 * ne[A.nd] : 0;
    g[c][t1] = 2 * E[t1] + c % 3;
    g[c][t2] = 2 * E[t2] + c / 3;
    const int64_t ci = brick_cindex(B, g[c][0], g[c][1], g[c][2]);
    Xf[c][0] = B.X0[ci];
    Xf[c][1] = B.X1[ci];
    Xf[c][2] = B.X2[ci];
    if (!MATRIX) Tf[c] = xstar[brick_xindex(B, 0, g[c][0], g[c][1], g[c][2])];
  }
  {
    if (g[a][0] < B.plo || g[a][0] >= B.phi) return;  // only owned rows
    double macc[9];
    for (int b = 0; b < 9; ++b) macc[b] = 0.0;
    double racc = 0.0;
    for (int q = 0; q < A.ng * A.ng; ++q) {
      double ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0};
      for (int c = 0; c < 9; ++c)
        for (int i = 0; i < 3; ++i) {
          ta[i] += A.tab->fdN[q][c][0] * Xf[c][i];
          tb[i] += A.tab->fdN[q][c][1] * Xf[c][i];
        }
      const double r0 = ta[1] * tb[2] - ta[2] * tb[1], r1 = -ta[0] * tb[2] + ta[2] * tb[0], r2 = ta[0] * tb[1] - ta[1] * tb[0];
      const double ws = A.tab->fw[q] * sqrt(r0 * r0 + r1 * r1 + r2 * r2);
      const double na = A.tab->fN[q][a];
      if (MATRIX) {
        for (int b = 0; b < 9; ++b) macc[b] += -A.h * ws * na * A.tab->fN[q][b];
      } else {
        double Tq = 0.0;
        for (int c = 0; c < 9; ++c) Tq += A.tab->fN[q][c] * Tf[c];
        racc += ws * na * A.h * (A.Tenv - Tq);
      }
    }
    if (MATRIX) {
      const int gi = g[a][0], gj = g[a][1], gk = g[a][2];
      const int64_t base = brick_prefix(B, gi, gj, gk);
      const int lo0 = B.lo0[gi], lo1 = B.lo1[gj], lo2 = B.lo2[gk], cc1 = B.c1[gj], cc2 = B.c2[gk];
      for (int b = 0; b < 9; ++b)
        out[base + ((int64_t)(g[b][0] - lo0) * cc1 + (g[b][1] - lo1)) * cc2 + (g[b][2] - lo2)] += macc[b];
    } else {
      out[(int64_t)(g[a][0] - B.plo) * B.plane_len + (int64_t)g[a][1] * B.m2 + g[a][2]] += racc;
    }
  }
}

// The knob word of mfem_debug_set_hex27, decoded where it is used (h27_knobs: hex27_decide.h); 0 = every default
static std::atomic<int> g_hex27_word{0};
static std::atomic<long long> g_hex27_direct_count{0};  // assemblies that took the scratch-free path (tests)
extern "C" int64_t mfem_debug_hex27_direct_count(void) { return g_hex27_direct_count; }
static std::atomic<long long> g_hex27_mixed_count{0};  // assemblies that took the per-element choice with at least one stored element (tests)
extern "C" int64_t mfem_debug_hex27_mixed_count(void) { return g_hex27_mixed_count; }
static std::atomic<long long> g_hex27_rows_count{0};  // assemblies that took the row-owner kernel of general elements (tests)
extern "C" int64_t mfem_debug_hex27_rows_count(void) { return g_hex27_rows_count; }
extern "C" int mfem_debug_set_hex27(int two_pass) try {
  ++mfem_debug_epoch;
  g_hex27_word = two_pass;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_hex27")

// What the stages of one assembly share: the element planes [elo, ehi) that touch the owned control-point planes, the dynamic LDS of k_hex27
struct Hex27Job {
  mfem_context_s* ctx;
  mfem_brick_s* m;
  const mfem_thermal_params* p;
  BrickView B;
  H27Knobs K;
  int elo, ehi, nq;
  size_t lds;
};

// the Robin faces, matrix or residual: the launches of h27_face_schedule
static int hex27_launch_faces(const Hex27Job& J, bool matrix, const double* xstar, double* out) {
  H27FaceLaunch sched[24];
  const int n = h27_face_schedule(J.p->robin_faces, J.p->h, J.m->ne, sched);
  for (int i = 0; i < n; ++i) {
    const H27FaceLaunch& F = sched[i];
    Face27Args A{J.B, g_tab, J.p->h, J.p->Tenv, F.nd, F.side, F.colour, J.m->ng};
    if (matrix)
      hipLaunchKernelGGL(k_hex27_faces<true>, dim3(F.grid), dim3(MFEM_BLOCK), 0, J.ctx->stream, A, xstar, out);
    else
      hipLaunchKernelGGL(k_hex27_faces<false>, dim3(F.grid), dim3(MFEM_BLOCK), 0, J.ctx->stream, A, xstar, out);
    MFEM_CHECK_LAUNCH();
  }
  return MFEM_OK;
}

// One launch per parity colour of the structured element grid: same-colour elements share no control point, so the waves add into `out` (matrix
// values / residual) with plain read-modify-write.  2 workgroups (16 waves) per CU, persistent over the colour's elements.
template <bool MATRIX>
static int hex27_launch_colours(const Hex27Job& J, const double* xstar, const double* src, double* out) {
  for (int colour = 0; colour < 8; ++colour) {
    const int64_t ne = hex27_colour_count(J.m->ne[1], J.m->ne[2], colour, J.elo, J.ehi);
    if (ne <= 0) continue;
    Hex27Args A{J.B, g_tab, J.p->k, J.K.affine, colour, J.nq, J.m->ng, J.elo, J.ehi - J.elo, 1};
    hipLaunchKernelGGL(k_hex27<MATRIX>, dim3(h27_wave_grid(ne, J.ctx->num_cus)), dim3(H27_THREADS), J.lds, J.ctx->stream, A, xstar, src, out);
    MFEM_CHECK_LAUNCH();
  }
  return MFEM_OK;
}

// FP64 atomics (what the reference's _Kval_Basic does): all elements in one launch
static int hex27_assemble_atomics(const Hex27Job& J, int64_t nnz, double* vals) {
  MFEM_CHECK_HIP(hipMemsetAsync(vals, 0, sizeof(double) * (size_t)nnz, J.ctx->stream));
  const int64_t nel = (int64_t)J.m->ne[0] * J.m->ne[1] * J.m->ne[2];
  Hex27Args A{J.B, g_tab, J.p->k, J.K.affine, -2, J.nq, J.m->ng, 0, J.m->ne[0], 1};
  hipLaunchKernelGGL(k_hex27<true>, dim3(h27_wave_grid(nel, J.ctx->num_cus)), dim3(H27_THREADS), J.lds, J.ctx->stream, A, nullptr, nullptr, vals);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

// Colour scatter straight from the MFMA accumulators.  Measured at 128^3 (profiles/r01_hex27_mfma_counters.txt): 19.7-22.9 ms
static int hex27_assemble_colours(const Hex27Job& J, int64_t nnz, double* vals) {
  MFEM_CHECK_HIP(hipMemsetAsync(vals, 0, sizeof(double) * (size_t)nnz, J.ctx->stream));
  return hex27_launch_colours<true>(J, nullptr, nullptr, vals);
}

// Two passes: every element's Ke on the matrix cores -> element-major scratch (no colours, no RMW), a ring of element planes (h27_ring); the
// row-owner gather -> CSR, chunk by chunk.
static int hex27_assemble_ring(const Hex27Job& J, double* vals) {
  mfem_context_s* ctx = J.ctx;
  const mfem_brick_s* m = J.m;
  const int64_t plane_el = (int64_t)m->ne[1] * m->ne[2];
  const H27Ring R = h27_ring(J.ehi - J.elo, plane_el, J.K.chunk_planes);
  int rc = mfem_ws_reserve(ctx, R.plane_bytes * (size_t)R.ring);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hex27<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)J.lds));
  for (int a = J.elo; a < J.ehi; a += R.P) {
    const int b = a + R.P < J.ehi ? a + R.P : J.ehi;
    Hex27Args A{J.B, g_tab, J.p->k, J.K.affine, -1, J.nq, m->ng, a, b - a, R.ring};
    hipLaunchKernelGGL((k_hex27<true, true>), dim3(h27_wave_grid((b - a) * plane_el, ctx->num_cus)), dim3(H27_THREADS), J.lds, ctx->stream, A, nullptr,
                       nullptr, (double*)ctx->ws);
    MFEM_CHECK_LAUNCH();
    int64_t row_lo, row_hi;
    h27_chunk_rows(a, b, J.ehi, m->plo, m->phi, J.B.plane_len, &row_lo, &row_hi);
    if (row_hi <= row_lo) continue;
    rc = hex27_launch_gather(ctx, J.B, (const double*)ctx->ws, vals, row_lo, row_hi, R.ring);
    if (rc) return rc;
  }
  return MFEM_OK;
}

// G0 of every element, the count of the non-affine ones and their maps, into the head of the workspace (H27Ws).  The tables are small: after a
// workspace move they are made again instead of copied.
static int hex27_launch_count(const Hex27Job& J, const H27Ws& W) {
  char* ws = (char*)J.ctx->ws;
  return hex27_launch_g0(J.ctx, J.B, J.p->k, J.elo, J.ehi - J.elo, (double*)ws, J.ctx->d_flags + 14, (int32_t*)(ws + W.slot), (int32_t*)(ws + W.elist));
}
// All elements affine?  One 4-byte read-back per assembly: the coordinates belong to the caller (mfem_brick_coords) and may have changed since the
// last call.
static int hex27_count_nonaffine(const Hex27Job& J, const H27Ws& W, int64_t* n_stored) {
  mfem_context_s* ctx = J.ctx;
  int rc = mfem_ws_reserve(ctx, W.count_bytes);
  if (rc) return rc;
  rc = hex27_launch_count(J, W);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 14, ctx->d_flags + 14, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  *n_stored = ctx->h_flags[14];
  return MFEM_OK;
}

// Direct (n_stored == 0) and mixed: affine elements are computed in place by the row owners of k_hex27_direct; the n_stored others go through pass 1
// (k_hex27 in list mode) into a scratch that holds ONLY them and are streamed in by the same kernel.
static int hex27_assemble_direct(const Hex27Job& J, const H27Ws& W, int64_t n_stored, double* vals) {
  mfem_context_s* ctx = J.ctx;
  if (n_stored) {
    if (ctx->ws_bytes < W.head + W.stored_bytes) {  // (growing the workspace moves it)
      int rc = mfem_ws_reserve(ctx, W.head + W.stored_bytes);
      if (rc) return rc;
      rc = hex27_launch_count(J, W);
      if (rc) return rc;
    }
    MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hex27<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)J.lds));
    Hex27Args A{J.B, g_tab, J.p->k, 0, -1, J.nq, J.m->ng, J.elo, J.ehi - J.elo, 1, (const int32_t*)((char*)ctx->ws + W.elist), n_stored};
    hipLaunchKernelGGL((k_hex27<true, true>), dim3(h27_wave_grid(n_stored, ctx->num_cus)), dim3(H27_THREADS), J.lds, ctx->stream, A, nullptr, nullptr,
                       (double*)((char*)ctx->ws + W.head));
    MFEM_CHECK_LAUNCH();
    ++g_hex27_mixed_count;
  }
  const char* ws = (const char*)ctx->ws;
  const int rc = hex27_launch_direct(ctx, J.B, (const double*)ws, vals, J.elo, n_stored ? (const int32_t*)(ws + W.slot) : nullptr, (const double*)(ws + W.head));
  if (rc) return rc;
  if (!n_stored) ++g_hex27_direct_count;
  return MFEM_OK;
}

// Mostly general elements: G_q of every element (1296 bytes each) -> the row owners compute their runs from it, no Ke anywhere (k_hex27_rows_gq;
// three Gauss points per direction -- its b-side tables are compile-time constants).
static int hex27_assemble_rows(const Hex27Job& J, const H27Ws& W, double* vals) {
  mfem_context_s* ctx = J.ctx;
  int rc = mfem_ws_reserve(ctx, W.gq_bytes);
  if (rc) return rc;
  rc = hex27_launch_gq(ctx, J.B, J.p->k, J.elo, J.ehi - J.elo, (double*)ctx->ws);
  if (rc) return rc;
  rc = hex27_launch_rows(ctx, J.B, (const double*)ctx->ws, vals, J.elo, J.ehi - J.elo, J.K.rows_ablate);
  if (rc) return rc;
  ++g_hex27_rows_count;
  return MFEM_OK;
}

// the job of an assembly (mode -1: of the matrix variant the knob word names) or of a residual (mode 0), tables uploaded
static int hex27_job(Hex27Job* J, mfem_context_s* ctx, mfem_brick_s* m, const mfem_thermal_params* p, int mode) {
  J->ctx = ctx; J->m = m; J->p = p;
  J->K = h27_knobs(g_hex27_word);
  if (mode < 0) {
    MFEM_REQUIRE(!h27_slab_refused(J->K, m->plo, m->phi, m->m[0]), "hex-27 slabs are assembled by the two-pass variant only");
    mode = J->K.variant == 1 ? 2 : 1;
  }
  hex27_element_planes(m->plo, m->phi, m->ne[0], &J->elo, &J->ehi);
  J->nq = m->ng * m->ng * m->ng;
  J->lds = hex27_lds_bytes(m->ng, mode);
  J->B = mfem_brick_view(m, 1);
  return hex27_upload_tables(m->ng);
}

int mfem_hex27_assemble_thermal(mfem_context_s* ctx, mfem_brick_s* m, mfem_csr_s* Acsr, const mfem_thermal_params* p,
                                double* vals) {
  Hex27Job J;
  int rc = hex27_job(&J, ctx, m, p, -1);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hex27<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)J.lds));
  const int64_t nel = (int64_t)(J.ehi - J.elo) * m->ne[1] * m->ne[2];
  int64_t n_stored = -1;  // non-affine elements (not counted)
  if (h27_needs_count(J.K, m->n_owned)) {
    rc = hex27_count_nonaffine(J, h27_ws(m->ng, nel, 0), &n_stored);
    if (rc) return rc;
  }
  const H27Ws W = h27_ws(m->ng, nel, n_stored);
  switch (h27_path(J.K, m->ng, nel, n_stored)) {
    case H27_ATOMICS: rc = hex27_assemble_atomics(J, Acsr->nnz, vals); break;
    case H27_COLOUR: rc = hex27_assemble_colours(J, Acsr->nnz, vals); break;
    case H27_TWO_PASS: rc = hex27_assemble_ring(J, vals); break;
    case H27_DIRECT:
    case H27_MIXED: rc = hex27_assemble_direct(J, W, n_stored, vals); break;
    case H27_ROWS: rc = hex27_assemble_rows(J, W, vals); break;
  }
  if (rc) return rc;
  return hex27_launch_faces(J, true, nullptr, vals);
}

int mfem_hex27_residual_thermal(mfem_context_s* ctx, mfem_brick_s* m, const mfem_thermal_params* p, const double* x_star,
                                const double* s, double* residue) {
  Hex27Job J;
  int rc = hex27_job(&J, ctx, m, p, 0);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hex27<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)J.lds));
  MFEM_CHECK_HIP(hipMemsetAsync(residue, 0, sizeof(double) * (size_t)m->n_owned, ctx->stream));
  rc = hex27_launch_colours<false>(J, x_star, s, residue);
  if (rc) return rc;
  return hex27_launch_faces(J, false, x_star, residue);
}
