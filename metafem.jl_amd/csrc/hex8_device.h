// What the two physics of the fused hex-8 assembly (hex8_thermal.hip, hex8_elasticity.hip) share on the device: the reference-cell tables in constant
// memory and their upload, the geometry of an element and of a face at a Gauss point, the coordinate loaders, the boundary-face visitor, and the device
// wrappers of the block-to-tile maps and of the boundary enumeration of hex8_decide.h.
// The library is one code object per .hip file: everything here is `static`, so each of the two files owns its copy of the tables, uploads it through its
// own mfem_hex8_upload_tables and guards it with its own cache of the rule last uploaded.
#pragma once
#include "brick.h"
#include "hex8_decide.h"
static_assert(H8_BLOCK == MFEM_BLOCK && H8_MAX_NG == BRICK_MAX_NG && H8_MAX_Q == BRICK_MAX_Q, "hex8_decide.h spells the shared constants out (it includes neither brick.h nor common.h)");

// reference-cell tables of the rule last uploaded (layouts and formulas: H8Tables, hex8_decide.h)
static __constant__ double c_w[BRICK_MAX_Q];
static __constant__ double c_N[BRICK_MAX_Q][8];
static __constant__ double c_dN[BRICK_MAX_Q][8][3];
static __constant__ double c_xi[BRICK_MAX_Q][6];
static __constant__ double c_fw[BRICK_MAX_NG * BRICK_MAX_NG];
static __constant__ double c_M[8][8][3][3];
static __constant__ double c_fN[BRICK_MAX_NG * BRICK_MAX_NG][4];
static __constant__ double c_fdN[BRICK_MAX_NG * BRICK_MAX_NG][4][2];
static std::atomic<int> g_tables_ng{0};

static int mfem_hex8_upload_tables(int ng) {
  static std::mutex mu;  // uploads from two host threads must not interleave (the tables themselves are process-wide: see the threading note in include/metafem_mi355x.h)
  std::lock_guard<std::mutex> lk(mu);
  if (g_tables_ng == ng) return MFEM_OK;
  static H8Tables T;  // (guarded by mu)
  h8_reference_tables(ng, &T);
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_M), T.M, sizeof(T.M)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_w), T.w, sizeof(T.w)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_N), T.N, sizeof(T.N)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_dN), T.dN, sizeof(T.dN)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_xi), T.xi, sizeof(T.xi)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_fw), T.fw, sizeof(T.fw)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_fN), T.fN, sizeof(T.fN)));
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_fdN), T.fdN, sizeof(T.fdN)));
  g_tables_ng = ng;
  return MFEM_OK;
}

// ---- geometry at one Gauss point: J = dx/dxi, det, J^-1 (adjugate, inv_Jac_3D :90-121),
//      physical gradients g[b][s] = sum_m dN_b/dxi_m Jinv[m][s] (:133-142); returns w_q * det (:30)
__device__ __forceinline__ double hex8_geom(const double (&X)[8][3], int q, double (&g)[8][3]) {
  double J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < 8; ++b) s += c_dN[q][b][m] * X[b][i];
      J[i][m] = s;
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
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int s = 0; s < 3; ++s)
      g[b][s] = c_dN[q][b][0] * I[0][s] + c_dN[q][b][1] * I[1][s] + c_dN[q][b][2] * I[2][s];
  return c_w[q] * det;
}

__device__ __forceinline__ void hex8_load_coords(const BrickView& B, int I, int J, int K, double (&X)[8][3]) {
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int64_t c = brick_cindex(B, I + (b & 1), J + ((b >> 1) & 1), K + (b >> 2));
    X[b][0] = B.X0[c];
    X[b][1] = B.X1[c];
    X[b][2] = B.X2[c];
  }
}

// the same, nodes b and b + 4 (neighbours along k: adjacent in memory) by one 16-byte load: 12 load instructions per element instead of 24
typedef double h8_d2 __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ void hex8_load_coords_pairs(const BrickView& B, int I, int J, int K, double (&X)[8][3]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int64_t c = brick_cindex(B, I + (b & 1), J + ((b >> 1) & 1), K);
    const h8_d2 v0 = *reinterpret_cast<const h8_d2*>(B.X0 + c), v1 = *reinterpret_cast<const h8_d2*>(B.X1 + c), v2 = *reinterpret_cast<const h8_d2*>(B.X2 + c);
    X[b][0] = v0.x; X[b + 4][0] = v0.y;
    X[b][1] = v1.x; X[b + 4][1] = v1.y;
    X[b][2] = v2.x; X[b + 4][2] = v2.y;
  }
}

// The same geometry from the element's trilinear map x(xi) = X_0 + sum_{b > 0} C[b - 1] prod_{d in b} xi_d (C: differences of the nodal
// coordinates along the set bits of b, one butterfly per element): a column of J is 3 multiply-adds instead of the 8 of the table form.
__device__ __forceinline__ void hex8_trilinear(const double (&X)[8][3], double (&C)[7][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) v[b] = X[b][i];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if (b & (1 << d)) v[b] -= v[b ^ (1 << d)];
#pragma unroll
    for (int b = 1; b < 8; ++b) C[b - 1][i] = v[b];
  }
}
__device__ __forceinline__ double hex8_geom_trilinear(const double (&C)[7][3], int q, double (&g)[8][3]) {
  const double x0 = c_xi[q][0], x1 = c_xi[q][1], x2 = c_xi[q][2], x12 = c_xi[q][3], x02 = c_xi[q][4], x01 = c_xi[q][5];
  double J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    J[i][0] = C[0][i] + x1 * C[2][i] + x2 * C[4][i] + x12 * C[6][i];
    J[i][1] = C[1][i] + x0 * C[2][i] + x2 * C[5][i] + x02 * C[6][i];
    J[i][2] = C[3][i] + x0 * C[4][i] + x1 * C[5][i] + x01 * C[6][i];
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
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int s = 0; s < 3; ++s)
      g[b][s] = c_dN[q][b][0] * I[0][s] + c_dN[q][b][1] * I[1][s] + c_dN[q][b][2] * I[2][s];
  return c_w[q] * det;
}

// Face quadrature on the brick face with normal dim nd (0,1,2) -- tangential dims follow the reference
// (103_Integrations.jl:37): nd=0 -> (1,2), nd=1 -> (2,0), nd=2 -> (0,1).  Xf[c][3] are the 4 face nodes,
// c = c1 + 2*c2.  Returns w^s = w_q * |t1 x t2| (4_Update_Integrator.jl:71,210-226); `nrm` (optional) is
// the OUTWARD unit normal: the first tangent is negated on the low face (103_Integrations.jl:45).
__device__ __forceinline__ double face_geom(const double (&Xf)[4][3], int q, bool low_face, double* nrm) {
  double t1[3], t2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a += c_fdN[q][c][0] * Xf[c][i];
      b += c_fdN[q][c][1] * Xf[c][i];
    }
    t1[i] = low_face ? -a : a;
    t2[i] = b;
  }
  const double r0 = t1[1] * t2[2] - t1[2] * t2[1];
  const double r1 = -t1[0] * t2[2] + t1[2] * t2[0];
  const double r2 = t1[0] * t2[1] - t1[1] * t2[0];
  const double ld = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
  if (nrm) {
    nrm[0] = r0 / ld;
    nrm[1] = r1 / ld;
    nrm[2] = r2 / ld;
  }
  return c_fw[q] * ld;
}

__device__ __forceinline__ int face_bit(int nd, int high) {
  // reference local face ids (002_Initialization.jl:8): 1 z=0, 2 y=0, 3 x=L, 4 y=L, 5 x=0, 6 z=L
  const int id = (nd == 0) ? (high ? 3 : 5) : (nd == 1) ? (high ? 4 : 2) : (high ? 6 : 1);
  return 1 << (id - 1);
}

__device__ __forceinline__ void node_ijk(const BrickView& B, int64_t node, int& i, int& j, int& k) {
  if (B.n_owned < ((int64_t)1 << 31)) {  // (uniform) two 32-bit divisions: ~60 instructions against ~300 for the 64-bit pair
    const uint32_t nd = (uint32_t)node, pl = (uint32_t)B.plane_len, m2 = (uint32_t)B.m2;
    const uint32_t ip = nd / pl, rem = nd - ip * pl, jj = rem / m2;
    i = (int)ip + B.plo;
    j = (int)jj;
    k = (int)(rem - jj * m2);
    return;
  }
  i = (int)(node / B.plane_len) + B.plo;
  const int64_t rem = node % B.plane_len;
  j = (int)(rem / B.m2);
  k = (int)(rem % B.m2);
}

// =================================================================================================
// Boundary-face visitor: for an owned node (i,j,k), every element face that (a) lies on a brick face
// selected in `mask` and (b) contains the node.  f(nd, side, ca, fn, Xf): nd normal dim, side 0 low /
// 1 high, ca = the node's id among the 4 face nodes, fn[c][3] lattice ids and Xf[c][3] coordinates.
// =================================================================================================
template <typename Fn>
__device__ __forceinline__ void visit_boundary_faces(const BrickView& B, int i, int j, int k, uint32_t mask, Fn f) {
  if (mask == 0u) return;
  const int idx[3] = {i, j, k};
  const int ne[3] = {B.ne0, B.ne1, B.ne2};
  for (int nd = 0; nd < 3; ++nd) {
    for (int side = 0; side < 2; ++side) {
      const bool on = side == 0 ? (idx[nd] == 0) : (idx[nd] == ne[nd]);
      if (!on || !(mask & face_bit(nd, side))) continue;
      const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
      for (int q4 = 0; q4 < 4; ++q4) {
        const int f1 = q4 & 1, f2 = q4 >> 1;
        const int E1 = idx[t1] - 1 + f1, E2 = idx[t2] - 1 + f2;
        if (E1 < 0 || E1 >= ne[t1] || E2 < 0 || E2 >= ne[t2]) continue;
        const int ca = (1 - f1) + 2 * (1 - f2);
        int fn[4][3];
        double Xf[4][3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          fn[c][nd] = idx[nd];
          fn[c][t1] = E1 + (c & 1);
          fn[c][t2] = E2 + (c >> 1);
          const int64_t ci = brick_cindex(B, fn[c][0], fn[c][1], fn[c][2]);
          Xf[c][0] = B.X0[ci];
          Xf[c][1] = B.X1[ci];
          Xf[c][2] = B.X2[ci];
        }
        f(nd, side, ca, fn, Xf);
      }
    }
  }
}

// this thread's boundary control point of the owned planes (a 1-D grid of h8_boundary_grid workgroups); false: it has none
__device__ __forceinline__ bool boundary_point(const BrickView& B, int& i, int& j, int& k) {
  return h8_boundary_point((int64_t)blockIdx.x * blockDim.x + threadIdx.x, B.plo, B.phi, B.ne0, B.ne1, B.ne2, B.plane_len, B.m1, B.m2, i, j, k);
}
static inline dim3 boundary_grid(const mfem_brick_s* m) { return dim3(h8_boundary_grid(m->plo, m->phi, m->ne[0], m->plane_len, m->m[1], m->m[2])); }
// this workgroup's tile of a plane sweep: 15 x 15 control points (the residual sweeps), 7 x 15 (the matrix sweep)
typedef H8SweepTile SweepTile;
__device__ __forceinline__ SweepTile sweep_tile(const BrickView& B, int L) { return h8_sweep_tile(blockIdx.x, B.m1, B.m2, B.plo, B.phi, L, SW_N, SW_N); }
__device__ __forceinline__ SweepTile sweep_tile_m(const BrickView& B, int L) { return h8_sweep_tile(blockIdx.x, B.m1, B.m2, B.plo, B.phi, L, MS_NJ, MS_NK); }

// brick_prefix of an order-1 lattice from closed forms (what upload_dim_tables of brick.hip tabulates: a point couples to itself and its neighbours -- 2 at the two
// ends of a direction, 3 in between -- so the entries of the points in front of point g are 3 g - 1 from the second point on): the matrix sweep's write-out asked the
// tables per tile line and plane, five dependent loads from memory in front of the stores of every wave (round 5: the same finding as PX[] in k_hex27_rows_gq)
__device__ __forceinline__ int sw1_cnt(int g, int m) { return (g > 0 ? 1 : 0) + 1 + (g < m - 1 ? 1 : 0); }
__device__ __forceinline__ int64_t sw1_pre(int g) { return g > 0 ? 3 * (int64_t)g - 1 : 0; }
__device__ __forceinline__ int64_t sw1_prefix(const BrickView& B, int i, int j, int k) {
  return (sw1_pre(i) - B.Pplo) * B.S1 * B.S2 + (int64_t)sw1_cnt(i, B.m0) * (sw1_pre(j) * B.S2 + (int64_t)sw1_cnt(j, B.m1) * sw1_pre(k));
}
// the four nodes (J + by, K + bz) of lattice plane ip -> slot [bx] of the element's nodal arrays
__device__ __forceinline__ void sweep_load_coords(const BrickView& B, int ip, int J, int K, int bx, double (&X)[3][2][4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t ci = brick_cindex(B, ip, J + (c & 1), K + (c >> 1));
    X[0][bx][c] = B.X0[ci];
    X[1][bx][c] = B.X1[ci];
    X[2][bx][c] = B.X2[ci];
  }
}
// affine to 16 ulp of the coordinates' magnitude (what the Jacobian's own cancellation error is made of): the four mixed coefficients against the element's scale
__device__ __forceinline__ bool hex8_is_affine(const double (&X)[8][3], const double (&C)[7][3]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double tol = 3.6e-15 * (fabs(X[0][i]) + fabs(C[0][i]) + fabs(C[1][i]) + fabs(C[3][i]));
    ok = ok && fabs(C[2][i]) <= tol && fabs(C[4][i]) <= tol && fabs(C[5][i]) <= tol && fabs(C[6][i]) <= tol;
  }
  return ok;
}
