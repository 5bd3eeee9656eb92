// The host decisions of the fused hex-8 assembly (hex8_thermal.hip, hex8_elasticity.hip; shared device code: hex8_device.h): the two knob words, which
// kernel an entry point launches and with which flag word, the planes per sweep segment, every grid, the face-launch predicates, the block-to-tile maps
// and the boundary enumeration (host and device: the kernels call the same functions), and the reference-cell tables the kernels read from constant
// memory.  Plain integers in, plain structs out; no HIP, no context: tools/host_check_hex8_decide.cpp walks them on the CPU.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define H8_HD __host__ __device__ __forceinline__
#else
#define H8_HD inline
#endif

// ---- tile constants the decisions share with the kernels ----------------------------------------------------------------------------------------
#define H8_BLOCK 256  // (= MFEM_BLOCK) threads of the one-thread-per-control-point kernels
#define H8_MAX_NG 4   // (= BRICK_MAX_NG) Gauss points per direction at the most
#define H8_MAX_Q (H8_MAX_NG * H8_MAX_NG * H8_MAX_NG)
// thermal tile kernels (k_thermal_matrix, k_thermal_residual): 4 x 4 x 8 control points, the 5 x 5 x 9 elements touching them
#define TT_NI 4
#define TT_NJ 4
#define TT_NK 8
#define TT_THREADS (TT_NI * TT_NJ * TT_NK)
#define TT_EI (TT_NI + 1)
#define TT_EJ (TT_NJ + 1)
#define TT_EK (TT_NK + 1)
#define TT_NEL (TT_EI * TT_EJ * TT_EK)
#define TT_KSTRIDE 37  // 36 unique entries + 1 pad (LDS bank spread)
// residual sweeps (k_thermal_residual_sweep, k_elasticity_residual_sweep): 16 x 16 elements, 15 x 15 control points in (j, k)
#define SW_E 16
#define SW_N (SW_E - 1)
#define SW_THREADS (SW_E * SW_E)
#define SW_KSTRIDE 37
#define ESW_STRIDE 25  // doubles per element of the elasticity sweep's LDS block: fe[3][8] + 1 pad
// matrix sweep (k_thermal_matrix_sweep): 8 x 16 elements, 7 x 15 control points
#define MS_EJ 8
#define MS_EK 16
#define MS_NJ (MS_EJ - 1)
#define MS_NK (MS_EK - 1)
#define MS_THREADS (MS_EJ * MS_EK)
// k_elasticity_matrix_lds
#define EL2_NODES 32
#define EL2_ROW 243  // 3 fields x 81 slots; an ODD number of doubles: the lanes of a step (one control point each) then spread over all banks (244: 1.94 -> 2.04 ms)
#define EL2_CH (EL2_NODES * 81)  // doubles of one row field's chunk of the LDS copy (32 rows of up to 81 values; a node's row starts at 3 x its prefix: an odd stride too)
// workgroups below which a sweep shortens its segments (the (j, k) tiles alone do not fill the chip)
#define SW_FILL 2048
#define MS_FILL 4096

// ---- knob word "hex8_thermal" (mfem_debug_set_hex8_thermal) -------------------------------------------------------------------------------------
struct alignas(8) H8ThermalKnobs {  // (8 bytes, aligned: the .hip keeps it in a lock-free std::atomic)
  bool tiles;   // bit 0 SET: the 4 x 4 x 8 tile kernels for every Gauss rule (1- and 4-point rules always take them)
  bool staged;  // bit 1 CLEAR: the matrix sweep writes its full rows through LDS, a wave per tile line (set: per thread)
  bool affine;  // bit 2 CLEAR: both sweeps take the one-adjugate shortcut on affine elements
  int ablate;   // bits 3-5: TIMING-ONLY ablations of the matrix sweep (wrong values): 1 no integration, 2 no gather from LDS, 4 no staged write-out
};
H8_HD H8ThermalKnobs h8_thermal_knobs(int word) {
  H8ThermalKnobs K;
  K.tiles = (word & 1) != 0;
  K.staged = !(word & 2);
  K.affine = !(word & 4);
  K.ablate = (word >> 3) & 7;
  return K;
}
// flag word `stage_rows` of k_thermal_matrix_sweep: bit 0 staged, bit 1 affine shortcut, bits 2-4 the ablations
H8_HD int h8_thermal_stage_rows(const H8ThermalKnobs& K) { return (K.staged ? 1 : 0) | (K.affine ? 2 : 0) | K.ablate << 2; }
// argument `affine_fast` of k_thermal_residual_sweep
H8_HD int h8_thermal_affine_fast(const H8ThermalKnobs& K) { return K.affine ? 1 : 0; }

// ---- knob word "elasticity" (mfem_debug_set_elasticity) -------------------------------------------------------------------------------------------
struct alignas(8) H8ElasticityKnobs {
  bool matrix_global;    // bit 0 SET: the row-owner matrix kernel accumulating in global memory (k_elasticity_matrix)
  bool residual_points;  // bit 1 SET: the residual kernel that integrates per adjacent control point, for every rule (k_elasticity_residual)
  bool affine;           // bit 5 CLEAR: k_elasticity_matrix_lds takes the reference-integral shortcut on affine elements
  int ablate;            // bits 2-4: TIMING-ONLY ablations of k_elasticity_matrix_lds (wrong values): 1 no accumulation steps, 2 no write-out, 4 no integration
};
H8_HD H8ElasticityKnobs h8_elasticity_knobs(int word) {
  H8ElasticityKnobs K;
  K.matrix_global = (word & 1) != 0;
  K.residual_points = (word & 2) != 0;
  K.ablate = (word >> 2) & 7;
  K.affine = !(word & 32);
  return K;
}
// flag word `abl` of k_elasticity_matrix_lds: bits 0-2 the ablations, bit 3 no affine shortcut
H8_HD int h8_elasticity_abl(const H8ElasticityKnobs& K) { return K.ablate | (K.affine ? 0 : 8); }

// ---- which kernel -----------------------------------------------------------------------------------------------------------------------------------
// mfem_brick_assemble_thermal and mfem_brick_residual_thermal choose alike: the sweeps exist for the 2- and 3-point rules
enum H8ThermalKernel { H8_THERMAL_SWEEP, H8_THERMAL_TILES };
H8_HD H8ThermalKernel h8_thermal_kernel(const H8ThermalKnobs& K, int ng) { return !K.tiles && (ng == 2 || ng == 3) ? H8_THERMAL_SWEEP : H8_THERMAL_TILES; }
enum H8ElasticityMatrixKernel { H8_EL_MATRIX_LDS, H8_EL_MATRIX_GLOBAL };
H8_HD H8ElasticityMatrixKernel h8_elasticity_matrix_kernel(const H8ElasticityKnobs& K) { return K.matrix_global ? H8_EL_MATRIX_GLOBAL : H8_EL_MATRIX_LDS; }
// the sweep: the 2-point rule (itg_order 2-3); the 3-point rule's 27 Gauss points of three fields do not fit the register file of that form (2 KB spilled per lane)
enum H8ElasticityResidualKernel { H8_EL_RESIDUAL_SWEEP, H8_EL_RESIDUAL_POINTS };
H8_HD H8ElasticityResidualKernel h8_elasticity_residual_kernel(const H8ElasticityKnobs& K, int ng) {
  return !K.residual_points && ng == 2 ? H8_EL_RESIDUAL_SWEEP : H8_EL_RESIDUAL_POINTS;
}

// ---- launch geometry ----------------------------------------------------------------------------------------------------------------------------------
// A sweep workgroup owns nj x nk control points in (j, k) and L lattice planes: L = 32, halved down to 4 while the grid stays below `fill` workgroups
struct H8Sweep {
  int L;
  int64_t grid;
};
H8_HD H8Sweep h8_sweep_segments(int m1, int m2, int planes, int nj, int nk, int64_t fill) {
  const int64_t ntj = (m1 + nj - 1) / nj, ntk = (m2 + nk - 1) / nk;
  H8Sweep S;
  S.L = 32;
  while (S.L > 4 && ntj * ntk * ((planes + S.L - 1) / S.L) < fill) S.L /= 2;
  S.grid = ntj * ntk * ((planes + S.L - 1) / S.L);
  return S;
}
H8_HD H8Sweep h8_matrix_sweep(int m1, int m2, int planes) { return h8_sweep_segments(m1, m2, planes, MS_NJ, MS_NK, MS_FILL); }    // k_thermal_matrix_sweep
H8_HD H8Sweep h8_residual_sweep(int m1, int m2, int planes) { return h8_sweep_segments(m1, m2, planes, SW_N, SW_N, SW_FILL); }  // the two residual sweeps
// k_thermal_matrix, k_thermal_residual: 4 x 4 x 8 tiles over the owned planes
H8_HD int64_t h8_tile_grid(int planes, int m1, int m2) {
  const int64_t nti = (planes + TT_NI - 1) / TT_NI, ntj = (m1 + TT_NJ - 1) / TT_NJ, ntk = (m2 + TT_NK - 1) / TT_NK;
  return nti * ntj * ntk;
}
H8_HD int h8_el2_grid(int64_t n_owned) { return (int)((n_owned + EL2_NODES - 1) / EL2_NODES); }  // k_elasticity_matrix_lds: 32 control points per workgroup
H8_HD int h8_point_grid(int64_t n_owned) { return (int)((n_owned + H8_BLOCK - 1) / H8_BLOCK); }   // k_elasticity_matrix, k_elasticity_residual: a thread per control point

// ---- the face launches ----------------------------------------------------------------------------------------------------------------------------------
H8_HD bool h8_robin_launch(double h, uint32_t robin_faces) { return h != 0.0 && robin_faces != 0u; }
H8_HD bool h8_elasticity_faces_launch(double tau, uint32_t penalty_faces, uint32_t traction_faces) {
  return ((penalty_faces && tau != 0.0) || traction_faces) != 0;
}

// ---- block -> tile ------------------------------------------------------------------------------------------------------------------------------------------
// first control point (global lattice ids) of tile `tile` of the 4 x 4 x 8 tiling of a slab that starts at plane plo
struct H8TileOrigin {
  int ti, tj, tk;
};
H8_HD H8TileOrigin h8_tile_origin(int64_t tile, int m1, int m2, int plo) {
  const int ntk = (m2 + TT_NK - 1) / TT_NK, ntj = (m1 + TT_NJ - 1) / TT_NJ;
  H8TileOrigin t;
  t.tk = (int)(tile % ntk) * TT_NK;
  t.tj = (int)((tile / ntk) % ntj) * TT_NJ;
  t.ti = (int)(tile / ((int64_t)ntk * ntj)) * TT_NI + plo;
  return t;
}
// first control point in (j, k) and the planes [i0, i1) of sweep workgroup `block`: nj x nk control points per tile, L planes per segment of [plo, phi)
struct H8SweepTile {
  int tj0, tk0, i0, i1;
};
H8_HD H8SweepTile h8_sweep_tile(unsigned block, int m1, int m2, int plo, int phi, int L, int nj, int nk) {
  const int ntk = (m2 + nk - 1) / nk, ntj = (m1 + nj - 1) / nj;
  H8SweepTile t;
  t.tk0 = (int)(block % ntk) * nk;
  t.tj0 = (int)((block / ntk) % ntj) * nj;
  t.i0 = plo + (int)(block / (ntk * ntj)) * L;
  t.i1 = t.i0 + L < phi ? t.i0 + L : phi;
  return t;
}

// ---- boundary control points -------------------------------------------------------------------------------------------------------------------------------
// Boundary control points of the owned planes [plo, phi), enumerated compactly by one 1-D grid: the whole first lattice plane (if owned), the whole
// last one (if owned), then the rim (2 m2 + 2 (m1 - 2) points) of every other owned plane.
H8_HD int64_t h8_boundary_count(int plo, int phi, int ne0, int64_t plane_len, int m1, int m2) {
  const int64_t rim = 2 * (int64_t)m2 + 2 * (int64_t)(m1 - 2);
  const int f0 = plo == 0 ? 1 : 0, f1 = phi - 1 == ne0 ? 1 : 0;
  return (f0 + f1) * plane_len + (int64_t)(phi - plo - f0 - f1) * rim;
}
H8_HD unsigned h8_boundary_grid(int plo, int phi, int ne0, int64_t plane_len, int m1, int m2) {  // a thread per boundary control point, one workgroup at least
  const int64_t cnt = h8_boundary_count(plo, phi, ne0, plane_len, m1, m2);
  return (unsigned)((cnt + H8_BLOCK - 1) / H8_BLOCK > 0 ? (cnt + H8_BLOCK - 1) / H8_BLOCK : 1);
}
// thread t of that grid -> its control point; false: none (t at or past the count)
H8_HD bool h8_boundary_point(int64_t t, int plo, int phi, int ne0, int ne1, int ne2, int64_t plane_len, int m1, int m2, int& i, int& j, int& k) {
  const int f0 = plo == 0 ? 1 : 0, f1 = phi - 1 == ne0 ? 1 : 0;
  if (t < (f0 + f1) * plane_len) {
    i = (f0 && t < plane_len) ? 0 : ne0;
    if (f0 && t >= plane_len) t -= plane_len;
    j = (int)(t / m2);
    k = (int)(t % m2);
    return true;
  }
  t -= (f0 + f1) * plane_len;
  const int64_t rim = 2 * (int64_t)m2 + 2 * (int64_t)(m1 - 2);
  const int64_t pl = t / rim;
  if (pl >= phi - plo - f0 - f1) return false;
  i = plo + f0 + (int)pl;
  t -= pl * rim;
  if (t < 2 * (int64_t)m2) {
    j = t < m2 ? 0 : ne1;
    k = (int)(t < m2 ? t : t - m2);
  } else {
    const int u = (int)(t - 2 * (int64_t)m2);
    j = 1 + (u >> 1);
    k = (u & 1) ? ne2 : 0;
  }
  return true;
}

// ---- reference-cell tables ------------------------------------------------------------------------------------------------------------------------------------
// The tensor hex-8 on [0,1]^3 (spatial_discretization/102_Interpolations.jl:30-39, 103_Integrations.jl:1-19): index [q][b], q = qx + ng*(qy + ng*qz)
// (x fastest), b = bx + 2*by + 4*bz.  Face tables: 2-D Gauss on [0,1]^2, bilinear face basis [q][c], c = c1 + 2*c2 (first tangential coord fastest).
struct H8Tables {
  double w[H8_MAX_Q];
  double N[H8_MAX_Q][8];
  double dN[H8_MAX_Q][8][3];
  double xi[H8_MAX_Q][6];  // xi0, xi1, xi2, xi1 xi2, xi0 xi2, xi0 xi1 at Gauss point q (trilinear-map form of the Jacobian)
  double fw[H8_MAX_NG * H8_MAX_NG];
  double fN[H8_MAX_NG * H8_MAX_NG][4];
  double fdN[H8_MAX_NG * H8_MAX_NG][4][2];
  double M[8][8][3][3];    // reference integrals M[a][b][m][n] = sum_q w_q dN_a,m dN_b,n of THIS quadrature (affine-element shortcut of the elasticity matrix)
};
static const double H8_GP[4][4] = {{0.0, 0, 0, 0},
                                   {-0.57735026918962576451, 0.57735026918962576451, 0, 0},
                                   {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                   {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double H8_GW[4][4] = {{2.0, 0, 0, 0},
                                   {1.0, 1.0, 0, 0},
                                   {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                   {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};
static inline void h8_reference_tables(int ng, H8Tables* T) {
  double gp[4], gw[4];
  for (int i = 0; i < ng; ++i) {
    gp[i] = H8_GP[ng - 1][i] / 2.0 + 0.5;  // shift_gauss_point  103_Integrations.jl:1
    gw[i] = H8_GW[ng - 1][i] / 2.0;        // shift_gauss_weight :2
  }
  memset(T, 0, sizeof(*T));
  for (int qz = 0; qz < ng; ++qz)
    for (int qy = 0; qy < ng; ++qy)
      for (int qx = 0; qx < ng; ++qx) {
        const int q = qx + ng * (qy + ng * qz);
        const double xi[3] = {gp[qx], gp[qy], gp[qz]};
        T->w[q] = gw[qx] * gw[qy] * gw[qz];
        T->xi[q][0] = xi[0]; T->xi[q][1] = xi[1]; T->xi[q][2] = xi[2];
        T->xi[q][3] = xi[1] * xi[2]; T->xi[q][4] = xi[0] * xi[2]; T->xi[q][5] = xi[0] * xi[1];
        for (int b = 0; b < 8; ++b) {
          double f[3], df[3];
          for (int d = 0; d < 3; ++d) {
            const int bd = (b >> d) & 1;
            f[d] = bd ? xi[d] : 1.0 - xi[d];
            df[d] = bd ? 1.0 : -1.0;
          }
          T->N[q][b] = f[0] * f[1] * f[2];
          T->dN[q][b][0] = df[0] * f[1] * f[2];
          T->dN[q][b][1] = f[0] * df[1] * f[2];
          T->dN[q][b][2] = f[0] * f[1] * df[2];
        }
      }
  for (int q2 = 0; q2 < ng; ++q2)
    for (int q1 = 0; q1 < ng; ++q1) {
      const int q = q1 + ng * q2;
      T->fw[q] = gw[q1] * gw[q2];
      const double xi[2] = {gp[q1], gp[q2]};
      for (int c = 0; c < 4; ++c) {
        const int c1 = c & 1, c2 = c >> 1;
        const double f1 = c1 ? xi[0] : 1.0 - xi[0], f2 = c2 ? xi[1] : 1.0 - xi[1];
        T->fN[q][c] = f1 * f2;
        T->fdN[q][c][0] = (c1 ? 1.0 : -1.0) * f2;
        T->fdN[q][c][1] = f1 * (c2 ? 1.0 : -1.0);
      }
    }
  const int nq3 = ng * ng * ng;
  for (int a = 0; a < 8; ++a)
    for (int b = 0; b < 8; ++b)
      for (int m = 0; m < 3; ++m)
        for (int n = 0; n < 3; ++n) {
          double acc = 0.0;
          for (int q = 0; q < nq3; ++q) acc += T->w[q] * (T->dN[q][a][m] * T->dN[q][b][n]);  // (w * (x * y): M[a][b][m][n] and M[b][a][n][m] are the same bits -- el2_affine's mirrored entries rely on it)
          T->M[a][b][m][n] = acc;
        }
}
