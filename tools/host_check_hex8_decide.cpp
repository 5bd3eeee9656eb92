// CPU walk through the host decisions of the fused hex-8 assembly (csrc/hex8_decide.h), three ways:
//   1. against the expressions of the driver these functions were cut out of (both physics in one file: two setters re-encoding their knob words into three
//      file-static atomics, four entry points testing those inline, sweep_planes / sweep_planes_m, boundary_grid, the grids spelled out at the launch
//      sites, boundary_point, the table arithmetic of mfem_hex8_upload_tables), transcribed below as old_*: the chosen kernel, every flag word handed to
//      a kernel, L, every grid, the face predicates, the boundary enumeration, the tables bit for bit -- swept, 0 differences allowed;
//   2. properties that hold whatever the driver did: the boundary enumeration visits each boundary control point of a slab's owned planes exactly once
//      and nothing else; each of the three block-to-tile maps puts every owned control point into exactly one (block, in-tile position) and no block
//      outside the owned planes; L of a sweep is 4, 8, 16 or 32 and halved only while the grid is below the threshold;
//   3. the reference tables for 1 to 4 Gauss points per direction: weights sum to 1, N to 1, dN to 0 (cell and face), and M[a][b][m][n] and
//      M[b][a][n][m] are the same bits (k_elasticity_matrix_lds mirrors entries through that).
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_hex8_decide.cpp -o tools/bin/host_check_hex8_decide && tools/bin/host_check_hex8_decide
#include <cmath>
#include <cstdio>
#include <vector>
#include "hex8_decide.h"

static long long cases = 0, diffs = 0, bad = 0;
#define SAME(a, b, ...) do { ++cases; if (!((a) == (b))) { if (++diffs <= 20) { printf("DIFFERS "); printf(__VA_ARGS__); printf(": %s = %lld, %s = %lld\n", #a, (long long)(a), #b, (long long)(b)); } } } while (0)
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

// ---- 1. the driver before the cut, verbatim ---------------------------------------------------------------------------------------------------------
#define OLD_MFEM_BLOCK 256
#define OLD_TT_NI 4
#define OLD_TT_NJ 4
#define OLD_TT_NK 8
#define OLD_SW_N 15
#define OLD_MS_NJ 7
#define OLD_MS_NK 15
#define OLD_EL2_NODES 32
struct old_brick {  // the members of mfem_brick_s the driver read
  int32_t ne[3], ng, m[3];
  int64_t plane_len;
  int32_t plo, phi;
  int64_t n_owned;
};
static old_brick old_make(int m0, int m1, int m2, int plo, int phi, int ng = 2) {
  old_brick b;
  b.m[0] = m0, b.m[1] = m1, b.m[2] = m2;
  for (int d = 0; d < 3; ++d) b.ne[d] = b.m[d] - 1;
  b.ng = ng, b.plane_len = (int64_t)m1 * m2, b.plo = plo, b.phi = phi, b.n_owned = (int64_t)(phi - plo) * b.plane_len;
  return b;
}
struct OldThermal {
  int g_thermal_variant, g_stage_word;  // (g_stage_word: the re-encoded knob word the matrix sweep received whole, named for its bit 0 in the driver)
};
static OldThermal old_set_hex8_thermal(int variant) {
  OldThermal g;
  g.g_thermal_variant = (variant & 1) ? 1 : 0;
  g.g_stage_word = ((variant & 2) ? 0 : 1) | ((variant & 4) ? 0 : 2) | ((variant >> 3) & 7) << 2;
  return g;
}
static int old_set_elasticity(int variant) { return variant & 0x3f; }
static int old_sweep_planes_m(const old_brick* m, int64_t* grid) {
  const int64_t ntj = (m->m[1] + OLD_MS_NJ - 1) / OLD_MS_NJ, ntk = (m->m[2] + OLD_MS_NK - 1) / OLD_MS_NK;
  const int planes = m->phi - m->plo;
  int L = 32;
  while (L > 4 && ntj * ntk * ((planes + L - 1) / L) < 4096) L /= 2;
  *grid = ntj * ntk * ((planes + L - 1) / L);
  return L;
}
static int old_sweep_planes(const old_brick* m, int64_t* grid) {
  const int64_t ntj = (m->m[1] + OLD_SW_N - 1) / OLD_SW_N, ntk = (m->m[2] + OLD_SW_N - 1) / OLD_SW_N;
  const int planes = m->phi - m->plo;
  int L = 32;
  while (L > 4 && ntj * ntk * ((planes + L - 1) / L) < 2048) L /= 2;
  *grid = ntj * ntk * ((planes + L - 1) / L);
  return L;
}
static int64_t old_boundary_count(int plo, int phi, int ne0, int64_t plane_len, int m1, int m2) {
  const int64_t rim = 2 * (int64_t)m2 + 2 * (int64_t)(m1 - 2);
  const int f0 = plo == 0 ? 1 : 0, f1 = phi - 1 == ne0 ? 1 : 0;
  return (f0 + f1) * plane_len + (int64_t)(phi - plo - f0 - f1) * rim;
}
static unsigned old_boundary_grid(const old_brick* m) {
  const int64_t cnt = old_boundary_count(m->plo, m->phi, m->ne[0], m->plane_len, m->m[1], m->m[2]);
  return (unsigned)((cnt + OLD_MFEM_BLOCK - 1) / OLD_MFEM_BLOCK > 0 ? (cnt + OLD_MFEM_BLOCK - 1) / OLD_MFEM_BLOCK : 1);
}
struct OldView {  // the members of BrickView boundary_point read
  int32_t ne0, ne1, ne2, m1, m2, plo, phi;
  int64_t plane_len;
};
static bool old_boundary_point(const OldView& B, int64_t t /* blockIdx.x * blockDim.x + threadIdx.x */, int& i, int& j, int& k) {
  const int f0 = B.plo == 0 ? 1 : 0, f1 = B.phi - 1 == B.ne0 ? 1 : 0;
  if (t < (f0 + f1) * B.plane_len) {
    i = (f0 && t < B.plane_len) ? 0 : B.ne0;
    if (f0 && t >= B.plane_len) t -= B.plane_len;
    j = (int)(t / B.m2);
    k = (int)(t % B.m2);
    return true;
  }
  t -= (f0 + f1) * B.plane_len;
  const int64_t rim = 2 * (int64_t)B.m2 + 2 * (int64_t)(B.m1 - 2);
  const int64_t pl = t / rim;
  if (pl >= B.phi - B.plo - f0 - f1) return false;
  i = B.plo + f0 + (int)pl;
  t -= pl * rim;
  if (t < 2 * (int64_t)B.m2) {
    j = t < B.m2 ? 0 : B.ne1;
    k = (int)(t < B.m2 ? t : t - B.m2);
  } else {
    const int u = (int)(t - 2 * (int64_t)B.m2);
    j = 1 + (u >> 1);
    k = (u & 1) ? B.ne2 : 0;
  }
  return true;
}
// what an entry point launched: kernel 0 = the sweep / LDS form, 1 = the other one; the flag word it handed over (-1: none), L (0: none), the grid
struct OldLaunch {
  int kernel, flags, L;
  int64_t grid;
};
static OldLaunch old_assemble_thermal(const OldThermal& g, const old_brick* m) {
  if (g.g_thermal_variant == 0 && (m->ng == 2 || m->ng == 3)) {
    int64_t grid;
    const int L = old_sweep_planes_m(m, &grid);
    return {0, g.g_stage_word, L, (int64_t)(unsigned)grid};
  }
  const int64_t nti = ((m->phi - m->plo) + OLD_TT_NI - 1) / OLD_TT_NI, ntj = (m->m[1] + OLD_TT_NJ - 1) / OLD_TT_NJ, ntk = (m->m[2] + OLD_TT_NK - 1) / OLD_TT_NK;
  return {1, -1, 0, (int64_t)(unsigned)(nti * ntj * ntk)};
}
static OldLaunch old_residual_thermal(const OldThermal& g, const old_brick* m) {
  if (g.g_thermal_variant == 0 && (m->ng == 2 || m->ng == 3)) {
    int64_t grid;
    const int L = old_sweep_planes(m, &grid);
    return {0, (g.g_stage_word >> 1) & 1, L, (int64_t)(unsigned)grid};
  }
  const int64_t nti = ((m->phi - m->plo) + OLD_TT_NI - 1) / OLD_TT_NI, ntj = (m->m[1] + OLD_TT_NJ - 1) / OLD_TT_NJ, ntk = (m->m[2] + OLD_TT_NK - 1) / OLD_TT_NK;
  return {1, -1, 0, (int64_t)(unsigned)(nti * ntj * ntk)};
}
static OldLaunch old_assemble_elasticity(int g_elasticity_variant, const old_brick* m) {
  if (!(g_elasticity_variant & 1)) {
    const int grid = (int)((m->n_owned + OLD_EL2_NODES - 1) / OLD_EL2_NODES);
    return {0, g_elasticity_variant >> 2, 0, grid};
  }
  const int grid = (int)((m->n_owned + OLD_MFEM_BLOCK - 1) / OLD_MFEM_BLOCK);
  return {1, -1, 0, grid};
}
static OldLaunch old_residual_elasticity(int g_elasticity_variant, const old_brick* m) {
  if (!(g_elasticity_variant & 2) && m->ng == 2) {
    int64_t grid;
    const int L = old_sweep_planes(m, &grid);
    return {0, -1, L, (int64_t)(unsigned)grid};
  }
  const int grid = (int)((m->n_owned + OLD_MFEM_BLOCK - 1) / OLD_MFEM_BLOCK);
  return {1, -1, 0, grid};
}
static bool old_robin(double h, uint32_t robin_faces) { return h != 0.0 && robin_faces != 0u; }
static bool old_el_faces(double tau, uint32_t penalty_faces, uint32_t traction_faces) { return ((penalty_faces && tau != 0.0) || traction_faces) != 0; }
// the host arithmetic of mfem_hex8_upload_tables
static const double OLD_GP[4][4] = {{0.0, 0, 0, 0},
                                    {-0.57735026918962576451, 0.57735026918962576451, 0, 0},
                                    {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                    {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double OLD_GW[4][4] = {{2.0, 0, 0, 0},
                                    {1.0, 1.0, 0, 0},
                                    {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                    {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};
static void old_tables(int ng, H8Tables* out) {
  double w[64], N[64][8], dN[64][8][3], xiq[64][6];
  double fw[16], fN[16][4], fdN[16][4][2];
  double gp[4], gw[4];
  for (int i = 0; i < ng; ++i) {
    gp[i] = OLD_GP[ng - 1][i] / 2.0 + 0.5;
    gw[i] = OLD_GW[ng - 1][i] / 2.0;
  }
  memset(w, 0, sizeof(w)); memset(N, 0, sizeof(N)); memset(dN, 0, sizeof(dN)); memset(xiq, 0, sizeof(xiq));
  memset(fw, 0, sizeof(fw)); memset(fN, 0, sizeof(fN)); memset(fdN, 0, sizeof(fdN));
  for (int qz = 0; qz < ng; ++qz)
    for (int qy = 0; qy < ng; ++qy)
      for (int qx = 0; qx < ng; ++qx) {
        const int q = qx + ng * (qy + ng * qz);
        const double xi[3] = {gp[qx], gp[qy], gp[qz]};
        w[q] = gw[qx] * gw[qy] * gw[qz];
        xiq[q][0] = xi[0]; xiq[q][1] = xi[1]; xiq[q][2] = xi[2];
        xiq[q][3] = xi[1] * xi[2]; xiq[q][4] = xi[0] * xi[2]; xiq[q][5] = xi[0] * xi[1];
        for (int b = 0; b < 8; ++b) {
          double f[3], df[3];
          for (int d = 0; d < 3; ++d) {
            const int bd = (b >> d) & 1;
            f[d] = bd ? xi[d] : 1.0 - xi[d];
            df[d] = bd ? 1.0 : -1.0;
          }
          N[q][b] = f[0] * f[1] * f[2];
          dN[q][b][0] = df[0] * f[1] * f[2];
          dN[q][b][1] = f[0] * df[1] * f[2];
          dN[q][b][2] = f[0] * f[1] * df[2];
        }
      }
  for (int q2 = 0; q2 < ng; ++q2)
    for (int q1 = 0; q1 < ng; ++q1) {
      const int q = q1 + ng * q2;
      fw[q] = gw[q1] * gw[q2];
      const double xi[2] = {gp[q1], gp[q2]};
      for (int c = 0; c < 4; ++c) {
        const int c1 = c & 1, c2 = c >> 1;
        const double f1 = c1 ? xi[0] : 1.0 - xi[0], f2 = c2 ? xi[1] : 1.0 - xi[1];
        fN[q][c] = f1 * f2;
        fdN[q][c][0] = (c1 ? 1.0 : -1.0) * f2;
        fdN[q][c][1] = f1 * (c2 ? 1.0 : -1.0);
      }
    }
  {
    static double M[8][8][3][3];
    const int nq3 = ng * ng * ng;
    for (int a = 0; a < 8; ++a)
      for (int b = 0; b < 8; ++b)
        for (int m = 0; m < 3; ++m)
          for (int n = 0; n < 3; ++n) {
            double acc = 0.0;
            for (int q = 0; q < nq3; ++q) acc += w[q] * (dN[q][a][m] * dN[q][b][n]);
            M[a][b][m][n] = acc;
          }
    memcpy(out->M, M, sizeof(M));
  }
  memcpy(out->w, w, sizeof(w)); memcpy(out->N, N, sizeof(N)); memcpy(out->dN, dN, sizeof(dN)); memcpy(out->xi, xiq, sizeof(xiq));
  memcpy(out->fw, fw, sizeof(fw)); memcpy(out->fN, fN, sizeof(fN)); memcpy(out->fdN, fdN, sizeof(fdN));
}

static std::vector<int> lattice_sizes() {
  std::vector<int> v;
  for (int m = 2; m <= 48; ++m) v.push_back(m);
  for (int m : {129, 257, 513, 1025}) v.push_back(m);
  return v;
}
static std::vector<int> plane_counts() {
  std::vector<int> v;
  for (int p = 1; p <= 70; ++p) v.push_back(p);
  v.push_back(513);
  return v;
}

static void check_knobs_and_kernels() {
  const old_brick geo = old_make(40, 33, 17, 0, 40);
  for (int w = 0; w < 64; ++w) {
    const OldThermal g = old_set_hex8_thermal(w);
    const H8ThermalKnobs K = h8_thermal_knobs(w);
    SAME((int)K.tiles, g.g_thermal_variant, "hex8_thermal %d", w);
    SAME(h8_thermal_stage_rows(K), g.g_stage_word, "hex8_thermal %d", w);
    SAME(h8_thermal_affine_fast(K), (g.g_stage_word >> 1) & 1, "hex8_thermal %d", w);
    const int ge = old_set_elasticity(w);
    const H8ElasticityKnobs E = h8_elasticity_knobs(w);
    SAME(h8_elasticity_abl(E), ge >> 2, "elasticity %d", w);
    for (int ng = 1; ng <= 4; ++ng) {
      old_brick b = geo;
      b.ng = ng;
      const OldLaunch at = old_assemble_thermal(g, &b), rt = old_residual_thermal(g, &b), ae = old_assemble_elasticity(ge, &b), re = old_residual_elasticity(ge, &b);
      const H8ThermalKernel kt = h8_thermal_kernel(K, ng);
      SAME((int)(kt != H8_THERMAL_SWEEP), at.kernel, "hex8_thermal %d, ng %d: matrix kernel", w, ng);
      SAME((int)(kt != H8_THERMAL_SWEEP), rt.kernel, "hex8_thermal %d, ng %d: residual kernel", w, ng);
      if (kt == H8_THERMAL_SWEEP) {
        SAME(h8_thermal_stage_rows(K), at.flags, "hex8_thermal %d, ng %d: stage_rows", w, ng);
        SAME(h8_thermal_affine_fast(K), rt.flags, "hex8_thermal %d, ng %d: affine_fast", w, ng);
      }
      SAME((int)(h8_elasticity_matrix_kernel(E) != H8_EL_MATRIX_LDS), ae.kernel, "elasticity %d, ng %d: matrix kernel", w, ng);
      if (h8_elasticity_matrix_kernel(E) == H8_EL_MATRIX_LDS) SAME(h8_elasticity_abl(E), ae.flags, "elasticity %d, ng %d: abl", w, ng);
      SAME((int)(h8_elasticity_residual_kernel(E, ng) != H8_EL_RESIDUAL_SWEEP), re.kernel, "elasticity %d, ng %d: residual kernel", w, ng);
    }
  }
  const H8ThermalKnobs D = h8_thermal_knobs(0);
  CHECK(!D.tiles && D.staged && D.affine && !D.ablate && h8_thermal_stage_rows(D) == 3, "hex8_thermal 0: every default (the old initial flag word was 3)");
  const H8ElasticityKnobs E = h8_elasticity_knobs(0);
  CHECK(!E.matrix_global && !E.residual_points && E.affine && !E.ablate && h8_elasticity_abl(E) == 0, "elasticity 0: every default");
  CHECK(h8_thermal_kernel(D, 2) == H8_THERMAL_SWEEP && h8_thermal_kernel(D, 3) == H8_THERMAL_SWEEP && h8_thermal_kernel(D, 1) == H8_THERMAL_TILES &&
        h8_thermal_kernel(D, 4) == H8_THERMAL_TILES && h8_thermal_kernel(h8_thermal_knobs(1), 2) == H8_THERMAL_TILES, "thermal: sweep iff the tile knob is clear and ng is 2 or 3");
  CHECK(h8_elasticity_residual_kernel(E, 2) == H8_EL_RESIDUAL_SWEEP && h8_elasticity_residual_kernel(E, 3) == H8_EL_RESIDUAL_POINTS &&
        h8_elasticity_residual_kernel(h8_elasticity_knobs(2), 2) == H8_EL_RESIDUAL_POINTS, "elasticity residual: sweep iff bit 1 is clear and ng is 2");
  static_assert(H8_BLOCK == OLD_MFEM_BLOCK && TT_NI == OLD_TT_NI && TT_NJ == OLD_TT_NJ && TT_NK == OLD_TT_NK && SW_N == OLD_SW_N && MS_NJ == OLD_MS_NJ && MS_NK == OLD_MS_NK &&
                EL2_NODES == OLD_EL2_NODES && SW_FILL == 2048 && MS_FILL == 4096, "the tile constants as the kernels had them");
  static_assert(TT_THREADS == 128 && TT_NEL == 225 && TT_KSTRIDE == 37 && SW_E == 16 && SW_THREADS == 256 && SW_KSTRIDE == 37 && MS_EJ == 8 && MS_EK == 16 && MS_THREADS == 128 &&
                EL2_ROW == 243 && EL2_CH == 2592 && ESW_STRIDE == 25, "the tile constants as the kernels had them");
}

static void check_geometry() {
  const std::vector<int> ms = lattice_sizes(), ps = plane_counts();
  const OldThermal g0 = old_set_hex8_thermal(0), g1 = old_set_hex8_thermal(1);
  for (int m1 : ms)
    for (int m2 : ms)
      for (int planes : ps)
        for (int plo : {0, 3}) {
          const old_brick b = old_make(plo + planes + (plo || planes == 1 ? 2 : 0), m1, m2, plo, plo + planes);  // a whole brick, or a slab short of the last plane
          const OldLaunch sm = old_assemble_thermal(g0, &b), sr = old_residual_thermal(g0, &b), tm = old_assemble_thermal(g1, &b), tr = old_residual_thermal(g1, &b);
          const OldLaunch em = old_assemble_elasticity(0, &b), eg = old_assemble_elasticity(1, &b), es = old_residual_elasticity(0, &b), ep = old_residual_elasticity(2, &b);
          const H8Sweep M = h8_matrix_sweep(m1, m2, planes), R = h8_residual_sweep(m1, m2, planes);
          SAME(M.L, sm.L, "matrix sweep, %d planes of %d x %d", planes, m1, m2);
          SAME((int64_t)(unsigned)M.grid, sm.grid, "matrix sweep, %d planes of %d x %d", planes, m1, m2);
          SAME(R.L, sr.L, "residual sweep, %d planes of %d x %d", planes, m1, m2);
          SAME((int64_t)(unsigned)R.grid, sr.grid, "residual sweep, %d planes of %d x %d", planes, m1, m2);
          SAME(R.L, es.L, "elasticity residual sweep, %d planes of %d x %d", planes, m1, m2);
          SAME((int64_t)(unsigned)R.grid, es.grid, "elasticity residual sweep, %d planes of %d x %d", planes, m1, m2);
          SAME((int64_t)(unsigned)h8_tile_grid(planes, m1, m2), tm.grid, "tile grid, %d planes of %d x %d", planes, m1, m2);
          SAME((int64_t)(unsigned)h8_tile_grid(planes, m1, m2), tr.grid, "tile grid, %d planes of %d x %d", planes, m1, m2);
          SAME(h8_el2_grid(b.n_owned), em.grid, "LDS matrix grid, %lld points", (long long)b.n_owned);
          SAME(h8_point_grid(b.n_owned), eg.grid, "row-owner matrix grid, %lld points", (long long)b.n_owned);
          SAME(h8_point_grid(b.n_owned), ep.grid, "pointwise residual grid, %lld points", (long long)b.n_owned);
          SAME(h8_boundary_count(b.plo, b.phi, b.ne[0], b.plane_len, m1, m2), old_boundary_count(b.plo, b.phi, b.ne[0], b.plane_len, m1, m2), "boundary count");
          SAME(h8_boundary_grid(b.plo, b.phi, b.ne[0], b.plane_len, m1, m2), old_boundary_grid(&b), "boundary grid, slab [%d, %d) of %d x %d x %d", b.plo, b.phi, b.m[0], m1, m2);
          // the sweep-segment function's own properties
          for (int matrix = 0; matrix < 2; ++matrix) {
            const H8Sweep& S = matrix ? M : R;
            const int nj = matrix ? MS_NJ : SW_N, nk = matrix ? MS_NK : SW_N;
            const int64_t fill = matrix ? MS_FILL : SW_FILL, tiles = (int64_t)((m1 + nj - 1) / nj) * ((m2 + nk - 1) / nk);
            CHECK(S.L == 4 || S.L == 8 || S.L == 16 || S.L == 32, "L = %d", S.L);
            CHECK(S.grid == tiles * ((planes + S.L - 1) / S.L), "the grid covers the tiles and the segments");
            CHECK(S.L == 32 || tiles * ((planes + 2 * S.L - 1) / (2 * S.L)) < fill, "L = %d: halved from a grid below %lld", S.L, (long long)fill);
            CHECK(S.L == 4 || S.grid >= fill, "L = %d: not halved further with %lld workgroups", S.L, (long long)S.grid);
          }
        }
  for (double s : {0.0, 25.0})
    for (uint32_t a : {0u, 1u, 0x3fu})
      for (uint32_t b : {0u, 4u, 0x3fu}) {
        SAME((int)h8_robin_launch(s, a), (int)old_robin(s, a), "Robin launch, h %g, faces %#x", s, a);
        SAME((int)h8_elasticity_faces_launch(s, a, b), (int)old_el_faces(s, a, b), "elasticity face launch, tau %g, penalty %#x, traction %#x", s, a, b);
      }
}

// ---- 2. properties ----------------------------------------------------------------------------------------------------------------------------------------
static void check_boundary() {
  for (int m0 = 2; m0 <= 5; ++m0)
    for (int m1 = 2; m1 <= 5; ++m1)
      for (int m2 = 2; m2 <= 5; ++m2)
        for (int plo = 0; plo < m0; ++plo)
          for (int phi = plo + 1; phi <= m0; ++phi) {
            const int ne0 = m0 - 1, ne1 = m1 - 1, ne2 = m2 - 1;
            const int64_t pl = (int64_t)m1 * m2, cnt = h8_boundary_count(plo, phi, ne0, pl, m1, m2);
            const unsigned grid = h8_boundary_grid(plo, phi, ne0, pl, m1, m2);
            const OldView B{ne0, ne1, ne2, m1, m2, plo, phi, pl};
            std::vector<int> seen((size_t)m0 * pl, 0);
            CHECK((int64_t)grid * H8_BLOCK >= cnt && grid >= 1, "a thread per boundary point");
            for (int64_t t = 0; t < (int64_t)grid * H8_BLOCK; ++t) {
              int i = -1, j = -1, k = -1, io = -1, jo = -1, ko = -1;
              const bool hit = h8_boundary_point(t, plo, phi, ne0, ne1, ne2, pl, m1, m2, i, j, k), ho = old_boundary_point(B, t, io, jo, ko);
              SAME((int)hit, (int)ho, "boundary_point, thread %lld", (long long)t);
              if (hit && ho) SAME((i * 100 + j) * 100 + k, (io * 100 + jo) * 100 + ko, "boundary_point, thread %lld", (long long)t);
              CHECK(hit == (t < cnt), "slab [%d, %d) of %d x %d x %d: thread %lld of %lld boundary points", plo, phi, m0, m1, m2, (long long)t, (long long)cnt);
              if (!hit) continue;
              const bool inside = i >= plo && i < phi && j >= 0 && j < m1 && k >= 0 && k < m2;
              CHECK(inside, "slab [%d, %d) of %d x %d x %d: thread %lld -> (%d, %d, %d)", plo, phi, m0, m1, m2, (long long)t, i, j, k);
              if (inside) ++seen[((size_t)i * m1 + j) * m2 + k];
            }
            for (int i = 0; i < m0; ++i)
              for (int j = 0; j < m1; ++j)
                for (int k = 0; k < m2; ++k) {
                  const bool want = i >= plo && i < phi && (i == 0 || i == ne0 || j == 0 || j == ne1 || k == 0 || k == ne2);
                  CHECK(seen[((size_t)i * m1 + j) * m2 + k] == (want ? 1 : 0), "slab [%d, %d) of %d x %d x %d: point (%d, %d, %d) visited %d times", plo, phi, m0, m1, m2, i, j, k,
                        seen[((size_t)i * m1 + j) * m2 + k]);
                }
          }
}

// lattice sizes that straddle a tile extent: the extent +- 1 and twice the extent +- 1 (2 points at the least)
static std::vector<int> straddle(int ext) {
  std::vector<int> v;
  for (int m : {ext - 1, ext, ext + 1, 2 * ext - 1, 2 * ext, 2 * ext + 1})
    if (m >= 2) v.push_back(m);
  return v;
}
// which: 0 the 4 x 4 x 8 tiles, 1 the residual sweeps' 15 x 15 tiles, 2 the matrix sweep's 7 x 15 tiles
static void check_tile_map(int which) {
  const int nj = which == 0 ? TT_NJ : which == 1 ? SW_N : MS_NJ, nk = which == 0 ? TT_NK : which == 1 ? SW_N : MS_NK;
  for (int m0 : {3, 4, 5, 7, 8, 9, 31, 32, 33, 65})  // the tile's 4 planes, segments of 4 (what the grid gives at these sizes) and of 32 (forced: pass 1)
    for (int m1 : straddle(nj))
      for (int m2 : straddle(nk))
        for (int s = 0; s < 4; ++s)
          for (int pass = 0; pass < (which == 0 ? 1 : 2); ++pass) {
          const int plo = s == 0 ? 0 : s == 1 ? 0 : s == 2 ? m0 / 2 : 1, phi = s == 0 ? m0 : s == 1 ? m0 / 2 : s == 2 ? m0 : m0 - 1;
          if (phi <= plo) continue;
          const int planes = phi - plo;
          std::vector<int> seen((size_t)m0 * m1 * m2, 0);
          auto own = [&](int i, int j, int k) {  // the kernels' own guards: a point past the owned planes or the lattice has no thread
            if (i < phi && j < m1 && k < m2) ++seen[((size_t)i * m1 + j) * m2 + k];
          };
          if (which == 0) {
            const int64_t grid = h8_tile_grid(planes, m1, m2);
            for (int64_t blk = 0; blk < grid; ++blk) {
              const H8TileOrigin T = h8_tile_origin(blk, m1, m2, plo);
              CHECK(T.ti >= plo && T.ti < phi && T.tj >= 0 && T.tj < m1 && T.tk >= 0 && T.tk < m2, "tile %lld starts inside the slab [%d, %d) of %d x %d x %d", (long long)blk, plo, phi, m0, m1, m2);
              for (int tid = 0; tid < TT_THREADS; ++tid) own(T.ti + tid / (TT_NK * TT_NJ), T.tj + (tid / TT_NK) % TT_NJ, T.tk + tid % TT_NK);  // phase B of k_thermal_matrix
            }
          } else {
            const H8Sweep S = pass ? h8_sweep_segments(m1, m2, planes, nj, nk, 0) : which == 1 ? h8_residual_sweep(m1, m2, planes) : h8_matrix_sweep(m1, m2, planes);
            CHECK(S.L == (pass ? 32 : 4), "L = %d", S.L);
            for (int64_t blk = 0; blk < S.grid; ++blk) {
              const H8SweepTile T = h8_sweep_tile((unsigned)blk, m1, m2, plo, phi, S.L, nj, nk);
              CHECK(T.i0 >= plo && T.i0 < T.i1 && T.i1 <= phi && T.i1 - T.i0 <= S.L && T.tj0 >= 0 && T.tj0 < m1 && T.tk0 >= 0 && T.tk0 < m2,
                    "sweep tile %lld: planes [%d, %d) inside the slab [%d, %d)", (long long)blk, T.i0, T.i1, plo, phi);
              for (int i = T.i0; i < T.i1; ++i)
                for (int ej = 0; ej < nj; ++ej)
                  for (int ek = 0; ek < nk; ++ek) own(i, T.tj0 + ej, T.tk0 + ek);  // nd_ok of the sweeps
            }
          }
          for (int i = 0; i < m0; ++i)
            for (int j = 0; j < m1; ++j)
              for (int k = 0; k < m2; ++k)
                CHECK(seen[((size_t)i * m1 + j) * m2 + k] == (i >= plo && i < phi ? 1 : 0), "map %d, slab [%d, %d) of %d x %d x %d: point (%d, %d, %d) owned %d times", which, plo, phi, m0, m1,
                      m2, i, j, k, seen[((size_t)i * m1 + j) * m2 + k]);
        }
}

// ---- 3. the reference tables ------------------------------------------------------------------------------------------------------------------------------
static void check_tables() {
  const double ulp = 2.220446049250313e-16;
  static H8Tables T, O;
  for (int ng = 1; ng <= 4; ++ng) {
    h8_reference_tables(ng, &T);
    old_tables(ng, &O);
    SAME(memcmp(&T, &O, sizeof(T)), 0, "ng %d: the tables of the upload before the cut, bit for bit", ng);
    const int nq = ng * ng * ng, nf = ng * ng;
    double sw = 0.0, sfw = 0.0;
    for (int q = 0; q < nq; ++q) {
      sw += T.w[q];
      double sn = 0.0, sd[3] = {0.0, 0.0, 0.0};
      for (int b = 0; b < 8; ++b) {
        sn += T.N[q][b];
        for (int d = 0; d < 3; ++d) sd[d] += T.dN[q][b][d];
      }
      CHECK(std::fabs(sn - 1.0) <= 4 * ulp && std::fabs(sd[0]) <= 4 * ulp && std::fabs(sd[1]) <= 4 * ulp && std::fabs(sd[2]) <= 4 * ulp, "ng %d, Gauss point %d: N sums to 1, dN to 0", ng, q);
      CHECK(T.xi[q][3] == T.xi[q][1] * T.xi[q][2] && T.xi[q][4] == T.xi[q][0] * T.xi[q][2] && T.xi[q][5] == T.xi[q][0] * T.xi[q][1], "ng %d, Gauss point %d: the xi products", ng, q);
    }
    for (int q = 0; q < nf; ++q) {
      sfw += T.fw[q];
      double sn = 0.0, sd[2] = {0.0, 0.0};
      for (int c = 0; c < 4; ++c) {
        sn += T.fN[q][c];
        for (int d = 0; d < 2; ++d) sd[d] += T.fdN[q][c][d];
      }
      CHECK(std::fabs(sn - 1.0) <= 4 * ulp && std::fabs(sd[0]) <= 4 * ulp && std::fabs(sd[1]) <= 4 * ulp, "ng %d, face Gauss point %d: N sums to 1, dN to 0", ng, q);
    }
    CHECK(std::fabs(sw - 1.0) <= 8 * ulp && std::fabs(sfw - 1.0) <= 8 * ulp, "ng %d: weights sum to 1 (cell %.17g, face %.17g)", ng, sw, sfw);
    for (int q = nq; q < H8_MAX_Q; ++q) CHECK(T.w[q] == 0.0 && T.N[q][0] == 0.0 && T.dN[q][7][2] == 0.0, "ng %d: nothing behind the rule's last Gauss point", ng);
    for (int a = 0; a < 8; ++a)
      for (int b = 0; b < 8; ++b)
        for (int m = 0; m < 3; ++m)
          for (int n = 0; n < 3; ++n)
            CHECK(memcmp(&T.M[a][b][m][n], &T.M[b][a][n][m], sizeof(double)) == 0, "ng %d: M[%d][%d][%d][%d] and its mirror are the same bits", ng, a, b, m, n);
  }
}

int main() {
  check_knobs_and_kernels();
  check_geometry();
  check_boundary();
  for (int which = 0; which < 3; ++which) check_tile_map(which);
  check_tables();
  printf("hex8_decide: %lld cases, %lld differences from the driver before the cut, %lld property checks failed\n", cases, diffs, bad);
  if (diffs || bad) return printf("FAILED\n"), 1;
  printf("hex8_decide: OK\n");
  return 0;
}
