// CPU walk through the host decisions of the matrix-free hex-8 brick operator on elasticity (csrc/brick_operator_decide.h: bop_elasticity_*), for
// lattices from 1^3 elements (2^3 control points) to 1024^3 (1025^3), and its diagonal formula on the CPU:
//   1. the kernel per Gauss rule: the sweep for the 2-point rule alone, the per-control-point form for 1, 3 and 4 -- the residual's own default choice;
//   2. ownership: every control point is in exactly one work item -- the boxes of the sweep (marked point by point on small lattices, through the axis
//      partitions on large ones), the ranges of 256 consecutive points of the point form;
//   3. the fold: workgroup b takes the items b, b + grid, ...: every item once, balanced; the volume kernel's partial sums never exceed
//      BOP_VOLUME_PARTIALS, the face kernel's BOP_FACE_PARTIALS, a product's BOP_MAX_PARTIALS = MFEM_MAX_PARTIALS; the sizes the tests name;
//   4. launches: one without penalty faces (whatever the traction faces), two with;
//   5. the diagonal: K_(f,a),(f,a) of an element = -sum_q w det [lam g_f^2 + mu (|g|^2 + g_f^2)] with g = grad N_a from the table geometry
//      (h8_reference_tables: what k_bop_elasticity_diagonal evaluates), against the diagonal of the element matrix built column by column from unit
//      vectors through sf_elasticity_fe (what the sweep integrates), on affine and distorted elements, for the 1- to 4-point rules.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_operator_elasticity.cpp -o tools/bin/host_check_brick_operator_elasticity
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
#include "brick_operator_decide.h"
#include "hex8_sumfac.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

// ---- 2a. point by point ------------------------------------------------------------------------------------------------------------------------------
static void mark_points(int ng, int m0, int m1, int m2) {
  const BopVolume V = bop_elasticity_volume(ng, m0, m1, m2);
  const int64_t n = (int64_t)m0 * m1 * m2;
  std::vector<unsigned char> seen((size_t)n, 0);
  for (int64_t w = 0; w < V.items; ++w) {
    if (V.kernel == BOP_SWEEP) {
      const BopBox b = bop_item_box(V, w, m0, m1, m2);
      const bool in = b.i0 >= 0 && b.i0 < b.i1 && b.i1 <= m0 && b.j0 >= 0 && b.j0 < b.j1 && b.j1 <= m1 && b.k0 >= 0 && b.k0 < b.k1 && b.k1 <= m2;
      CHECK(in, "ng %d, %d x %d x %d, item %lld: an empty box or one outside the lattice", ng, m0, m1, m2, (long long)w);
      if (!in) continue;
      for (int i = b.i0; i < b.i1; ++i)
        for (int j = b.j0; j < b.j1; ++j)
          for (int k = b.k0; k < b.k1; ++k) ++seen[((size_t)i * m1 + j) * m2 + k];
    } else {
      const BopRange r = bop_point_range(w, n);
      CHECK(r.first >= 0 && r.first < r.last && r.last <= n && r.last - r.first <= H8_BLOCK, "ng %d, %d x %d x %d, item %lld: an empty range or one outside the lattice", ng, m0,
            m1, m2, (long long)w);
      if (r.first < 0 || r.last > n) continue;
      for (int64_t t = r.first; t < r.last; ++t) ++seen[(size_t)t];
    }
  }
  long long wrong = 0;
  for (unsigned char c : seen) wrong += c != 1;
  CHECK(wrong == 0, "ng %d, %d x %d x %d: %lld control points not owned exactly once", ng, m0, m1, m2, wrong);
}

// ---- 2b. the large lattices ---------------------------------------------------------------------------------------------------------------------------
struct Axis {
  std::set<std::pair<int, int>> iv;
  bool partitions(int m) const {
    int at = 0;
    for (const auto& p : iv) {  // (sorted by first)
      if (p.first != at || p.second <= p.first) return false;
      at = p.second;
    }
    return at == m;
  }
};
static void large(int ng, int m0, int m1, int m2) {
  const BopVolume V = bop_elasticity_volume(ng, m0, m1, m2);
  const int64_t n = (int64_t)m0 * m1 * m2;
  if (V.kernel == BOP_POINTS) {  // consecutive ranges: item w starts where item w - 1 ended, the last ends at n
    int64_t at = 0;
    bool ok = true;
    for (int64_t w = 0; w < V.items; ++w) {
      const BopRange r = bop_point_range(w, n);
      ok = ok && r.first == at && r.last > r.first;
      at = r.last;
    }
    CHECK(ok && at == n, "ng %d, %d x %d x %d: the ranges do not partition the control points", ng, m0, m1, m2);
    return;
  }
  Axis a[3];
  long long volume = 0;
  for (int64_t w = 0; w < V.items; ++w) {
    const BopBox b = bop_item_box(V, w, m0, m1, m2);
    a[0].iv.insert({b.i0, b.i1});
    a[1].iv.insert({b.j0, b.j1});
    a[2].iv.insert({b.k0, b.k1});
    volume += (long long)(b.i1 - b.i0) * (b.j1 - b.j0) * (b.k1 - b.k0);
  }
  CHECK(a[0].partitions(m0) && a[1].partitions(m1) && a[2].partitions(m2), "ng %d, %d x %d x %d: the boxes' extents do not partition an axis", ng, m0, m1, m2);
  const int64_t n0 = (int64_t)a[0].iv.size(), n1 = (int64_t)a[1].iv.size(), n2 = (int64_t)a[2].iv.size();
  CHECK(n0 * n1 * n2 == V.items && volume == n, "ng %d, %d x %d x %d: %lld items for %lld boxes holding %lld points", ng, m0, m1, m2, (long long)V.items,
        (long long)(n0 * n1 * n2), volume);
  if (n0 * n1 * n2 != V.items) return;
  std::vector<int> s0, s1, s2;
  for (const auto& p : a[0].iv) s0.push_back(p.first);
  for (const auto& p : a[1].iv) s1.push_back(p.first);
  for (const auto& p : a[2].iv) s2.push_back(p.first);
  const int st0 = n0 > 1 ? s0[1] : m0, st1 = n1 > 1 ? s1[1] : m1, st2 = n2 > 1 ? s2[1] : m2;
  std::vector<unsigned char> seen((size_t)V.items, 0);
  for (int64_t w = 0; w < V.items; ++w) {
    const BopBox b = bop_item_box(V, w, m0, m1, m2);
    const int64_t t = ((int64_t)(b.i0 / st0) * n1 + b.j0 / st1) * n2 + b.k0 / st2;
    if (t >= 0 && t < V.items) ++seen[(size_t)t];
  }
  long long wrong = 0;
  for (unsigned char c : seen) wrong += c != 1;
  CHECK(wrong == 0, "ng %d, %d x %d x %d: %lld boxes not taken exactly once", ng, m0, m1, m2, wrong);
}

// ---- 3. the fold and the caps ---------------------------------------------------------------------------------------------------------------------------
static void caps(int ng, int m0, int m1, int m2) {
  const BopVolume V = bop_elasticity_volume(ng, m0, m1, m2);
  CHECK(V.items >= 1 && V.grid >= 1 && V.grid <= BOP_VOLUME_PARTIALS && V.grid <= V.items, "ng %d, %d x %d x %d: grid %d for %lld items", ng, m0, m1, m2,
        V.grid, (long long)V.items);
  const int64_t q = V.items / V.grid, r = V.items % V.grid;
  CHECK(r * (q + 1) + (V.grid - r) * q == V.items, "ng %d, %d x %d x %d: the fold loses items", ng, m0, m1, m2);
  CHECK(V.rounds == (V.items + BOP_VOLUME_PARTIALS - 1) / BOP_VOLUME_PARTIALS && (r == 0 ? q == V.rounds : q + 1 == V.rounds), "ng %d, %d x %d x %d: %d rounds, %lld or %lld items per workgroup",
        ng, m0, m1, m2, V.rounds, (long long)q, (long long)q + 1);
  CHECK((V.items <= BOP_VOLUME_PARTIALS) == (V.grid == V.items), "ng %d, %d x %d x %d: a grid below the cap is one workgroup per item", ng, m0, m1, m2);
  CHECK(bop_volume_grid(V, true) == V.grid && bop_volume_grid(V, false) == V.items && V.items < ((int64_t)1 << 31), "ng %d, %d x %d x %d: the grid with and without partial sums", ng, m0, m1, m2);
  if (V.kernel == BOP_SWEEP) {
    const H8Sweep S = h8_residual_sweep(m1, m2, m0);
    CHECK(V.L == S.L && V.items == S.grid && V.threads == SW_THREADS, "ng %d, %d x %d x %d: not the residual sweep's segments", ng, m0, m1, m2);
  } else {
    CHECK(V.L == 0 && V.items == h8_point_grid((int64_t)m0 * m1 * m2) && V.threads == H8_BLOCK, "ng %d, %d x %d x %d: not the residual's point grid", ng, m0, m1, m2);
  }
  const int fg = bop_face_grid(bop_boundary_count(m0, m1, m2));
  CHECK(fg >= 1 && fg <= BOP_FACE_PARTIALS && V.grid + fg <= BOP_MAX_PARTIALS, "%d x %d x %d: %d partial sums", m0, m1, m2, V.grid + fg);
}

// ---- 5. the diagonal formula -----------------------------------------------------------------------------------------------------------------------------
// bop_geom on the CPU: g[b][s] and w det at Gauss point q from the tables (node b = bx + 2 by + 4 bz)
static double table_geom(const H8Tables& T, const double (&X)[8][3], int q, double (&g)[8][3]) {
  double J[3][3];
  for (int i = 0; i < 3; ++i)
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
      for (int b = 0; b < 8; ++b) s += T.dN[q][b][m] * X[b][i];
      J[i][m] = s;
    }
  const double det = J[0][0] * J[1][1] * J[2][2] - J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] + J[0][1] * J[1][2] * J[2][0] +
                     J[0][2] * J[1][0] * J[2][1] - J[0][2] * J[1][1] * J[2][0];
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
  for (int b = 0; b < 8; ++b)
    for (int s = 0; s < 3; ++s) g[b][s] = T.dN[q][b][0] * I[0][s] + T.dN[q][b][1] * I[1][s] + T.dN[q][b][2] * I[2][s];
  return T.w[q] * det;
}
template <int NG>
static void diagonal_formula(const double (&X8)[8][3], double lam, double mu, const char* what) {
  static H8Tables T;
  h8_reference_tables(NG, &T);
  double Xs[3][2][4];  // the sweep's layout: X[d][bx][by + 2 bz]
  for (int b = 0; b < 8; ++b)
    for (int d = 0; d < 3; ++d) Xs[d][b & 1][b >> 1] = X8[b][d];
  double scale = 0.0, worst = 0.0;
  for (int a = 0; a < 8; ++a)
    for (int f = 0; f < 3; ++f) {
      double formula = 0.0;
      for (int q = 0; q < NG * NG * NG; ++q) {
        double g[8][3];
        const double wd = table_geom(T, X8, q, g);
        const double g2 = g[a][0] * g[a][0] + g[a][1] * g[a][1] + g[a][2] * g[a][2];
        formula -= wd * (lam * (g[a][f] * g[a][f]) + mu * (g2 + g[a][f] * g[a][f]));
      }
      double U[3][2][4], fe[3][2][4];
      memset(U, 0, sizeof(U));
      U[f][a & 1][a >> 1] = 1.0;  // the unit vector of unknown (f, a): fe is column (f, a) of the element matrix
      sf_elasticity_fe<NG>(Xs, U, lam, mu, fe);
      const double entry = fe[f][a & 1][a >> 1];
      scale = fmax(scale, fabs(entry));
      worst = fmax(worst, fabs(entry - formula));
      CHECK(entry < 0.0, "%s, ng %d: a diagonal entry of K that is not negative", what, NG);
    }
  // two evaluations of the same sums of 8 - 64 products in different orders: a few hundred ulp at the most
  CHECK(worst <= 1e-13 * scale, "%s, ng %d: the diagonal formula is off by %.3e of %.3e", what, NG, worst, scale);
}
static void diagonals() {
  double cube[8][3], skew[8][3], bent[8][3];
  for (int b = 0; b < 8; ++b) {
    const double r[3] = {(double)(b & 1), (double)((b >> 1) & 1), (double)(b >> 2)};
    for (int d = 0; d < 3; ++d) cube[b][d] = 0.3 * r[d] + 0.1 * d;
    skew[b][0] = 0.5 * r[0] + 0.1 * r[1] - 0.05 * r[2] + 1.0;  // affine: a parallelepiped
    skew[b][1] = 0.05 * r[0] + 0.4 * r[1] + 0.1 * r[2] - 2.0;
    skew[b][2] = -0.1 * r[0] + 0.02 * r[1] + 0.6 * r[2];
    bent[b][0] = skew[b][0] + 0.04 * r[1] * r[2] - 0.03 * r[0] * r[1] * r[2];  // trilinear: the Jacobian varies in the element
    bent[b][1] = skew[b][1] + 0.05 * r[0] * r[2];
    bent[b][2] = skew[b][2] - 0.06 * r[0] * r[1] + 0.02 * r[0] * r[1] * r[2];
  }
  const double lam = 0.5769230769230769, mu = 0.3846153846153846;
  diagonal_formula<1>(cube, lam, mu, "cube"); diagonal_formula<2>(cube, lam, mu, "cube"); diagonal_formula<3>(cube, lam, mu, "cube"); diagonal_formula<4>(cube, lam, mu, "cube");
  diagonal_formula<1>(skew, lam, mu, "skew"); diagonal_formula<2>(skew, lam, mu, "skew"); diagonal_formula<3>(skew, lam, mu, "skew"); diagonal_formula<4>(skew, lam, mu, "skew");
  diagonal_formula<1>(bent, lam, mu, "bent"); diagonal_formula<2>(bent, lam, mu, "bent"); diagonal_formula<3>(bent, lam, mu, "bent"); diagonal_formula<4>(bent, lam, mu, "bent");
  diagonal_formula<2>(bent, 0.0, 1.0, "bent, lam = 0"); diagonal_formula<2>(bent, 1.0, 0.0, "bent, mu = 0 (may vanish in a field: only the sign)");
}

int main() {
  // 1. the kernel per rule
  const BopKernel want[5] = {BOP_POINTS, BOP_POINTS, BOP_SWEEP, BOP_POINTS, BOP_POINTS};
  for (int ng = 1; ng <= 4; ++ng) {
    CHECK(bop_elasticity_kernel(ng) == want[ng], "ng %d", ng);
    CHECK((bop_elasticity_kernel(ng) == BOP_SWEEP) == (h8_elasticity_residual_kernel(h8_elasticity_knobs(0), ng) == H8_EL_RESIDUAL_SWEEP), "ng %d: not the residual's choice", ng);
    CHECK(bop_elasticity_volume(ng, 9, 9, 9).kernel == want[ng], "ng %d: the volume launch's kernel", ng);
  }
  // 2a.: every lattice from 1^3 to 6^3 elements, then shapes around the tile (15 / 16), segment (4) and block (256) edges
  for (int ng = 1; ng <= 2; ++ng)
    for (int m0 = 2; m0 <= 7; ++m0)
      for (int m1 = 2; m1 <= 7; ++m1)
        for (int m2 = 2; m2 <= 7; ++m2) mark_points(ng, m0, m1, m2);
  const int edge[][3] = {{10, 15, 16}, {6, 17, 31}, {41, 46, 46}, {5, 5, 4}, {4, 5, 3}, {9, 8, 7}, {33, 16, 30}, {34, 31, 17}, {13, 45, 2}, {2, 2, 65}, {65, 2, 2}, {9, 9, 9},
                         {4, 8, 8}, {16, 16, 1 + 1}, {16, 16, 16}, {257, 1 + 1, 1 + 1}};
  for (const auto& e : edge)
    for (int ng = 1; ng <= 4; ++ng) {
      mark_points(ng, e[0], e[1], e[2]);
      large(ng, e[0], e[1], e[2]);
    }
  // 2b.: the large lattices, cubes and not
  const int big[][3] = {{129, 129, 129}, {257, 257, 257}, {513, 513, 513}, {769, 769, 769}, {1025, 1025, 1025}, {1025, 2, 513}, {2, 1025, 1025}, {1024, 1023, 1021}};
  for (const auto& e : big)
    for (int ng = 1; ng <= 2; ++ng) large(ng, e[0], e[1], e[2]);
  // 3.: every combination of sizes that hold every tile, segment and cap boundary up to 1025
  std::vector<int> sizes;
  for (int m = 2; m <= 34; ++m) sizes.push_back(m);
  for (int m : {45, 46, 47, 60, 61, 63, 64, 65, 66, 90, 91, 97, 100, 127, 128, 129, 130, 255, 256, 257, 258, 383, 384, 385, 511, 512, 513, 514, 621, 639, 640, 641, 767, 768, 769, 770,
                895, 896, 897, 959, 960, 961, 1009, 1010, 1011, 1020, 1021, 1022, 1023, 1024, 1025})
    sizes.push_back(m);
  for (int ng = 1; ng <= 2; ++ng)
    for (int m0 : sizes)
      for (int m1 : sizes)
        for (int m2 : sizes) caps(ng, m0, m1, m2);
  {  // the sizes the GPU tests name
    const BopVolume S = bop_elasticity_volume(2, 5, 641, 621);
    CHECK(S.kernel == BOP_SWEEP && S.items == 43 * 42 * 2 && S.rounds == 2 && S.grid == 1806, "(4, 640, 620): %lld items, grid %d", (long long)S.items, S.grid);
    const BopVolume P = bop_elasticity_volume(1, 97, 97, 100);
    CHECK(P.kernel == BOP_POINTS && P.items == 3676 && P.rounds == 2 && P.grid == 1838, "(96, 96, 99): %lld items, grid %d", (long long)P.items, P.grid);
    const BopVolume W = bop_elasticity_volume(2, 513, 513, 513);
    CHECK(W.items == 35 * 35 * 17 && W.rounds == 6 && W.grid == 3471, "512^3: %lld items, grid %d", (long long)W.items, W.grid);
    const BopVolume Q = bop_elasticity_volume(3, 513, 513, 513);
    CHECK(Q.items == 527367 && Q.rounds == 148 && Q.grid == 3564, "512^3, point form: %lld items, grid %d", (long long)Q.items, Q.grid);
  }
  // 4.: launches
  CHECK(bop_elasticity_launches(0.0, 0x3f) == 1 && bop_elasticity_launches(1000.0, 0) == 1, "no penalty term: one launch");
  CHECK(bop_elasticity_launches(1000.0, 0x10) == 2 && bop_elasticity_face_launch(1.0, 0x3f), "penalty faces: two launches");
  CHECK(bop_elasticity_face_launch(1.0, 0x10) == h8_elasticity_faces_launch(1.0, 0x10, 0) && !bop_elasticity_face_launch(0.0, 0x10), "the residual's launch test without traction");
  CHECK(bop_refusal(1, 0, 9, 9) == nullptr && bop_refusal(2, 0, 9, 9) != nullptr && bop_refusal(1, 2, 9, 9) != nullptr, "the refusals are the thermal operator's");
  // 5.
  diagonals();
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
