// CPU walk through the host decisions of the matrix-free hex-27 brick operator (csrc/brick_operator_hex27_decide.h), for lattices from 1^3 to 513^3
// elements:
//   1. ownership: the work items of the volume kernel put every control point into exactly one item -- marked point by point on small lattices, and
//      through the axis partitions the boxes are a product of on the large ones;
//   2. adjacency: every element adjacent to a point an item owns is among the elements the item integrates, the element-vector block (B27_EH^2 slots
//      from (Jb, Kb)) holds every integrated column, a tile owns at most B27_NP lines per direction, and the first element plane whose lower two
//      control-point planes an item writes is its first owned one;
//   3. the fold: every item once, at most BOP_VOLUME_PARTIALS partial sums of the volume kernel, BOP_MAX_PARTIALS of a product;
//   4. the LDS block of every Gauss rule stays within the limit the header declares, the limit itself within a gfx950 CU's 160 KB, and the per-wave
//      carve-up's overlays do not collide;
//   5. the redundancy R = elements integrated / elements of the brick, printed for the cubes and asserted <= 1.3 at 128^3, 256^3 and 512^3;
//   6. the diagonal formula of k_brick27_diagonal, evaluated on the CPU, against element matrices built from unit vectors on distorted elements, and
//      the adjacent-element enumeration (b27_face_elements) against a brute-force search;
//   7. the refusals.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_operator_hex27.cpp -o tools/bin/host_check_brick_operator_hex27
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
#include "brick_operator_hex27_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

// ---- 1a. + 2. point by point -----------------------------------------------------------------------------------------------------------------------
static void mark_points(int ne0, int ne1, int ne2) {
  const int m0 = 2 * ne0 + 1, m1 = 2 * ne1 + 1, m2 = 2 * ne2 + 1;
  const B27Volume V = b27_volume(ne0, ne1, ne2);
  std::vector<unsigned char> seen((size_t)m0 * m1 * m2, 0);
  for (int64_t w = 0; w < V.items; ++w) {
    const B27Item b = b27_item(V, w, ne0, ne1, ne2);
    const bool in = b.i0 >= 0 && b.i0 < b.i1 && b.i1 <= m0 && b.j0 >= 0 && b.j0 < b.j1 && b.j1 <= m1 && b.k0 >= 0 && b.k0 < b.k1 && b.k1 <= m2;
    CHECK(in, "%d x %d x %d elements, item %lld: an empty box or one outside the lattice", ne0, ne1, ne2, (long long)w);
    if (!in) continue;
    long long miss = 0;
    for (int i = b.i0; i < b.i1; ++i)
      for (int j = b.j0; j < b.j1; ++j)
        for (int k = b.k0; k < b.k1; ++k) {
          ++seen[((size_t)i * m1 + j) * m2 + k];
          int E[3][2], c[3][2];
          const int n0 = b27_face_elements(i, ne0, E[0], c[0]), n1 = b27_face_elements(j, ne1, E[1], c[1]), n2 = b27_face_elements(k, ne2, E[2], c[2]);
          for (int a = 0; a < n0; ++a) miss += !(E[0][a] >= b.I0 && E[0][a] < b.I1);
          for (int a = 0; a < n1; ++a) miss += !(E[1][a] >= b.J0 && E[1][a] < b.J1);
          for (int a = 0; a < n2; ++a) miss += !(E[2][a] >= b.K0 && E[2][a] < b.K1);
        }
    CHECK(miss == 0, "%d x %d x %d elements, item %lld: %lld adjacent elements not integrated", ne0, ne1, ne2, (long long)w, miss);
  }
  long long wrong = 0;
  for (unsigned char c : seen) wrong += c != 1;
  CHECK(wrong == 0, "%d x %d x %d elements: %lld control points not owned exactly once", ne0, ne1, ne2, wrong);
}

// ---- 1b. + 2. + 5. through the axes ------------------------------------------------------------------------------------------------------------------
struct Axis {
  std::set<std::pair<int, int>> iv;
  bool partitions(int m) const {
    int at = 0;
    for (const auto& p : iv) {
      if (p.first != at || p.second <= p.first) return false;
      at = p.second;
    }
    return at == m;
  }
};
static int lowest_element(int p) { return p % 2 ? (p - 1) / 2 : (p / 2 - 1 < 0 ? 0 : p / 2 - 1); }           // of those that contain lattice index p
static int highest_element(int p, int ne) { return p % 2 ? (p - 1) / 2 : (p / 2 < ne ? p / 2 : p / 2 - 1); }
static double walk_items(int ne0, int ne1, int ne2, bool print) {
  const int m0 = 2 * ne0 + 1, m1 = 2 * ne1 + 1, m2 = 2 * ne2 + 1;
  const B27Volume V = b27_volume(ne0, ne1, ne2);
  Axis a[3];
  long long integrated = 0, volume = 0;
  std::set<std::pair<std::pair<int, int>, int>> boxes;
  for (int64_t w = 0; w < V.items; ++w) {
    const B27Item b = b27_item(V, w, ne0, ne1, ne2);
    a[0].iv.insert({b.i0, b.i1});
    a[1].iv.insert({b.j0, b.j1});
    a[2].iv.insert({b.k0, b.k1});
    boxes.insert({{b.i0, b.j0}, b.k0});
    volume += (long long)(b.i1 - b.i0) * (b.j1 - b.j0) * (b.k1 - b.k0);
    integrated += (long long)(b.I1 - b.I0) * (b.J1 - b.J0) * (b.K1 - b.K0);
    // the elements adjacent to the box's extreme points are integrated, and no others (the axes are independent: the extremes decide)
    CHECK(b.I0 == lowest_element(b.i0) && b.I1 == highest_element(b.i1 - 1, ne0) + 1, "%d x %d x %d, item %lld: element planes [%d, %d) for points [%d, %d)", ne0, ne1, ne2,
          (long long)w, b.I0, b.I1, b.i0, b.i1);
    CHECK(b.J0 == lowest_element(b.j0) && b.J1 == highest_element(b.j1 - 1, ne1) + 1, "%d x %d x %d, item %lld: element columns [%d, %d) for lines [%d, %d)", ne0, ne1, ne2,
          (long long)w, b.J0, b.J1, b.j0, b.j1);
    CHECK(b.K0 == lowest_element(b.k0) && b.K1 == highest_element(b.k1 - 1, ne2) + 1, "%d x %d x %d, item %lld: element columns [%d, %d) for points [%d, %d)", ne0, ne1, ne2,
          (long long)w, b.K0, b.K1, b.k0, b.k1);
    // the workgroup's blocks hold them
    CHECK(b.j1 - b.j0 <= B27_NP && b.k1 - b.k0 <= B27_NP, "item %lld: more than B27_NP lines", (long long)w);
    CHECK(b.J0 - b.Jb >= 0 && b.J1 - 1 - b.Jb < B27_EH && b.K0 - b.Kb >= 0 && b.K1 - 1 - b.Kb < B27_EH, "item %lld: an element column outside the 9 x 9 block", (long long)w);
    CHECK(2 * b.Iown == b.i0 && b.Iown >= b.I0 && b.Iown <= b.I0 + 1 && b.Iown < b.I1, "item %lld: first written plane", (long long)w);
    CHECK(b.last_seg == (b.i1 == m0) && (b.last_seg ? b.i1 == 2 * b.I1 + 1 : b.i1 == 2 * b.I1), "item %lld: last plane", (long long)w);
  }
  CHECK(a[0].partitions(m0) && a[1].partitions(m1) && a[2].partitions(m2), "%d x %d x %d elements: the boxes' extents do not partition an axis", ne0, ne1, ne2);
  CHECK((int64_t)a[0].iv.size() * (int64_t)a[1].iv.size() * (int64_t)a[2].iv.size() == V.items && (int64_t)boxes.size() == V.items,
        "%d x %d x %d elements: %lld items, %zu distinct boxes", ne0, ne1, ne2, (long long)V.items, boxes.size());
  CHECK(volume == (long long)m0 * m1 * m2, "%d x %d x %d elements: the boxes hold %lld points", ne0, ne1, ne2, volume);
  const double R = (double)integrated / ((double)ne0 * ne1 * ne2);
  if (print) printf("R(%d x %d x %d elements) = %.4f  (L = %d, %lld items, grid %d in %d rounds)\n", ne0, ne1, ne2, R, V.L, (long long)V.items, V.grid, V.rounds);
  return R;
}

// ---- 3. the fold and the caps ---------------------------------------------------------------------------------------------------------------------------
static void caps(int ne0, int ne1, int ne2) {
  const B27Volume V = b27_volume(ne0, ne1, ne2);
  CHECK(V.items >= 1 && V.grid >= 1 && V.grid <= BOP_VOLUME_PARTIALS && V.grid <= V.items, "%d x %d x %d: grid %d for %lld items", ne0, ne1, ne2, V.grid, (long long)V.items);
  const int64_t q = V.items / V.grid, r = V.items % V.grid;
  CHECK(r * (q + 1) + (V.grid - r) * q == V.items, "%d x %d x %d: the fold loses items", ne0, ne1, ne2);
  CHECK(V.rounds == (V.items + BOP_VOLUME_PARTIALS - 1) / BOP_VOLUME_PARTIALS && (r == 0 ? q == V.rounds : q + 1 == V.rounds), "%d x %d x %d: %d rounds", ne0, ne1, ne2, V.rounds);
  CHECK((V.items <= BOP_VOLUME_PARTIALS) == (V.grid == V.items), "%d x %d x %d: a grid below the cap is one workgroup per item", ne0, ne1, ne2);
  CHECK(b27_volume_grid(V, true) == V.grid && b27_volume_grid(V, false) == V.items && V.items < ((int64_t)1 << 31), "%d x %d x %d: the grids", ne0, ne1, ne2);
  CHECK(V.L >= B27_LMIN && V.L <= B27_LMAX && (V.L & (V.L - 1)) == 0 && V.nseg == (ne0 + V.L - 1) / V.L, "L = %d", V.L);
  const int fg = bop_face_grid(bop_boundary_count(2 * ne0 + 1, 2 * ne1 + 1, 2 * ne2 + 1));
  CHECK(fg >= 1 && fg <= BOP_FACE_PARTIALS && V.grid + fg <= BOP_MAX_PARTIALS && BOP_MAX_PARTIALS <= 4096, "%d x %d x %d: %d partial sums", ne0, ne1, ne2, V.grid + fg);
}

// ---- 6. the diagonal formula ----------------------------------------------------------------------------------------------------------------------------
static const double GP[4][4] = {{0.0, 0, 0, 0}, {-0.57735026918962576451, 0.57735026918962576451, 0, 0}, {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double GW[4][4] = {{2.0, 0, 0, 0}, {1.0, 1.0, 0, 0}, {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};
static void lag2(double x, double* L, double* dL) {
  L[0] = 2.0 * (x - 0.5) * (x - 1.0); L[1] = -4.0 * x * (x - 1.0); L[2] = 2.0 * x * (x - 0.5);
  dL[0] = 4.0 * x - 3.0; dL[1] = -8.0 * x + 4.0; dL[2] = 4.0 * x - 1.0;
}
struct Quad {  // one Gauss point of an element: w det and the physical gradients of the 27 basis functions
  double wd, g[27][3];
};
static Quad quad_point(const double X[27][3], int ng, int q) {
  const int q0 = q % ng, q1 = (q / ng) % ng, q2 = q / (ng * ng);
  double L[3][3], dL[3][3];
  lag2(GP[ng - 1][q0] / 2 + 0.5, L[0], dL[0]);
  lag2(GP[ng - 1][q1] / 2 + 0.5, L[1], dL[1]);
  lag2(GP[ng - 1][q2] / 2 + 0.5, L[2], dL[2]);
  double dn[27][3], J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int b = 0; b < 27; ++b) {
    const int b0 = b % 3, b1 = (b / 3) % 3, b2 = b / 9;
    dn[b][0] = dL[0][b0] * L[1][b1] * L[2][b2];
    dn[b][1] = L[0][b0] * dL[1][b1] * L[2][b2];
    dn[b][2] = L[0][b0] * L[1][b1] * dL[2][b2];
    for (int i = 0; i < 3; ++i)
      for (int m = 0; m < 3; ++m) J[i][m] += dn[b][m] * X[b][i];
  }
  const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
  double Iv[3][3];
  Iv[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) / det; Iv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det; Iv[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) / det;
  Iv[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) / det; Iv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det; Iv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
  Iv[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) / det; Iv[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) / det; Iv[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) / det;
  Quad Q;
  Q.wd = GW[ng - 1][q0] * GW[ng - 1][q1] * GW[ng - 1][q2] / 8 * det;
  for (int b = 0; b < 27; ++b)
    for (int s = 0; s < 3; ++s) Q.g[b][s] = dn[b][0] * Iv[0][s] + dn[b][1] * Iv[1][s] + dn[b][2] * Iv[2][s];
  return Q;
}
// fe = Ke T, the way the product integrates it: grad T at the Gauss point first
static void element_vector(const double X[27][3], int ng, double k, const double T[27], double fe[27]) {
  for (int a = 0; a < 27; ++a) fe[a] = 0.0;
  for (int q = 0; q < ng * ng * ng; ++q) {
    const Quad Q = quad_point(X, ng, q);
    double gT[3] = {0, 0, 0};
    for (int b = 0; b < 27; ++b)
      for (int s = 0; s < 3; ++s) gT[s] += Q.g[b][s] * T[b];
    for (int a = 0; a < 27; ++a) fe[a] += -k * Q.wd * (Q.g[a][0] * gT[0] + Q.g[a][1] * gT[1] + Q.g[a][2] * gT[2]);
  }
}
// the kernel's formula: sum_q (-k w det) |grad N_a|^2
static double diagonal_entry(const double X[27][3], int ng, double k, int a) {
  double acc = 0.0;
  for (int q = 0; q < ng * ng * ng; ++q) {
    const Quad Q = quad_point(X, ng, q);
    acc += (-k * Q.wd) * (Q.g[a][0] * Q.g[a][0] + Q.g[a][1] * Q.g[a][1] + Q.g[a][2] * Q.g[a][2]);
  }
  return acc;
}
static void lattice_point(int i, int j, int k, int m0, int m1, int m2, double x[3]) {  // a smooth distortion of the unit lattice
  const double u = (double)i / (m0 - 1), v = (double)j / (m1 - 1), w = (double)k / (m2 - 1);
  x[0] = 1.3 * u + 0.06 * sin(2.1 * v + 0.4) * cos(1.7 * w);
  x[1] = 0.9 * v + 0.05 * sin(1.9 * w + 0.3) * cos(2.3 * u);
  x[2] = 1.1 * w + 0.04 * sin(2.2 * u + 0.2) * cos(1.3 * v);
}
static void diagonal(int ng, int ne0, int ne1, int ne2) {
  const int m0 = 2 * ne0 + 1, m1 = 2 * ne1 + 1, m2 = 2 * ne2 + 1;
  const double kc = 0.6;
  std::vector<double> brute((size_t)m0 * m1 * m2, 0.0);
  auto coords = [&](int I, int J, int K, double X[27][3]) {
    for (int b = 0; b < 27; ++b) lattice_point(2 * I + b % 3, 2 * J + (b / 3) % 3, 2 * K + b / 9, m0, m1, m2, X[b]);
  };
  for (int I = 0; I < ne0; ++I)
    for (int J = 0; J < ne1; ++J)
      for (int K = 0; K < ne2; ++K) {
        double X[27][3];
        coords(I, J, K, X);
        for (int a = 0; a < 27; ++a) {  // Ke[a][a] from the unit vector e_a
          double T[27] = {0}, fe[27];
          T[a] = 1.0;
          element_vector(X, ng, kc, T, fe);
          brute[((size_t)(2 * I + a % 3) * m1 + 2 * J + (a / 3) % 3) * m2 + 2 * K + a / 9] += fe[a];
        }
      }
  double worst = 0.0, scale = 0.0;
  for (int i = 0; i < m0; ++i)
    for (int j = 0; j < m1; ++j)
      for (int k = 0; k < m2; ++k) {
        int E[3][2], c[3][2];
        const int n0 = b27_face_elements(i, ne0, E[0], c[0]), n1 = b27_face_elements(j, ne1, E[1], c[1]), n2 = b27_face_elements(k, ne2, E[2], c[2]);
        double sum = 0.0;
        for (int e0 = 0; e0 < n0; ++e0)
          for (int e1 = 0; e1 < n1; ++e1)
            for (int e2 = 0; e2 < n2; ++e2) {
              double X[27][3];
              coords(E[0][e0], E[1][e1], E[2][e2], X);
              sum += diagonal_entry(X, ng, kc, c[0][e0] + 3 * c[1][e1] + 9 * c[2][e2]);
            }
        const double ref = brute[((size_t)i * m1 + j) * m2 + k];
        worst = fmax(worst, fabs(sum - ref));
        scale = fmax(scale, fabs(ref));
      }
  CHECK(scale > 0.0 && worst <= 1e-13 * scale, "ng %d, %d x %d x %d elements: diagonal formula off by %.3e of %.3e", ng, ne0, ne1, ne2, worst, scale);
}

int main() {
  // 1a. + 2.: every lattice from 1^3 to 5^3 elements, then shapes around the tile (8) and segment (4 .. 32) edges
  for (int a = 1; a <= 5; ++a)
    for (int b = 1; b <= 5; ++b)
      for (int c = 1; c <= 5; ++c) mark_points(a, b, c);
  const int edge[][3] = {{9, 9, 9}, {8, 8, 8}, {7, 16, 17}, {33, 9, 1}, {65, 7, 9}, {1, 40, 41}, {4, 24, 25}, {5, 1, 64}, {17, 15, 23}};
  for (const auto& e : edge) {
    mark_points(e[0], e[1], e[2]);
    walk_items(e[0], e[1], e[2], false);
  }
  // 1b. + 2. + 5.: the large lattices
  const int big[][3] = {{1, 1, 1}, {16, 16, 16}, {32, 32, 32}, {64, 64, 64}, {128, 128, 128}, {256, 256, 256}, {512, 512, 512}, {513, 513, 513}, {513, 1, 257}, {1, 513, 513}, {511, 509, 127}};
  for (const auto& e : big) {
    const double R = walk_items(e[0], e[1], e[2], true);
    if (e[0] == e[1] && e[1] == e[2] && e[0] >= 128 && e[0] % B27_LMAX == 0) CHECK(R <= 1.3, "R at %d^3 = %.4f", e[0], R);  // (whole tiles and segments: the flagship's 128^3 among them)
  }
  // 3.: every combination of sizes that hold every tile, segment and cap boundary up to 513
  std::vector<int> sizes;
  for (int n = 1; n <= 18; ++n) sizes.push_back(n);
  for (int n : {31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 479, 480, 481, 511, 512, 513}) sizes.push_back(n);
  for (int a : sizes)
    for (int b : sizes)
      for (int c : sizes) caps(a, b, c);
  {  // a one-element-thick brick whose items exceed the cap: folded
    const B27Volume V = b27_volume(1, 513, 513);
    CHECK(V.items == 65 * 65 && V.rounds == 2 && V.grid == 2113 && V.grid <= BOP_VOLUME_PARTIALS, "1 x 513 x 513: %lld items, grid %d", (long long)V.items, V.grid);
  }
  // 4.: LDS
  CHECK(B27_LDS_LIMIT <= 160 * 1024, "the declared limit is a gfx950 CU's LDS");
  for (int ng = 1; ng <= 4; ++ng) {
    const int nq = ng * ng * ng;
    CHECK(b27_lds_bytes(ng) <= B27_LDS_LIMIT, "ng %d: %zu bytes of LDS", ng, b27_lds_bytes(ng));
    CHECK(b27_w_t1() + b27_n1(ng) <= b27_w_t2(ng) && b27_n3(ng) <= b27_w_t2(ng) && b27_pad(b27_na(ng)) + b27_nb(ng) <= b27_w_t2(ng), "ng %d: X | T1, J | GX and VA | WB below T2", ng);
    CHECK(b27_n2(ng) <= b27_w_d(ng) - b27_w_t2(ng) && 3 * nq <= b27_w_d(ng) - b27_w_t2(ng) && b27_w_d(ng) + nq <= b27_w_size(ng), "ng %d: T2 / flux below w det", ng);
    CHECK(b27_off_tab1(ng) >= nq && b27_off_dec(ng) - b27_off_tab1(ng) >= 8 * ng && 2 * (b27_off_fe(ng) - b27_off_dec(ng)) >= b27_ndec(ng) &&
              b27_off_waves(ng) - b27_off_fe(ng) >= B27_EH * B27_EH * 27, "ng %d: the shared block", ng);
    CHECK(3 * (ng * ng - 1) + 2 < (1 << 12) && 4 * (2 * ng) < (1 << 15) && b27_w_size(ng) < (1 << 16), "ng %d: the decode words' fields", ng);
    printf("LDS(ng = %d) = %zu bytes\n", ng, b27_lds_bytes(ng));
  }
  CHECK(B27_NP * B27_NP <= B27_THREADS && B27_EH * B27_EH >= B27_WAVES, "a thread per owned column");
  // 6.
  for (int ng = 1; ng <= 4; ++ng) diagonal(ng, 2, 2, 2);
  diagonal(3, 1, 1, 1);
  diagonal(3, 1, 2, 3);
  // 7.
  CHECK(bop27_refusal(2, 0, 9, 9) == nullptr, "a whole hex-27 brick is taken");
  CHECK(bop27_refusal(1, 0, 9, 9) != nullptr && strstr(bop27_refusal(1, 0, 9, 9), "hex-8") && strstr(bop27_refusal(1, 0, 9, 9), "mfem_brick_operator_create"), "hex-8");
  CHECK(bop27_refusal(2, 2, 9, 9) != nullptr && strstr(bop27_refusal(2, 2, 9, 9), "slab") && bop27_refusal(2, 0, 8, 9) != nullptr, "slab");
  CHECK(strcmp(bop27_refusal(2, 2, 9, 9), bop_refusal(1, 2, 9, 9)) == 0, "the existing slab message");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
