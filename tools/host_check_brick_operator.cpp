// CPU walk through the host decisions of the matrix-free hex-8 brick operator (csrc/brick_operator_decide.h), for lattices from 1^3 elements
// (2^3 control points) to 1024^3 (1025^3):
//   1. ownership: the work items of the volume kernel (sweep and tile form) put every control point into exactly one item -- marked point by point
//      on small lattices, and through the axis partitions the boxes are a product of on the large ones (513^3, 769^3, 1025^3 included);
//   2. the fold: workgroup b takes the items b, b + grid, ...: every item once; the volume kernel's partial sums never exceed BOP_VOLUME_PARTIALS, the
//      face kernel's BOP_FACE_PARTIALS, a product's BOP_MAX_PARTIALS -- on every combination of a set of sizes that holds every tile, segment and cap
//      boundary up to 1025;
//   3. the kernel per Gauss rule: the sweep for 2 and 3 points per direction, the tiles for 1 and 4 -- the residual's own default choice;
//   4. the face kernel: its count is the number of boundary control points, the enumeration visits each exactly once, the strided grid covers the
//      count; one launch without face terms, two with; the refusals.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_operator.cpp -o tools/bin/host_check_brick_operator && tools/bin/host_check_brick_operator
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
#include "brick_operator_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

// ---- 1a. point by point ------------------------------------------------------------------------------------------------------------------------------
static void mark_points(int ng, int m0, int m1, int m2) {
  const BopVolume V = bop_volume(ng, m0, m1, m2);
  std::vector<unsigned char> seen((size_t)m0 * m1 * m2, 0);
  for (int64_t w = 0; w < V.items; ++w) {
    const BopBox b = bop_item_box(V, w, m0, m1, m2);
    CHECK(b.i0 >= 0 && b.i0 < b.i1 && b.i1 <= m0 && b.j0 >= 0 && b.j0 < b.j1 && b.j1 <= m1 && b.k0 >= 0 && b.k0 < b.k1 && b.k1 <= m2,
          "ng %d, %d x %d x %d, item %lld: an empty box or one outside the lattice", ng, m0, m1, m2, (long long)w);
    if (b.i1 > m0 || b.j1 > m1 || b.k1 > m2 || b.i0 < 0 || b.j0 < 0 || b.k0 < 0) continue;
    for (int i = b.i0; i < b.i1; ++i)
      for (int j = b.j0; j < b.j1; ++j)
        for (int k = b.k0; k < b.k1; ++k) ++seen[((size_t)i * m1 + j) * m2 + k];
  }
  long long wrong = 0;
  for (unsigned char c : seen) wrong += c != 1;
  CHECK(wrong == 0, "ng %d, %d x %d x %d: %lld control points not owned exactly once", ng, m0, m1, m2, wrong);
}

// ---- 1b. through the axis partitions ------------------------------------------------------------------------------------------------------------------
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
static void product_of_partitions(int ng, int m0, int m1, int m2) {
  const BopVolume V = bop_volume(ng, m0, m1, m2);
  Axis a[3];
  for (int64_t w = 0; w < V.items; ++w) {
    const BopBox b = bop_item_box(V, w, m0, m1, m2);
    a[0].iv.insert({b.i0, b.i1});
    a[1].iv.insert({b.j0, b.j1});
    a[2].iv.insert({b.k0, b.k1});
  }
  CHECK(a[0].partitions(m0) && a[1].partitions(m1) && a[2].partitions(m2), "ng %d, %d x %d x %d: the boxes' extents do not partition an axis", ng, m0, m1, m2);
  const int64_t n0 = (int64_t)a[0].iv.size(), n1 = (int64_t)a[1].iv.size(), n2 = (int64_t)a[2].iv.size();
  CHECK(n0 * n1 * n2 == V.items, "ng %d, %d x %d x %d: %lld items for %lld boxes", ng, m0, m1, m2, (long long)V.items, (long long)(n0 * n1 * n2));
  if (n0 * n1 * n2 != V.items) return;
  // every (interval, interval, interval) triple exactly once; the maps are arithmetic progressions per axis: index = start / step
  std::vector<int> s0, s1, s2;
  for (const auto& p : a[0].iv) s0.push_back(p.first);
  for (const auto& p : a[1].iv) s1.push_back(p.first);
  for (const auto& p : a[2].iv) s2.push_back(p.first);
  const int st0 = n0 > 1 ? s0[1] : m0, st1 = n1 > 1 ? s1[1] : m1, st2 = n2 > 1 ? s2[1] : m2;
  std::vector<unsigned char> seen((size_t)V.items, 0);
  long long volume = 0;
  for (int64_t w = 0; w < V.items; ++w) {
    const BopBox b = bop_item_box(V, w, m0, m1, m2);
    const int64_t t = ((int64_t)(b.i0 / st0) * n1 + b.j0 / st1) * n2 + b.k0 / st2;
    if (t >= 0 && t < V.items) ++seen[(size_t)t];
    volume += (long long)(b.i1 - b.i0) * (b.j1 - b.j0) * (b.k1 - b.k0);
  }
  long long wrong = 0;
  for (unsigned char c : seen) wrong += c != 1;
  CHECK(wrong == 0, "ng %d, %d x %d x %d: %lld boxes not taken exactly once", ng, m0, m1, m2, wrong);
  CHECK(volume == (long long)m0 * m1 * m2, "ng %d, %d x %d x %d: the boxes hold %lld points", ng, m0, m1, m2, volume);
}

// ---- 2. the fold and the caps ---------------------------------------------------------------------------------------------------------------------------
static void caps(int ng, int m0, int m1, int m2) {
  const BopVolume V = bop_volume(ng, m0, m1, m2);
  CHECK(V.items >= 1 && V.grid >= 1 && V.grid <= BOP_VOLUME_PARTIALS && V.grid <= V.items, "ng %d, %d x %d x %d: grid %d for %lld items", ng, m0, m1, m2,
        V.grid, (long long)V.items);
  CHECK(V.items < ((int64_t)1 << 32), "ng %d, %d x %d x %d: the item number does not fit the tile map's 32 bits", ng, m0, m1, m2);
  // workgroup b: items b, b + grid, ... below items -- ceil((items - b) / grid) of them; summed over b: every item once
  const int64_t q = V.items / V.grid, r = V.items % V.grid;
  CHECK(r * (q + 1) + (V.grid - r) * q == V.items, "ng %d, %d x %d x %d: the fold loses items", ng, m0, m1, m2);
  // balanced: the rounds of the cap, and every workgroup sweeps that many items or one fewer
  CHECK(V.rounds == (V.items + BOP_VOLUME_PARTIALS - 1) / BOP_VOLUME_PARTIALS && (r == 0 ? q == V.rounds : q + 1 == V.rounds), "ng %d, %d x %d x %d: %d rounds, %lld or %lld items per workgroup",
        ng, m0, m1, m2, V.rounds, (long long)q, (long long)q + 1);
  CHECK((V.items <= BOP_VOLUME_PARTIALS) == (V.grid == V.items), "ng %d, %d x %d x %d: a grid below the cap is one workgroup per item", ng, m0, m1, m2);
  CHECK(bop_volume_grid(V, true) == V.grid && bop_volume_grid(V, false) == V.items && V.items < ((int64_t)1 << 31), "ng %d, %d x %d x %d: the grid with and without partial sums", ng, m0, m1, m2);
  if (V.kernel == BOP_SWEEP) {
    CHECK(V.L == 4 || V.L == 8 || V.L == 16 || V.L == 32, "L = %d", V.L);
    CHECK(V.threads == SW_THREADS, "threads");
  } else {
    CHECK(V.threads == TT_THREADS, "threads");
  }
  const int64_t count = bop_boundary_count(m0, m1, m2);
  const int fg = bop_face_grid(count);
  CHECK(count == (int64_t)m0 * m1 * m2 - (int64_t)(m0 - 2) * (m1 - 2) * (m2 - 2), "%d x %d x %d: %lld boundary points", m0, m1, m2, (long long)count);
  CHECK(fg >= 1 && fg <= BOP_FACE_PARTIALS, "%d x %d x %d: face grid %d", m0, m1, m2, fg);
  CHECK(V.grid + fg <= BOP_MAX_PARTIALS, "%d x %d x %d: %d partial sums", m0, m1, m2, V.grid + fg);
  // the strided face grid reaches the last point: thread t, t + fg * 256, ...
  const int64_t stride = (int64_t)fg * H8_BLOCK, rounds = (count + stride - 1) / stride;
  CHECK(rounds * stride >= count && (fg == BOP_FACE_PARTIALS || rounds == 1), "%d x %d x %d: face rounds", m0, m1, m2);
}

// ---- 4. the boundary enumeration on the whole lattice ------------------------------------------------------------------------------------------------
static void boundary(int m0, int m1, int m2) {
  const int64_t count = bop_boundary_count(m0, m1, m2), PL = (int64_t)m1 * m2;
  std::vector<unsigned char> seen((size_t)m0 * m1 * m2, 0);
  for (int64_t t = 0; t < count + 3; ++t) {
    int i, j, k;
    const bool has = h8_boundary_point(t, 0, m0, m0 - 1, m1 - 1, m2 - 1, PL, m1, m2, i, j, k);
    CHECK(has == (t < count), "%d x %d x %d: thread %lld", m0, m1, m2, (long long)t);
    if (!has) continue;
    const bool in = i >= 0 && i < m0 && j >= 0 && j < m1 && k >= 0 && k < m2;
    CHECK(in, "%d x %d x %d: thread %lld outside the lattice", m0, m1, m2, (long long)t);
    if (in) ++seen[((size_t)i * m1 + j) * m2 + k];
  }
  long long wrong = 0;
  for (int i = 0; i < m0; ++i)
    for (int j = 0; j < m1; ++j)
      for (int k = 0; k < m2; ++k) {
        const bool bnd = i == 0 || i == m0 - 1 || j == 0 || j == m1 - 1 || k == 0 || k == m2 - 1;
        wrong += seen[((size_t)i * m1 + j) * m2 + k] != (bnd ? 1 : 0);
      }
  CHECK(wrong == 0, "%d x %d x %d: %lld points not visited as their place asks", m0, m1, m2, wrong);
}

int main() {
  // 3. the kernel per rule (and: what the residual launches under its default knobs)
  const BopKernel want[5] = {BOP_TILES, BOP_TILES, BOP_SWEEP, BOP_SWEEP, BOP_TILES};
  for (int ng = 1; ng <= 4; ++ng) {
    CHECK(bop_kernel(ng) == want[ng], "ng %d", ng);
    CHECK((bop_kernel(ng) == BOP_SWEEP) == (h8_thermal_kernel(h8_thermal_knobs(0), ng) == H8_THERMAL_SWEEP), "ng %d: not the residual's choice", ng);
  }
  // 1a. + 4.: every lattice from 1^3 to 6^3 elements, then shapes around the tile (15 / 16 / 4 / 8) and segment (4) edges
  for (int ng = 1; ng <= 2; ++ng)  // (1: the tile form, 2: the sweep)
    for (int m0 = 2; m0 <= 7; ++m0)
      for (int m1 = 2; m1 <= 7; ++m1)
        for (int m2 = 2; m2 <= 7; ++m2) {
          mark_points(ng, m0, m1, m2);
          if (ng == 1) boundary(m0, m1, m2);
        }
  const int edge[][3] = {{10, 15, 16}, {6, 17, 31}, {41, 46, 46}, {5, 5, 4}, {4, 5, 3}, {9, 8, 7}, {33, 16, 30}, {34, 31, 17}, {13, 45, 2}, {2, 2, 65}, {65, 2, 2}, {9, 9, 9}};
  for (const auto& e : edge)
    for (int ng = 1; ng <= 4; ++ng) {
      mark_points(ng, e[0], e[1], e[2]);
      product_of_partitions(ng, e[0], e[1], e[2]);
      boundary(e[0], e[1], e[2]);
    }
  // 1b.: the large lattices, cubes and not
  const int big[][3] = {{129, 129, 129}, {257, 257, 257}, {513, 513, 513}, {769, 769, 769}, {1025, 1025, 1025}, {1025, 2, 513}, {2, 1025, 1025}, {1024, 1023, 1021}};
  for (const auto& e : big)
    for (int ng = 1; ng <= 2; ++ng) product_of_partitions(ng, e[0], e[1], e[2]);
  // 2.: every combination of sizes that hold every tile, segment and cap boundary up to 1025
  std::vector<int> sizes;
  for (int m = 2; m <= 34; ++m) sizes.push_back(m);
  for (int m : {45, 46, 47, 60, 61, 63, 64, 65, 66, 90, 91, 127, 128, 129, 130, 255, 256, 257, 258, 383, 384, 385, 511, 512, 513, 514, 639, 640, 641, 767, 768, 769, 770, 895, 896,
                897, 959, 960, 961, 1009, 1010, 1011, 1020, 1021, 1022, 1023, 1024, 1025})
    sizes.push_back(m);
  for (int ng = 1; ng <= 2; ++ng)
    for (int m0 : sizes)
      for (int m1 : sizes)
        for (int m2 : sizes) caps(ng, m0, m1, m2);
  // the sizes the issue names: the residual's own grid at 512^3 against the operator's
  {
    const H8Sweep S = h8_residual_sweep(513, 513, 513);
    const BopVolume V = bop_volume(2, 513, 513, 513);
    CHECK(S.grid == 35 * 35 * 17 && V.items == S.grid && V.L == S.L && V.rounds == 6 && V.grid == 3471, "512^3: %lld items, grid %d", (long long)V.items, V.grid);
    const BopVolume W = bop_volume(2, 1025, 1025, 1025);
    CHECK(W.items == 69 * 69 * 33 && W.rounds == 44 && W.grid == 3571, "1024^3: %lld items, grid %d", (long long)W.items, W.grid);
  }
  // 4.: launches and refusals
  CHECK(bop_launches(0.6, 0.0, 0x3f, 0.0, 0) == 1 && bop_launches(0.6, 25.0, 0, 0.0, 0) == 1, "no face terms: one launch");
  CHECK(bop_launches(0.6, 25.0, 0x3f, 0.0, 0) == 2 && bop_launches(0.6, 0.0, 0, 0.0, 0x10) == 2 && bop_launches(0.0, 0.0, 0, 1000.0, 0x10) == 2, "face terms: two launches");
  CHECK(bop_launches(0.0, 0.0, 0, 0.0, 0x10) == 1, "Nitsche faces with k = h_penalty = 0 add nothing");
  CHECK(bop_refusal(1, 0, 9, 9) == nullptr, "a whole hex-8 brick is taken");
  CHECK(bop_refusal(2, 0, 9, 9) != nullptr && strstr(bop_refusal(2, 0, 9, 9), "hex-27"), "hex-27");
  CHECK(bop_refusal(1, 2, 9, 9) != nullptr && strstr(bop_refusal(1, 2, 9, 9), "slab") && bop_refusal(1, 0, 8, 9) != nullptr, "slab");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
