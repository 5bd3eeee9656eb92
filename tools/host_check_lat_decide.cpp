// CPU walk through every branch of the host decisions of solver layout modes 4 and 5 (csrc/lat_decide.h): both knob words, which lattices the tiles
// take, the lattice read off row 0 of a pattern without a hint, the geometry and the sizes of the copies, the split of a slab's launch, the gather
// grid and the symmetry gate.  Expected values are written out, not recomputed with the header's own expressions.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_lat_decide.cpp -o tools/bin/host_check_lat_decide && tools/bin/host_check_lat_decide
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "lat_decide.h"

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf(": %s\n", #cond); ++bad; } } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }
static int w27(int m) { return m >= 5 ? 5 : 3; }  // longest reach of a hex-27 row along a direction of m points
static int w8(int m) { return m >= 3 ? 3 : m; }
// whole hex-27 brick of a x b x c points, hint given; whole F-field 27-point brick
static LatShape brick27(int a, int b, int c) { return {(int64_t)a * b * c, (int64_t)a * b * c, w27(a) * w27(b) * w27(c), a, b, c, 1, 0, 2, 0}; }
static LatShape brick8(int F, int a, int b, int c) { return {(int64_t)F * a * b * c, (int64_t)F * a * b * c, F * w8(a) * w8(b) * w8(c), a, b, c, F, 0, 1, 0}; }
// m0 owned planes from plo on of such a brick
static LatShape slab27(int a, int b, int c, int plo, int m0) {
  LatShape S = brick27(a, b, c);
  S.n = (int64_t)m0 * b * c, S.ncols = S.n + 4 * (int64_t)b * c, S.lat_plo = plo;
  return S;
}
static LatShape slab8(int F, int a, int b, int c, int plo, int m0) {
  LatShape S = brick8(F, a, b, c);
  S.n = (int64_t)F * m0 * b * c, S.ncols = S.n + 2 * (int64_t)F * b * c, S.lat_plo = plo;
  return S;
}

static void check_knobs() {
  for (int w = 0; w < 16; ++w) {
    const Lat27Knobs K = lat27_knobs_decode(w);
    CHECK(K.enable == ((w & 1) != 0) && K.gather_staged == ((w & 2) == 0) && K.cg_fused == ((w & 4) == 0) && K.det == ((w & 8) == 0), "lat27 word %d", w);
  }
  const Lat27Knobs D = lat27_knobs_decode(LAT27_WORD_DEFAULT);
  CHECK(D.enable && D.gather_staged && D.cg_fused && D.det, "lat27 default: on, staged gather, fused CG, deterministic");
  const Lat27Knobs Q = lat27_knobs_decode(9);
  CHECK(Q.enable && Q.gather_staged && Q.cg_fused && !Q.det, "lat27 word 9: the four-lanes-per-row form");
  for (int w = 0; w < 8; ++w) {
    const Lat8Knobs K = lat8_knobs_decode(w);
    CHECK(K.enable == ((w & 1) != 0) && K.one_field_everywhere == ((w & 2) != 0) && K.gather_staged == ((w & 4) != 0), "lat8 word %d", w);
    for (int F = 1; F <= 3; ++F) {
      CHECK(lat8_for_method(F, false, K), "lat8 word %d, %d fields: every solver but cg! takes the tiles", w, F);
      CHECK(lat8_for_method(F, true, K) == (F != 1 || (w & 2) != 0), "lat8 word %d, %d fields, cg!", w, F);
    }
  }
  const Lat8Knobs E = lat8_knobs_decode(LAT8_WORD_DEFAULT);
  CHECK(E.enable && !E.one_field_everywhere && !E.gather_staged, "lat8 default: on, plain gather");
}

static void check_eligibility() {
  for (int a = 1; a <= 9; ++a)
    for (int b = 1; b <= 9; ++b)
      for (int c = 1; c <= 9; ++c) {
        const bool odd3 = a >= 3 && b >= 3 && c >= 3 && (a & 1) && (b & 1) && (c & 1);
        LatShape S = brick27(a, b, c);
        CHECK(lat27_eligible(S) == (odd3 ? 1 : -1), "hex-27 %d x %d x %d", a, b, c);
        S.lat_m0 = 0;  // (the hint need not give the plane count of a whole brick)
        CHECK(lat27_eligible(S) == (odd3 ? 1 : -1), "hex-27 %d x %d x %d, planes not given", a, b, c);
        S = brick27(a, b, c);
        for (int d = -1; d <= 1; d += 2) {
          S.max_row_nnz = w27(a) * w27(b) * w27(c) + d;
          CHECK(lat27_eligible(S) == -1, "hex-27 %d x %d x %d, longest row off by %d", a, b, c, d);
        }
        for (int F = 1; F <= 3; ++F) {
          const bool ok = b >= 2 && c >= 2;
          LatShape T = brick8(F, a, b, c);
          CHECK(lat8_eligible(T) == (ok ? 1 : -1), "27-point %d x %d x %d, %d fields", a, b, c, F);
          for (int d = -1; d <= 1; d += 2) {
            T.max_row_nnz = F * w8(a) * w8(b) * w8(c) + d;
            CHECK(lat8_eligible(T) == -1, "27-point %d x %d x %d, %d fields, longest row off by %d", a, b, c, F, d);
          }
        }
      }
  {  // the row threshold: below it the pattern is not inspected (state 0: asked again), whatever else it is
    LatShape S = brick27(5, 7, 9), T = brick8(3, 4, 5, 6), U = brick27(4, 4, 4);
    S.min_rows = S.n + 1, T.min_rows = T.n + 1, U.min_rows = U.n + 1;
    CHECK(lat27_eligible(S) == 0 && lat8_eligible(T) == 0 && lat27_eligible(U) == 0, "below the row threshold");
    CHECK(!lat_serves(1, true, S), "... and not served");
    S.min_rows = S.n, T.min_rows = T.n, U.min_rows = U.n;
    CHECK(lat27_eligible(S) == 1 && lat8_eligible(T) == 1 && lat27_eligible(U) == -1, "at the row threshold");
    CHECK(lat_serves(1, true, S) && !lat_serves(1, false, S) && !lat_serves(-1, true, S) && !lat_serves(0, true, S), "served when verified and on");
    CHECK(lat27_eligible(brick8(1, 5, 7, 9)) == -1 || brick8(1, 5, 7, 9).max_row_nnz == 125, "a hex-8 lattice with odd counts carries the hex-27 hint: 27 against 125");
    S = brick27(5, 7, 9), S.lat_fields = 2;
    CHECK(lat27_eligible(S) == -1, "hex-27 is one field");
    T = brick8(3, 4, 5, 6), T.lat_fields = 4, T.n = 4 * 120, T.ncols = T.n;
    CHECK(lat8_eligible(T) == -1, "27-point: three fields at most");
    S = brick27(5, 7, 9), S.n += 1, S.ncols += 1;
    CHECK(lat27_eligible(S) == -1, "rows that are no whole planes");
    S = brick27(5, 7, 9), S.lat_m0 = 7;
    CHECK(lat27_eligible(S) == -1, "a whole brick whose hint names another plane count");
    S = brick27(5, 7, 9), S.lat_plo = 2;
    CHECK(lat27_eligible(S) == -1, "a whole brick that does not start at plane 0");
  }
  // slabs of the 21-plane hex-27 brick and of the 20-plane 27-point brick
  CHECK(lat27_eligible(slab27(21, 9, 5, 6, 8)) == 1, "hex-27 slab (6, 14)");
  CHECK(lat27_eligible(slab27(21, 9, 5, 5, 8)) == -1, "hex-27 slab cut inside an element (plo odd)");
  CHECK(lat27_eligible(slab27(21, 9, 5, 14, 7)) == 1 && lat27_eligible(slab27(21, 9, 5, 14, 8)) == -1, "hex-27 slab: plo + m0 against the lattice");
  CHECK(lat27_eligible(slab27(21, 9, 5, 0, 1)) == 1, "hex-27 slab of one plane");
  {
    LatShape S = slab27(21, 9, 5, 6, 8);
    S.ncols -= 45;
    CHECK(lat27_eligible(S) == -1, "hex-27 slab: ghost columns one plane short");
    S = slab27(21, 9, 5, 6, 8), S.ncols += 45;
    CHECK(lat27_eligible(S) == -1, "hex-27 slab: ghost columns one plane long");
    S = slab27(21, 9, 5, 6, 8), S.lat_gw = 1;
    CHECK(lat27_eligible(S) == -1, "hex-27 slab: two ghost planes per side");
    S = slab27(21, 9, 5, 6, 8), S.lat_m0 = 20;
    CHECK(lat27_eligible(S) == -1, "hex-27 slab of an even lattice");
  }
  for (int F = 1; F <= 3; ++F) {
    CHECK(lat8_eligible(slab8(F, 20, 9, 6, 7, 8)) == 1 && lat8_eligible(slab8(F, 20, 9, 6, 6, 8)) == 1, "27-point slab (7, 15) / (6, 14), %d fields: any plo", F);
    CHECK(lat8_eligible(slab8(F, 20, 9, 6, 12, 8)) == 1 && lat8_eligible(slab8(F, 20, 9, 6, 13, 8)) == -1, "27-point slab: plo + m0 against the lattice, %d fields", F);
    LatShape S = slab8(F, 20, 9, 6, 7, 8);
    S.ncols -= 54;
    CHECK(lat8_eligible(S) == -1, "27-point slab: ghost columns one plane short, %d fields", F);
    S = slab8(F, 20, 9, 6, 7, 8), S.lat_gw = 2;
    CHECK(lat8_eligible(S) == -1, "27-point slab: one ghost plane per side, %d fields", F);
  }
  {  // the caps: 2^20 planes, 2^28 tiles
    LatShape S = {(int64_t)((1 << 20) + 1) * 9, (int64_t)((1 << 20) + 1) * 9, 45, 0, 3, 3, 1, 0, 2, 0};
    CHECK(lat27_eligible(S) == -1, "more than 2^20 planes");
    S.n = S.ncols = (int64_t)((1 << 20) - 1) * 9;
    CHECK(lat27_eligible(S) == 1, "2^20 - 1 planes");
    LatShape T = {(int64_t)(1 << 20) * 2048 * 2048, (int64_t)(1 << 20) * 2048 * 2048, 27, 0, 2048, 2048, 1, 0, 1, 0};  // 2^17 x 2^8 x 2^7 tiles
    CHECK(lat8_eligible(T) == -1, "2^32 tiles");
    T.lat_m1 = T.lat_m2 = 16, T.n = T.ncols = (int64_t)(1 << 20) * 256;
    CHECK(lat8_eligible(T) == 1, "2^18 tiles");
  }
}

static std::vector<int32_t> row0_27(int m1, int m2) {
  std::vector<int32_t> c;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      for (int k = 0; k < 3; ++k) c.push_back((a * m1 + b) * m2 + k);
  return c;
}
static std::vector<int32_t> row0_8(int F, int m0, int m1, int m2) {
  std::vector<int32_t> c;
  for (int g = 0; g < F; ++g)
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
        for (int k = 0; k < 2; ++k) c.push_back(g * m0 * m1 * m2 + (a * m1 + b) * m2 + k);
  return c;
}
static bool hint_is(const LatHint& H, int F, int m0, int m1, int m2, int gw) {
  return H.fields == F && H.m0 == m0 && H.m1 == m1 && H.m2 == m2 && H.plo == 0 && H.gw == gw;
}
static void check_row0() {
  const int h27[3][3] = {{3, 3, 3}, {5, 7, 9}, {3, 3, 41}}, h8[3][3] = {{2, 2, 2}, {4, 5, 6}, {9, 3, 17}};
  std::vector<int32_t> pad(32, 0);
  for (auto& m : h27) {
    const int64_t n = (int64_t)m[0] * m[1] * m[2];
    std::vector<int32_t> c = row0_27(m[1], m[2]);
    CHECK(hint_is(lattice_from_row0(27, c.data(), n), 1, m[0], m[1], m[2], 2), "hex-27 %d x %d x %d", m[0], m[1], m[2]);
    for (int i = 1; i < 27; ++i) {
      std::vector<int32_t> d = c;
      d[i] += 1;
      CHECK(lattice_from_row0(27, d.data(), n).fields == 0, "hex-27 %d x %d x %d, column %d moved", m[0], m[1], m[2], i);
    }
    std::vector<int32_t> d = c;
    d[0] = 1;
    CHECK(lattice_from_row0(27, d.data(), n).fields == 0, "hex-27: row 0 does not start at column 0");
    CHECK(lattice_from_row0(27, c.data(), n + 1).fields == 0, "hex-27: rows that are no whole planes");
    c.resize(32, 0);
    CHECK(lattice_from_row0(26, c.data(), n).fields == 0 && lattice_from_row0(28, c.data(), n).fields == 0, "hex-27: row lengths 26 and 28");
  }
  for (auto& m : h8)
    for (int F = 1; F <= 3; ++F) {
      const int64_t n = (int64_t)F * m[0] * m[1] * m[2];
      std::vector<int32_t> c = row0_8(F, m[0], m[1], m[2]);
      CHECK(hint_is(lattice_from_row0(8 * F, c.data(), n), F, m[0], m[1], m[2], 1), "27-point %d x %d x %d, %d fields", m[0], m[1], m[2], F);
      for (int i = 1; i < 8 * F; ++i) {
        std::vector<int32_t> d = c;
        d[i] += 1;
        CHECK(lattice_from_row0(8 * F, d.data(), n).fields == 0, "27-point %d x %d x %d, %d fields, column %d moved", m[0], m[1], m[2], F, i);
      }
      std::vector<int32_t> d = c;
      d[0] = 1;
      CHECK(lattice_from_row0(8 * F, d.data(), n).fields == 0, "27-point: row 0 does not start at column 0");
      CHECK(lattice_from_row0(8 * F, c.data(), n + F).fields == 0, "27-point: rows that are no whole planes");
      c.resize(32, 0);
      CHECK(lattice_from_row0(7, c.data(), n).fields == 0 && lattice_from_row0(9, c.data(), n).fields == 0, "27-point: row lengths 7 and 9");
    }
  CHECK(lattice_row0_len(8) && lattice_row0_len(16) && lattice_row0_len(24) && lattice_row0_len(27) && !lattice_row0_len(0) && !lattice_row0_len(32), "row lengths worth a read");
}

static void check_geometry() {
  CHECK(L27_CELLS == 4320 && L27_UNIT_D == 64 * 68 && L27D_CUBE_D == 260 * 64 && L8_FC == 1620, "cells of a y block, doubles of a unit and of a cube");
  CHECK(lat8_pair_doubles(1) == 2 * 14 * 64 && lat8_pair_doubles(2) == 2 * 55 * 64 && lat8_pair_doubles(3) == 2 * 123 * 64, "steps of a pair: 14, 55, 123 per unit");
  const int sizes[] = {3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 41};
  for (int a : sizes)
    for (int b : sizes)
      for (int c : sizes) {
        if ((a & 1) && (b & 1) && (c & 1)) {
          const Lat27Geom G = lat27_geom(brick27(a, b, c));
          CHECK(G.m0 == a && G.m1 == b && G.m2 == c && G.n == (int64_t)a * b * c && G.plo == 0 && G.mg == a && G.gw == 2, "hex-27 %d x %d x %d: points", a, b, c);
          CHECK(G.nui == ceil_div(a, 4) && G.nuj == ceil_div(b, 4) && G.nuk == ceil_div(c, 8), "hex-27 %d x %d x %d: units of 4 x 4 x 8", a, b, c);
          CHECK(G.nti == ceil_div(a, 8) && G.ntj == ceil_div(b, 8) && G.ntk == ceil_div(c, 32), "hex-27 %d x %d x %d: tiles of 8 x 8 x 32", a, b, c);
          const size_t tiles = (size_t)ceil_div(a, 8) * ceil_div(b, 8) * ceil_div(c, 32);
          const size_t det = (size_t)ceil_div(a, 8) * ceil_div(b, 8) * ceil_div(c, 8) * 16640, quad = (size_t)ceil_div(a, 4) * ceil_div(b, 4) * ceil_div(c, 8) * 4352;
          CHECK(lat27d_vals_doubles(G) == det && lat27q_vals_doubles(G) == quad, "hex-27 %d x %d x %d: stored doubles of both forms", a, b, c);
          CHECK(lat27_vals_doubles(G) >= det && lat27_vals_doubles(G) >= quad && (lat27_vals_doubles(G) == det || lat27_vals_doubles(G) == quad), "... and what the workspace reserves");
          CHECK(lat27_read_doubles(G, true) == det && lat27_read_doubles(G, false) == quad && lat27_entries(G, true) == (int64_t)det && lat27_entries(G, false) == (int64_t)quad, "... and what pass 1 streams");
          CHECK(lat27_dump_doubles(G) == tiles * 4320 && lat27_dot_partials(G) == (int)tiles && lat27_dot_offset(G) == tiles * 4320, "hex-27 %d x %d x %d: dump, partials right behind it", a, b, c);
          CHECK(lat27_ws_bytes(G) == 8 * ((det > quad ? det : quad) + tiles * 4321), "hex-27 %d x %d x %d: workspace", a, b, c);
          for (int f = 0; f < 2; ++f) {
            const int64_t rd = f ? (int64_t)det : (int64_t)quad;
            CHECK(lat27_design_bytes(G, f, false) == rd * 8 + (int64_t)tiles * 4320 * 24 + G.n * 8 && lat27_design_bytes(G, f, true) == rd * 8 + (int64_t)tiles * 4320 * 32 + G.n * 8, "hex-27: design bytes, form %d", f);
            CHECK(lat27_pass1_bytes(G, f) == rd * 8 + (int64_t)tiles * 4320 * 16, "hex-27: pass-1 bytes, form %d", f);
          }
        }
        for (int F = 1; F <= 3; ++F) {
          const Lat8Geom G = lat8_geom(brick8(F, a, b, c));
          CHECK(G.F == F && G.m0 == a && G.m1 == b && G.m2 == c && G.N == (int64_t)a * b * c && G.plo == 0 && G.mg == a && G.gw == 1, "27-point %d x %d x %d: nodes", a, b, c);
          CHECK(G.nui == ceil_div(a, 4) && G.nuj == ceil_div(b, 4) && G.nuk == ceil_div(c, 4), "27-point %d x %d x %d: units of 4 x 4 x 4", a, b, c);
          CHECK(G.nti == ceil_div(a, 8) && G.ntj == ceil_div(b, 8) && G.ntk == ceil_div(c, 16), "27-point %d x %d x %d: tiles of 8 x 8 x 16", a, b, c);
          const size_t tiles = (size_t)ceil_div(a, 8) * ceil_div(b, 8) * ceil_div(c, 16);
          const size_t vals = (size_t)ceil_div(ceil_div(a, 4), 2) * ceil_div(b, 4) * ceil_div(c, 4) * 128 * (F == 1 ? 14 : F == 2 ? 55 : 123);
          CHECK(lat8_vals_doubles(G) == vals && lat8_entries(G) == (int64_t)vals && lat8_dump_doubles(G) == tiles * F * 1620, "27-point %d x %d x %d, %d fields: pairs and dump", a, b, c, F);
          CHECK(lat8_ws_bytes(G) == 8 * (vals + tiles * F * 1620), "27-point: workspace");
          CHECK(lat8_design_bytes(G, false) == (int64_t)vals * 8 + (int64_t)tiles * F * 1620 * 24 + (int64_t)F * a * b * c * 8 &&
                lat8_design_bytes(G, true) == (int64_t)vals * 8 + (int64_t)tiles * F * 1620 * 32 + (int64_t)F * a * b * c * 8, "27-point: design bytes");
        }
      }
  const Lat27Geom S = lat27_geom(slab27(21, 9, 5, 6, 8));
  CHECK(S.m0 == 8 && S.plo == 6 && S.mg == 21 && S.gw == 2 && S.n == 360 && S.nti == 1 && S.nui == 2, "hex-27 slab (6, 14)");
  const Lat8Geom T = lat8_geom(slab8(3, 20, 9, 6, 7, 8));
  CHECK(T.m0 == 8 && T.plo == 7 && T.mg == 20 && T.gw == 1 && T.N == 432 && T.F == 3, "27-point slab (7, 15)");
}

static void check_parts() {
  for (int gw = 1; gw <= 2; ++gw)
    for (int m0 = 1; m0 <= 40; ++m0)
      for (int up = 0; up < 2; ++up) {
        const int nti = ceil_div(m0, 8), ntj = 2, ntk = 3;
        // a layer ti stages the planes up to 8 ti + 7 + gw: interior while that is an owned plane
        int layer = 0;
        while (layer < nti && (!up || 8 * layer + 7 + gw < m0)) ++layer;
        CHECK(mfem_lat_first_ghost_layer(m0, gw, nti, up != 0) == layer, "first ghost layer: m0 %d, gw %d, upper %d", m0, gw, up);
        const LatPart P0 = lat_part_tiles(m0, gw, nti, ntj, ntk, up != 0, 0), P1 = lat_part_tiles(m0, gw, nti, ntj, ntk, up != 0, 1),
                      P2 = lat_part_tiles(m0, gw, nti, ntj, ntk, up != 0, 2);
        CHECK(P0.tile0 == 0 && P0.tcount == nti * 6, "part 0 is everything: m0 %d", m0);
        CHECK(P1.tile0 == 0 && P1.tcount == layer * 6 && P2.tile0 == layer * 6 && P1.tcount + P2.tcount == P0.tcount, "parts 1 and 2 partition part 0: m0 %d, gw %d, upper %d", m0, gw, up);
        for (const LatPart& P : {P0, P1, P2}) CHECK(P.grid == 8 * ceil_div(P.tcount, 8) && P.grid >= P.tcount && P.grid < P.tcount + 8, "grid: whole eighths, m0 %d", m0);
      }
}

static void check_grid_and_gate() {
  CHECK(lat_gather_grid(256, 3, 10000) == 768 && lat_gather_grid(256, 3, 768) == 768 && lat_gather_grid(256, 3, 767) == 767 && lat_gather_grid(256, 3, 1) == 1, "gather grid: resident, or a workgroup per tile");
  CHECK(lat_gather_grid(256, 16, 100000) == 4096 && lat_gather_grid(256, 17, 4097) == 4096 && lat_gather_grid(1024, 4, 4095) == 4095, "gather grid: one partial per workgroup at most");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(LAT_SYM_GATE == 4e-13, "the gate");
  CHECK(lat_accepts(0.0) && lat_accepts(4e-13) && lat_accepts(std::nextafter(4e-13, 0.0)) && !lat_accepts(std::nextafter(4e-13, 1.0)), "at, just below and just above the gate");
  CHECK(!lat_accepts(1.0) && !lat_accepts(inf) && !lat_accepts(nan), "non-finite measures are refused");
  const Lat27Knobs on = lat27_knobs_decode(1), off = lat27_knobs_decode(5);
  CHECK(lat27_cg_fusable(on, true, false, false, false), "fused CG: bound, unscaled, one rank, no remainder");
  CHECK(!lat27_cg_fusable(off, true, false, false, false) && !lat27_cg_fusable(on, false, false, false, false) && !lat27_cg_fusable(on, true, true, false, false) &&
        !lat27_cg_fusable(on, true, false, true, false) && !lat27_cg_fusable(on, true, false, false, true), "fused CG: each condition alone refuses");
}

int main() {
  check_knobs();
  check_eligibility();
  check_row0();
  check_geometry();
  check_parts();
  check_grid_and_gate();
  if (bad) return printf("%d checks FAILED\n", bad), 1;
  printf("lat_decide: OK\n");
  return 0;
}
