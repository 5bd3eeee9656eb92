// CPU walk through the host decisions of the hex-27 thermal assembly (csrc/hex27_decide.h), three ways:
//   1. against the expressions of the driver these functions were cut out of (mfem_hex27_assemble_thermal as one 145-line function with eleven
//      knob globals), transcribed below as old_*: the knob decode, the counting gate, the path choice in its order of tests, the workspace bytes and
//      offsets, P and ring, the rows of a chunk, the grids, the face launches -- swept, 0 differences allowed;
//   2. properties that hold whatever the driver did: colour counts sum to the element count of a slab, the chunks of the ring gather every owned
//      plane once and read only planes that are still in the ring, workspace regions are disjoint and aligned, the face schedule covers every
//      flagged face and colour class once;
//   3. the LDS carve-up as functions (the host sizes the block with them) against the macros k_hex27 expands, for every ng, mode and field.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_hex27.cpp -o tools/bin/host_check_hex27 && tools/bin/host_check_hex27
#include <cstdio>
#include <vector>
#include "hex27_decide.h"

static long long cases = 0, diffs = 0, bad = 0;
#define SAME(a, b, ...) do { ++cases; if (!((a) == (b))) { if (++diffs <= 20) { printf("DIFFERS "); printf(__VA_ARGS__); printf(": %s = %lld, %s = %lld\n", #a, (long long)(a), #b, (long long)(b)); } } } while (0)
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

// ---- 1. the driver before the cut, verbatim ---------------------------------------------------------------------------------------------------------
struct OldKnobs {
  int g_hex27_two_pass, g_hex27_chunk_planes, g_hex27_affine, g_hex27_direct, g_hex27_mixed, g_hex27_rows, g_hex27_rows_min, g_hex27_rows_ablate,
      g_hex27_mixed_max;
};
static OldKnobs old_set_hex27(int two_pass) {
  OldKnobs g;
  g.g_hex27_two_pass = (two_pass & 3) == 0 ? 1 : (two_pass & 3);
  g.g_hex27_chunk_planes = (two_pass >> 16) & 255;
  g.g_hex27_affine = ((two_pass >> 8) & 1) ? 0 : 1;
  g.g_hex27_direct = ((two_pass >> 9) & 1) ? 0 : 1;
  g.g_hex27_mixed = ((two_pass >> 10) & 1) ? 0 : 1;
  g.g_hex27_rows = ((two_pass >> 11) & 1) ? 0 : 1;
  g.g_hex27_rows_min = (two_pass >> 2) & 63;
  g.g_hex27_rows_ablate = (two_pass >> 12) & 7;
  g.g_hex27_mixed_max = ((two_pass >> 24) & 127) ? ((two_pass >> 24) & 127) : 80;
  return g;
}
#define OLD_R27_MIN_PERCENT 30
struct OldWs {
  size_t g_bytes, map_bytes, reserve, slot, elist, head, stored_bytes, gq_bytes;
};
// the control flow of the old driver from its first test to the path's first launch; *counted: the count of non-affine elements was made
static H27Path old_driver(const OldKnobs& g, int ng, int64_t nel, int64_t n_owned, int64_t n_stored, size_t g_hex27_scratch_budget, bool* counted,
                          OldWs* W) {
  const int nq = ng * ng * ng;
  *counted = false;
  if (g.g_hex27_two_pass == 2) return H27_ATOMICS;
  if (g.g_hex27_two_pass == 1 && g.g_hex27_direct && g.g_hex27_affine && n_owned < ((int64_t)1 << 31)) {
    *counted = true;
    const size_t g_bytes = sizeof(double) * 6 * (size_t)nel, map_bytes = (sizeof(int32_t) * (size_t)nel + 255) & ~(size_t)255;
    W->g_bytes = g_bytes, W->map_bytes = map_bytes, W->reserve = g_bytes + 2 * map_bytes, W->slot = g_bytes, W->elist = g_bytes + map_bytes;
    const size_t gq_bytes = sizeof(double) * 6 * (size_t)nq * (size_t)nel;
    W->gq_bytes = gq_bytes;
    if (g.g_hex27_rows && ng == 3 && n_stored * 100 >= nel * (int64_t)(g.g_hex27_rows_min ? (int)g.g_hex27_rows_min : OLD_R27_MIN_PERCENT) && n_stored > 0 &&
        gq_bytes <= g_hex27_scratch_budget && g.g_hex27_chunk_planes == 0)
      return H27_ROWS;
    const size_t stored_bytes = sizeof(double) * 729 * (size_t)n_stored;
    W->stored_bytes = stored_bytes;
    if (n_stored == 0 || (g.g_hex27_mixed && n_stored * 100 <= nel * (int64_t)g.g_hex27_mixed_max && stored_bytes <= g_hex27_scratch_budget)) {
      const size_t head = (g_bytes + 2 * map_bytes + 255) & ~(size_t)255;
      W->head = head;
      return n_stored ? H27_MIXED : H27_DIRECT;
    }
  }
  if (g.g_hex27_two_pass == 1) return H27_TWO_PASS;
  return H27_COLOUR;
}
static void old_ring(int npl, int64_t plane_el, int g_hex27_chunk_planes, size_t g_hex27_scratch_budget, int* P_, int* ring_, size_t* plane_bytes_) {
  const size_t plane_bytes = sizeof(double) * 729 * (size_t)plane_el;
  int P = npl;
  if (g_hex27_chunk_planes > 0) P = g_hex27_chunk_planes;
  else if (plane_bytes * (size_t)npl > g_hex27_scratch_budget) P = (int)(g_hex27_scratch_budget / plane_bytes) - 1;
  if (P < 1) P = 1;
  if (P > npl) P = npl;
  const int ring = P >= npl ? npl : P + 1;
  *P_ = P, *ring_ = ring, *plane_bytes_ = plane_bytes;
}
static void old_element_planes(int plo, int phi, int ne0, int* elo, int* ehi) {
  *elo = plo / 2 - 1 < 0 ? 0 : plo / 2 - 1;
  *ehi = phi / 2 > ne0 ? ne0 : phi / 2;
}
static int64_t old_colour_count(int ne1, int ne2, int colour, int elo, int ehi) {
  const int o0 = elo + (((colour & 1) - elo) & 1);
  const int64_t n0 = o0 < ehi ? (ehi - o0 + 1) >> 1 : 0, n1 = (ne1 - ((colour >> 1) & 1) + 1) >> 1, n2 = (ne2 - (colour >> 2) + 1) >> 1;
  return n0 * n1 * n2;
}
// the persistent cap as the old driver spelled it: (a) atomics, ring and colours, (b) pass 1 of the mixed path, (c) k_hex27_direct and k_hex27_rows_gq
static int old_grid_a(int64_t n, int num_cus) {
  int64_t grid = (n + 8 - 1) / 8;
  const int64_t cap = (int64_t)num_cus * 2;
  if (grid > cap) grid = cap;
  return (int)grid;
}
static int old_grid_b(int64_t n_stored, int num_cus) {
  int64_t grid1 = (n_stored + 8 - 1) / 8;
  if (grid1 > (int64_t)num_cus * 2) grid1 = (int64_t)num_cus * 2;
  return (int)grid1;
}
static int old_grid_c(int64_t nblk, int num_cus) { return (int)(nblk < (int64_t)num_cus * 2 ? nblk : (int64_t)num_cus * 2); }
static std::vector<H27FaceLaunch> old_faces(uint32_t robin, double h, const int* ne) {
  std::vector<H27FaceLaunch> L;
  if (h == 0.0 || robin == 0u) return L;
  for (int nd = 0; nd < 3; ++nd) {
    const int id_lo = (nd == 0) ? 5 : (nd == 1) ? 2 : 1, id_hi = (nd == 0) ? 3 : (nd == 1) ? 4 : 6;
    const bool lo = robin & (1u << (id_lo - 1)), hi = robin & (1u << (id_hi - 1));
    for (int pass = 0; pass < 2; ++pass) {
      int side;
      if (lo && hi) {
        if (pass) break;
        side = -1;
      } else {
        side = pass;
        if (!(side ? hi : lo)) continue;
      }
      const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
      for (int colour = 0; colour < 4; ++colour) {
        const int n1 = (ne[t1] - (colour & 1) + 1) >> 1, n2 = (ne[t2] - (colour >> 1) + 1) >> 1;
        if (n1 <= 0 || n2 <= 0) continue;
        const int64_t nthreads = (int64_t)n1 * n2 * 9 * (side < 0 ? 2 : 1);
        const int grid = (int)((nthreads + 256 - 1) / 256);
        L.push_back({nd, side, colour, n1, n2, grid});
      }
    }
  }
  return L;
}

static std::vector<int> knob_words() {
  std::vector<int> w;
  for (int b = 0; b < 31; ++b) w.push_back(1 << b);
  // what the tests and tools set
  for (int v : {0, 1, 2, 3, 1 << 9, (1 << 9) | (1 << 8), 1 << 11, (1 << 10) | (1 << 11), (100 << 24) | (1 << 11), 1 << 2, 1 | (1 << 16), 1 | (2 << 16),
                1 | (3 << 16), 1 | (4 << 16), 1 | (255 << 16), 1 | 4 | (1 << 8) | (2 << 16), (1 << 11) | (1 << 12), (7 << 12),
                // forced thresholds
                (50 << 2), (63 << 2), (10 << 24), (127 << 24), (1 << 2) | (1 << 24), (50 << 2) | (50 << 24), 0x7fffffff})
    w.push_back(v);
  return w;
}

static void check_knobs(const std::vector<int>& words) {
  for (int w : words) {
    const OldKnobs g = old_set_hex27(w);
    const H27Knobs K = h27_knobs(w);
    SAME(K.variant, g.g_hex27_two_pass, "word %#x", w);
    SAME(K.chunk_planes, g.g_hex27_chunk_planes, "word %#x", w);
    SAME((int)K.affine, g.g_hex27_affine, "word %#x", w);
    SAME((int)K.direct, g.g_hex27_direct, "word %#x", w);
    SAME((int)K.mixed, g.g_hex27_mixed, "word %#x", w);
    SAME((int)K.rows, g.g_hex27_rows, "word %#x", w);
    SAME(K.rows_min, (g.g_hex27_rows_min ? g.g_hex27_rows_min : OLD_R27_MIN_PERCENT), "word %#x", w);
    SAME(K.rows_ablate, g.g_hex27_rows_ablate, "word %#x", w);
    SAME(K.mixed_max, g.g_hex27_mixed_max, "word %#x", w);
  }
  const H27Knobs D = h27_knobs(0);
  CHECK(D.variant == 1 && D.rows_min == 30 && D.mixed_max == 80 && D.affine && D.direct && D.mixed && D.rows && !D.rows_ablate && !D.chunk_planes,
        "word 0: every default");
  CHECK(H27_SCRATCH_BUDGET == ((size_t)16 << 30), "the scratch budget: 16 GiB");
}

static void check_paths(const std::vector<int>& words) {
  // element counts: small ones, and the ones at which G_q (1296 bytes per element at ng = 3) and a plane's Ke cross the 16 GiB budget
  const int64_t gq_edge = (int64_t)(H27_SCRATCH_BUDGET / 1296), ke_edge = (int64_t)(H27_SCRATCH_BUDGET / 5832);
  const int64_t nels[] = {1, 2, 3, 7, 10, 27, 64, 99, 100, 101, 1000, 4096, ke_edge, ke_edge + 1, gq_edge, gq_edge + 1, 4 * gq_edge};
  const int64_t owned[] = {27, 1000, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 1};
  for (int w : words) {
    const OldKnobs g = old_set_hex27(w);
    const H27Knobs K = h27_knobs(w);
    for (int ng = 1; ng <= 4; ++ng)
      for (int64_t nel : nels) {
        // n_stored: none, one, all, both sides of every percentage in play
        std::vector<int64_t> ns = {0, 1, nel, ke_edge, ke_edge + 1};
        for (int pc : {30, 80, K.rows_min, K.mixed_max})
          for (int d = -1; d <= 1; ++d) ns.push_back(nel * pc / 100 + d);
        for (int64_t n_stored : ns) {
          if (n_stored < 0 || n_stored > nel) continue;
          const size_t gq = sizeof(double) * 6 * (size_t)(ng * ng * ng) * (size_t)nel, st = sizeof(double) * 729 * (size_t)n_stored;
          for (size_t budget : {H27_SCRATCH_BUDGET, gq - 1, gq, gq + 1, st - 1, st, st + 1})
            for (int64_t n_owned : owned) {
              bool counted;
              OldWs O{};
              const H27Path po = old_driver(g, ng, nel, n_owned, n_stored, budget, &counted, &O);
              SAME((int)h27_needs_count(K, n_owned), (int)counted, "word %#x, n_owned %lld", w, (long long)n_owned);
              SAME((int)h27_path(K, ng, nel, counted ? n_stored : -1, budget), (int)po, "word %#x, ng %d, nel %lld, n_stored %lld, budget %zu", w, ng,
                   (long long)nel, (long long)n_stored, budget);
              if (!counted) continue;
              const H27Ws W = h27_ws(ng, nel, n_stored);
              SAME(W.g_bytes, O.g_bytes, "nel %lld", (long long)nel);
              SAME(W.map_bytes, O.map_bytes, "nel %lld", (long long)nel);
              SAME(W.count_bytes, O.reserve, "nel %lld", (long long)nel);
              SAME(W.slot, O.slot, "nel %lld", (long long)nel);
              SAME(W.elist, O.elist, "nel %lld", (long long)nel);
              SAME(W.gq_bytes, O.gq_bytes, "nel %lld, ng %d", (long long)nel, ng);
              if (po != H27_ROWS) SAME(W.stored_bytes, O.stored_bytes, "n_stored %lld", (long long)n_stored);
              if (po == H27_MIXED || po == H27_DIRECT) SAME(W.head, O.head, "nel %lld", (long long)nel);
            }
        }
      }
  }
  // the budget as the library has it (no argument)
  const H27Knobs D = h27_knobs(0);
  CHECK(h27_path(D, 3, gq_edge, gq_edge) == H27_ROWS && h27_path(D, 3, gq_edge + 1, gq_edge + 1) == H27_TWO_PASS, "G_q at the 16 GiB budget, and past it");
  CHECK(h27_path(D, 4, 4 * ke_edge, ke_edge) == H27_MIXED && h27_path(D, 4, 4 * ke_edge, ke_edge + 1) == H27_TWO_PASS, "stored Ke at the 16 GiB budget, and past it");
  CHECK(h27_path(D, 3, 100, -1) == H27_TWO_PASS && h27_path(h27_knobs(3), 3, 100, -1) == H27_COLOUR && h27_path(h27_knobs(2), 3, 100, 50) == H27_ATOMICS, "not counted");
  CHECK(h27_path(D, 3, 100, 0) == H27_DIRECT && h27_path(D, 3, 100, 29) == H27_MIXED && h27_path(D, 3, 100, 30) == H27_ROWS && h27_path(D, 2, 100, 80) == H27_MIXED &&
        h27_path(D, 2, 100, 81) == H27_TWO_PASS, "the defaults: 30 %% and 80 %%");
  CHECK(h27_path(h27_knobs(1 << 10), 2, 100, 1) == H27_TWO_PASS && h27_path(h27_knobs(1 << 10), 2, 100, 0) == H27_DIRECT, "a failed mixed gate falls through to the ring");
}

static void check_planes_and_ring() {
  // equality: planes, colour counts, chunk rows, ring
  for (int ne0 = 1; ne0 <= 7; ++ne0) {
    const int m0 = 2 * ne0 + 1;
    for (int plo = 0; plo < m0; plo += 2)
      for (int phi = plo + 2; phi <= m0; phi += (phi + 2 > m0 && phi < m0) ? 1 : 2) {
        int elo, ehi, eo, eh;
        hex27_element_planes(plo, phi, ne0, &elo, &ehi);
        old_element_planes(plo, phi, ne0, &eo, &eh);
        SAME(elo, eo, "slab [%d, %d) of %d", plo, phi, m0);
        SAME(ehi, eh, "slab [%d, %d) of %d", plo, phi, m0);
        for (int w : {0, 1, 2, 3}) {
          const H27Knobs K = h27_knobs(w);
          const bool slab = !(plo == 0 && phi == m0);
          SAME((int)h27_slab_refused(K, plo, phi, m0), (int)!(!slab || old_set_hex27(w).g_hex27_two_pass == 1), "slab [%d, %d) of %d, word %d", plo, phi, m0, w);
        }
        for (int ne1 = 1; ne1 <= 7; ++ne1)
          for (int ne2 = 1; ne2 <= 7; ++ne2) {
            int64_t sum = 0;
            for (int c = 0; c < 8; ++c) {
              SAME(hex27_colour_count(ne1, ne2, c, elo, ehi), old_colour_count(ne1, ne2, c, elo, ehi), "colour %d", c);
              sum += hex27_colour_count(ne1, ne2, c, elo, ehi);
            }
            CHECK(sum == (int64_t)(ehi - elo) * ne1 * ne2, "slab [%d, %d) of %d x %d x %d elements: the eight colours are the elements of [%d, %d)", plo, phi, ne0, ne1, ne2, elo, ehi);
          }
        // the ring over this slab's element planes
        const int npl = ehi - elo;
        const int64_t plane_rows = 35;
        for (int chunk = 0; chunk <= npl + 1; ++chunk) {
          const H27Ring R = h27_ring(npl, 12, chunk);
          CHECK(R.P >= 1 && R.P <= npl && (chunk < 1 || chunk > npl || R.P == chunk) && R.ring == (R.P >= npl ? npl : R.P + 1), "P and ring, %d planes, knob %d", npl, chunk);
          std::vector<int> seen(phi - plo, 0), slot(R.ring, -1);
          for (int a = elo; a < ehi; a += R.P) {
            const int b = a + R.P < ehi ? a + R.P : ehi;
            for (int I = a; I < b; ++I) slot[I % R.ring] = I;  // pass 1 of the chunk
            int64_t row_lo, row_hi;
            h27_chunk_rows(a, b, ehi, plo, phi, plane_rows, &row_lo, &row_hi);
            {  // as the old loop had it
              const int gp_lo = 2 * a < plo ? plo : 2 * a, gp_hi = b == ehi ? phi : 2 * b;
              SAME(row_lo, (int64_t)(gp_lo - plo) * plane_rows, "chunk [%d, %d)", a, b);
              SAME(row_hi, (int64_t)(gp_hi - plo) * plane_rows, "chunk [%d, %d)", a, b);
            }
            CHECK(row_lo % plane_rows == 0 && row_hi % plane_rows == 0 && row_lo >= 0 && row_hi <= (int64_t)(phi - plo) * plane_rows, "chunk [%d, %d): whole owned planes", a, b);
            for (int64_t pl = row_lo / plane_rows; pl < row_hi / plane_rows; ++pl) {
              ++seen[pl];
              const int g = plo + (int)pl;  // the control-point plane reads the element planes it lies in
              for (int I = (g & 1) ? g / 2 : g / 2 - 1; I <= g / 2; ++I) {  // (an even plane is shared by two element planes)
                if (I < elo || I >= ehi) continue;
                CHECK(I >= a - 1 && I <= b - 1, "plane %d of chunk [%d, %d) reads element plane %d", g, a, b, I);
                CHECK(slot[I % R.ring] == I, "element plane %d is still in the ring of %d when chunk [%d, %d) gathers plane %d", I, R.ring, a, b, g);
              }
            }
          }
          for (int pl = 0; pl < phi - plo; ++pl) CHECK(seen[pl] == 1, "slab [%d, %d), P %d: plane %d gathered %d times", plo, phi, R.P, plo + pl, seen[pl]);
        }
      }
  }
  // the issue's own statement of the ring property on whole bricks: npl <= 12, P 1..npl
  for (int npl = 1; npl <= 12; ++npl)
    for (int P = 1; P <= npl; ++P) {
      const H27Ring R = h27_ring(npl, 9, P);
      CHECK(R.P == P, "forced P");
      std::vector<int> seen(2 * npl + 1, 0), slot(R.ring, -1);
      for (int a = 0; a < npl; a += R.P) {
        const int b = a + R.P < npl ? a + R.P : npl;
        for (int I = a; I < b; ++I) slot[I % R.ring] = I;
        for (int I = (a > 0 ? a - 1 : 0); I <= b - 1; ++I) CHECK(slot[I % R.ring] == I, "%d planes, P %d: element plane %d in the ring for chunk [%d, %d)", npl, P, I, a, b);
        int64_t row_lo, row_hi;
        h27_chunk_rows(a, b, npl, 0, 2 * npl + 1, 1, &row_lo, &row_hi);
        for (int64_t g = row_lo; g < row_hi; ++g) ++seen[g];
      }
      for (int g = 0; g <= 2 * npl; ++g) CHECK(seen[g] == 1, "%d planes, P %d: control-point plane %d gathered %d times", npl, P, g, seen[g]);
    }
  // P and ring against the old expressions: knob, budget just below / at / above the whole scratch, and far below it
  for (int npl : {1, 2, 3, 5, 12, 64, 255, 300})
    for (int64_t plane_el : {(int64_t)1, (int64_t)9, (int64_t)1024, (int64_t)16384, (int64_t)1 << 20})
      for (int chunk : {0, 1, 2, 3, 12, 255}) {
        const size_t pb = sizeof(double) * 729 * (size_t)plane_el, whole = pb * (size_t)npl;
        for (size_t budget : {H27_SCRATCH_BUDGET, whole - 1, whole, whole + 1, pb - 1, pb, 2 * pb - 1, 2 * pb, 3 * pb + 1, whole / 2}) {
          int P, ring;
          size_t plane_bytes;
          old_ring(npl, plane_el, chunk, budget, &P, &ring, &plane_bytes);
          const H27Ring R = h27_ring(npl, plane_el, chunk, budget);
          SAME(R.P, P, "%d planes of %lld elements, knob %d, budget %zu", npl, (long long)plane_el, chunk, budget);
          SAME(R.ring, ring, "%d planes of %lld elements, knob %d, budget %zu", npl, (long long)plane_el, chunk, budget);
          SAME(R.plane_bytes, plane_bytes, "plane of %lld elements", (long long)plane_el);
          CHECK(chunk > 0 || whole <= budget || budget < 2 * pb || R.plane_bytes * (size_t)R.ring <= budget, "a ring from the budget fits it");
        }
      }
}

static void check_ws() {
  for (int64_t nel : {(int64_t)1, (int64_t)2, (int64_t)27, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)100, (int64_t)1000, (int64_t)4097, (int64_t)2097152})
    for (int64_t n_stored : {(int64_t)0, (int64_t)1, nel / 2, nel}) {
      const H27Ws W = h27_ws(3, nel, n_stored);
      // G0 | slot | elist | stored Ke, in this order, none overlapping
      CHECK(W.g_bytes == 48 * (size_t)nel && W.slot >= W.g_bytes, "G0 of %lld elements ends before the slot map", (long long)nel);
      CHECK(W.slot + 4 * (size_t)nel <= W.elist, "slot map ends before the element list");
      CHECK(W.elist + 4 * (size_t)nel <= W.count_bytes && W.count_bytes <= W.head, "element list ends before the stored Ke");
      CHECK(W.map_bytes % 256 == 0 && W.head % 256 == 0 && (W.elist - W.slot) % 256 == 0 && W.slot % 8 == 0, "256-byte padding of the maps and of the head");
      CHECK(W.head - W.count_bytes < 256, "no more than the padding in front of the stored Ke");
      CHECK(W.stored_bytes == 5832 * (size_t)n_stored && W.gq_bytes == 1296 * (size_t)nel, "729 doubles per stored element, 6 x 27 per element of G_q");
    }
}

static void check_grids() {
  for (int cus : {1, 8, 104, 256, 304})
    for (int64_t n : {(int64_t)1, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)16 * cus - 1, (int64_t)16 * cus, (int64_t)16 * cus + 1, (int64_t)128 * cus - 1, (int64_t)128 * cus,
                      (int64_t)128 * cus + 1, (int64_t)2097152, ((int64_t)1 << 31) - 1, (int64_t)1 << 33}) {
      SAME(h27_wave_grid(n, cus), old_grid_a(n, cus), "%lld elements, %d CUs", (long long)n, cus);
      SAME(h27_wave_grid(n, cus), old_grid_b(n, cus), "%lld stored elements, %d CUs", (long long)n, cus);
      SAME(h27_direct_grid(n, cus), old_grid_c((n + 64 - 1) / 64, cus), "%lld owned rows, %d CUs", (long long)n, cus);
      SAME(h27_persistent_grid(n, cus), old_grid_c(n, cus), "%lld blocks, %d CUs", (long long)n, cus);
      SAME((long long)h27_gather_grid(5, 5 + n), (long long)(unsigned)((n + 32 - 1) / 32), "%lld gathered rows", (long long)n);
    }
  for (int cus : {1, 256})
    for (int ne0 = 1; ne0 <= 9; ++ne0)
      for (int plo = 0; plo < 2 * ne0 + 1; plo += 2)
        for (int phi = plo + 2; phi <= 2 * ne0 + 1; ++phi) {
          if ((phi & 1) && phi != 2 * ne0 + 1) continue;
          for (int m1 : {3, 5, 7, 9, 257})
            for (int m2 : {3, 5, 11, 129}) {
              const int T0lo = plo / 4, nT0 = (phi - 1) / 4 - T0lo + 1, nT1 = (m1 + 3) / 4, nT2 = (m2 + 3) / 4;
              const int64_t ntiles = (int64_t)nT0 * nT1 * nT2;
              const int gridr = (int)(ntiles < (int64_t)cus * 2 ? ntiles : (int64_t)cus * 2);
              const H27RowsGrid G = h27_rows_grid(plo, phi, m1, m2, cus);
              SAME(G.T0lo, T0lo, "rows tiles"); SAME(G.nT0, nT0, "rows tiles"); SAME(G.nT1, nT1, "rows tiles"); SAME(G.nT2, nT2, "rows tiles");
              SAME(G.grid, gridr, "rows grid");
              CHECK(4 * G.T0lo <= plo && 4 * (G.T0lo + G.nT0) >= phi && 4 * (G.T0lo + G.nT0 - 1) < phi && 4 * G.nT1 >= m1 && 4 * G.nT2 >= m2, "the tiles cover the owned planes");
            }
        }
}

static void check_faces() {
  const int id[3][2] = {{5, 3}, {2, 4}, {1, 6}};  // face ids of (direction, side)
  for (int n0 = 1; n0 <= 4; ++n0)
    for (int n1 = 1; n1 <= 4; ++n1)
      for (int n2 = 1; n2 <= 5; n2 += 2) {
        const int ne[3] = {n0, n1, n2};
        for (uint32_t robin = 0; robin < 64; ++robin)
          for (double h : {0.0, 25.0}) {
            H27FaceLaunch S[24];
            const int n = h27_face_schedule(robin, h, ne, S);
            const std::vector<H27FaceLaunch> O = old_faces(robin, h, ne);
            SAME(n, (int)O.size(), "robin %#x, h %g", robin, h);
            for (int i = 0; i < n && i < (int)O.size(); ++i)
              SAME(S[i].nd * 1000000 + (S[i].side + 1) * 100000 + S[i].colour * 10000 + S[i].n1 * 1000 + S[i].n2 * 100 + S[i].grid,
                   O[i].nd * 1000000 + (O[i].side + 1) * 100000 + O[i].colour * 10000 + O[i].n1 * 1000 + O[i].n2 * 100 + O[i].grid, "robin %#x, launch %d", robin, i);
            CHECK(n <= 24, "at most 3 x 2 x 4 launches");
            for (int nd = 0; nd < 3; ++nd)
              for (int side = 0; side < 2; ++side) {
                const bool flagged = h != 0.0 && (robin & (1u << (id[nd][side] - 1)));
                const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
                for (int colour = 0; colour < 4; ++colour) {
                  const int c1 = (ne[t1] - (colour & 1) + 1) >> 1, c2 = (ne[t2] - (colour >> 1) + 1) >> 1;  // face elements of the class (k_hex27_faces)
                  int covered = 0;
                  for (int i = 0; i < n; ++i)
                    if (S[i].nd == nd && (S[i].side == side || S[i].side < 0) && S[i].colour == colour) {
                      ++covered;
                      const int64_t threads = (int64_t)c1 * c2 * 9 * (S[i].side < 0 ? 2 : 1);
                      CHECK(S[i].n1 == c1 && S[i].n2 == c2 && S[i].n1 > 0 && S[i].n2 > 0, "the class as the kernel counts it");
                      CHECK((int64_t)S[i].grid * 256 >= threads && (int64_t)(S[i].grid - 1) * 256 < threads, "a thread per (face element, face node), no spare workgroup");
                    }
                  CHECK(covered == (flagged && c1 > 0 && c2 > 0 ? 1 : 0), "face %d (direction %d, side %d), colour %d, robin %#x: covered %d times", id[nd][side], nd, side, colour, robin, covered);
                }
              }
          }
      }
}

// ---- 3. the functions against the macros of k_hex27 ----------------------------------------------------------------------------------------------------
static void check_lds() {
  for (int ng = 1; ng <= 4; ++ng)
    for (int mode = 0; mode < 3; ++mode) {
      const int nq = ng * ng * ng, NI = mode == 0 ? 5 : 3;  // (the names the macros read)
      SAME(h27_mode_ni(mode), NI, "mode %d", mode);
      SAME(h27_n1(ng, NI), H27_N1, "ng %d, mode %d", ng, mode);
      SAME(h27_n2(ng, NI), H27_N2, "ng %d, mode %d", ng, mode);
      SAME(h27_n3(nq, NI), H27_N3, "ng %d, mode %d", ng, mode);
      SAME(h27_na(ng), H27_NA, "ng %d", ng);
      SAME(h27_nb(ng), H27_NB, "ng %d", ng);
      SAME(h27_w_t1(NI), W_T1, "ng %d, mode %d", ng, mode);
      SAME(h27_w_t2(ng, nq, NI), W_T2, "ng %d, mode %d", ng, mode);
      SAME(h27_w_d(ng, nq, NI), W_D, "ng %d, mode %d", ng, mode);
      SAME(h27_w_info(ng, nq, NI), W_INFO, "ng %d, mode %d", ng, mode);
      SAME(h27_w_size(ng, nq, NI, false), W_SIZE(false), "ng %d, mode %d", ng, mode);
      SAME(h27_w_size(ng, nq, NI, true), W_SIZE(true), "ng %d, mode %d", ng, mode);
      SAME(h27_ndec(ng, nq, NI), H27_NDEC, "ng %d, mode %d", ng, mode);
      // the old host-side size, through the macros
      const size_t old_bytes = sizeof(double) * ((size_t)(mode == 0 ? 0 : (H27_NQP(nq) + 1) * 81) + ((nq + 1) & ~1) + 8 * ng + (h27_pad(H27_NDEC) >> 1) +
                                                 H27_WAVES * (size_t)(W_SIZE(mode == 1)));
      SAME(hex27_lds_bytes(ng, mode), old_bytes, "ng %d, mode %d", ng, mode);
      // the residual's overlays stay inside the spaces they reuse: s at the Gauss points and stage B in front of T2, flux and source in front of w det
      if (mode == 0)
        CHECK(W_SV + nq <= W_T2 && W_WB + H27_NB <= W_T2 && W_G + 3 * h27_pad(nq) + nq <= W_D && W_D + nq <= W_INFO, "ng %d: the residual's overlays fit", ng);
      CHECK(hex27_lds_bytes(ng, mode) <= 160 * 1024, "ng %d, mode %d: %zu bytes fit the 160 KB of a CU", ng, mode, hex27_lds_bytes(ng, mode));
    }
  static_assert(hex27_lds_bytes(3, 2) == sizeof(double) * ((28 + 1) * 81 + 28 + 24 + ((162 + 243 + 243) >> 1) + 8 * (244 + 244 + 28)), "ng = 3, matrix -> scratch");
}

int main() {
  const std::vector<int> words = knob_words();
  check_knobs(words);
  check_paths(words);
  check_planes_and_ring();
  check_ws();
  check_grids();
  check_faces();
  check_lds();
  printf("hex27_decide: %lld cases, %lld differences from the driver before the cut, %lld property checks failed\n", cases, diffs, bad);
  if (diffs || bad) return printf("FAILED\n"), 1;
  printf("hex27_decide: OK\n");
  return 0;
}
