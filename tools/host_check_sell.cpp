// CPU walk through every branch of the host decisions of solver layout mode 3 (csrc/sell_decide.h): the knob words, which patterns get the row-sorted
// or the node-blocked form, the sort key widths, the padding limits and thresholds at their edges, the copy of the node-blocked values, the grid
// caps and part ranges of a launch, which instantiation every knob value gets, and the byte accounting of the three kinds of plan.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_sell.cpp -o tools/bin/host_check_sell && tools/bin/host_check_sell
#include <cstdio>
#include "sell_decide.h"

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf(": %s\n", #cond); ++bad; } } while (0)

// a pattern of n rows, `m` entries in the longest, `mean` on average; no ghosts, no lattice hint, threshold 0
static SellShape shape(int64_t n, int m, int mean = 0) { return {n, n, n * (int64_t)(mean ? mean : m), m, 0, 0, 0, 0}; }
static SellShape ghosts(SellShape S, int64_t extra) { S.ncols = S.n + extra; return S; }
static SellShape lattice(SellShape S, int m1, int m2, int fields) { S.lat_m1 = m1; S.lat_m2 = m2; S.lat_fields = fields; return S; }
static bool same(const SellKnobs& a, const SellKnobs& b) {
  return a.enable == b.enable && a.offsets == b.offsets && a.xcd == b.xcd && a.periodic == b.periodic && a.region == b.region &&
         a.window_log2 == b.window_log2 && a.unroll == b.unroll && a.per_u == b.per_u && a.wg_per_cu == b.wg_per_cu;
}

static void check_knobs() {
  const SellKnobs off = {false, true, false, true, 0, 0, 5, 0, 8}, on = {true, true, false, true, 0, 0, 5, 0, 8};
  CHECK(same(sell_knobs_decode(0), off), "all zero: off, and the defaults 5 and 8");
  CHECK(same(sell_knobs_decode(SELL_WORD_DEFAULT), on), "the library's default word");
  SellKnobs k = off;
  k.offsets = false;
  CHECK(same(sell_knobs_decode(2), k), "bit 1: explicit columns");
  k = off, k.xcd = true;
  CHECK(same(sell_knobs_decode(4), k), "bit 2: XCD walk");
  k = off, k.periodic = false;
  CHECK(same(sell_knobs_decode(8), k), "bit 3: periodic off");
  k = off, k.region = 120;
  CHECK(same(sell_knobs_decode(15 << 4), k) && sell_knobs_decode(1 << 4).region == 8, "bits 4-7: region edge x 8");
  k = off, k.window_log2 = 63;
  CHECK(same(sell_knobs_decode(63 << 8), k), "bits 8-13: window");
  k = off, k.unroll = 31;
  CHECK(same(sell_knobs_decode(31 << 16), k), "bits 16-20: unroll");
  k = off, k.per_u = 3;
  CHECK(same(sell_knobs_decode(3 << 21), k), "bits 21-22: node slots in flight");
  k = off, k.wg_per_cu = 31;
  CHECK(same(sell_knobs_decode(31 << 24), k), "bits 24-28: workgroups per CU");
  CHECK(same(sell_knobs_decode((1 << 14) | (1 << 15) | (1 << 23) | (1 << 29) | (1 << 30)), off), "bits without a meaning");
  CHECK(same(sell_knobs_decode(1 | 8), {true, true, false, false, 0, 0, 5, 0, 8}), "the word 1 | 8 of the tests");
  for (int w = 0; w < 4; ++w) {
    const BsellKnobs B = bsell_knobs_decode(w);
    CHECK(B.enable == ((w & 1) != 0) && B.fill_quads == ((w & 2) != 0), "bsell word %d", w);
  }
  CHECK(bsell_knobs_decode(BSELL_WORD_DEFAULT).enable && !bsell_knobs_decode(BSELL_WORD_DEFAULT).fill_quads, "bsell default: on, LDS transpose");
}

static void check_eligibility() {
  const SellKnobs K = sell_knobs_decode(1);
  CHECK(sell_state_wanted(shape(127, 27)) == -1 && sell_state_wanted(shape(128, 27)) == 1, "a block of rows at least");
  CHECK(sell_state_wanted(shape(((int64_t)1 << 31) - 1, 27)) == 1 && sell_state_wanted(shape((int64_t)1 << 31, 27)) == -1, "row numbers are 31 bits");
  CHECK(sell_state_wanted({1000, 1000, 0, 0, 0, 0, 0, 0}) == -1 && sell_state_wanted({1000, 1000, 5, 0, 0, 0, 0, 0}) == -1, "an empty pattern");
  SellShape S = shape(1000, 27);
  S.min_rows = 1001;
  CHECK(sell_state_wanted(S) == 0 && !sell_serves(1, K, S), "below the row threshold: not planned, not served");
  S.min_rows = 1000;
  CHECK(sell_state_wanted(S) == 1 && sell_serves(1, K, S) && !sell_serves(-1, K, S) && !sell_serves(0, K, S) && !sell_serves(1, sell_knobs_decode(0), S),
        "at the threshold: served when ready and on");
  SellShape tiny = shape(100, 27);
  tiny.min_rows = 200;
  CHECK(sell_state_wanted(tiny) == 0, "the threshold is asked before the eligibility");
  CHECK(sell_blocks(128) == 1 && sell_blocks(129) == 2 && bsell_blocks(64) == 1 && bsell_blocks(65) == 2, "block counts");
}

static void check_node_blocks() {
  const BsellKnobs B = bsell_knobs_decode(1);
  // (n, longest row) divisible by 4 / 3 / 2 / none
  const struct { int64_t n; int m; bool f4, f3, f2; } cases[] = {{1200, 120, true, true, true}, {1203, 81, false, true, false}, {1202, 46, false, false, true},
                                                                 {1201, 120, false, false, false}, {1200, 119, false, false, false}, {1200, 90, false, true, true}};
  for (const auto& c : cases) {
    const SellShape S = shape(c.n, c.m);
    CHECK(sell_fields_divide(S, 4) == c.f4 && sell_fields_divide(S, 3) == c.f3 && sell_fields_divide(S, 2) == c.f2, "fields that divide (%lld, %d)", (long long)c.n, c.m);
  }
  CHECK(SELL_NODE_FIELDS[0] == 4 && SELL_NODE_FIELDS[1] == 3 && SELL_NODE_FIELDS[2] == 2, "node-blocked: the largest F first");
  CHECK(SELL_PERIODIC_FIELDS[0] == 3 && SELL_PERIODIC_FIELDS[1] == 2 && SELL_PERIODIC_FIELDS[2] == 4, "field-periodic: 3, 2, 4");
  CHECK(bsell_may_try(shape(1200, 81), B) && !bsell_may_try(shape(1200, 81), bsell_knobs_decode(0)) && bsell_may_try(shape(1200, 81), bsell_knobs_decode(3)), "the bsell switch");
  CHECK(!bsell_may_try(lattice(shape(1200, 81), 10, 10, 3), B), "a lattice hint keeps the row-sorted form");
  CHECK(!bsell_may_try(ghosts(shape(1200, 81), 100), B) && !sell_node_check_possible(ghosts(shape(1200, 81), 1)), "ghost columns keep the row-sorted form");
  CHECK(!bsell_may_try(shape(255, 81), B) && bsell_may_try(shape(256, 81), B), "n = 255 / 256");
  CHECK(sell_node_check_possible(shape(2, 2)) && !sell_node_check_possible(shape(1, 2)) && !sell_node_check_possible(shape(2, 1)), "what the entry-by-entry check needs");
  CHECK(!bsell_enough_nodes(shape(63 * 3, 81), 3) && bsell_enough_nodes(shape(64 * 3, 81), 3) && !bsell_enough_nodes(shape(1200, 81), 0), "n / F = 63 / 64, no F");
  const SellKnobs K = sell_knobs_decode(1);
  CHECK(sell_periodic_may_try(shape(1280, 81), K, 4, 10) && !sell_periodic_may_try(shape(1280, 81), K, 5, 10), "periodic blocks: fewer than half the blocks regular");
  CHECK(!sell_periodic_may_try(shape(1280, 81), sell_knobs_decode(1 | 8), 0, 10) && !sell_periodic_may_try(ghosts(shape(1280, 81), 5), K, 0, 10), "periodic blocks: knob, ghosts");
}

static void check_keys() {
  const SellKnobs K = sell_knobs_decode(1);
  CHECK(sell_len_bits(0) == 1 && sell_len_bits(1) == 1 && sell_len_bits(2) == 2 && sell_len_bits(127) == 7 && sell_len_bits(128) == 8 && sell_len_bits(0x7fffffff) == 31, "length bits");
  CHECK(sell_window_shift(K) == 63 && sell_window_shift(sell_knobs_decode(1 | (10 << 8))) == 10, "window shift");
  const SellShape S = shape(262144, 125, 60);  // 7 length bits
  CHECK(sell_regions(S, K).R == 0 && sell_key_bits(S, K, sell_regions(S, K)) == 39, "plain: signature and length");
  {
    const SellKnobs Kw = sell_knobs_decode(1 | (10 << 8));  // 256 windows of 1024 rows: 8 bits
    CHECK(sell_key_bits(S, Kw, sell_regions(S, Kw)) == 47, "windowed");
    CHECK(sell_key_bits(shape(1024, 125), Kw, SellRegions{}) == 39, "one window: no window bits");
  }
  {
    const SellKnobs Kr = sell_knobs_decode(1 | (2 << 4));  // regions of 16^3 lattice points
    const SellShape L = lattice(shape(64 * 64 * 64, 125, 60), 64, 64, 1);
    const SellRegions G = sell_regions(L, Kr);
    CHECK(G.R == 16 && G.n_nodes == 262144 && G.PL == 4096 && G.m2 == 64 && G.nri == 4 && G.nrj == 4 && G.nrk == 4 && sell_region_count(L, G) == 64, "regions of a 64^3 lattice");
    CHECK(sell_key_bits(L, Kr, G) == 45, "regions: 6 bits on top");
    const SellShape L3 = lattice(shape(3 * 33 * 20 * 24, 81), 20, 24, 3);
    const SellRegions G3 = sell_regions(L3, Kr);
    CHECK(G3.R == 16 && G3.n_nodes == 33 * 480 && G3.nri == 3 && G3.nrj == 2 && G3.nrk == 2 && sell_region_count(L3, G3) == 36, "three fields, edges that R does not divide");
    CHECK(sell_regions(lattice(shape(262144 + 64, 125), 64, 64, 1), Kr).R == 0, "rows that are no whole planes: no regions");
    CHECK(sell_regions(lattice(shape(262144, 125), 64, 64, 3), Kr).R == 0, "rows that the fields do not divide");
    CHECK(sell_regions(S, Kr).R == 0 && sell_regions(L, K).R == 0, "no hint, or no knob");
    CHECK(sell_regions(L, sell_knobs_decode(1 | (2 << 4) | (10 << 8))).R == 0, "a row window overrides the regions");
    CHECK(sell_key_bits(ghosts(L, 4096), Kr, sell_regions(ghosts(L, 4096), Kr)) == 64, "ghosts with regions");
  }
  CHECK(sell_key_bits(ghosts(S, 1), K, SellRegions{}) == 64, "ghosts: the whole key");
}

static void check_thresholds() {
  const SellRegions none{}, reg = {16, 1, 1, 1, 1, 1, 1};
  const SellShape S = shape(1000, 100, 80);  // nnz 80000: 1.15 x = 92000, + 128 x 100
  CHECK(sell_padding_ok(S, none, 92000 + 12800) && !sell_padding_ok(S, none, 92000 + 12800 + 1), "row-sorted padding limit");
  CHECK(sell_padding_ok(S, reg, 100000 + 12800) && !sell_padding_ok(S, reg, 100000 + 12800 + 1), "... with regions (1.25)");
  CHECK(sell_padding_ok(ghosts(S, 9), none, 92000 + 25600) && !sell_padding_ok(ghosts(S, 9), none, 92000 + 25600 + 1), "... with ghosts (256 rows)");
  const SellShape E = shape(1200, 120, 100);  // nnz 120000: 1.15 x = 138000, + 128 x 120 x 3 = 46080; slots x 9
  CHECK(bsell_padding_ok(E, 3, 184080 / 9) && !bsell_padding_ok(E, 3, 184080 / 9 + 1), "node-blocked padding limit (%d)", 184080 / 9);
  CHECK(184080 % 9 != 0 && bsell_padding_ok(shape(1200, 120, 90), 2, (124200 + 30720) / 4) && !bsell_padding_ok(shape(1200, 120, 90), 2, (124200 + 30720) / 4 + 1), "... at equality, F = 2");
  CHECK(sell_signatures_repeat(800, 100) && !sell_signatures_repeat(800, 99) && sell_signatures_repeat(807, 100) && sell_signatures_repeat(7, 0), "signatures repeat: n / 8");
  CHECK(sell_periodic_taken(400, 100) && !sell_periodic_taken(400, 99) && sell_periodic_taken(403, 100) && !sell_periodic_taken(404, 100) && sell_periodic_taken(3, 0), "periodic taken: nblk / 4");
  CHECK(sell_nb_int(shape(1000, 27), 0) == 8 && sell_nb_int(ghosts(shape(1000, 27), 50), 0) == 7 && sell_nb_int(ghosts(shape(1000, 27), 50), 104) == 7 &&
        sell_nb_int(ghosts(shape(1000, 27), 50), 105) == 6 && sell_nb_int(ghosts(shape(1000, 27), 50), 1000) == 0, "interior blocks from the ghost-reading rows");
  CHECK(sell_inspect_grid(10, 256) == 10 && sell_inspect_grid(1 << 20, 256) == 16384, "inspection grid");
}

static void check_bind() {
  const BsellKnobs T = bsell_knobs_decode(1), Q = bsell_knobs_decode(3);
  BsellCopy C = bsell_copy(BSELL_T_MAXL, 3, T);
  CHECK(C.transpose && C.ldl == 127 && C.lds_bytes == 8u * 64 * 127 + 3 * 64 * 8 + 64 * 4, "the longest list the transpose takes");
  CHECK(C.lds_bytes <= 160 * 1024, "... fits the 160 KiB of LDS of a gfx950 CU (%zu bytes)", C.lds_bytes);
  CHECK(!bsell_copy(BSELL_T_MAXL + 1, 3, T).transpose && !bsell_copy(27, 3, Q).transpose && bsell_copy(27, 3, T).transpose, "one above, and the quads switch");
  C = bsell_copy(28, 4, T);
  CHECK(C.ldl == 29 && C.lds_bytes == 8u * 64 * 29 + 4 * 64 * 8 + 64 * 4 && bsell_copy(27, 2, T).ldl == 27, "ldl odd");
  CHECK(bsell_copy(BSELL_T_MAXL, 4, T).lds_bytes <= 160 * 1024 && 2 * 64 > BSELL_T_MAXL, "four fields; two entries per lane cover the list");
  CHECK(bsell_copy_grid(100, 3, 256) == 300 && bsell_copy_grid(10000, 3, 256) == 3072, "copy grid");
}

static void check_launch() {
  const SellKnobs K = sell_knobs_decode(1);
  CHECK(sell_grid_cap(256, K, 4096, 0) == 2048 && sell_grid_cap(256, K, 4096, 1) == 1024 && sell_grid_cap(256, K, 4096, 2) == 1024, "grid cap and its halving");
  CHECK(sell_grid_cap(256, sell_knobs_decode(1 | (31 << 24)), 4096, 0) == 4096 && sell_grid_cap(256, sell_knobs_decode(1 | (31 << 24)), 4096, 2) == 2048, "clamped to the partial sums");
  CHECK(sell_grid_cap(1, K, 4096, 0) == 8 && sell_grid_cap(1, sell_knobs_decode(1 | (1 << 24)), 4096, 1) == 0, "one CU");
  for (int nb_int = 0; nb_int <= 10; nb_int += 5) {
    const SellRange a = sell_part_range(0, nb_int, 10), i = sell_part_range(1, nb_int, 10), b = sell_part_range(2, nb_int, 10);
    CHECK(a.lo == 0 && a.hi == 10 && i.lo == 0 && i.hi == nb_int && b.lo == nb_int && b.hi == 10, "part ranges with %d interior blocks of 10", nb_int);
  }
  for (int u = 0; u < 32; ++u) {
    const int r = sell_unroll_resolved(sell_knobs_decode(1 | (u << 16)));
    const bool inst = u == 4 || u == 8 || u == 9 || u == 10 || u == 15;
    CHECK(r == (inst ? u : 5), "unroll %d -> %d", u, r);
  }
  const int u3[4] = {3, 2, 4, 1};
  for (int p = 0; p < 4; ++p) {
    const SellKnobs Kp = sell_knobs_decode(1 | (p << 21));
    const BsellFU f3 = bsell_fu_resolved(3, Kp), f2 = bsell_fu_resolved(2, Kp), f4 = bsell_fu_resolved(4, Kp);
    CHECK(f3.F == 3 && f3.U == u3[p] && f2.F == 2 && f2.U == 4 && f4.F == 4 && f4.U == 2, "(F, U) with per_u %d", p);
    CHECK(sell_periodic_word(Kp, 3) == (3 | (p << 4)) && sell_periodic_word(Kp, 0) == (p << 4) && sell_periodic_word(sell_knobs_decode(1 | 8 | (p << 21)), 3) == 0, "periodic word, per_u %d", p);
  }
  CHECK(sell_xcd_flag(sell_knobs_decode(1 | 4), 2048) == 1 && sell_xcd_flag(sell_knobs_decode(1 | 4), 2047) == 0 && sell_xcd_flag(K, 2048) == 0, "XCD walk: the knob, and a grid of whole eighths");
}

static void check_bytes() {
  SellLayout L{};
  L.state = 1, L.form = SELL_NODE_BLOCKED, L.total = 9000, L.nblk = 4;
  L.nodes.F = 3, L.nodes.ncp = 250, L.nodes.slots = 1000;
  CHECK(sell_design_bytes(L, 750) == 9000 * 8 + 1000 * 4 + 750 * 16 + 250 * 4 && sell_padded_rows(L) == 4 * 64 * 3, "node-blocked: one column per F x F values");
  L = SellLayout{};
  L.state = 1, L.form = SELL_ROW_SORTED, L.total = 100000, L.nblk = 8;
  CHECK(sell_design_bytes(L, 1000) == 100000 * 8 + 100000 * 4 + 1000 * 20 && sell_padded_rows(L) == 1024, "row-sorted, every block generic");
  L.rows.regular_blocks = 6;
  CHECK(sell_design_bytes(L, 1000) == 100000 * 8 + 25000 * 4 + 1000 * 20, "regular fraction: three quarters of the column stream not read");
  L.rows.regular_blocks = 0, L.rows.fields = 3, L.rows.periodic_blocks = 4;
  CHECK(sell_design_bytes(L, 1000) == 100000 * 8 + (int64_t)((0.5 + 0.5 / 3.0) * 100000.0) * 4 + 1000 * 20, "periodic fraction: a third of half the column stream");
  L.rows.fields = 0;
  CHECK(sell_design_bytes(L, 1000) == 100000 * 8 + 100000 * 4 + 1000 * 20, "periodic blocks count only with their field count");
  L.nblk = 0;
  CHECK(sell_design_bytes(L, 0) == 100000 * 12, "no blocks");
}

int main() {
  check_knobs();
  check_eligibility();
  check_node_blocks();
  check_keys();
  check_thresholds();
  check_bind();
  check_launch();
  check_bytes();
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
