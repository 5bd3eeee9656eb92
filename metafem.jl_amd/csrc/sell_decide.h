// The host decisions of solver layout mode 3 -- the row-sorted sliced layout (spmv_sell.hip) and its node-blocked form (spmv_bsell.hip): which
// patterns get which form, how their sort keys are laid out, how much padding is accepted, which copy and which product instantiation a launch
// takes -- and the record of what a plan built (mfem_csr_s::sell).  The plan, the bind, the launch and the accounting all ask here.  No HIP, no
// context: tools/host_check_sell.cpp walks every branch on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define SELL_B 128        // rows of a block of the row-sorted form
#define BSELL_B 64        // nodes of a block of the node-blocked form
#define BSELL_T_MAXL 127  // longest coupling list (nodes) the LDS-transpose copy of the node-blocked form takes (k_bsell_fill_t: two entries per lane)

// The word of mfem_debug_set_sell, decoded once.
struct SellKnobs {
  bool enable;      // bit 0: the layout on / off
  bool offsets;     // bit 1 CLEAR: blocks with one diagonal list skip their column stream (set: always read explicit columns)
  bool xcd;         // bit 2: every XCD walks a contiguous eighth of the block list
  bool periodic;    // bit 3 CLEAR: field-periodic blocks read one column slot per node (set: their whole column stream)
  int region;       // bits 4-7 x 8: edge of the lattice regions of the row sort (0 = global sort)
  int window_log2;  // bits 8-13: rows are sorted within windows of 2^w consecutive rows (0 = over the whole matrix)
  int unroll;       // bits 16-20: slots in flight per lane (0 = the default, 5)
  int per_u;        // bits 21-22: node slots in flight of a field-periodic block of three fields (0: 3 -- the default --, 1: 2, 2: 4) and of the
                    // node-blocked product (0: 3, 1: 2, 2: 4, 3: 1)
  int wg_per_cu;    // bits 24-28: workgroups per CU of the product's grid (0 = the default, 8)
};
#define SELL_WORD_DEFAULT 1
static inline SellKnobs sell_knobs_decode(int word) {
  const int u = (word >> 16) & 31, w = (word >> 24) & 31;
  return {(word & 1) != 0, !(word & 2), (word & 4) != 0, !(word & 8), ((word >> 4) & 15) * 8, (word >> 8) & 63, u ? u : 5, (word >> 21) & 3, w ? w : 8};
}
// mfem_debug_set("bsell", on): bit 0 the node-blocked form on / off, bit 1 its layout copy by lane quads per row instead of the LDS transpose
struct BsellKnobs {
  bool enable, fill_quads;
};
#define BSELL_WORD_DEFAULT 1
static inline BsellKnobs bsell_knobs_decode(int on) { return {(on & 1) != 0, (on & 2) != 0}; }

// what the decisions know of a pattern
struct SellShape {
  int64_t n, ncols, nnz;
  int max_row_nnz;
  int lat_m1, lat_m2, lat_fields;  // lattice hint (0 = none)
  int64_t min_rows;                // below: launch-bound sizes stay on the CSR tile kernel (mfem_debug_set_layout_min_rows)
};
static inline bool sell_has_ghosts(const SellShape& S) { return S.ncols > S.n; }  // a slab pattern: columns numbered behind the n owned ones
static inline int64_t sell_blocks(int64_t n) { return (n + SELL_B - 1) / SELL_B; }
static inline int64_t bsell_blocks(int64_t ncp) { return (ncp + BSELL_B - 1) / BSELL_B; }

// ---- plan ---------------------------------------------------------------------------------------------------------------------------------
// The value SellLayout::state gets before anything is built: 0 = not planned (too few rows: do not even sort, ask again when the threshold
// changes), -1 = not eligible, 1 = go on and plan
static inline int sell_state_wanted(const SellShape& S) {
  if (S.n < S.min_rows) return 0;
  if (S.n < SELL_B || S.nnz < 1 || S.max_row_nnz < 1 || S.n >= ((int64_t)1 << 31)) return -1;
  return 1;
}
// does a bound copy serve the products (mfem_sell_vals_bytes, and so the layout choice)?
static inline bool sell_serves(int state, const SellKnobs& K, const SellShape& S) { return state == 1 && K.enable && S.n >= S.min_rows; }

// Field counts F tried for a field-major pattern of n = F * nodes rows, in order: the node-blocked form takes the largest that fits (four fields
// also read as two super-fields of two), the field-periodic blocks of the row-sorted form the first that covers a quarter of the blocks.
static const int SELL_NODE_FIELDS[3] = {4, 3, 2};
static const int SELL_PERIODIC_FIELDS[3] = {3, 2, 4};
static inline bool sell_fields_divide(const SellShape& S, int F) { return S.n % F == 0 && S.max_row_nnz % F == 0; }
// is the entry-by-entry check of the node-blocked form (mfem_node_block_fields) worth asking at all?
static inline bool sell_node_check_possible(const SellShape& S) { return !(sell_has_ghosts(S) || S.n < 2 || S.max_row_nnz < 2); }
// may the node-blocked form be tried?  (slab patterns with ghost columns and lattice patterns keep the row-sorted form)
static inline bool bsell_may_try(const SellShape& S, const BsellKnobs& B) {
  return B.enable && !sell_has_ghosts(S) && S.lat_fields <= 0 && S.n >= BSELL_B * 4;
}
// ... and taken with the F the check found (0: none)?  At least one full block of nodes.
static inline bool bsell_enough_nodes(const SellShape& S, int F) { return F != 0 && S.n / F >= BSELL_B; }
static inline bool sell_periodic_may_try(const SellShape& S, const SellKnobs& K, int64_t regular_blocks, int64_t nblk) {
  return K.periodic && !sell_has_ghosts(S) && regular_blocks < nblk / 2;
}

// bits that hold max_len - len of a row (or of a node's coupling list): the whole sort key of the node-blocked form
static inline int sell_len_bits(int max_len) {
  int bits = 1;
  while ((1 << bits) <= max_len && bits < 31) ++bits;
  return bits;
}
static inline int sell_window_shift(const SellKnobs& K) { return K.window_log2 > 0 ? K.window_log2 : 63; }  // (63: one window)

struct SellRegions {  // lattice regions of the row sort (R = 0: none); an argument of k_sell_keys
  int R;
  int64_t n_nodes, PL, m2, nri, nrj, nrk;
};
// cubes of R^3 lattice points per field, when the knob asks for them (and no row window), the pattern has a lattice hint and whole planes
static inline SellRegions sell_regions(const SellShape& S, const SellKnobs& K) {
  SellRegions G{};
  if (K.region > 0 && K.window_log2 == 0 && S.lat_m1 > 0 && S.lat_m2 > 0 && S.lat_fields > 0 && S.n % S.lat_fields == 0 &&
      (S.n / S.lat_fields) % ((int64_t)S.lat_m1 * S.lat_m2) == 0) {
    G.R = K.region;
    G.n_nodes = S.n / S.lat_fields;
    G.PL = (int64_t)S.lat_m1 * S.lat_m2;
    G.m2 = S.lat_m2;
    G.nri = (G.n_nodes / G.PL + G.R - 1) / G.R;
    G.nrj = (S.lat_m1 + G.R - 1) / G.R;
    G.nrk = (S.lat_m2 + G.R - 1) / G.R;
  }
  return G;
}
static inline uint64_t sell_region_count(const SellShape& S, const SellRegions& G) {
  return G.R > 0 ? (uint64_t)S.lat_fields * G.nri * G.nrj * G.nrk : 1;
}
// Key bits the row sort looks at.  The 64-bit key of k_sell_keys: [63] reads a ghost column | region or window index | max_len - len (lenbits)
// | [31:0] signature of the diagonal list.
static inline int sell_key_bits(const SellShape& S, const SellKnobs& K, const SellRegions& G) {
  const int lenbits = sell_len_bits(S.max_row_nnz), wshift = sell_window_shift(K);
  int bits = 32 + lenbits;
  if (G.R > 0) {
    const uint64_t nwin = sell_region_count(S, G);
    while (bits < 63 && ((nwin - 1) >> (bits - 32 - lenbits))) ++bits;  // region index on top
  } else if (wshift < 63) {
    while (bits < 64 && ((uint64_t)(S.n - 1) >> wshift) >> (bits - 32 - lenbits)) ++bits;  // window index on top
  }
  return sell_has_ghosts(S) ? 64 : bits;  // ... and the ghost-reading rows behind everything else
}

// Do the diagonal-list signatures repeat (count: rows that share theirs with one of the next two)?  Then they take part in the sort.
static inline bool sell_signatures_repeat(int64_t n, int64_t count) { return count >= n / 8; }
// Padding accepted.  Row-sorted: up to one block of the longest rows at the tail; with ghost-reading rows sorted last, one more where they begin;
// with lattice regions every region pads each of its row lengths to whole blocks (the regions are sized so that this stays small).
static inline bool sell_padding_ok(const SellShape& S, const SellRegions& G, int64_t total) {
  return (double)total <= (G.R > 0 ? 1.25 : 1.15) * (double)S.nnz + (sell_has_ghosts(S) ? 256.0 : 128.0) * S.max_row_nnz;
}
// ... node-blocked (slots: node slots x 64 over all blocks, F x F values each)
static inline bool bsell_padding_ok(const SellShape& S, int F, int64_t slots) {
  return (double)slots * F * F <= 1.15 * (double)S.nnz + 128.0 * S.max_row_nnz * F;
}
// are `count` field-periodic blocks enough to take the form?  (a few that happened to fit are put back to "generic")
static inline bool sell_periodic_taken(int64_t nblk, int64_t count) { return count >= nblk / 4; }
// The rows that read ghost columns are the last n_ghost sorted rows: the blocks in front of the first of them form the interior part of a
// split SpMV (the block that holds both kinds belongs to the boundary part).
static inline int64_t sell_nb_int(const SellShape& S, int64_t n_ghost) { return sell_has_ghosts(S) ? (S.n - n_ghost) / SELL_B : sell_blocks(S.n); }
// grid of the per-block inspections (a workgroup per block)
static inline int sell_inspect_grid(int64_t nblk, int num_cus) { return (int)(nblk < (int64_t)num_cus * 64 ? nblk : (int64_t)num_cus * 64); }

// ---- what a plan built (mfem_csr_s::sell) --------------------------------------------------------------------------------------------------
enum SellForm : int { SELL_NONE = 0, SELL_ROW_SORTED, SELL_NODE_BLOCKED };
struct SellLayout {
  int state;      // 0 = not planned, -1 = no, 1 = ready
  SellForm form;  // (SELL_NONE unless ready)
  int64_t total;  // value entries of the copy, padding included
  int64_t nblk;   // blocks: of SELL_B sorted rows / of BSELL_B sorted nodes
  // Row-sorted form: element (sorted row r', slot s) at ptr[b] + s * 128 + (r' & 127), b = r' / 128.
  struct Rows {
    int64_t nb_int;          // leading blocks without a ghost-reading row (= nblk without ghost columns): the interior part of a split SpMV
    int32_t* rowid;          // owned, [n]: sorted position -> row
    int64_t* ptr;            // owned, [nblk + 1]: start of each block in the sliced arrays
    int32_t* cols;           // owned, [total], 0-based
    int32_t* flags;          // owned, [nblk]: 1 = all 128 rows share one diagonal list, 2 = field-periodic
    int32_t* off;            // owned, [total / 128 + 1]: that list, at ptr[b] / 128
    int32_t regular_blocks;  // blocks with flag 1
    // field-periodic blocks: a field-major multi-field matrix repeats the node list of a row once per column field, shifted by the rows of a field; a
    // block whose 128 rows have one length K = F * P and columns col[f * P + t] = col[t] + f * shift reads the first P slots' columns only
    int32_t fields;          // F (0: none found)
    int64_t shift;           // column shift between two fields
    int32_t periodic_blocks;
    int32_t sig_sorted;      // 1: the diagonal-list signature took part in the row sort (lattice patterns); 0: mesh order within a length (unstructured)
  } rows;
  // Node-blocked form: a field-major F-field matrix whose F rows of a node share the node's coupling list -- a lane owns a NODE: per coupled node
  // one column index, F gathers of x and F x F values.  Slot t of block b: F * F runs of 64 values at (ptr[b] + t * 64) * F * F.
  struct Nodes {
    int32_t F;
    int64_t ncp;      // nodes (n / F)
    int64_t slots;    // node slots x 64 over all blocks (total = slots * F * F)
    int32_t* nodeid;  // owned, [ncp]: sorted position -> node
    int64_t* ptr;     // owned, [nblk + 1]: start of each block in node slots x 64
    int32_t* cols;    // owned, [slots]: node-level columns, 0-based
  } nodes;
  const double* src;  // the CSR-ordered values the bound copy mirrors (identity of the `vals` argument)
  double* vals;       // not owned (solver workspace), [total]; null = nothing bound
};
static inline int64_t sell_padded_rows(const SellLayout& L) {
  return L.form == SELL_NODE_BLOCKED ? L.nblk * BSELL_B * L.nodes.F : L.nblk * SELL_B;
}
// Bytes one SpMV moves by design: the values, 4-byte columns where the kernel reads them, x and y once, the permutation.  Blocks whose 128 rows
// share one diagonal list read it instead of their column stream; field-periodic blocks read one column slot per node: 1 / F of theirs; the
// node-blocked form reads one column per F x F values.
static inline int64_t sell_design_bytes(const SellLayout& L, int64_t n) {
  if (L.form == SELL_NODE_BLOCKED) return L.total * 8 + L.nodes.slots * 4 + n * 16 + L.nodes.ncp * 4;
  const SellLayout::Rows& R = L.rows;
  const double regf = L.nblk > 0 ? (double)R.regular_blocks / (double)L.nblk : 0.0;
  const double per = (L.nblk > 0 && R.fields > 1) ? (double)R.periodic_blocks / (double)L.nblk : 0.0;
  const double colfrac = (1.0 - regf - per) + (R.fields > 1 ? per / (double)R.fields : 0.0);
  return L.total * 8 + (int64_t)(colfrac * (double)L.total) * 4 + n * 16 + n * 4;
}

// ---- bind ---------------------------------------------------------------------------------------------------------------------------------
// The copy of the node-blocked values: through an LDS transpose (k_bsell_fill_t) for coupling lists of up to BSELL_T_MAXL nodes, by lane quads
// per row (k_bsell_fill) beyond, or when the knob asks.  ldl: the odd row stride of the LDS tile (phase 2's lanes -- one node each -- spread
// over the banks); the tile is followed by [F][64] segment starts (int64) and [64] lengths (int).
struct BsellCopy {
  bool transpose;
  int ldl;
  size_t lds_bytes;
};
static inline BsellCopy bsell_copy(int maxL, int F, const BsellKnobs& B) {
  const int ldl = maxL | 1;
  return {maxL <= BSELL_T_MAXL && !B.fill_quads, ldl, sizeof(double) * (size_t)BSELL_B * ldl + (size_t)F * BSELL_B * sizeof(int64_t) + BSELL_B * sizeof(int)};
}
// grid of the transpose copy: a workgroup per (block, column field)
static inline int bsell_copy_grid(int64_t nblk, int F, int num_cus) {
  const int64_t jobs = nblk * F;
  return (int)(jobs < (int64_t)num_cus * 12 ? jobs : (int64_t)num_cus * 12);
}

// ---- launch -------------------------------------------------------------------------------------------------------------------------------
// Workgroups at most: they write one partial sum each; the two parts of a split SpMV share one partial-sum array (max_partials: MFEM_MAX_PARTIALS).
static inline int sell_grid_cap(int num_cus, const SellKnobs& K, int max_partials, int part) {
  int cap = num_cus * K.wg_per_cu;
  if (cap > max_partials) cap = max_partials;
  return part != 0 ? cap / 2 : cap;
}
// blocks of part 0 (all), 1 (the leading blocks, whose rows read no ghost column), 2 (the rest: mfem_spmv_halo)
struct SellRange {
  int64_t lo, hi;
};
static inline SellRange sell_part_range(int part, int64_t nb_int, int64_t nblk) { return {part == 2 ? nb_int : 0, part == 1 ? nb_int : nblk}; }
// the instantiation k_spmv_sell<U> a knob value gets
static inline int sell_unroll_resolved(const SellKnobs& K) {
  switch (K.unroll) {
    case 4: case 8: case 9: case 10: case 15: return K.unroll;
    default: return 5;
  }
}
// ... and k_spmv_bsell<F, U> (hex-20 elasticity 96^3, one box, F = 3: 1 node slot in flight 2.98 ms, 2: 2.89, 3: 2.80)
struct BsellFU {
  int F, U;
};
static inline BsellFU bsell_fu_resolved(int F, const SellKnobs& K) {
  if (F == 3) return {3, K.per_u == 1 ? 2 : K.per_u == 2 ? 4 : K.per_u == 3 ? 1 : 3};
  if (F == 2) return {2, 4};
  return {4, 2};
}
static inline int sell_xcd_flag(const SellKnobs& K, int grid) { return (K.xcd && (grid & 7) == 0) ? 1 : 0; }  // (eight XCDs share the grid evenly)
// the periodic word of k_spmv_sell: fields | node slots in flight << 4; 0 = field-periodic blocks read their whole column stream
static inline int sell_periodic_word(const SellKnobs& K, int fields) { return K.periodic ? (fields | (K.per_u << 4)) : 0; }
