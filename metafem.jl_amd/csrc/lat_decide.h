// The host decisions of solver layout modes 4 and 5 -- the symmetric lattice tiles of the hex-27 matrix (spmv_lat27.hip, spmv_lat27_gather.hip) and
// of the F-field 27-point matrix (spmv_lat8.hip): the knob words, which patterns are taken, the lattice read off row 0 of a pattern without a hint,
// the geometry the kernels receive, what the copies hold and move, how a slab's launch is split, the gather grid and the symmetry gate -- and the
// record of what a bind left (mfem_csr_s::lat27, ::lat8).  The plans, binds, launches, the accounting and the debug entries all ask here.  No HIP, no
// context: tools/host_check_lat_decide.cpp walks every branch on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "spmv_lat_tables.h"

// mode 4: tiles of 8 x 8 x 32 lattice points (one y block of L27_CELLS cells each), stored as units of 4 x 4 x 8 points (four lanes per row) or as
// cubes of 8 x 8 x 8 points (lane = row, phase-major: the deterministic form)
#define L27_TI 8
#define L27_TJ 8
#define L27_TK 32
#define L27_SJ (L27_TJ + 4)
#define L27_SK (L27_TK + 4)
#define L27_CELLS ((L27_TI + 2) * L27_SJ * L27_SK)  // 4320
#define L27_UNIT_D 4352                             // doubles per unit: 64 lanes x 68 steps
#define L27D_CUBE_D (L27D_CUBE_STEPS * 64)          // doubles per cube
// mode 5: tiles of 8 x 8 x 16 nodes (F blocks of L8_FC cells), stored as pairs of i-stacked units of 4 x 4 x 4 nodes
#define L8_TI 8
#define L8_TJ 8
#define L8_TK 16
#define L8_SJ (L8_TJ + 2)
#define L8_SK (L8_TK + 2)
#define L8_PI (L8_SJ * L8_SK)        // 180
#define L8_FC ((L8_TI + 1) * L8_PI)  // cells per field: 1620

// ---- knob words -----------------------------------------------------------------------------------------------------------------------------
// mfem_debug_set_lat27
struct Lat27Knobs {
  bool enable;         // bit 0: the layout on / off
  bool gather_staged;  // bit 1 CLEAR: pass 2 by k_lat27_gather_st (set: k_lat27_gather -- masked blocks, a round trip per covering block)
  bool cg_fused;       // bit 2 CLEAR: CG iterations as pass 1 + k_lat27_gather_cg (set: SpMV (pass 1 + pass 2) + k_cg_update)
  bool det;            // bit 3 CLEAR: pass 1 lane = row, phase-major (set: the four-lanes-per-row kernel, not bitwise reproducible)
};
#define LAT27_WORD_DEFAULT 1
static inline Lat27Knobs lat27_knobs_decode(int word) { return {(word & 1) != 0, !(word & 2), !(word & 4), !(word & 8)}; }
// mfem_debug_set_lat8
struct Lat8Knobs {
  bool enable;                // bit 0
  bool one_field_everywhere;  // bit 1: the query / diagnostic SpMV entry also report and take mode 5 for ONE field
  bool gather_staged;         // bit 2: pass 2 by k_lat8_gather_st (measured on C3, tools/gather_ab.py: 1.6 % SLOWER per solve than k_lat8_gather -- its two
                              // barriers and the LDS round trip cost more than the round trips it saves on these small tiles; the hex-27 tiles gain 1 %)
};
#define LAT8_WORD_DEFAULT 1
static inline Lat8Knobs lat8_knobs_decode(int word) { return {(word & 1) != 0, (word & 2) != 0, (word & 4) != 0}; }
// One field: cg! keeps the bitwise patch sweep of mode 2 (it moves the same bytes); the solvers that work on A D^-1 (idrs!, bicgstabl_GS!, cgs2!) cannot
// use that sweep -- the scaled copy is not symmetric -- and take the tiles.  The layout query and the diagnostic SpMV entry answer for cg!.
static inline bool lat8_for_method(int fields, bool is_cg, const Lat8Knobs& K) { return fields != 1 || !is_cg || K.one_field_everywhere; }

// ---- eligibility ----------------------------------------------------------------------------------------------------------------------------
// what the decisions know of a pattern
struct LatShape {
  int64_t n, ncols;
  int max_row_nnz;
  int lat_m0, lat_m1, lat_m2, lat_fields, lat_plo, lat_gw;  // the lattice hint (mfem_csr_s; 0 = not given)
  int64_t min_rows;  // below: launch-bound sizes stay on the CSR tile kernel (mfem_debug_set_layout_min_rows: its hex-27 / its diagonal-slotted value)
};

struct Lat27Geom {
  int m0, m1, m2;     // OWNED lattice points per direction (m0 = owned planes of a slab; m1, m2 odd)
  int nui, nuj, nuk;  // units of 4 x 4 x 8 points
  int nti, ntj, ntk;  // tiles of 8 x 8 x 32 points
  int64_t n;          // m0 * m1 * m2 owned rows
  // slab: the owned planes are [plo, plo + m0) (plo even: slabs are cut on element boundaries) of a lattice of mg planes; x carries, behind the n
  // owned entries, a low and a high block of gw = 2 ghost planes (brick_xindex); plo = 0, mg = m0 for a whole brick
  int plo, mg, gw;
};
static inline Lat27Geom lat27_geom(const LatShape& S) {
  Lat27Geom G{};
  G.m1 = S.lat_m1;
  G.m2 = S.lat_m2;
  G.n = S.n;
  G.m0 = (int)(S.n / ((int64_t)S.lat_m1 * S.lat_m2));
  G.plo = S.lat_plo;
  G.mg = S.lat_m0 > 0 ? S.lat_m0 : G.m0;
  G.gw = 2;
  G.nui = (G.m0 + 3) / 4;
  G.nuj = (G.m1 + 3) / 4;
  G.nuk = (G.m2 + 7) / 8;
  G.nti = (G.m0 + L27_TI - 1) / L27_TI;
  G.ntj = (G.m1 + L27_TJ - 1) / L27_TJ;
  G.ntk = (G.m2 + L27_TK - 1) / L27_TK;
  return G;
}
struct Lat8Geom {
  int m0, m1, m2;     // OWNED nodes per direction (m0 = owned lattice planes of a slab)
  int nui, nuj, nuk;  // units of 4 x 4 x 4 nodes
  int nti, ntj, ntk;  // tiles of 8 x 8 x 16 nodes
  int64_t N;          // m0 * m1 * m2 owned nodes
  // slab: the owned planes are [plo, plo + m0) of a lattice of mg planes; x carries, behind the F N owned entries, per field a low and a high
  // block of gw ghost planes (brick_xindex); plo = 0, mg = m0 for a whole brick
  int plo, mg, gw, F;
};
static inline Lat8Geom lat8_geom(const LatShape& S) {
  Lat8Geom G{};
  G.F = S.lat_fields;
  G.m1 = S.lat_m1;
  G.m2 = S.lat_m2;
  G.N = S.n / G.F;
  G.m0 = (int)(G.N / ((int64_t)S.lat_m1 * S.lat_m2));
  G.plo = S.lat_plo;
  G.mg = S.lat_m0 > 0 ? S.lat_m0 : G.m0;
  G.gw = S.lat_gw > 0 ? S.lat_gw : 1;
  G.nui = (G.m0 + 3) / 4;
  G.nuj = (G.m1 + 3) / 4;
  G.nuk = (G.m2 + 3) / 4;
  G.nti = (G.m0 + L8_TI - 1) / L8_TI;
  G.ntj = (G.m1 + L8_TJ - 1) / L8_TJ;
  G.ntk = (G.m2 + L8_TK - 1) / L8_TK;
  return G;
}
static inline int64_t lat27_tiles(const Lat27Geom& G) { return (int64_t)G.nti * G.ntj * G.ntk; }
static inline int64_t lat8_tiles(const Lat8Geom& G) { return (int64_t)G.nti * G.ntj * G.ntk; }

// The value LatTiles::state gets before the entry-by-entry check of the pattern: 0 = too few rows (not inspected: ask again when the threshold
// changes), -1 = not the lattice this layout stores, 1 = go on and verify every entry.
// Mode 4: one field, odd point counts (whole order-2 elements) in every direction.
static inline int lat27_eligible(const LatShape& S) {
  if (S.n < S.min_rows) return 0;
  if (S.lat_fields != 1 || S.lat_m1 < 3 || S.lat_m2 < 3 || !(S.lat_m1 & 1) || !(S.lat_m2 & 1)) return -1;
  const int64_t PL = (int64_t)S.lat_m1 * S.lat_m2;
  if (S.n % PL != 0) return -1;
  const int64_t m0 = S.n / PL;
  if (m0 < 1 || m0 > (1 << 20) || S.max_row_nnz > 125) return -1;
  if (S.ncols > S.n) {  // slab pattern (ghost columns): the hint must place the owned planes in the lattice (on element boundaries) and describe the ghost blocks
    if (S.lat_m0 < 3 || !(S.lat_m0 & 1) || S.lat_gw != 2 || S.lat_plo < 0 || (S.lat_plo & 1) || S.lat_plo + m0 > S.lat_m0 || S.ncols != S.n + 4 * PL)
      return -1;
  } else {
    if (m0 < 3 || !(m0 & 1)) return -1;
    if (S.lat_m0 > 0 && (S.lat_m0 != m0 || S.lat_plo != 0)) return -1;
  }
  {  // cheap refusal before the entry-by-entry check: the longest row of the stencil is known from the lattice sizes (a hex-8 lattice with odd point
     // counts carries the same hint: 27 against 125)
    const int64_t mg = S.lat_m0 > 0 ? S.lat_m0 : m0;
    auto w = [](int64_t m) { return m >= 5 ? 5 : 3; };
    if (S.max_row_nnz != w(mg) * w(S.lat_m1) * w(S.lat_m2)) return -1;
  }
  if (lat27_tiles(lat27_geom(S)) >= ((int64_t)1 << 28)) return -1;
  return 1;
}
// Mode 5: F = 1..3 fields, field-major rows.
static inline int lat8_eligible(const LatShape& S) {
  if (S.n < S.min_rows) return 0;
  const int F = S.lat_fields;
  if (F < 1 || F > 3 || S.lat_m1 < 2 || S.lat_m2 < 2 || S.n % F != 0) return -1;
  const int64_t PL = (int64_t)S.lat_m1 * S.lat_m2, N = S.n / F;
  if (N % PL != 0) return -1;
  const int64_t m0 = N / PL;
  if (m0 < 1 || m0 > (1 << 20) || S.max_row_nnz > 27 * F) return -1;
  if (S.ncols > S.n) {  // slab pattern (ghost columns): the hint must say where the owned planes sit in the lattice and how the ghost blocks are laid out
    if (S.lat_m0 < m0 || S.lat_gw != 1 || S.lat_plo < 0 || S.lat_plo + m0 > S.lat_m0 || S.ncols != S.n + 2 * F * PL) return -1;
  } else if (S.lat_m0 > 0 && (S.lat_m0 != m0 || S.lat_plo != 0)) {
    return -1;
  }
  {  // cheap refusal before the entry-by-entry check: the longest row of the stencil is known from the lattice sizes
    const int64_t mg = S.lat_m0 > 0 ? S.lat_m0 : m0;
    auto w = [](int64_t m) { return m >= 3 ? 3 : (int)m; };
    if (S.max_row_nnz != F * w(mg) * w(S.lat_m1) * w(S.lat_m2)) return -1;
  }
  if (lat8_tiles(lat8_geom(S)) >= ((int64_t)1 << 28)) return -1;
  return 1;
}
// does a verified pattern's copy serve the products (mfem_lat27_bytes / mfem_lat8_bytes, and so the layout choice)?
static inline bool lat_serves(int state, bool enable, const LatShape& S) { return state == 1 && enable && S.n >= S.min_rows; }

// ---- the lattice of a pattern without a hint ---------------------------------------------------------------------------------------------------
// Proposed from the columns of row 0 -- the corner node of a lattice numbered plane by plane, line by line -- for the two stencils the tiles know.
// Only a proposal: the plans check every entry.
//   hex-27, one field:      row 0 = 27 columns {a PL + b m2 + c : a, b, c in 0..2}  ->  m2 = col[3], PL = col[9]
//   27-point, F = 1..3 fields: row 0 = F x 8 columns {g N + a PL + b m2 + c : a, b, c in 0..1}  ->  m2 = col[2], PL = col[4], N = col[8] (F > 1)
struct LatHint {
  int fields;  // 0: neither fits
  int m0, m1, m2, plo, gw;
};
static inline bool lattice_row0_len(int64_t len) { return len == 27 || len == 24 || len == 16 || len == 8; }  // (worth reading the columns at all?)
// c: the `len` columns of row 0, 0-based; n rows
static inline LatHint lattice_from_row0(int64_t len, const int32_t* c, int64_t n) {
  const LatHint none{};
  if (!lattice_row0_len(len) || c[0] != 0) return none;
  if (len == 27) {
    const int64_t m2 = c[3], PL = c[9];
    if (m2 < 3 || PL < 3 * m2 || PL % m2 != 0 || n % PL != 0) return none;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        for (int k = 0; k < 3; ++k)
          if (c[(a * 3 + b) * 3 + k] != a * PL + b * m2 + k) return none;
    return {1, (int32_t)(n / PL), (int32_t)(PL / m2), (int32_t)m2, 0, 2};
  }
  const int F = (int)(len / 8);
  if (n % F != 0) return none;
  const int64_t m2 = c[2], PL = c[4], N = F > 1 ? c[8] : n;
  if (m2 < 2 || PL < 2 * m2 || PL % m2 != 0 || N < 2 * PL || N % PL != 0 || n != F * N) return none;
  for (int g = 0; g < F; ++g)
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
        for (int k = 0; k < 2; ++k)
          if (c[g * 8 + (a * 2 + b) * 2 + k] != g * N + a * PL + b * m2 + k) return none;
  return {F, (int32_t)(N / PL), (int32_t)(PL / m2), (int32_t)m2, 0, 1};
}

// ---- sizes and accounting -------------------------------------------------------------------------------------------------------------------
// Mode 4.  Stored doubles of the deterministic (cubes) and of the four-lanes-per-row (units) form; the workspace is sized for whichever needs more:
// the knob may change between the plan and a bind.
static inline size_t lat27d_vals_doubles(const Lat27Geom& G) { return (size_t)G.nti * G.ntj * ((G.m2 + 7) / 8) * L27D_CUBE_D; }
static inline size_t lat27q_vals_doubles(const Lat27Geom& G) { return (size_t)G.nui * G.nuj * G.nuk * L27_UNIT_D; }
static inline size_t lat27_vals_doubles(const Lat27Geom& G) { const size_t a = lat27d_vals_doubles(G), b = lat27q_vals_doubles(G); return a > b ? a : b; }
static inline size_t lat27_read_doubles(const Lat27Geom& G, bool det) { return det ? lat27d_vals_doubles(G) : lat27q_vals_doubles(G); }  // what pass 1 streams
static inline size_t lat27_dump_doubles(const Lat27Geom& G) { return (size_t)G.nti * G.ntj * G.ntk * L27_CELLS; }
// the fused CG iteration: one dot-product partial per tile, right behind the dump
static inline int lat27_dot_partials(const Lat27Geom& G) { return G.nti * G.ntj * G.ntk; }
static inline size_t lat27_dot_offset(const Lat27Geom& G) { return lat27_dump_doubles(G); }  // (doubles from the dump's start)
// workspace of the layout: the stored entries, then the per-tile y blocks, then the partials
static inline size_t lat27_ws_bytes(const Lat27Geom& G) {
  return sizeof(double) * (lat27_vals_doubles(G) + lat27_dump_doubles(G) + (size_t)G.nti * G.ntj * G.ntk);
}
static inline int64_t lat27_entries(const Lat27Geom& G, bool det) { return (int64_t)lat27_read_doubles(G, det); }
// bytes one SpMV moves by design: the stored entries, x (and d) as the tiles stage it, the y blocks written and read again, y (the caller adds the
// remainder's)
static inline int64_t lat27_design_bytes(const Lat27Geom& G, bool det, bool scaled) {
  return (int64_t)lat27_read_doubles(G, det) * 8 + lat27_tiles(G) * L27_CELLS * 8 * (scaled ? 4 : 3) + G.n * 8;
}
// ... and pass 1 alone: the stored entries, x as the tiles stage it, the y blocks written
static inline int64_t lat27_pass1_bytes(const Lat27Geom& G, bool det) {
  return (int64_t)lat27_read_doubles(G, det) * 8 + (int64_t)G.nti * G.ntj * G.ntk * L27_CELLS * 8 * 2;
}
// Mode 5.  Doubles of one stored pair of i-stacked units (the stream of a wave of pass 1: 2 x nsteps steps of 64 lanes)
static inline int lat8_pair_doubles(int F) { return 2 * (F == 1 ? l8_nsteps(1) : F == 2 ? l8_nsteps(2) : l8_nsteps(3)) * 64; }
static inline size_t lat8_vals_doubles(const Lat8Geom& G) { return (size_t)((G.nui + 1) / 2) * G.nuj * G.nuk * lat8_pair_doubles(G.F); }
static inline size_t lat8_dump_doubles(const Lat8Geom& G) { return (size_t)G.nti * G.ntj * G.ntk * G.F * L8_FC; }
static inline size_t lat8_ws_bytes(const Lat8Geom& G) { return sizeof(double) * (lat8_vals_doubles(G) + lat8_dump_doubles(G)); }
static inline int64_t lat8_entries(const Lat8Geom& G) { return (int64_t)lat8_vals_doubles(G); }
static inline int64_t lat8_design_bytes(const Lat8Geom& G, bool scaled) {
  return (int64_t)lat8_vals_doubles(G) * 8 + lat8_tiles(G) * G.F * L8_FC * 8 * (scaled ? 4 : 3) + (int64_t)G.F * G.N * 8;
}

// ---- launch -----------------------------------------------------------------------------------------------------------------------------------
// First i-layer of lattice tiles (8 planes each, `gw` planes of upward reach) that stages a ghost plane of the upper neighbour: the layers below it
// are the interior part of a slab's split SpMV.  m0 = owned planes; without an upper neighbour every layer is interior.
static inline int mfem_lat_first_ghost_layer(int m0, int gw, int nti, bool has_upper) {
  if (!has_upper) return nti;
  int t = m0 - 7 - gw;  // a layer's staged planes end at 8 ti + 7 + gw
  t = t <= 0 ? 0 : (t + 7) / 8;
  return t < nti ? t : nti;
}
// Split SpMV of a slab (mfem_spmv_halo): part 1 = the tiles that stage no ghost plane of the upper neighbour (the i-layers below
// mfem_lat_first_ghost_layer: a contiguous prefix of the i-major tile list), launched beside the halo exchange; part 2 = the remaining layers and
// the gather pass (which reads the lower ghost planes for the first owned rows), launched after it.  part 0 = everything.  Pass 1 covers the tiles
// [tile0, tile0 + tcount) with `grid` workgroups: every XCD (blockIdx % 8) walks a contiguous eighth of them.
struct LatPart {
  int tile0, tcount, grid;
};
static inline LatPart lat_part_tiles(int m0, int gw, int nti, int ntj, int ntk, bool has_upper, int part) {
  const int ntiles = nti * ntj * ntk;
  const int tb = mfem_lat_first_ghost_layer(m0, gw, nti, has_upper) * ntj * ntk;
  const int tile0 = part == 2 ? tb : 0;
  const int tcount = part == 1 ? tb : ntiles - tile0;
  return {tile0, tcount, 8 * ((tcount + 7) / 8)};
}
// Persistent grid of pass 2 = what is resident (mfem_resident_per_cu: a workgroup more per CU than fits runs as a second round), one partial sum
// per workgroup at most, a tile per workgroup at least.
#define LAT_MAX_GATHER_GRID 4096  // (= MFEM_MAX_PARTIALS: common.h asserts it)
static inline int lat_gather_grid(int num_cus, int resident_per_cu, int ntiles) {
  int cap = num_cus * resident_per_cu;
  if (cap > LAT_MAX_GATHER_GRID) cap = LAT_MAX_GATHER_GRID;
  return ntiles < cap ? ntiles : cap;
}

// ---- the values of a solve ------------------------------------------------------------------------------------------------------------------
// The tiles store one triangle and mirror it: they are taken when the symmetry probe (sym_probe.hip) measures at most this, max over the rows of
// |y_tiles - y_csr| relative to the row's diagonal entry (NaN: no).  spmv_rem.hip repairs the rows above the same gate.
#define LAT_SYM_GATE 4e-13
static inline bool lat_accepts(double asym) { return asym <= LAT_SYM_GATE; }
// The fused CG iteration of mode 4 (krylov_cg.hip): pass 1 alone, then pass 2 inside the residual update.  One rank, no column scaling, no remainder.
static inline bool lat27_cg_fusable(const Lat27Knobs& K, bool bound, bool scaled, bool has_comm, bool rem_active) {
  return K.cg_fused && bound && !scaled && !has_comm && !rem_active;
}

// ---- what a bind left (mfem_csr_s::lat27, ::lat8) ---------------------------------------------------------------------------------------------
struct LatTiles {
  int state;          // 0 = not inspected, -1 = not the lattice stencil, 1 = the pattern is the stencil
  int det;            // mode 4: the bound copy is in the deterministic form (the launches follow the copy, not the knob)
  const double* src;  // the CSR-ordered values the bound copy mirrors (identity of the `vals` argument)
  const double* dsc;  // not owned: right Jacobi scaling applied to x while it is staged (nullptr: none)
  double* vals;       // not owned (solver workspace): the stored (diagonal + upper) entries; null = nothing bound
  double* dump;       // not owned (behind vals): one y block per tile
  double asym;        // what the symmetry probe of the last bind measured
  int scaled;         // the last bind carried a right Jacobi scaling (accounting)
};
