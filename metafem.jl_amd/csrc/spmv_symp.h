// Geometry of the wave-private patch sweep (spmv_sym.hip: k_spmv_symp; the layout copy k_dia_vals of spmv_dia.hip places the same entries): patch shape, LDS mirror tables and the per-step edge block.
// Host + device: tools/host_check_symp.cpp replays the table bookkeeping on the CPU (tests/test_host_checks.py).
#pragma once
#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define SP_L 4            // lattice lines per patch (8 x 16: 5 % fewer bytes -- rim and x halo -- but no faster: 0.885 against 0.878 ms per CG iteration at 256^3)
#define SP_W 32           // lattice points per line segment; a lane owns two neighbouring points: SP_L * SP_W / 2 = 64 lanes
#define SP_PW (SP_W / 2)  // lane pairs per line
#define SP_ROWS (SP_L * SP_W)
#define SP_XL (SP_L + 2)
#define SP_XC (SP_W + 2)  // staged x points per line: k0 - 1 .. k0 + SP_W
#define SP_XW (SP_W + 4)  // line stride of the x tile: lines stay 16-byte aligned
#define SP_XN (SP_XL * SP_XC)
#define SP_XU ((SP_XN + 63) / 64)  // x entries per lane and plane
#define SP_WG_PER_CU 7
// Mirror tables: one per lower slot s = (di, dj, dk), holding slot 26 - s of the SOURCE rows (row + offset), indexed by source
// cell (line lj + dj, column 2 pk + dk): lines of SP_W + 4 doubles, column c at index c + 2 (column -1 and column SP_W are halo cells), a
// halo line on the side the slot points to.  A halo cell cannot be mirrored (its source row belongs to another patch): it
// receives the referencing row's OWN slot-s entry from the step's edge block, so that the reads are the same two LDS loads for
// every lane and slot.
#define SP_LS (SP_W + 4)
// Bands: a wave's patch is B bands of SP_L lines each (B = 1: the patch above; B = 2: 8 x 32 points, swept per plane as two sub-steps of the same
// step body, band 0 first).  Tables, x ring and edge block cover all SP_L * B lines: the rows on the seam between two bands find their neighbours'
// entries in the tables like any interior row and own no edge entry.  Every function below takes the band count; B = 1 gives the macros' values.
#define SP_BMAX 2
__host__ __device__ constexpr int sp_dj(int s) { return (s / 3) % 3 - 1; }
__host__ __device__ constexpr int sp_dk(int s) { return s % 3 - 1; }
__host__ __device__ constexpr int sp_tsize(int s, int B = 1) { return (sp_dj(s) == 0 ? SP_L * B : SP_L * B + 1) * SP_LS; }
__host__ __device__ constexpr int sp_tbase(int s, int B = 1) {
  int b = 0;
  for (int t = 0; t < s; ++t) b += sp_tsize(t, B);
  return b;
}
__host__ __device__ constexpr int sp_adj(int s) { return sp_dj(s) == -1 ? 1 : 0; }  // table line of source line 0
__host__ __device__ constexpr int sp_tab(int B) { return sp_tbase(13, B); }  // 2196 doubles for B = 1, 4068 for B = 2
#define SP_TAB sp_tab(1)
// edge block of a step: for s = 0..12 the halo cells of table s -- the halo line (SP_W cells) if dj != 0, then the halo column
// (lines in ascending order) if dk != 0
__host__ __device__ constexpr int sp_ecnt(int s, int B = 1) {
  return (sp_dj(s) != 0 ? SP_W : 0) + (sp_dk(s) != 0 ? (sp_dj(s) != 0 ? SP_L * B - 1 : SP_L * B) : 0);
}
__host__ __device__ constexpr int sp_ebase(int s, int B = 1) {
  int b = 0;
  for (int t = 0; t < s; ++t) b += sp_ecnt(t, B);
  return b;
}
__host__ __device__ constexpr int sp_ne(int B) { return sp_ebase(13, B); }  // 318 for one band (210 for 8 x 16), 354 for two
__host__ __device__ constexpr int sp_eu(int B) { return (sp_ne(B) + 63) / 64; }  // edge entries per lane
__host__ __device__ constexpr int sp_epad(int B) { return 64 * sp_eu(B); }
#define SP_NE sp_ne(1)
#define SP_EU sp_eu(1)
#define SP_EPAD sp_epad(1)
// doubles per (plane, patch) in the patch-major copy, in two parts:
//   main: what every step reads -- per band the slots 13..26 (14 x SP_ROWS, band after band), then the edge block -- contiguous per step, steps [plane][patch]
//   low: per band the lower slots 0..12 (read where a run starts and by the symmetry check), behind all main parts
// The main part has a second form, DC = 1 (coded diagonal; k_symp_fill with the symmetric scaling of the scaled CG): slot 13 of the scaled matrix is
// a_ii * (t_i * t_i), t_i = 1 / sqrt|a_ii| -- 1.0 up to a few roundings, or -1.0 (the thermal K is negative definite) -- and is carried as one signed byte per
// row, bits(v) - bits(+-1.0): the unit is the bind's, +-1.0 with the sign of the first swept row's diagonal (sp_unit_bits).  Per band the 13
// slots 14..26, then the edge block, then the code block: SP_ROWS bytes per band (byte = row of the band, band after band; 128 B bytes keep the next
// step 16-byte aligned).  B = 2: 3744 instead of 3968 doubles per step.  DC = 0, the default, is the stored form.
// Behind all main and low parts lies the rim copy of a trimmed sweep (symp_trim_decide.h) and behind that, where k_symp_fill made the copy, ONE BYTE PER STEP
// [plane][patch], padded to whole doubles (symp_const_decide.h): 1 = every value of the step equals the bind's reference row's of the same slot, bit for bit.  The
// copy itself is complete either way -- the constant form (CS = 1) of the sweep does not read the main part, the edge block or the codes of a flagged step.
#define SP_ONE_BITS 0x3FF0000000000000ll  // bits(1.0)
#define SP_CODE_MAX 127                   // a diagonal further than this many ulps from the unit (the other sign, zero, non-finite) refuses the coded form
__host__ __device__ constexpr long long sp_unit_bits(int negative) { return negative ? (long long)(0xBFF0000000000000ull) : SP_ONE_BITS; }  // bits(-1.0) / bits(1.0)
__host__ __device__ constexpr int sp_nslots(int DC = 0) { return 14 - DC; }                // slots per band in the main part
__host__ __device__ constexpr int sp_cpad(int B, int DC = 0) { return DC ? B * SP_ROWS / 8 : 0; }  // doubles of the code block
__host__ __device__ constexpr int sp_eoff(int B, int DC = 0) { return sp_nslots(DC) * SP_ROWS * B; }  // the edge block's place in the main part
__host__ __device__ constexpr int sp_coff(int B, int DC = 0) { return sp_eoff(B, DC) + sp_epad(B); }  // the code block's (DC = 1)
__host__ __device__ constexpr int sp_main(int B, int DC = 0) { return sp_coff(B, DC) + sp_cpad(B, DC); }
__host__ __device__ constexpr int sp_low(int B) { return 13 * SP_ROWS * B; }
__host__ __device__ constexpr int sp_step(int B, int DC = 0) { return sp_main(B, DC) + sp_low(B); }
// code <-> double: IEEE ordering (of the magnitudes) is monotonic in the bits, so the code crosses the binade boundary at the unit like any other step; a
// value of the other sign lies 2^63 away
__host__ __device__ inline bool sp_diag_code(double v, int& code, long long unit = SP_ONE_BITS) {
  long long b = 0;
  __builtin_memcpy(&b, &v, 8);
  const long long d = (long long)((unsigned long long)b - (unsigned long long)unit);
  code = (int)(d < -SP_CODE_MAX ? -SP_CODE_MAX - 1 : d > SP_CODE_MAX ? SP_CODE_MAX + 1 : d);
  return d >= -SP_CODE_MAX && d <= SP_CODE_MAX;
}
__host__ __device__ inline double sp_diag_value(int code, long long unit = SP_ONE_BITS) {
  const long long b = unit + (long long)code;
  double v = 0.0;
  __builtin_memcpy(&v, &b, 8);
  return v;
}
#define SP_STEP sp_step(1)
#define SP_MAIN sp_main(1)
#define SP_LOW sp_low(1)
// staged x neighbourhood of a patch
__host__ __device__ constexpr int sp_xl(int B) { return SP_L * B + 2; }
__host__ __device__ constexpr int sp_xn(int B) { return sp_xl(B) * SP_XC; }
__host__ __device__ constexpr int sp_xu(int B) { return (sp_xn(B) + 63) / 64; }
// resident one-wave workgroups per CU: 22.8 KB of LDS each for one band, 41.2 KB for two
__host__ __device__ constexpr int sp_wg_per_cu(int B) { return B == 1 ? SP_WG_PER_CU : 3; }
// entry e of the edge block: lower slot s, the referencing row's (line, column) in the patch, the LDS cell of table s it fills
__host__ __device__ inline bool sp_edge(int e, int& s, int& line, int& col, int& cell, int B = 1) {
  if (e >= sp_ne(B)) return false;
  s = 0;
  while (e >= sp_ebase(s, B) + sp_ecnt(s, B)) ++s;
  int q = e - sp_ebase(s, B);
  const int dj = sp_dj(s), dk = sp_dk(s);
  int sl, sc;
  if (dj != 0 && q < SP_W) {
    sl = dj < 0 ? -1 : SP_L * B;
    sc = dk + q;
  } else {
    if (dj != 0) q -= SP_W;
    sl = dj > 0 ? q + 1 : q;
    sc = dk < 0 ? -1 : SP_W;
  }
  line = sl - dj;
  col = sc - dk;
  cell = sp_tbase(s, B) + (sl + sp_adj(s)) * SP_LS + sc + 2;
  return true;
}
// inverse of sp_edge for the row at (line, col) of its patch (line counted over all bands): the edge block entry that holds the row's own slot-s
// entry (s = 0..12), or -1 when the row's slot-s neighbour lies inside the patch.  A row owns at most one entry per slot: the halo line takes the corner cells.
__host__ __device__ constexpr int sp_edge_of(int s, int line, int col, int B = 1) {
  const int dj = sp_dj(s), dk = sp_dk(s);
  if (dj != 0 && line == (dj < 0 ? 0 : SP_L * B - 1)) return sp_ebase(s, B) + col;
  if (dk != 0 && col == (dk < 0 ? 0 : SP_W - 1)) {
    const int q = dj < 0 ? line - 1 : line;  // dj < 0: lines 1 .. L - 1; dj > 0: lines 0 .. L - 2; dj = 0: all lines
    return sp_ebase(s, B) + (dj != 0 ? SP_W : 0) + q;
  }
  return -1;
}
