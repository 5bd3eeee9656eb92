// Which part of a lattice plane the patch sweep (spmv_sym.hip: k_spmv_symp) sweeps, decided once per bind, and the enumeration of the rows it leaves out.
// Integer arithmetic alone (but for the filling ratio of spt_nseg, the sweep's run-count rule as it was), host + device, no HIP: tools/host_check_symp_trim.cpp walks it on the CPU (tests/test_symp_trim_decide.py).
//
// A plane of m1 lines x m2 points is cut into patches of SP_L * B lines x SP_W points.  The usual meshes have 32 q elements per side, so a line has
// 32 q + 1 points and a plane 8 q + 1 lines: the last patch column holds ONE valid column and the last patch row ONE valid line (512^3: 81 of 1105 patches per
// plane).  Such a straggler step still reads its whole edge block and x neighbourhood, passes both barriers and occupies a wave slot.  Trimmed, the sweep
// covers whole patches only -- ms1 <= m1 lines, ms2 <= m2 points -- and the RIM rows (k >= ms2 or j >= ms1) are computed row by row from a compact copy of
// their 27 slots (spmv_dia.hip: k_symp_rim_fill; spmv_sym.hip: symp_rim_unit).
//
// The byte model behind the two limits (doubles read per plane step, B = 2):
//   a straggler step   edge block 354 + x neighbourhood 340 + 26 per valid lane pair (13 or 14 upper slots of two rows; the codes)
//   a rim row          27 slots + its x sectors (9 sectors of 4 doubles serve the 27 products of a line-rim row, up to 27 those of a column-rim row) + one y
//   column remainder of c points (8 lines):  694 + 26 * 8 * ceil(c / 2)  against  8 c * (27 + 27 + 1):  c = 1: 902 / 440,  c = 2: 902 / 880,  c = 3: 1110 / 1320
//   line remainder of l lines (32 points):   694 + 26 * 16 l             against  32 l * (27 + 9 + 1):  l = 1: 1110 / 1184, l = 2: 1526 / 2368
// so the forms break even near 2 points and 1 line (the line remainder of one line also frees a wave slot and a whole patch row of runs: it is trimmed).
// Widen a limit only with a measurement written beside it.
#pragma once
#include <stdint.h>

#include "spmv_symp.h"

#define SPT_MAX_POINTS 2  // a remainder of at most this many points per line (one lane pair) leaves the sweep
#define SPT_MAX_LINES 1   // a remainder of at most this many lines per plane leaves the sweep
#define SPT_UNIT 64       // rim rows per unit of the compact copy: slot-major inside a unit, 27 x 64 doubles -- every slot of a unit is one 512-byte piece
#define SPT_UNIT_DOUBLES (27 * SPT_UNIT)

// swept extent of a direction of m points cut into patches of `patch`: whole patches when the remainder is narrow, never zero patches
__host__ __device__ constexpr int spt_extent(int m, int patch, int max_rem) {
  return (m % patch >= 1 && m % patch <= max_rem && m - m % patch >= patch) ? m - m % patch : m;
}
__host__ __device__ constexpr int spt_ms1(int m1, int B, bool trim = true) { return trim ? spt_extent(m1, SP_L * B, SPT_MAX_LINES) : m1; }
__host__ __device__ constexpr int spt_ms2(int m2, bool trim = true) { return trim ? spt_extent(m2, SP_W, SPT_MAX_POINTS) : m2; }
// patch rows / patch columns of the swept part
__host__ __device__ constexpr int spt_rows(int ms1, int B) { return (ms1 + SP_L * B - 1) / (SP_L * B); }
__host__ __device__ constexpr int spt_cols(int ms2) { return (ms2 + SP_W - 1) / SP_W; }

// The rim of a plane, enumerated: first the column rim (k >= ms2, lines 0 .. ms1 - 1; the rim points of a line are neighbours, consecutive lines adjacent),
// then the line rim (j >= ms1, all k).  The corner rows (j >= ms1 and k >= ms2) belong to the line rim only.
__host__ __device__ constexpr int spt_rim_cols(int ms1, int m2, int ms2) { return ms1 * (m2 - ms2); }                       // rows of the column rim
__host__ __device__ constexpr int spt_rim(int m1, int m2, int ms1, int ms2) { return ms1 * (m2 - ms2) + (m1 - ms1) * m2; }  // rim rows per plane
// (j, k) -> index in the plane's rim, -1 for a swept row
__host__ __device__ constexpr int spt_rim_index(int j, int k, int m2, int ms1, int ms2) {
  return j >= ms1 ? spt_rim_cols(ms1, m2, ms2) + (j - ms1) * m2 + k : k >= ms2 ? j * (m2 - ms2) + (k - ms2) : -1;
}
// index in the plane's rim -> (j, k)
__host__ __device__ inline void spt_rim_row(int idx, int m2, int ms1, int ms2, int& j, int& k) {
  const int nc = spt_rim_cols(ms1, m2, ms2);
  if (idx < nc) {
    const int w = m2 - ms2;  // (> 0 here: nc > 0)
    j = idx / w;
    k = ms2 + idx % w;
  } else {
    j = ms1 + (idx - nc) / m2;
    k = (idx - nc) % m2;
  }
}
__host__ __device__ constexpr int64_t spt_units(int64_t rim_rows) { return (rim_rows + SPT_UNIT - 1) / SPT_UNIT; }

// Runs per patch of the sweep: the smallest count that fills >= 90 % of the resident one-wave workgroups (`slots`) in whole rounds, else the best filling;
// a run's first step has no history, so runs stay >= 16 planes long.  (512^3, B = 2, 768 slots: 1105 patches -> 2 runs, three rounds at 0.96;
// the 1024 whole patches -> 3 runs, four rounds filled exactly.)
__host__ __device__ inline int spt_nseg(int64_t NP, int64_t slots, int nplanes) {
  int best = 1;
  double best_eff = 0.0;
  for (int ns = 1; ns <= (nplanes / 16 > 1 ? nplanes / 16 : 1) && ns <= 64; ++ns) {
    const int64_t R = NP * ns, rounds = (R + slots - 1) / slots;
    const double eff = (double)R / (double)(rounds * slots);
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = ns;
    }
    if (eff >= 0.9) {
      best = ns;
      break;
    }
  }
  return best;
}
