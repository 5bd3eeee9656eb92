// The constant form of the patch sweep (spmv_sym.hip: k_spmv_symp_const<B, DC>, the sweep's body with CS = 1), decided once per bind: a patch step whose every matrix value
// equals, bit for bit, the value one reference row holds in the same slot is computed from the kernel's arguments -- no matrix load, no mirror table, no edge
// block.  Integer arithmetic alone, host + device, no HIP: tools/host_check_symp_const.cpp walks it on the CPU (tests/test_symp_const_decide.py).
//
// Where it applies: a constant-coefficient scalar operator on a uniform brick whose assembly gives bitwise identical rows.  That needs dyadic spacing
// (coordinates h * i and their differences exact), e.g. the unit cube at a power-of-two element count.  Otherwise no step is flagged and the bind keeps the
// stored form.
//
// k_symp_const_ref (spmv_dia.hip) forms the 27 values of the row at the centre of the swept region as the fill forms them; k_symp_fill compares every value it
// writes with the constant of its slot and leaves one byte per step [plane][patch] behind the rim copy: 1 = whole patch, every row full, all
// 27 x 64 B x 2 values (and, coded diagonal, the codes) match.  The count of flagged steps comes back with the fill's fingerprint (mfem_sym_verdict).
#pragma once
#include <stdint.h>

#include "spmv_symp.h"

// ---- the flag array: one byte per step, padded to whole doubles (it lies behind the rim copy in the layout's buffer; the sweep reads the aligned 32-bit
// word that holds a step's byte)
__host__ __device__ constexpr int64_t spc_flag_doubles(int64_t steps) { return (steps + 7) / 8; }

// ---- the gate: the bind takes the constant form when the flagged share of its steps reaches twice the break-even share c / (c + g), where
//   c = what an UNFLAGGED step costs more under CS = 1 than under CS = 0 (its flag, the branch, the restart behind a flagged step), and
//   g = what a FLAGGED step gains.
// Measured (profiles/r12_symp_const_ab_512.txt), per step of the B = 2 sweep, from the SpMV time per launch:
//   c: bench.py --n 511 (no flagged step), CS = 1 forced by bit 5 of the "ell" knob against the default          -> SPC_COST_PS picoseconds per step
//   g: bench.py at 512^3 (84.8 % flagged), the default against the stored form forced by bit 4                   -> SPC_GAIN_PS picoseconds per flagged step
//   511: 3.799 / 3.800 ms forced against 3.417 / 3.414 ms, 1024 x 508 steps: c = 736 ps.  512^3: 2.401 ms against 3.547 ms, 441 812 flagged steps: g = 2594 ps.
//   Gate = 2 x 736 / (736 + 2594) = 44 % of the steps (512^3: 84.8 %, 256^3: 72.7 %).  The cost is the CS = 1 instantiation's register allocation (170
//   against 138 AGPRs for B = 2), which every unflagged step pays.
#define SPC_COST_PS 736
#define SPC_GAIN_PS 2594
__host__ __device__ constexpr int64_t spc_cost_ps() { return SPC_COST_PS > 0 ? SPC_COST_PS : 0; }  // (a measured cost inside the noise, or below zero, counts as none)
__host__ __device__ constexpr bool spc_gate(int64_t flagged, int64_t steps) {
  // flagged / steps >= 2 c / (c + g), and never without a flagged step
  return flagged > 0 && steps > 0 && flagged * (spc_cost_ps() + SPC_GAIN_PS) >= 2 * spc_cost_ps() * steps;
}
// THE decision.  usable: the copy was filled by k_symp_fill (no flags otherwise) and its flagged steps, if any, may take the sweep's path for them (dia_bind: the
// symmetry verdict is the fingerprint's, the reference row is its own mirror image); ref_valid: the reference row had its 27 entries (and, coded diagonal, a
// code); force_stored / force_const: bits 4 / 5 of the "ell" knob
__host__ __device__ constexpr int spc_form(bool usable, bool ref_valid, int64_t flagged, int64_t steps, bool force_stored, bool force_const) {
  return !usable || force_stored ? 0 : force_const ? 1 : (ref_valid && spc_gate(flagged, steps)) ? 1 : 0;
}

// ---- runs and waves.  Round rk gives the W waves of an XCD its runs [W rk, W rk + W), wave jw the (jw + rot rk) % W-th of them.  With W a multiple of the patch
// columns NPk an unrotated wave meets the same patch column in every round (512^3: W = 96, NPk = 16, 4 rounds), and the waves of the first and last column,
// whose steps are never flagged, would sweep four slow runs where the others sweep four fast ones; a quarter of the columns per round spreads them.  The runs
// of a round are the same set either way (the XCD's patches still advance through the planes together).
__host__ __device__ constexpr int spc_rot(int NPk) { return NPk / 4; }
__host__ __device__ constexpr int spc_run(int W, int jw, int rk, int rot) { return W * rk + (jw + rot * rk) % W; }

// ---- accounting: matrix entries (8 B) a flagged step no longer reads -- per lane pair the 14 upper slots of two rows (coded diagonal: 13 slots and the
// codes, counted by the caller), and the edge block; all patches of a flagged step are whole: 64 B lane pairs
__host__ __device__ constexpr int64_t spc_saved_entries(int B) { return 28 * 64 * (int64_t)B + sp_ne(B); }
__host__ __device__ constexpr int64_t spc_saved_codes(int B) { return 2 * 64 * (int64_t)B; }  // diagonal entries of a step (stored: doubles; coded: bytes)
// flagged steps of a lattice by geometry: whole patches whose lines lie in [2, m1 - 3] and points in [2, m2 - 3] (all 27 neighbours of every row interior
// nodes: on a lattice of n + 1 points per direction, 2 <= i <= n - 2), times the swept planes in the same range -- the scaled copy S^-1 A S^-1 of a
// constant-coefficient operator with boundary terms; its unscaled copy is constant one node further out
__host__ __device__ inline int64_t spc_expected(int planes, int m1, int m2, int p0, int p1, int ms1, int ms2, int B) {
  const int L = SP_L * B;
  int64_t pr = 0, pc = 0, pp = 0;
  for (int j0 = 0; j0 + L <= ms1; j0 += L) pr += j0 >= 2 && j0 + L - 1 <= m1 - 3;
  for (int k0 = 0; k0 + SP_W <= ms2; k0 += SP_W) pc += k0 >= 2 && k0 + SP_W - 1 <= m2 - 3;
  for (int p = p0; p < p1; ++p) pp += p >= 2 && p <= planes - 3;
  return pr * pc * pp;
}
