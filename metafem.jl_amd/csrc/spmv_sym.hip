// The two symmetric sweeps on the diagonal-slotted copy (spmv_dia.hip makes the copies; which kernel a copy gets: mfem_dia_kernel_wanted,
// spmv_ell.hip): the workgroup-tile sweep k_spmv_sym27 and the wave-private patch sweep k_spmv_symp, each with the check of the pairs it mirrors.
// One file: the patch sweep's call of dia_rows with a row range to skip keeps that code general, and k_spmv_sym27's instructions as they were.
#include "blas1.h"
#include "spmv_ell.h"

// ---------------------------------------------------------------------------------------------------------------
// Symmetric sweep kernel for the 27-point lattice stencil (offsets di PL + dj m2 + dk).  For a symmetric matrix the entry of
// row r on a lower diagonal -o equals the entry of row r - o on the upper diagonal +o.  A workgroup owns an in-plane tile
// of 512 rows and sweeps it through consecutive lattice planes (chunks c, c + S, c + 2 S, ...): the nine upper diagonals
// that point to the next plane are kept in LDS when they are loaded, and the next plane's rows read their nine
// previous-plane (lower) diagonals from there instead of from HBM.  Same products, same summation order as the plain
// diagonal-slotted kernel: the result is bitwise the same whenever the matrix is bitwise symmetric (checked at bind time).
// ---------------------------------------------------------------------------------------------------------------
#define SYM_ROWS 512                 // rows of a tile = 4 blocks of 128 (768 rows / 384 threads / 2 workgroups per CU mirror more but run at 1.07 instead of 0.93 ms per CG iteration)
#define SYM_THREADS (SYM_ROWS / 2)
#define SYM_WG_PER_CU 3              // 53 KB of LDS per workgroup
__global__ __launch_bounds__(SYM_THREADS) void k_spmv_sym27(int64_t n, int64_t npad, int K, const DiaOffsets* __restrict__ Op,
                                                             const int32_t* __restrict__ flags, const int32_t* __restrict__ cols,
                                                             const double* __restrict__ vals, const double* __restrict__ x,
                                                             double* __restrict__ y, double alpha, double beta,
                                                             const double* __restrict__ dotw, double* __restrict__ partials,
                                                             const int32_t* __restrict__ done_flag, int64_t c0, int64_t c1, int S, int nsteps, int cls, int gs,
                                                             int part) {  // 0: sweep + the chunks outside it; 1: sweep only; 2: only the chunks outside the sweep (every row that reads a ghost column of a slab is among them)
  __shared__ __attribute__((aligned(16))) double hist[9][SYM_ROWS];  // diagonals 18..26 (into the next plane) of the previous chunk
  __shared__ __attribute__((aligned(16))) double exch[4][SYM_ROWS];  // diagonals 14..17 (+z, +y) of this chunk
  __shared__ double red[16];
  if (done_flag && done_flag[0]) return;
  const int32_t* off = Op->off[cls];
  const int tid = threadIdx.x;
  double dot_acc = 0.0;
  // gs workgroups over S tiles: tile t is swept by nseg (+ 1 for the first gs % S tiles) workgroups, each taking a contiguous
  // range of the tile's nsteps plane steps
  const int tile = blockIdx.x % S, seg = blockIdx.x / S;
  const int nseg = gs / S + (tile < gs % S ? 1 : 0);
  const int seg_len = part == 2 ? 0 : (nsteps + nseg - 1) / nseg;
  bool have_hist = false;
  e_d2 up_next[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
  {
    const int64_t chunk = c0 + tile + (int64_t)S * ((int64_t)seg * seg_len);
    if (part != 2 && seg * seg_len < nsteps && chunk < c1) {
      const double* v = vals + ell_base(chunk * SYM_ROWS + 2 * tid, K);
#pragma unroll
      for (int u = 0; u < 4; ++u) up_next[u] = SYM_LD(reinterpret_cast<const e_d2*>(v + (14 + u) * ELL_B));
    }
  }
  for (int it = 0; it < seg_len; ++it) {
    const int step = seg * seg_len + it;
    const int64_t chunk = c0 + tile + (int64_t)S * step;
    if (step >= nsteps || chunk >= c1) break;  // workgroup-uniform
    const int64_t r = chunk * SYM_ROWS + 2 * tid;
    const double* v = vals + ell_base(r, K);
    e_d2 acc = {0.0, 0.0};
    // ---- the lane's own +z / +y diagonals first: the rows behind it in this chunk read them as their -z / -y diagonals
    e_d2 up[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      up[u] = up_next[u];  // requested during the previous chunk (or before the loop)
      *reinterpret_cast<e_d2*>(&exch[u][2 * tid]) = up[u];
    }
    __syncthreads();  // exch complete; also: every wave has finished writing the previous chunk's history
    // a slot's value pair, mirrored from LDS (row `lp` of table `tab`) when both source rows are in it, else from the row itself
    auto slot = [&](int s, const double* tab, int lp, bool ok) -> e_d2 {
      e_d2 w;
      if (ok && lp >= 0 && lp + 1 < SYM_ROWS) {
        w.x = tab[lp];
        w.y = tab[lp + 1];
      } else {
        w = SYM_LD(reinterpret_cast<const e_d2*>(v + s * ELL_B));
      }
      return w;
    };
#define SYM_RUN(va, vb, vc, s0)                                          \
  {                                                                      \
    const u_d2* xp = reinterpret_cast<const u_d2*>(x + r + off[s0]);     \
    const u_d2 xa = xp[0], xb = xp[1];                                   \
    acc.x += va.x != 0.0 ? va.x * xa.x : 0.0;                            \
    acc.y += va.y != 0.0 ? va.y * xa.y : 0.0;                            \
    acc.x += vb.x != 0.0 ? vb.x * xa.y : 0.0;                            \
    acc.y += vb.y != 0.0 ? vb.y * xb.x : 0.0;                            \
    acc.x += vc.x != 0.0 ? vc.x * xb.x : 0.0;                            \
    acc.y += vc.y != 0.0 ? vc.y * xb.y : 0.0;                            \
    if (s0 == 12) {                                                      \
      xself0 = xa.y;                                                     \
      xself1 = xb.x;                                                     \
    }                                                                    \
  }
    double xself0 = 0.0, xself1 = 0.0;
    // ---- the nine diagonals into the previous plane: entry (r, r + o) = entry (r + o, r) on diagonal 26 - s of row r + o,
    //      kept in `hist` if that row was in the previous chunk of this sweep
    const int lph = 2 * tid + S * SYM_ROWS;
#pragma unroll
    for (int s = 0; s < 9; s += 3) {
      const e_d2 va = slot(s, hist[8 - s], lph + off[s], have_hist);
      const e_d2 vb = slot(s + 1, hist[7 - s], lph + off[s + 1], have_hist);
      const e_d2 vc = slot(s + 2, hist[6 - s], lph + off[s + 2], have_hist);
      SYM_RUN(va, vb, vc, s);
    }
    {  // -y diagonals 9..11 <- +y diagonals 17..15 of the rows one lattice line behind, if those are in this chunk
      const e_d2 va = slot(9, exch[3], 2 * tid + off[9], true);
      const e_d2 vb = slot(10, exch[2], 2 * tid + off[10], true);
      const e_d2 vc = slot(11, exch[1], 2 * tid + off[11], true);
      SYM_RUN(va, vb, vc, 9);
    }
    {  // -z (12) <- +z (14) of the row before; main diagonal 13; +z from the registers
      e_d2 va;
      va.y = up[0].x;  // row r + 1: entry (r + 1, r) = entry (r, r + 1)
      if (tid > 0) va.x = exch[0][2 * tid - 1];
      else va.x = v[12 * ELL_B];
      const e_d2 vb = SYM_LD(reinterpret_cast<const e_d2*>(v + 13 * ELL_B));
      SYM_RUN(va, vb, up[0], 12);
    }
    SYM_RUN(up[1], up[2], up[3], 15);
    if (it + 1 < seg_len && step + 1 < nsteps && chunk + S < c1) {  // the next chunk's +z / +y diagonals: their latency hides behind
      const double* vn = vals + ell_base((chunk + S) * SYM_ROWS + 2 * tid, K);  // the rest of this chunk
#pragma unroll
      for (int u = 0; u < 4; ++u) up_next[u] = SYM_LD(reinterpret_cast<const e_d2*>(vn + (14 + u) * ELL_B));
    }
    __syncthreads();  // every wave is done reading hist and exch
    // ---- the nine diagonals into the next plane: they also go to LDS for the next chunk of the sweep
#pragma unroll
    for (int s = 18; s < 27; s += 3) {
      const e_d2 va = SYM_LD(reinterpret_cast<const e_d2*>(v + s * ELL_B));
      const e_d2 vb = SYM_LD(reinterpret_cast<const e_d2*>(v + (s + 1) * ELL_B));
      const e_d2 vc = SYM_LD(reinterpret_cast<const e_d2*>(v + (s + 2) * ELL_B));
      SYM_RUN(va, vb, vc, s);
      *reinterpret_cast<e_d2*>(&hist[s - 18][2 * tid]) = va;
      *reinterpret_cast<e_d2*>(&hist[s - 17][2 * tid]) = vb;
      *reinterpret_cast<e_d2*>(&hist[s - 16][2 * tid]) = vc;
    }
#undef SYM_RUN
    have_hist = true;
    double y0 = alpha * acc.x, y1 = alpha * acc.y;
    if (beta != 0.0) {
      y0 += beta * y[r];
      y1 += beta * y[r + 1];
    }
    y[r] = y0;
    y[r + 1] = y1;
    if (dotw) {
      if (dotw == x) dot_acc += y0 * xself0 + y1 * xself1;
      else dot_acc += y0 * dotw[r] + y1 * dotw[r + 1];
    }
  }
  // after its sweep every workgroup takes a share of the chunks outside the regular range (first / last lattice planes, ghost
  // planes of a slab) through the plain per-row code: no extra workgroups, no tail behind the sweeps
  if (part != 1) {
    const int64_t nchunks = (n + SYM_ROWS - 1) / SYM_ROWS;
    for (int64_t q = blockIdx.x;; q += gridDim.x) {
      const int64_t ch = q < c0 ? q : c1 + (q - c0);
      if (ch >= nchunks) break;
      const int64_t r = ch * SYM_ROWS + 2 * tid;
      if (r < n) dia_rows<2, 3, true>(r, n, npad, K, *Op, flags, cols, vals, x, y, alpha, beta, dotw, 0, dot_acc);
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// bad[0] |= 1 unless, for every row r of the regular chunk range and every lower diagonal s < 13 whose source row r + off[s]
// is in the range too, entry (r, s) equals entry (r + off[s], 26 - s) bitwise: exactly the substitutions k_spmv_sym27 makes
__global__ __launch_bounds__(MFEM_BLOCK) void k_sym27_check(int K, const DiaOffsets* __restrict__ Op, const double* __restrict__ vals,
                                                              int64_t row_lo, int64_t row_hi, int cls, int32_t* __restrict__ bad) {
  const int32_t* off = Op->off[cls];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int fail = 0;
  for (int64_t r = row_lo + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < row_hi; r += stride) {
    const double* v = vals + ell_base(r, K);
    for (int s = 0; s < 13; ++s) {
      const int64_t rs = r + off[s];
      if (rs < row_lo) continue;
      const double a = v[s * ELL_B], b = vals[ell_base(rs, K) + (26 - s) * ELL_B];
      if (__double_as_longlong(a) != __double_as_longlong(b) && !(a == 0.0 && b == 0.0)) fail = 1;
    }
  }
  if (fail) atomicOr(bad, 1);
}

// ---------------------------------------------------------------------------------------------------------------
// Symmetric sweep, wave-private patches (k_spmv_symp; default when the lattice form is recognised).  The workgroup-tile kernel
// above cuts a lattice plane into contiguous 512-row ranges: a lattice line longer than the tile (512^3: 513 points) leaves
// only the in-line diagonals mirrorable (31 %), and two workgroup barriers per chunk bound what three workgroups per CU can keep
// in flight.  Here a WAVE owns a (j, k) patch of 4 lattice lines x 32 points (lane <-> two neighbouring points of one line) and
// sweeps it through consecutive lattice planes with no workgroup barrier at all:
//   * the matrix values of the swept planes live in a patch-major copy, made when the solve binds its values (k_symp_fill, spmv_dia.hip; k_symp_bind): what every
//     step reads -- slots 13..26 and the edge block, 16.9 KB (coded diagonal, below: slots 14..26, the edge block and a byte per row) -- contiguous per step [plane][patch], the lower slots (read where a run
//     starts and by the symmetry check) behind;
//   * the upper diagonals of a step go to the wave's LDS block when they are loaded: +z / +y (slots 14..17) for the rows behind
//     them in this plane, the nine next-plane diagonals (18..26) for the same patch one plane on -- 10.5 of the 13 lower
//     diagonals of a row are mirrored from there whatever the line length (the rest: patch edges, read from the row's own slot);
//   * x is staged per plane: the (4 + 2) x (32 + 2) neighbourhood of the patch enters LDS once and serves the 27 products of three
//     consecutive steps -- four global loads per lane and step instead of eighteen gathers.
// Same products, same summation order as the plain diagonal-slotted kernel (v_mul_f64 + v_add_f64, no contraction): y is bitwise the
// same whenever the mirrored pairs are bitwise equal (MODE 1 checks exactly those pairs when the values are bound).
//   * A halo cell of a mirror table (its source row belongs to another patch) is filled from the step's EDGE BLOCK -- the own
//     slot-s entries of the rows at the patch rim, 318 doubles stored behind the step's 27 slots -- so that every lane reads every
//     lower slot with the same two LDS loads; a step reads 14 slots x 1 KB + 2.5 KB of edge block + 1.6 KB of x.
//   * Everything a step needs from memory is requested one step ahead into registers (its loads are in flight during the products
//     of the current step); two wave-level barriers per step order the LDS phases.
//   * Runs: a run = one patch through nplanes / nseg consecutive planes, one wave (one-wave workgroups, 7 per CU: 22.8 KB of LDS
//     each); a run's first step has no history and fills the previous-plane tables from the rows' own slots.  XCD c (workgroups
//     with blockIdx % 8 == c) sweeps a contiguous eighth of the patches, segment by segment, so neighbouring patches advance
//     through the planes together on one L2 (512^3: CG iteration 7.29 -> 6.66 ms against arbitrary equal cuts of the step list).  That is the IDENTITY
//     schedule, computed by the sweep itself (equal shares, round rk gives wave jw the run spc_run(W, jw, rk, rot) of the share's segment-major list); the
//     constant form may walk a table instead (Schedule, below).
//   * Partial sums of the fused dotw . y (p . Ap of CG) per RUN (sps_per_run, symp_sched_decide.h: when runs + workgroups + what the launches behind the
//     sweep need fit MFEM_MAX_PARTIALS; 512^3: 3072 + 768): at the end of a run the wave reduces its sum, lane 0 stores it at partials[patch * nseg + seg] and
//     the accumulator starts again at zero; the tail and rim units a workgroup takes after its runs keep one sum per workgroup behind the runs'.  A run's sum
//     is formed from zero in step order by whichever wave sweeps it, so the sums -- and with them alpha, every iterate and every statistic of a CG solve -- do
//     not depend on the assignment of runs to waves: a schedule is a pure speed decision and every schedule can be tested bit for bit against every other
//     (tests/test_gpu_symp_sched.py).  Where the runs do not fit (256^3: 3584 runs + 1792 workgroups) the sums stay per workgroup with the identity schedule.
//   * Bands (k_spmv_symp<MODE, B>; the count is decided per bind, mfem_symp_bands_wanted): with B = 2 a wave owns 8 lines x 32 points and runs them per
//     plane as two sub-steps of the same step body.  The nine halo lines of 32 cells dominate the edge block (9 W + 6 (L - 1) + 3 L entries), so per 256
//     rows it falls from 2 x 318 to 354 entries and the x neighbourhood from 2 x 6 x 34 to 10 x 34: 3968 instead of 4224 matrix doubles, at 41.2 KB of
//     LDS per wave (three resident one-wave workgroups per CU instead of seven).  Same lane <-> row mapping, products and slot order: y is the same bit for bit.
//   * Coded diagonal (k_spmv_symp<MODE, B, DC>, DC = 1; the form is decided per bind, mfem_symp_coded_wanted): the copy k_symp_fill makes for the scaled CG holds
//     S^-1 A S^-1, whose diagonal a_ii * (t_i * t_i), t_i = 1 / sqrt|a_ii|, is +-1.0 up to a few roundings (codes -4 .. +2 on the thermal matrices; the sign is
//     the matrix's: the thermal K is negative definite).  Slot 13 then costs 8 of the 15.5 matrix doubles-equivalents a row streams for almost no information, so
//     the main part carries 13 slots per band and, behind the edge block, one signed byte per row: bits(v) - bits(unit), unit = +-1.0 with the sign of the first
//     swept row's diagonal (spmv_symp.h; 3744 instead of 3968 doubles per step for B = 2).  A lane's two codes are one 2-byte load requested with its band's main
//     part a plane ahead and kept in one VGPR; the sweep rebuilds v = bits^-1(unit + code) and multiplies and adds it where the stored slot stood: y, the partial
//     sums and every iterate are the stored form's bit for bit (tests/test_gpu_symp_diag_code.py).  The fill raises a flag beside its fingerprint when a swept
//     row's diagonal has no code (the other sign, zero, non-finite: more than 127 ulps from the unit) and the bind refills in the stored form (dia_bind): only
//     the speed depends on the gate.  MODE 1 does not use the diagonal and only follows the layout; the tail rows, k_symp_bind and k_dia_vals keep the stored
//     form.  512^3: 3.62 -> 3.45 ms per launch, 256^3 (B = 1): 0.543 -> 0.518 ms (profiles/r09_symp_diag_code_ab_512.txt); 256 VGPRs + 138 AGPRs, no scratch,
//     41.2 KB of LDS as before.
//   * Whole patches only (the form is decided per bind, mfem_symp_trim_wanted; symp_trim_decide.h): a 513-point line leaves a 17th patch column with ONE valid column,
//     a 513-line plane a 65th patch row with one line -- 81 of 1105 patches per plane whose steps read a whole edge block and x neighbourhood, pass both barriers
//     and hold a wave slot.  Trimmed, Gm.NR x Gm.NPk patches cover lines [0, ms1) x points [0, ms2) and the rim rows are computed a lane per row from a compact
//     copy behind the patch-major one (symp_rim_unit: the sweep's waves take its 64-row units after their runs).  Nothing changes in the step body: lane
//     validity and the x offsets keep using m1, m2, and a halo cell next to the rim is filled from the edge block as before.  512^3: 1024 patches, 3 runs per
//     patch = 4 x 768 slots exactly; 3.46 -> 3.30 ms per launch, 256^3 0.518 -> 0.482 ms (profiles/r10_symp_trim_ab_512.txt).
//   * Constant steps (k_spmv_symp_const<B, DC>: the body below with CS = 1; the form is decided per bind, spc_form; symp_const_decide.h): on a uniform brick with dyadic spacing a
//     constant-coefficient operator is assembled to bitwise identical rows, and every row of the benchmark's scaled matrix whose 27 neighbours are interior nodes
//     holds the same 27 doubles.  k_symp_fill compares every value it forms with one reference row's (k_symp_const_ref), bit by bit, and flags the steps -- whole
//     patches -- in which all of them match: a byte per step behind the rim copy (512^3: 62 x 14 of the 1024 patches in each of the 509 swept planes, 84.8 %).  A
//     flagged step takes a path of its own: the next plane's x into the ring, then per band the 27 products with the reference row's values (27 doubles in the wave's LDS, read as broadcasts),
//     rounded, then added, in slot order -- no matrix load, no mirror table, no edge block, two barriers per step instead of two per band.  Its own slots are the
//     constants because the fill compared them, the mirrored ones because the bind's fingerprint found every pair among the swept rows bitwise equal and the
//     reference row is its own mirror image (dia_bind asks both): y, the partial sums and every iterate are the stored form's bit for bit
//     (tests/test_gpu_symp_const.py).  The tables are left stale, so an unflagged step behind a flagged one starts like a run; a run's flags come in one gathered
//     load per 63 steps.  What it showed: with the constants merely put where the loads had put their values (the registers of the unchanged step body) the launch
//     moved 5.3 instead of 18.45 GB and took as long as before, 3.33 against 3.35 ms -- a wave has its SIMD to itself and the step body's ~2500 instructions at
//     4 cycles each ARE the 4.9 us of a step; the time follows the instructions of a step, not its bytes.  The path above is ~450 instructions.  Runs are rotated
//     among an XCD's waves from round to round (spc_run) so that no wave keeps the first or last patch column, whose steps are never flagged.  512^3: 3.31 ->
//     2.60 ms per launch (profiles/r12_symp_const_ab_512.txt).  At n = 511, on a 0.3 m box, or with variable conductivity, no step is flagged: the bind keeps the
//     stored kernel and pays nothing.
//   * Schedule (k_spmv_symp_const alone; symp_sched_decide.h): with flagged steps the runs no longer cost the same -- per-run clocks of a probe build at 512^3: a
//     never-flagged run of 170 steps 830 us, a flagged one 408 us -- and four runs per wave whatever they cost leave the launch waiting for the waves that drew
//     two slow ones (2.51 ms against a mean load of 1.86 ms).  At bind time the host counts the flagged steps per run from the fill's flag bytes, cuts the XCDs'
//     contiguous patch ranges by cost and gives an XCD's runs, costliest first, each to the least loaded of its waves (mfem_symp_sched_bind); the table --
//     offset[grid + 1], run[nruns], behind the flags in the layout's buffer, rebuilt at every bind at the same place -- replaces the round loop by a walk over
//     the wave's list: its two offsets and up to 64 run ids per gathered load, read from their lanes (a scalar load per run would show its latency as the
//     flag's did).  The step body is untouched; the stored form, the identity mode of the "symp_sched" knob and a bind without per-run sums keep the
//     arithmetic form.  The walk is a template parameter (k_spmv_symp_const<B, DC, SCH>), instantiated apart: as a run-time branch it cost the launches that
//     never take it 0.2 - 0.4 % per step at 256^3 (74 instead of 39 spilled scalar registers for B = 2); apart, 0.15 %, inside the parent's spread.  512^3: model makespan 2.05 ms (whole runs allow 2.04), measured: profiles/r13_symp_sched_ab_512.txt.
//   * Rows outside the swept planes (first / last lattice plane, the planes next to the ghost planes of a slab) come from the slot-major
//     copy through the per-row code: the sweep's waves take them in 128-row units after their runs (unsplit SpMV: one launch, no tail);
//     in a split (multi-rank) SpMV they are the boundary part, a launch of their own (k_spmv_dia_outside) after the halo has arrived.
// Measured (CG iteration, tools/probe_sym.py): see mfem_sym_wanted().  What bounds it: 2.78 GB of fabric traffic per SpMV at 256^3
// (2.61 GB by the count above) in 0.59 ms = 4.7 TB/s; the time does not depend on the number of resident waves (2 .. 7 per CU), the
// y stores cost 0.1 ms of it (non-temporal 16-byte stores: -1.5 %), the edge block 0.07 ms, the x staging 0.03 ms
// (profiles/r02_symp_experiments.txt).
// ---------------------------------------------------------------------------------------------------------------

__constant__ int32_t c_sp_ecell[SP_BMAX][sp_epad(SP_BMAX)];  // per band count: edge block entry -> LDS cell of its mirror table (padding entries: a spare cell)
static int symp_upload_tables(int device) {  // __constant__ data is per device
  static bool done[64] = {};
  if (device >= 0 && device < 64 && done[device]) return MFEM_OK;
  int32_t h[SP_BMAX][sp_epad(SP_BMAX)];
  for (int B = 1; B <= SP_BMAX; ++B)
    for (int e = 0; e < sp_epad(SP_BMAX); ++e) {
      int s_, l_, c_, cell = 0;
      h[B - 1][e] = sp_edge(e, s_, l_, c_, cell, B) ? cell : sp_tab(B);
    }
  MFEM_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_sp_ecell), h, sizeof(h)));
  if (device >= 0 && device < 64) done[device] = true;
  return MFEM_OK;
}

// One unit of SPT_UNIT rim rows of a trimmed sweep (symp_trim_decide.h), a lane per row: the row's 27 slots from the compact copy (slot-major inside the
// unit: every slot one 512-byte piece), x at r + off[s] -- clamped as xidx clamps: a position outside the vector is only ever met by an absent entry, a
// stored zero --, 27 products rounded, then added, in slot order with a zero slot skipped: what dia_rows computes for the row, bit for bit.
__device__ __forceinline__ void symp_rim_unit(const SympGeom& Gm, const double* __restrict__ rimv, int64_t u, int lane, const double* __restrict__ x,
                                              double* __restrict__ y, double alpha, double beta, const double* __restrict__ dotw, double& dot_acc) {
  const int64_t g = u * SPT_UNIT + lane;
  if (g >= Gm.rim_rows) return;
  const int pl = (int)(g / Gm.rim_pp);
  int j = 0, k = 0;
  spt_rim_row((int)(g - (int64_t)pl * Gm.rim_pp), Gm.m2, Gm.ms1, Gm.ms2, j, k);
  const int64_t r = (int64_t)(Gm.p0 + pl) * Gm.PL + (int64_t)j * Gm.m2 + k;
  const double* v = rimv + u * SPT_UNIT_DOUBLES + lane;
  double vv[27], xv[27];
#pragma unroll
  for (int s = 0; s < 27; ++s) {
    vv[s] = SYM_LD(v + s * SPT_UNIT);
    int64_t idx = r + (int64_t)(s / 9 - 1) * Gm.PL + (int64_t)(sp_dj(s) * Gm.m2 + sp_dk(s));
    idx = idx < 0 ? 0 : idx;
    xv[s] = x[idx < Gm.nx ? idx : Gm.nx - 1];
  }
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < 27; ++s) acc += vv[s] != 0.0 ? vv[s] * xv[s] : 0.0;  // (the select keeps the product and the sum apart, as in dia_rows)
  double y0 = alpha * acc;
  if (beta != 0.0) y0 += beta * y[r];
  y[r] = y0;
  if (dotw) dot_acc += y0 * dotw[r];
}
// the rim rows in a launch of their own: beside the boundary part of a split SpMV, or with bit 26 of the "ell" knob
__global__ __launch_bounds__(64) void k_symp_rim(SympGeom Gm, const double* __restrict__ rimv, const double* __restrict__ x, double* __restrict__ y,
                                                  double alpha, double beta, const double* __restrict__ dotw, double* __restrict__ partials,
                                                  const int32_t* __restrict__ done_flag) {
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  for (int64_t u = blockIdx.x; u < Gm.rim_units; u += gridDim.x) symp_rim_unit(Gm, rimv, u, threadIdx.x, x, y, alpha, beta, dotw, dot_acc);
  if (partials) {
    const double w = wave_reduce_sum(dot_acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = w;
  }
}

#ifdef SYMP_SCHED_CLOCKS
// Probe builds only (-DSYMP_SCHED_CLOCKS; tools/symp_sched_probe.py measures the constants of symp_sched_decide.h with it): per run id four 64-bit words --
// wall clock at the run's start and end, the workgroup that swept it, its place in that workgroup's list.  Never in the shipped library.
// Only launches with per-run sums stamp, and only run ids below the buffer's capacity: no geometry can write past the caller's buffer.
__device__ long long* g_symp_clocks = nullptr;
__device__ int g_symp_clocks_runs = 0;
extern "C" int mfem_debug_symp_clocks(long long* buf /* [device, 4 x runs] or null */, int runs) {
  if (!buf || runs < 0) runs = 0;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_symp_clocks_runs), &runs, sizeof(runs)) != hipSuccess) return MFEM_ERR_HIP;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_symp_clocks), &buf, sizeof(buf)) == hipSuccess ? MFEM_OK : MFEM_ERR_HIP;
}
#endif
// B bands of SP_L lines per patch.  Per plane the wave runs its bands top to bottom as sub-steps of one step body (lane <-> two points of line lj of the
// band): the tables, the x ring and the edge block cover all SP_L * B lines, so band 1 finds band 0's +y entries of this plane (slots 9..11) and
// its next-plane entries of the previous plane (slots 0..2) in the tables -- the latter because band 0 holds its writes to the tables of slots 0..2 back
// until the last band of the plane has read them.  A band with no valid line (the last patch row) is skipped wave-uniformly.
// DC: form of the copy's main part (spmv_symp.h) -- 0 the diagonal stored as slot 13, 1 carried as one-byte codes counted from Gm.unit.
// CS: 1 = the constant form (symp_const_decide.h; MODE 0 only) -- a step whose byte in sflags is set is computed from the reference row cst alone.
// The body of both kernels below: k_spmv_symp<MODE, B, DC> is CS = 0, k_spmv_symp_const<B, DC, SCH> is MODE 0 with CS = 1.
// SCH: 1 = the wave walks its list of the schedule's table (symp_sched_decide.h; CS = 1 only) instead of the arithmetic rounds -- a parameter, not a run-time branch:
// an instantiation that is never given a table (256^3: one band, sums per workgroup) keeps the loop it had.
template <int MODE, int B, int DC, int CS, int SCH>
__device__ __forceinline__ void symp_sweep(const SympGeom& Gm, const double* __restrict__ pv, const double* __restrict__ x,
                                           double* __restrict__ y, double alpha, double beta,
                                           const double* __restrict__ dotw, double* __restrict__ partials,
                                           const int32_t* __restrict__ done_flag, int32_t* __restrict__ bad, const SympTail& tail, const SympConst& cst,
                                           const uint32_t* __restrict__ sflags, const int32_t* __restrict__ sched, int nruns_pr) {
  static_assert(CS == 0 || MODE == 0, "the check pass reads the stored copy");
  static_assert(SCH == 0 || CS == 1, "only the constant form is scheduled");
  constexpr int XL = sp_xl(B), XN = sp_xn(B), XU = sp_xu(B), NE = sp_ne(B), EU = sp_eu(B), MAINB = sp_main(B, DC), LOWB = sp_low(B);
  constexpr int NSL = sp_nslots(DC), S0 = 27 - NSL;  // slots S0..26 of a band are stored in its main part (DC = 1: the diagonal comes as a code)
  constexpr int BM = NSL * SP_ROWS, BL = 13 * SP_ROWS, BT = SP_L * SP_LS;  // a band's share of the main part, of the low part, of a table
  __shared__ __attribute__((aligned(16))) double xs[3][XL][SP_XW];
  __shared__ __attribute__((aligned(16))) double tab[sp_tab(B) + 2 + (CS ? 28 : 0)];  // CS: behind the tables and the spare cells the reference row's 27 values
  double* const ctab = tab + sp_tab(B) + 2;
  if (done_flag && done_flag[0]) return;
  const int lane = threadIdx.x, lj = lane / SP_PW, pk = lane % SP_PW, lb0 = lj * SP_LS + 2 * pk;
  const int NP = Gm.NR * Gm.NPk, nplanes = Gm.p1 - Gm.p0;
  // Runs and XCDs: workgroups with equal blockIdx % 8 share an XCD (round-robin dispatch; gridDim.x is a multiple of 8).  XCD c sweeps
  // a contiguous eighth of the patches, segment by segment, so that the runs resident on it at any time are neighbouring patches at
  // about the same plane: their overlapping x neighbourhoods meet in that XCD's L2.
  const int xcd = blockIdx.x & 7, pc = NP / 8, prem = NP % 8, pcnt = pc + (xcd < prem ? 1 : 0), pfirst = xcd * pc + (xcd < prem ? xcd : prem);
  // the LDS cells this lane fills from the edge block (5 or 6 entries per lane; table made on the host once: decoding the entries with
  // sp_edge() at the top of every launch cost every wave a few thousand instructions)
  int ecell[EU];
#pragma unroll
  for (int u = 0; u < EU; ++u) ecell[u] = c_sp_ecell[B - 1][lane + 64 * u];
  // the reference row goes to LDS once per launch (the barrier every run starts with orders it before the first read): 54 scalar registers held through the
  // sweep spilled 117 of them into lanes and cost every UNFLAGGED step a quarter more (the 512-point lattice with the form forced: 4.01 against 3.17 ms)
  if (CS && lane == 0) {
#pragma unroll
    for (int s = 0; s < 27; ++s) ctab[s] = cst.v[s];
  }
  // The flags of up to 64 consecutive steps of a run, lane i <-> step ft0 + i, in ONE gathered load per 63 steps: a scalar load per step showed its whole
  // latency (the wave has its SIMD to itself, and a scalar load shares its counter with the LDS traffic of the step body).  A step's flag is read from its lane.
  int fw = 0;
  int64_t ft0 = 0;
  int cur_patch = -1, bp = 0, bc = 1, bn = 2;  // x ring: previous / current / next plane
  int nb = 1;            // bands of the patch with a valid line
  bool have_hist = false;
  bool vxb[B], vyb[B];   // per band: the lane's first / second point lies in the lattice
  int64_t rin = 0;       // in-plane row offset j * m2 + k of the lane's first row in band 0
  int xo[XU], xa[XU];  // x staging: in-plane offset (may be negative) and LDS slot of the lane's neighbourhood points
  double dot_acc = 0.0;
  int fail = 0;
  e_d2 cur[B][NSL];      // per band: slots S0..26 of its sub-step, requested a full step (one plane) ahead -- with three resident waves per CU one
                         // sub-step in flight left the stream short (512^3, B = 2: 1142 against 1131 ms per step with the four-line form)
  int cdc[B];            // DC = 1: per band the codes of the lane's two diagonals (two signed bytes), requested with the band's main part
  e_d2 keep[3];          // band 0's slots 24..26, held back from the tables of slots 2..0 while a later band of the plane still reads the previous plane's
  double ed[EU], xr[XU];  // the step's edge block entries and the x neighbourhood of the plane after it, requested with band 0
  // x neighbourhood entry of plane `plane`: positions outside the vector's owned entries (beyond the last lattice line of the last
  // plane) are only ever multiplied by structurally absent entries -- any finite value serves: clamp
  auto xidx = [&](int plane, int u) -> int64_t {
    int64_t idx = (int64_t)plane * Gm.PL + xo[u];
    idx = idx < 0 ? 0 : idx;
    return idx < Gm.nx ? idx : Gm.nx - 1;
  };
  // the main part of band b of the step at v
  auto request = [&](const double* v, int b, bool fl) {
    if (CS && fl) return;  // (wave-uniform) a flagged step reads no matrix value
    if (vxb[b]) {
#pragma unroll
      for (int u = 0; u < NSL; ++u) cur[b][u] = SYM_LD(reinterpret_cast<const e_d2*>(v + b * BM + 2 * lane + u * SP_ROWS));
      if (DC && MODE == 0) cdc[b] = SYM_LD(reinterpret_cast<const unsigned short*>(v + sp_coff(B, DC)) + b * (SP_ROWS / 2) + lane);
    } else {
#pragma unroll
      for (int u = 0; u < NSL; ++u) cur[b][u] = (e_d2){0.0, 0.0};
      if (DC) cdc[b] = 0;  // (a lane outside the lattice: its sums are never stored)
    }
  };
  // the edge block of the step at v and the x neighbourhood of plane pnext
  auto request_step = [&](const double* v, int pnext, bool fl) {
    if (MODE == 0) {
      if (!(CS && fl)) {
#pragma unroll
        for (int u = 0; u < EU - 1; ++u) ed[u] = SYM_LD(v + B * BM + lane + 64 * u);
        ed[EU - 1] = lane < NE - 64 * (EU - 1) ? SYM_LD(v + B * BM + lane + 64 * (EU - 1)) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < XU - 1; ++u) xr[u] = x[xidx(pnext, u)];
      xr[XU - 1] = lane < XN - 64 * (XU - 1) ? x[xidx(pnext, XU - 1)] : 0.0;
    }
  };
  auto stage_x = [&](int buf, int plane) {
    double* dst = &xs[buf][0][0];
#pragma unroll
    for (int u = 0; u < XU - 1; ++u) dst[xa[u]] = x[xidx(plane, u)];
    if (lane < XN - 64 * (XU - 1)) dst[xa[XU - 1]] = x[xidx(plane, XU - 1)];
  };
  // round rk: the XCD's runs [W rk, W rk + W), rotated among its W waves from round to round (spc_run, symp_const_decide.h: a wave does not keep its patch column)
  // With a schedule (sched: symp_sched_decide.h; the constant form alone) the wave walks its list instead: offset[blockIdx], offset[blockIdx + 1] and up to
  // 64 run ids come in one gathered load each, lane i <-> the list's (lw0 + i)-th run, as a run's flags do.
  const int W = gridDim.x >> 3, jw = blockIdx.x >> 3, rot = spc_rot(Gm.NPk);
  int l0 = 0, nlist = (pcnt * Gm.nseg + W - 1) / W, lw = 0;
  if (SCH) {
    const int ov = lane < 2 ? sched[blockIdx.x + lane] : 0;
    l0 = __builtin_amdgcn_readlane(ov, 0);
    nlist = __builtin_amdgcn_readlane(ov, 1) - l0;
  }
  for (int rk = 0; rk < nlist; ++rk) {
  int patch, seg;
  if (SCH) {
    if ((rk & 63) == 0) lw = rk + lane < nlist ? sched[gridDim.x + 1 + l0 + rk + lane] : 0;  // (wave-uniform)
    const int rid = __builtin_amdgcn_readlane(lw, rk & 63);
    patch = rid / Gm.nseg;
    seg = rid - patch * Gm.nseg;
  } else {
    const int run = spc_run(W, jw, rk, rot);
    if (run >= pcnt * Gm.nseg) continue;
    patch = pfirst + run % pcnt;
    seg = run / pcnt;
  }
#ifdef SYMP_SCHED_CLOCKS  // probe builds only (tools/symp_sched_probe.py): the run's start and end on the 100 MHz wall clock
  const long long clk0 = wall_clock64();
#endif
  const int64_t t0 = (int64_t)patch * nplanes + (int64_t)nplanes * seg / Gm.nseg, t1 = (int64_t)patch * nplanes + (int64_t)nplanes * (seg + 1) / Gm.nseg;
  cur_patch = -1;
  for (int64_t t = t0; t < t1; ++t) {
    const int p = Gm.p0 + (int)(t - (int64_t)patch * nplanes);
    const int64_t step = (int64_t)(p - Gm.p0) * NP + patch;  // [plane][patch]: the runs of a segment advance plane by plane together
    const double* v = pv + step * MAINB;                                         // per band slots 13..26, then the edge block of the step
    const double* vlow = pv + (int64_t)NP * nplanes * MAINB + step * LOWB;      // per band its slots 0..12
    const bool more = t + 1 < t1 && p + 1 < Gm.p1;  // the next step continues this sweep
    if (CS && (patch != cur_patch || t - ft0 >= 63)) {  // (wave-uniform)
      ft0 = t;
      const int64_t tl = t + lane, sl = (tl - (int64_t)patch * nplanes) * NP + patch;  // the step of the run's (t + lane)-th entry
      fw = tl < t1 ? (int)((sflags[sl >> 2] >> (8 * (int)(sl & 3))) & 255u) : 0;
    }
    const bool fnow = CS && __builtin_amdgcn_readlane(fw, (int)(t - ft0)) != 0;
    const bool fnext = CS && more && __builtin_amdgcn_readlane(fw, (int)(t + 1 - ft0)) != 0;
    if (patch != cur_patch) {  // wave-uniform: a run or a patch starts -- nothing was requested ahead, no history
      cur_patch = patch;
      const int j0 = (patch / Gm.NPk) * (SP_L * B), k0 = (patch % Gm.NPk) * SP_W;
      const int k = k0 + 2 * pk;
      nb = 1;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int j = j0 + SP_L * b + lj;
        vxb[b] = j < Gm.m1 && k < Gm.m2;
        vyb[b] = j < Gm.m1 && k + 1 < Gm.m2;
        if (b > 0 && j0 + SP_L * b < Gm.m1) nb = b + 1;
      }
      rin = (int64_t)(j0 + lj) * Gm.m2 + k;
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int tt = lane + 64 * u, xl = tt / SP_XC, xc = tt - SP_XC * xl;
        xo[u] = (j0 - 1 + xl) * Gm.m2 + (k0 - 1 + xc);
        xa[u] = xl * SP_XW + xc;  // (the last u: only the first lanes belong to the neighbourhood)
      }
      have_hist = false;
      __syncthreads();  // the previous patch's last products may still be reading the x ring
#pragma unroll
      for (int b = 0; b < B; ++b)
        if (b < nb) request(v, b, fnow);
      request_step(v, p + 1, fnow);
      if (MODE == 0) {
        stage_x(bp, p - 1);
        stage_x(bc, p);
        // no history: the row's own previous-plane slots go where the mirror reads would look for them
#pragma unroll
        for (int b = 0; b < B; ++b) {
          if (b < nb && !fnow) {
#pragma unroll
            for (int s = 0; s < 9; ++s) {
              const e_d2 w = vxb[b] ? SYM_LD(reinterpret_cast<const e_d2*>(vlow + b * BL + 2 * lane + s * SP_ROWS)) : (e_d2){0.0, 0.0};
              double* c = tab + sp_tbase(s, B) + (sp_dj(s) + sp_adj(s)) * SP_LS + sp_dk(s) + 2 + b * BT + lb0;
              c[0] = w.x;
              c[1] = w.y;
            }
          }
        }
      }
    }
    if (CS && fnow) {
      // ---- a flagged step: whole patch, every row's 27 entries are the reference row's, bit for bit -- its own slots (compared by the fill) and therefore the
      // mirrored ones (the bind's fingerprint: every pair among the swept rows is bitwise equal; dia_bind: cst.v[s] = cst.v[26 - s] bit for bit).
      // No table, no edge block, no matrix load: the next plane's x into the ring, then per band the 27 products with the constants (a broadcast read of the wave's LDS copy) -- rounded,
      // then added, in slot order, the sums the step body below forms.  The tables are left stale: an unflagged step behind a flagged one starts like a run.
      {
        double* dst = &xs[bn][0][0];
#pragma unroll
        for (int u = 0; u < XU - 1; ++u) dst[xa[u]] = xr[u];
        if (lane < XN - 64 * (XU - 1)) dst[xa[XU - 1]] = xr[XU - 1];
      }
      __syncthreads();  // the ring's three planes are complete
      if (more && fnext) request_step(v + (int64_t)NP * MAINB, p + 2, true);  // (x alone)
#pragma unroll
      for (int b = 0; b < B; ++b) {
        e_d2 acc = {0.0, 0.0};
        double xself0 = 0.0, xself1 = 0.0;
        auto crun = [&](int s, int buf, int dj, bool self) {
#pragma clang fp contract(off)
          const double* xp = &xs[buf][SP_L * b + lj + 1 + dj][2 * pk];
          const e_d2 xa2 = *reinterpret_cast<const e_d2*>(xp), xb2 = *reinterpret_cast<const e_d2*>(xp + 2);
          const double c0 = ctab[s], c1 = ctab[s + 1], c2 = ctab[s + 2];  // (every lane the same address: a broadcast read)
          acc.x = acc.x + c0 * xa2.x;
          acc.y = acc.y + c0 * xa2.y;
          acc.x = acc.x + c1 * xa2.y;
          acc.y = acc.y + c1 * xb2.x;
          acc.x = acc.x + c2 * xb2.x;
          acc.y = acc.y + c2 * xb2.y;
          if (self) {
            xself0 = xa2.y;
            xself1 = xb2.x;
          }
        };
        crun(0, bp, -1, false);
        crun(3, bp, 0, false);
        crun(6, bp, 1, false);
        crun(9, bc, -1, false);
        crun(12, bc, 0, true);
        crun(15, bc, 1, false);
        crun(18, bn, -1, false);
        crun(21, bn, 0, false);
        crun(24, bn, 1, false);
        const int64_t r = (int64_t)p * Gm.PL + rin + (int64_t)(SP_L * b) * Gm.m2;
        double y0 = alpha * acc.x, y1 = alpha * acc.y;
        if (beta != 0.0) {
          y0 += beta * y[r];
          y1 += beta * y[r + 1];
        }
        __builtin_nontemporal_store((u_d2){y0, y1}, reinterpret_cast<u_d2*>(y + r));
        if (dotw) {
          if (dotw == x) {
            dot_acc += y0 * xself0;
            dot_acc += y1 * xself1;
          } else {
            dot_acc += y0 * dotw[r];
            dot_acc += y1 * dotw[r + 1];
          }
        }
      }
      __syncthreads();  // every lane is done with the ring's oldest plane: the next step overwrites it
      const int b_ = bp;
      bp = bc;
      bc = bn;
      bn = b_;
      if (!(more && fnext)) cur_patch = -1;  // the sweep ends, or an unflagged step follows: it starts like a run (requests, x ring, no history)
      continue;
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {   // (unrolled: the bands' registers are indexed at compile time)
    if (b < nb) {                   // wave-uniform
    const int lb = lb0 + b * BT;    // the lane's place in a table line block: line SP_L * b + lj of the patch
    const bool vx = vxb[b], vy = vyb[b], lastb = b + 1 >= nb;
    // ---- phase B: this sub-step's +z / +y slots go to LDS; with band 0 the step's edge entries and the next plane's x
#pragma unroll
    for (int s = 9; s < 13; ++s) *reinterpret_cast<e_d2*>(tab + sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb) = cur[b][26 - s - S0];
    e_d2 low[13];
    if (MODE == 0) {
      if (b == 0) {
#pragma unroll
        for (int u = 0; u < EU; ++u) tab[ecell[u]] = ed[u];
        double* dst = &xs[bn][0][0];
#pragma unroll
        for (int u = 0; u < XU - 1; ++u) dst[xa[u]] = xr[u];
        if (lane < XN - 64 * (XU - 1)) dst[xa[XU - 1]] = xr[XU - 1];
      }
    } else {
#pragma unroll
      for (int s = 0; s < 13; ++s) low[s] = vx ? SYM_LD(reinterpret_cast<const e_d2*>(vlow + b * BL + 2 * lane + s * SP_ROWS)) : (e_d2){0.0, 0.0};
    }
    // the sub-step's own upper slots stay in `mine`; the next sub-step of the same sweep is requested now and arrives during the products
    e_d2 mine[NSL];
#pragma unroll
    for (int u = 0; u < NSL; ++u) mine[u] = cur[b][u];
    const int mcd = DC && MODE == 0 ? cdc[b] : 0;
    __syncthreads();  // one wave: orders its LDS writes before the reads of other lanes
    if (more) {  // this band of the next plane; with the plane's last band the next step's edge block and the x of the plane behind it
      request(v + (int64_t)NP * MAINB, b, fnext);
      if (lastb) request_step(v + (int64_t)NP * MAINB, p + 2, fnext);
    }
    auto mirrored = [&](int s) -> e_d2 {
      const double* c = tab + sp_tbase(s, B) + (sp_dj(s) + sp_adj(s)) * SP_LS + sp_dk(s) + 2 + lb;
      e_d2 w;
      w.x = c[0];
      w.y = c[1];
      return w;
    };
    e_d2 acc = {0.0, 0.0};
    double xself0 = 0.0, xself1 = 0.0;
    // products rounded, then added, in slot order: what the plain kernel computes.  A structurally absent entry is an explicit zero
    // and every staged x is an owned entry of the vector (finite whenever x is), so its product is a signed zero that leaves the sum
    // unchanged -- no select needed here.
    auto run = [&](const e_d2& va, const e_d2& vb, const e_d2& vc, int buf, int dj, bool self) {
#pragma clang fp contract(off)  // v_mul_f64 + v_add_f64 like the plain kernel, not v_fma_f64
      const double* xp = &xs[buf][SP_L * b + lj + 1 + dj][2 * pk];
      const e_d2 xa2 = *reinterpret_cast<const e_d2*>(xp), xb2 = *reinterpret_cast<const e_d2*>(xp + 2);
      acc.x = acc.x + va.x * xa2.x;
      acc.y = acc.y + va.y * xa2.y;
      acc.x = acc.x + vb.x * xa2.y;
      acc.y = acc.y + vb.y * xb2.x;
      acc.x = acc.x + vc.x * xb2.x;
      acc.y = acc.y + vc.y * xb2.y;
      if (self) {
        xself0 = xa2.y;
        xself1 = xb2.x;
      }
    };
    if (MODE == 1) {
      // exactly the pairs the sweep mirrors: source rows inside the patch's valid bands (the seam between two bands included), previous-plane
      // slots only where a history exists
#pragma unroll
      for (int s = 0; s < 13; ++s) {
        const int dj = sp_dj(s), dk = sp_dk(s), gl = SP_L * b + lj;
        const bool in = gl + dj >= 0 && gl + dj < SP_L * nb && (dk < 0 ? pk > 0 : dk > 0 ? pk < SP_PW - 1 : true);
        if (in && vx && (s >= 9 || have_hist)) {
          const e_d2 m = mirrored(s);
          if (__double_as_longlong(m.x) != __double_as_longlong(low[s].x) && !(m.x == 0.0 && low[s].x == 0.0)) fail = 1;
          if (vy && __double_as_longlong(m.y) != __double_as_longlong(low[s].y) && !(m.y == 0.0 && low[s].y == 0.0)) fail = 1;
        }
      }
    } else {
      run(mirrored(0), mirrored(1), mirrored(2), bp, -1, false);
      run(mirrored(3), mirrored(4), mirrored(5), bp, 0, false);
      run(mirrored(6), mirrored(7), mirrored(8), bp, 1, false);
      run(mirrored(9), mirrored(10), mirrored(11), bc, -1, false);
      e_d2 dg;  // the diagonal: stored, or the bind's unit (+-1.0) moved by the row's code -- the same double bit for bit
      if (DC) {
        dg.x = __longlong_as_double(Gm.unit + (long long)(signed char)(mcd & 255));
        dg.y = __longlong_as_double(Gm.unit + (long long)(signed char)((mcd >> 8) & 255));
      } else {
        dg = mine[0];
      }
      run(mirrored(12), dg, mine[14 - S0], bc, 0, true);
      run(mine[15 - S0], mine[16 - S0], mine[17 - S0], bc, 1, false);
    }
    __syncthreads();  // every lane is done with the tables
    // the next-plane slots become the history of the next plane; slots 24..26 of a band that is not the plane's last wait in `keep`: the band below
    // still reads the previous plane's from the table line this band would overwrite
#pragma unroll
    for (int s = 3; s < 9; ++s) *reinterpret_cast<e_d2*>(tab + sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb) = mine[26 - s - S0];
    if (B > 1 && !lastb) {
#pragma unroll
      for (int s = 0; s < 3; ++s) keep[s] = mine[26 - s - S0];
    } else {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        *reinterpret_cast<e_d2*>(tab + sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb) = mine[26 - s - S0];
        if (B > 1 && b > 0) *reinterpret_cast<e_d2*>(tab + sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb - BT) = keep[s];
      }
    }
    if (MODE == 0) {
      run(mine[18 - S0], mine[19 - S0], mine[20 - S0], bn, -1, false);
      run(mine[21 - S0], mine[22 - S0], mine[23 - S0], bn, 0, false);
      run(mine[24 - S0], mine[25 - S0], mine[26 - S0], bn, 1, false);
      const int64_t r = (int64_t)p * Gm.PL + rin + (int64_t)(SP_L * b) * Gm.m2;
      double y0 = alpha * acc.x, y1 = alpha * acc.y;
      if (beta != 0.0) {
        if (vx) y0 += beta * y[r];
        if (vy) y1 += beta * y[r + 1];
      }
      {
        // one 16-byte store (8-byte aligned), non-temporal: 0.910 -> 0.896 ms per CG iteration at 256^3
        if (vy) __builtin_nontemporal_store((u_d2){y0, y1}, reinterpret_cast<u_d2*>(y + r));
        else if (vx) __builtin_nontemporal_store(y0, y + r);
      }
      if (dotw) {
        if (dotw == x) {
          if (vx) dot_acc += y0 * xself0;
          if (vy) dot_acc += y1 * xself1;
        } else {
          if (vx) dot_acc += y0 * dotw[r];
          if (vy) dot_acc += y1 * dotw[r + 1];
        }
      }
    }
    }
    }
    have_hist = true;
    if (MODE == 0) {
      const int b_ = bp;
      bp = bc;
      bc = bn;
      bn = b_;
    }
    if (!more) cur_patch = -1;  // nothing requested: the next step (if any) starts like a run
  }
  // partial sums per run (sps_per_run): the run's p . Ap sum goes to its own place and the accumulator starts again -- the sums do not depend on the schedule
  if (MODE == 0 && nruns_pr > 0 && partials) {
    const double w = wave_reduce_sum(dot_acc);
    if (lane == 0) partials[sps_run_id(patch, seg, Gm.nseg)] = w;
    dot_acc = 0.0;
  }
#ifdef SYMP_SCHED_CLOCKS
  if (MODE == 0 && nruns_pr > 0 && g_symp_clocks && sps_run_id(patch, seg, Gm.nseg) < g_symp_clocks_runs && lane == 0) {
    long long* c = g_symp_clocks + 4 * (int64_t)sps_run_id(patch, seg, Gm.nseg);
    c[0] = clk0;
    c[1] = wall_clock64();
    c[2] = blockIdx.x;
    c[3] = rk;
  }
#endif
  }
  if (MODE == 0 && tail.on) {
    // 128-row units in front of and behind the swept planes (a unit straddling the boundary is masked row by row), shared among the waves
    const int64_t UA = (tail.lo + 127) / 128, ub = tail.hi / 128, UB = (tail.n + 127) / 128 - ub;
    for (int64_t u = blockIdx.x; u < UA + UB; u += gridDim.x) {
      const int64_t r = (u < UA ? u : ub + (u - UA)) * 128 + 2 * lane;
      if (r < tail.n)
        dia_rows<2, 3, true>(r, tail.n, tail.npad, tail.K, *tail.Op, tail.flags, tail.cols, tail.ell, x, y, alpha, beta, dotw, 0, dot_acc,
                             tail.lo, tail.hi);
    }
  }
  if (MODE == 0 && tail.rim) {  // the rim rows of a trimmed sweep: their compact copy lies behind the patch-major one
    const double* rimv = pv + (int64_t)NP * nplanes * (MAINB + LOWB);
    for (int64_t u = blockIdx.x; u < Gm.rim_units; u += gridDim.x) symp_rim_unit(Gm, rimv, u, lane, x, y, alpha, beta, dotw, dot_acc);
  }
  if (MODE == 1) {
    if (fail) atomicOr(bad, 1);
  } else if (partials) {
    const double w = wave_reduce_sum(dot_acc);
    if (lane == 0) partials[nruns_pr + blockIdx.x] = w;  // (per-run sums: the workgroup's tail and rim units alone, behind the runs')
  }
}

template <int MODE, int B, int DC>
__global__ __launch_bounds__(64) void k_spmv_symp(SympGeom Gm, const double* __restrict__ pv, const double* __restrict__ x,
                                                   double* __restrict__ y, double alpha, double beta,
                                                   const double* __restrict__ dotw, double* __restrict__ partials,
                                                   const int32_t* __restrict__ done_flag, int32_t* __restrict__ bad, SympTail tail, int nruns_pr) {
  symp_sweep<MODE, B, DC, 0, 0>(Gm, pv, x, y, alpha, beta, dotw, partials, done_flag, bad, tail, SympConst{}, nullptr, nullptr, nruns_pr);
}
template <int B, int DC, int SCH>
__global__ __launch_bounds__(64) void k_spmv_symp_const(SympGeom Gm, const double* __restrict__ pv, const double* __restrict__ x,
                                                         double* __restrict__ y, double alpha, double beta,
                                                         const double* __restrict__ dotw, double* __restrict__ partials,
                                                         const int32_t* __restrict__ done_flag, SympTail tail, SympConst cst,
                                                         const uint32_t* __restrict__ sflags, const int32_t* __restrict__ sched, int nruns_pr) {
  symp_sweep<0, B, DC, 1, SCH>(Gm, pv, x, y, alpha, beta, dotw, partials, done_flag, nullptr, tail, cst, sflags, sched, nruns_pr);
}

// patch-major copy of the swept planes from the slot-major copy: per step [plane - p0][patch] and band the slots 13..26, then the edge block (main
// part) and, behind all main parts, per band the slots 0..12 (low part), zero
// where the patch sticks out of the lattice; one wave per (plane, patch)
__global__ __launch_bounds__(MFEM_BLOCK) void k_symp_bind(SympGeom Gm, int K, const double* __restrict__ ell, double* __restrict__ pv) {
  const int lane = threadIdx.x & 63, lj = lane / SP_PW, pk = lane % SP_PW;
  const int NP = Gm.NR * Gm.NPk, B = Gm.B;
  const int MAINB = sp_main(B), LOWB = sp_low(B), NEB = sp_ne(B), EPADB = sp_epad(B);
  const int64_t T = (int64_t)NP * (Gm.p1 - Gm.p0);
  for (int64_t t = (int64_t)blockIdx.x * (MFEM_BLOCK / 64) + (threadIdx.x >> 6); t < T; t += (int64_t)gridDim.x * (MFEM_BLOCK / 64)) {
    const int nplanes = Gm.p1 - Gm.p0, patch = (int)(t / nplanes), p = Gm.p0 + (int)(t % nplanes);
    const int j0 = (patch / Gm.NPk) * (SP_L * B), k0 = (patch % Gm.NPk) * SP_W;
    const int64_t step = (int64_t)(p - Gm.p0) * NP + patch;
    double* out = pv + step * MAINB;
    double* outlow = pv + T * MAINB + step * LOWB;
    for (int b = 0; b < B; ++b) {
      const int j = j0 + SP_L * b + lj, k = k0 + 2 * pk;
      const bool vx = j < Gm.m1 && k < Gm.m2, vy = j < Gm.m1 && k + 1 < Gm.m2;
      const int64_t r = (int64_t)p * Gm.PL + (int64_t)j * Gm.m2 + k;
      const int64_t b0 = ell_base(r, K), b1 = ell_base(r + 1, K);
      for (int s0 = 0; s0 < 27; s0 += 9) {
        e_d2 w[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) {
          w[u].x = vx ? ell[b0 + (s0 + u) * ELL_B] : 0.0;
          w[u].y = vy ? ell[b1 + (s0 + u) * ELL_B] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 9; ++u) {
          const int sl = s0 + u;  // slots 0..12 to the low part, 13..26 to the main part
          double* dst = sl < 13 ? outlow + b * 13 * SP_ROWS + sl * SP_ROWS : out + b * 14 * SP_ROWS + (sl - 13) * SP_ROWS;
          *reinterpret_cast<e_d2*>(dst + 2 * lane) = w[u];
        }
      }
    }
    for (int e = lane; e < EPADB; e += 64) {
      int s = 0, line = 0, col = 0, cell = 0;
      double val = 0.0;
      if (e < NEB && sp_edge(e, s, line, col, cell, B) && j0 + line < Gm.m1 && k0 + col < Gm.m2)
        val = ell[ell_base((int64_t)p * Gm.PL + (int64_t)(j0 + line) * Gm.m2 + k0 + col, K) + s * ELL_B];
      out[B * 14 * SP_ROWS + e] = val;
    }
  }
}

// Structure of the tile sweep (once per pattern): list `lc` with offsets `off` has the lattice form with PL rows per plane; blocks [run_lo, run_hi)
// are the longest run of regular blocks, cut here to whole chunks (4 blocks)
static void sym27_plan(mfem_csr_s* A, const int32_t* off, int lc, int64_t PL, int64_t run_lo, int64_t run_hi) {
  const int64_t Sc = (PL + SYM_ROWS / 2) / SYM_ROWS;  // chunks per plane, rounded: the tiles drift by PL - Sc * 512 rows per plane
  if (Sc < 8 || Sc > MFEM_MAX_PARTIALS / 2) return;   // any drift between tile and plane: the mirrored-fraction rule below decides
  const int64_t bpc = SYM_ROWS / ELL_B, c0 = (run_lo + bpc - 1) / bpc, c1 = run_hi / bpc;
  if (c1 - c0 < 4 * Sc) return;
  // entries per chunk that k_spmv_sym27 mirrors instead of loading (same lane pattern in every chunk)
  int64_t mx = 0, myz = 0;
  for (int t = 0; t < SYM_ROWS / 2; ++t) {
    for (int q = 0; q < 9; ++q) {
      const int64_t lp = 2 * t + Sc * SYM_ROWS + off[q];
      if (lp >= 0 && lp + 1 < SYM_ROWS) mx += 2;
    }
    for (int q = 9; q < 12; ++q) {
      const int64_t lp = 2 * t + off[q];
      if (lp >= 0 && lp + 1 < SYM_ROWS) myz += 2;
    }
    myz += t > 0 ? 2 : 1;
  }
  // worth it from a quarter of the 13 lower diagonals mirrored (hex-8 256^3: 65 %; 512^3, where a 513-point lattice line is
  // longer than the tile and only the dj = 0 and -z diagonals qualify: 31 %, CG iteration 8.70 -> 7.91 ms)
  if (20 * (mx + myz) < 5 * 13 * SYM_ROWS) return;
  A->sym_state = 1;
  A->sym_c0 = c0;
  A->sym_c1 = c1;
  A->sym_S = (int)Sc;
  A->sym_cls = lc;
  A->sym_mx = mx;
  A->sym_myz = myz;
}
// Structure of the patch sweep: the lattice planes (m2 points per line) that lie entirely in that run
static void symp_plan(mfem_csr_s* A, int lc, int64_t m2, int64_t PL, int64_t run_lo, int64_t run_hi) {
  A->symp_state = -1;
  if (PL % m2 != 0 || PL / m2 < 2 || PL >= (int64_t)1 << 30) return;
  const int64_t p0 = (run_lo * ELL_B + PL - 1) / PL, p1 = run_hi * ELL_B / PL;
  // a swept row reads x[r - PL - m2 - 1 .. r + PL + m2 + 1]: plane p0 >= 1 and p1 <= (rows / PL) - 1 follow from the
  // regular-block test (r + off in [0, nx) for every row of the block)
  if (p1 - p0 < 4 || p0 < 1) return;
  A->symp_state = 1;
  A->symp_m2 = (int)m2;
  A->symp_m1 = (int)(PL / m2);
  A->symp_PL = PL;
  A->symp_p0 = (int)p0;
  A->symp_p1 = (int)p1;
  A->symp_NS = (A->symp_m1 + SP_L - 1) / SP_L;
  A->symp_NPk = (A->symp_m2 + SP_W - 1) / SP_W;
  A->sym_cls = lc;
}
void mfem_sym_plan(mfem_csr_s* A, const int32_t* off, int lc, int64_t m2, int64_t PL, int64_t run_lo, int64_t run_hi) {
  sym27_plan(A, off, lc, PL, run_lo, run_hi);
  symp_plan(A, lc, m2, PL, run_lo, run_hi);
}

// Is sweep k wanted on this structure?  (mfem_debug_set_layout_min_rows(0, ...) lifts the size limits for the parity tests.)
// Tile sweep: it needs ~2 workgroups per CU of >= 8 steps each to beat the plain kernel -- chunk ranges below ~2700 chunks (1.4 M rows, measured crossover
// between 96^3 and 112^3) stay on the plain kernel.  Patch sweep: measured CG iteration, workgroup-tile sweep / patch sweep (tools/probe_sym.py): 128^3
// 0.142 / 0.173 ms, 192^3 0.369 / 0.397, 256^3 0.896 / 0.896, 320^3 1.82 / 1.72, 384^3 3.28 / 2.89, 512^3 7.95 / 6.66 -- the patch sweep from 2.4e7 swept
// rows on, or where a lattice line no longer fits the 512-row tile twice.
bool mfem_sym_wanted(const mfem_csr_s* A, DiaKernel k) {
  if (!g_ell.sym || !A->dia_triples) return false;
  const bool all = g_layout_min_rows_dia == 0;
  if (k == DIA_SYM27) return A->sym_state == 1 && (all || A->sym_c1 - A->sym_c0 >= 2700);
  return A->symp_state == 1 && g_ell.symp && (all || (int64_t)(A->symp_p1 - A->symp_p0) * A->symp_PL >= 24000000 || A->symp_m2 > 256);
}

static int sym27_grid(const mfem_context_s* ctx, const mfem_csr_s* A, int64_t* nsteps_out) {
  // 53 KB of LDS per workgroup: three per CU; equal segments for every tile and all workgroups resident in one round
  // (645 workgroups of 51 steps beat 768 of 43 / 51 at 256^3: the longest segment sets the time)
  const int64_t nsteps = (A->sym_c1 - A->sym_c0 + A->sym_S - 1) / A->sym_S;
  const int resident = SYM_WG_PER_CU * ctx->num_cus;
  int nseg = resident / A->sym_S;
  if (nseg < 1) nseg = 1;
  // tiles that cannot fill the resident slots in whole rounds (512^3: 514 tiles on 768 slots) are cut into ~2.7 rounds of shorter
  // segments instead: 8.92 -> 7.91 ms per CG iteration there; at 256^3 (645 of 768) more segments change nothing
  if ((int64_t)A->sym_S * nseg * 10 < (int64_t)resident * 8) nseg = (8 * ctx->num_cus + A->sym_S - 1) / A->sym_S;
  while (nseg > 1 && (int64_t)A->sym_S * nseg > MFEM_MAX_PARTIALS - 512) --nseg;  // one partial sum per workgroup (+ <= 512 of the boundary part of a split SpMV)
  if (nseg > nsteps / 8) nseg = (int)(nsteps / 8);  // a segment's first step has no history: keep segments >= 8 steps long
  if (nseg < 1) nseg = 1;
  if (nsteps_out) *nsteps_out = nsteps;
  return A->sym_S * nseg;
}
// runs per patch: the smallest count that fills >= 90 % of the resident one-wave workgroups in whole rounds (a run's first step has no
// history: runs stay >= 16 planes long)
struct SympExt { int ms1, ms2, NS, NPk, NR; };  // swept extents of a plane and the strips, patch columns and patch rows that cover them
static SympExt symp_ext(const mfem_csr_s* A, int B, int trim) {
  SympExt e;
  e.ms1 = spt_ms1(A->symp_m1, B, trim != 0);
  e.ms2 = spt_ms2(A->symp_m2, trim != 0);
  e.NS = (e.ms1 + SP_L - 1) / SP_L;
  e.NPk = spt_cols(e.ms2);
  e.NR = spt_rows(e.ms1, B);
  return e;
}
static SympExt symp_ext(const mfem_csr_s* A) { return symp_ext(A, mfem_symp_bands(A), mfem_symp_trim(A)); }
static int symp_nseg(const mfem_context_s* ctx, const mfem_csr_s* A) {  // (the rule: spt_nseg, symp_trim_decide.h)
  const SympExt e = symp_ext(A);
  return spt_nseg((int64_t)e.NR * e.NPk, (int64_t)sp_wg_per_cu(mfem_symp_bands(A)) * ctx->num_cus, A->symp_p1 - A->symp_p0);  // the form's own resident slots
}
SympGeom mfem_symp_geom(const mfem_context_s* ctx, const mfem_csr_s* A) {  // (nx = n: the sweep stages owned entries of x only -- swept rows reference no ghost column)
  const int B = mfem_symp_bands(A);
  const SympExt e = symp_ext(A);
  SympGeom G{A->symp_PL, A->n, A->symp_m1, A->symp_m2, A->symp_p0, A->symp_p1, e.NS, e.NPk, symp_nseg(ctx, A), B, e.NR, A->symp_DC, sp_unit_bits(A->symp_dneg)};
  G.ms1 = e.ms1;
  G.ms2 = e.ms2;
  G.rim_pp = spt_rim(G.m1, G.m2, G.ms1, G.ms2);
  G.rim_rows = (int64_t)G.rim_pp * (G.p1 - G.p0);
  G.rim_units = spt_units(G.rim_rows);
  return G;
}
int64_t mfem_symp_steps(const mfem_csr_s* A, int B, int trim) {
  if (B < 1) B = mfem_symp_bands(A);
  const SympExt e = symp_ext(A, B, trim < 0 ? mfem_symp_trim(A) : trim);
  return (int64_t)e.NR * e.NPk * (A->symp_p1 - A->symp_p0);
}
int64_t mfem_symp_copy_doubles(const mfem_csr_s* A, int B, int trim) {
  const SympExt e = symp_ext(A, B, trim);
  return mfem_symp_steps(A, B, trim) * sp_step(B) + spt_units((int64_t)spt_rim(A->symp_m1, A->symp_m2, e.ms1, e.ms2) * (A->symp_p1 - A->symp_p0)) * SPT_UNIT_DOUBLES +
         spc_flag_doubles(mfem_symp_steps(A, B, trim)) + SPS_TABLE_DOUBLES;
}
unsigned char* mfem_symp_flags_of(double* pvals, const SympGeom& G) {
  return (unsigned char*)(pvals + (int64_t)G.NR * G.NPk * (G.p1 - G.p0) * sp_step(G.B, G.DC) + G.rim_units * SPT_UNIT_DOUBLES);
}
// the schedule's table lies behind the step flags (symp_sched_decide.h: SPS_TABLE_DOUBLES at the most)
static int32_t* symp_sched_of(double* pvals, const SympGeom& G) {
  return (int32_t*)(mfem_symp_flags_of(pvals, G) + 8 * spc_flag_doubles((int64_t)G.NR * G.NPk * (G.p1 - G.p0)));
}
int64_t mfem_symp_swept_rows(const mfem_csr_s* A) {
  const SympExt e = symp_ext(A);
  return (int64_t)(A->symp_p1 - A->symp_p0) * e.ms1 * e.ms2;
}
#define SYMP_RIM_GRID 256  // workgroups of k_symp_rim at the most (one partial sum each)
static_assert(SPS_MAX_PARTIALS == MFEM_MAX_PARTIALS && SPS_OUTSIDE_RESERVE == 1024 + SYMP_RIM_GRID, "symp_sched_decide.h spells both out");
// mfem_debug_set("symp_sched", mode | seed << 8, grid cap): the schedule of the constant form's runs (symp_sched_decide.h) -- 0 the decision's own, 1 the identity
// schedule, 2 a pseudo-random assignment under `seed` -- read when a layout is bound; the cap on the sweep's grid (0: none; rounded down to a multiple of 8)
// puts several runs on a wave of a small lattice and is read per product.  Same y, same partial sums bit for bit under every mode.
static std::atomic<int> g_symp_sched_mode{SPS_AUTO}, g_symp_sched_cap{0};
static std::atomic<long long> g_symp_sched_seed{0};
extern "C" int mfem_debug_set_symp_sched(int64_t a, int64_t b) {
  ++mfem_debug_epoch;
  g_symp_sched_mode = (int)(a & 255);
  g_symp_sched_seed = (long long)(a >> 8);
  g_symp_sched_cap = b > 0 ? (int)(b < MFEM_MAX_PARTIALS ? b : MFEM_MAX_PARTIALS) : 0;
  return MFEM_OK;
}
static std::atomic<long long> g_symp_sched_binds{0};  // binds that built a schedule table (tests, the A/B)
extern "C" long long mfem_debug_symp_sched_count(void) { return g_symp_sched_binds; }
static int symp_grid(const mfem_context_s* ctx, const mfem_csr_s* A) {
  const int B = mfem_symp_bands(A);
  const SympExt e = symp_ext(A);
  const int64_t NP = (int64_t)e.NR * e.NPk;
  int64_t g = 8 * ((NP + 7) / 8) * symp_nseg(ctx, A);  // every XCD's share of the runs, padded to the largest share
  int64_t cap = (int64_t)sp_wg_per_cu(B) * ctx->num_cus;
  if (cap > MFEM_MAX_PARTIALS - 1024 - SYMP_RIM_GRID) cap = MFEM_MAX_PARTIALS - 1024 - SYMP_RIM_GRID;  // (the boundary part's and the rim launch's partial sums follow)
  if (g_symp_sched_cap > 0 && cap > g_symp_sched_cap) cap = g_symp_sched_cap;
  cap &= ~(int64_t)7;
  if (g > cap) g = cap;
  return g < 8 ? 8 : (int)g;
}

// The schedule of a bind that ended on the constant form (symp_sched_decide.h): the step flags come to the host (a byte per step; the bind has just
// synchronised for the fill's verdict), the flagged steps per run are counted, the table is built and goes into the layout's buffer behind the flags.
// Nothing to schedule -- the stored form, the identity mode of the knob, runs that do not fit the partial-sum array -- leaves A->symp_sched null.
int mfem_symp_sched_bind(mfem_context_s* ctx, mfem_csr_s* A, const SympGeom& G) {
  A->symp_sched = nullptr;
  A->symp_sched_grid = 0;
  if (!A->symp_vals) return MFEM_OK;
  const SpsGeom g{G.NR * G.NPk, G.NPk, G.nseg, G.p1 - G.p0, symp_grid(ctx, A)};
  // (the reserve as the launch will count it where the bind can know: bit 26 of the "ell" knob; whether a product is split among ranks is decided per
  // product -- a table such a launch does not take costs this bind 0.5 MB of flags and two synchronisations, nothing else)
  const int kind = sps_kind(A->symp_CS != 0, sps_per_run(sps_nruns(g), g.grid, g_ell.symp_tail ? 0 : SPS_OUTSIDE_RESERVE), g_symp_sched_mode);
  if (!kind) return MFEM_OK;
  const int64_t steps = (int64_t)g.NP * g.nplanes;
  const int nruns = sps_nruns(g);
  std::vector<unsigned char> fl((size_t)steps);
  MFEM_CHECK_HIP(hipMemcpyAsync(fl.data(), mfem_symp_flags_of(A->symp_vals, G), (size_t)steps, hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> flagged((size_t)nruns), table((size_t)g.grid + 1 + nruns), work(2 * (size_t)nruns + g.grid);
  std::vector<int64_t> load((size_t)g.grid);
  int32_t first[9];
  for (int p = 0; p < g.NP; ++p)
    for (int s = 0; s < g.nseg; ++s) flagged[sps_run_id(p, s, g.nseg)] = sps_run_flagged(g, fl.data(), p, s);
  sps_build(g, flagged.data(), kind == SPS_RANDOM ? SPS_RANDOM : SPS_AUTO, (uint64_t)g_symp_sched_seed.load(), table.data(), table.data() + g.grid + 1, first,
            load.data(), work.data());
  static_assert(sizeof(int32_t) * (2 * SPS_MAX_PARTIALS + 1) <= sizeof(double) * SPS_TABLE_DOUBLES, "the table's room in the layout's buffer");
  int32_t* d = symp_sched_of(A->symp_vals, G);
  MFEM_CHECK_HIP(hipMemcpyAsync(d, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // (the host copy goes away)
  A->symp_sched = d;
  A->symp_sched_grid = g.grid;
  ++g_symp_sched_binds;
  return MFEM_OK;
}

// Matrix entries (8 B) one product by sweep k reads from memory.  Tile sweep: K per padded row less what it takes from LDS.  Patch sweep: the rows
// outside the swept planes read their K slots; the sweep reads the 14 upper slots of every valid lane pair and the edge block per step + the nine
// previous-plane slots wherever a run or a patch starts; a trimmed sweep has whole patches only and its rim rows read their 27 slots.  (The form of the
// diagonal: the bound copy's; unbound: the last patch-sweep bind's.)
int64_t mfem_sym_entries(const mfem_context_s* ctx, const mfem_csr_s* A, DiaKernel k) {
  if (k == DIA_SYM27) {
    const int64_t nch = A->sym_c1 - A->sym_c0;
    return (int64_t)A->ell_K * A->ell_npad - ((nch - sym27_grid(ctx, A, nullptr)) * A->sym_mx + nch * A->sym_myz);
  }
  const int B = mfem_symp_bands(A);
  const SympExt x = symp_ext(A);
  const int NP = x.NR * x.NPk, nplanes = A->symp_p1 - A->symp_p0, nseg = symp_nseg(ctx, A);
  int64_t e = (int64_t)A->ell_K * (A->ell_npad - (int64_t)nplanes * A->symp_PL), codes = 0;
  e += 27 * (int64_t)spt_rim(A->symp_m1, A->symp_m2, x.ms1, x.ms2) * nplanes;
  for (int patch = 0; patch < NP; ++patch) {
    int64_t nv = 0;  // valid lane pairs of all bands (a band without a valid line is skipped: none of its lanes is valid)
    for (int lp = 0; lp < 64 * B; ++lp) {
      const int j = (patch / x.NPk) * (SP_L * B) + lp / SP_PW, kk = (patch % x.NPk) * SP_W + 2 * (lp % SP_PW);
      if (j < A->symp_m1 && kk < A->symp_m2) ++nv;
    }
    e += (28 * nv + sp_ne(B)) * nplanes + 18 * nv * nseg;
    codes += 2 * nv * nplanes;
  }
  // the constant form reads neither the upper slots, the edge block nor the codes of a flagged step (a whole patch), and one flag byte per step
  if (A->symp_vals ? A->symp_CS : A->symp_cs_last) {
    const int64_t fl = A->symp_vals ? A->symp_flagged : A->symp_flagged_last;
    e -= fl * spc_saved_entries(B) - spc_flag_doubles((int64_t)NP * nplanes);
    codes -= fl * spc_saved_codes(B);
  }
  // the coded form reads two bytes instead of two doubles of diagonal per valid lane pair and step (whole entries: rounded up)
  if (mfem_symp_coded(A)) e -= codes - (codes + 7) / 8;
  return e;
}

// the sweep's instantiation for a geometry: pass (MODE), bands, form of the diagonal; the constant form (MODE 0 only)
template <int SCH>
static auto symp_const_kernel(const SympGeom& G) {
  if (G.DC) return G.B == 2 ? k_spmv_symp_const<2, 1, SCH> : k_spmv_symp_const<1, 1, SCH>;
  return G.B == 2 ? k_spmv_symp_const<2, 0, SCH> : k_spmv_symp_const<1, 0, SCH>;
}
template <int MODE>
static auto symp_kernel(const SympGeom& G) {
  if (G.DC) return G.B == 2 ? k_spmv_symp<MODE, 2, 1> : k_spmv_symp<MODE, 1, 1>;
  return G.B == 2 ? k_spmv_symp<MODE, 2, 0> : k_spmv_symp<MODE, 1, 0>;
}

static std::atomic<long long> g_symp_fp_checks{0};  // binds whose symmetry verdict came from the fill's fingerprint (tests)
extern "C" long long mfem_debug_symp_fingerprint_count(void) { return g_symp_fp_checks; }

// Are the pairs sweep k mirrors bitwise equal in the copies of this bind (buf: slot-major, pvals: patch-major)?  The patch sweep's copy is completed
// first when it was not filled directly; its verdict is the fill's fingerprint when it made one (zero = symmetric among the swept rows), else a
// check pass, as for the tile sweep.
// *dc_refused: the copy has the coded form (G.DC) and the fill met a swept row whose scaled diagonal has no code (d_flags[18], beside the fingerprint): the
// bind refills in the stored form and asks again.  *dneg: the unit its codes count from is -1.0 (d_flags[19]).
// flags_made: the fill also left its count of constant steps (d_flags[SPC_COUNT_AT]) and their reference row (d_flags[SPC_REF_AT..]): *flagged, *cst come
// back in the same copy as the fingerprint.
int mfem_sym_verdict(mfem_context_s* ctx, mfem_csr_s* A, DiaKernel k, const double* buf, double* pvals, const SympGeom& G, bool direct, bool fp_made, bool* ok,
                     bool* dc_refused, int* dneg, bool flags_made, SympConst* cst, int64_t* flagged) {
  int32_t* d_bad = ctx->d_flags + 9;
  const size_t fp_ints = flags_made && k == DIA_SYMP ? MFEM_NFLAGS - 16 : 4;  // the fingerprint, the coded form's two flags (and the constant form's count and reference row)
  auto read_const = [&]() {
    if (!(flags_made && k == DIA_SYMP && cst && flagged)) return;
    *flagged = ctx->h_flags[SPC_COUNT_AT];
    memcpy(cst, ctx->h_flags + SPC_REF_AT, sizeof(SympConst));
  };
  *dc_refused = false;
  *dneg = 0;
  if (k == DIA_SYMP) {
    { const int rt = symp_upload_tables(ctx->device); if (rt) return rt; }
    if (!direct) {
      const int64_t T = mfem_symp_steps(A);
      const int gb = (int)(T / 4 + 1 < (int64_t)ctx->num_cus * 32 ? T / 4 + 1 : (int64_t)ctx->num_cus * 32);
      hipLaunchKernelGGL(k_symp_bind, dim3(gb), dim3(MFEM_BLOCK), 0, ctx->stream, G, A->ell_K, buf, pvals);
      MFEM_CHECK_LAUNCH();
    }
    if (fp_made) {
      MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 16, ctx->d_flags + 16, fp_ints * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
      unsigned long long fpv;
      memcpy(&fpv, ctx->h_flags + 16, sizeof(fpv));
      *ok = fpv == 0;
      *dc_refused = G.DC && ctx->h_flags[18] != 0;
      *dneg = G.DC && ctx->h_flags[19] != 0;
      read_const();
      ++g_symp_fp_checks;
      return MFEM_OK;
    }
  }
  MFEM_CHECK_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), ctx->stream));
  if (k == DIA_SYMP)
    hipLaunchKernelGGL(symp_kernel<1>(G), dim3(symp_grid(ctx, A)), dim3(64), 0, ctx->stream, G, (const double*)pvals,
                       (const double*)nullptr, (double*)nullptr, 0.0, 0.0, (const double*)nullptr, (double*)nullptr, (const int32_t*)nullptr, d_bad,
                       SympTail{}, 0);
  else
    hipLaunchKernelGGL(k_sym27_check, dim3(ctx->num_cus * 8), dim3(MFEM_BLOCK), 0, ctx->stream, A->ell_K, (const DiaOffsets*)A->dia_dev, buf,
                       A->sym_c0 * SYM_ROWS, A->sym_c1 * SYM_ROWS, A->sym_cls, d_bad);
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 9, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (k == DIA_SYMP && (G.DC || flags_made)) MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 18, ctx->d_flags + 18, (fp_ints - 2) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  *ok = ctx->h_flags[9] == 0;
  *dc_refused = k == DIA_SYMP && G.DC && ctx->h_flags[18] != 0;
  *dneg = k == DIA_SYMP && G.DC && ctx->h_flags[19] != 0;
  read_const();
  return MFEM_OK;
}

// The product by sweep k.  Tile sweep: the rows of the regular chunk range by the sweep, the rest by the per-row code in the same launch (part 2 of a
// split SpMV: those chunks alone, after the halo has arrived, one workgroup each).  Patch sweep: the swept planes on the patch-major copy, the other
// rows by the per-row code on the slot-major copy -- unsplit SpMV: the sweep's waves take them after their runs (bit 26 of the "ell" knob: a launch
// of their own); split SpMV: part 1 = the sweep alone (it reads no ghost column), part 2 = the other rows in a launch of their own.
int mfem_sym_launch(mfem_context_s* ctx, mfem_csr_s* A, DiaKernel k, const SpmvArgs& a) {
  const DiaOffsets* O = (const DiaOffsets*)A->dia_dev;
  int np = 0;
  if (k == DIA_SYM27) {
    int64_t nsteps = 0;
    const int gs = sym27_grid(ctx, A, &nsteps);
    const int64_t outside = (A->n + SYM_ROWS - 1) / SYM_ROWS - (A->sym_c1 - A->sym_c0);
    np = a.part.part == 2 ? (int)(outside < 1 ? 1 : outside < 512 ? outside : 512) : gs;
    hipLaunchKernelGGL(k_spmv_sym27, dim3(np), dim3(SYM_THREADS), 0, ctx->stream, A->n, A->ell_npad, A->ell_K, O, A->dia_flags, A->ell_cols, A->ell_vals,
                       a.x, a.y, a.alpha, a.beta, a.dotw, a.partials, a.done_flag, A->sym_c0, A->sym_c1, A->sym_S, (int)nsteps, A->sym_cls, gs, a.part.part);
    MFEM_CHECK_LAUNCH();
  } else {
    const SympGeom G = mfem_symp_geom(ctx, A);
    const int64_t lo = (int64_t)G.p0 * G.PL, hi = (int64_t)G.p1 * G.PL;
    SympTail tl{};
    if (a.part.part == 0 && g_ell.symp_tail) tl = SympTail{1, A->ell_K, G.rim_units > 0, A->n, A->ell_npad, lo, hi, O, A->dia_flags, A->ell_cols, A->ell_vals};
    if (a.part.part != 2) {
      const int grid = symp_grid(ctx, A), nruns = G.NR * G.NPk * G.nseg;
      // partial sums per run or per workgroup (sps_per_run: the geometry and the launches that follow alone decide, so the stored and the constant form
      // agree); the bind's schedule where it applies to this grid, else the arithmetic form
      const int nruns_pr = sps_per_run(nruns, grid, tl.on ? 0 : SPS_OUTSIDE_RESERVE) ? nruns : 0;
      const int32_t* sched = nruns_pr && A->symp_CS && A->symp_sched && A->symp_sched_grid == grid ? A->symp_sched : nullptr;
      np = nruns_pr + grid;
      if (A->symp_CS) {
        SympConst cst{};
        memcpy(cst.v, A->symp_cst, sizeof(cst.v));
        cst.code = A->symp_ccode;
        cst.valid = 1;
        hipLaunchKernelGGL(sched ? symp_const_kernel<1>(G) : symp_const_kernel<0>(G), dim3(grid), dim3(64), 0, ctx->stream, G, (const double*)A->symp_vals, a.x, a.y, a.alpha, a.beta, a.dotw,
                           a.partials, a.done_flag, tl, cst, (const uint32_t*)mfem_symp_flags_of(A->symp_vals, G), sched, nruns_pr);
      } else {
        hipLaunchKernelGGL(symp_kernel<0>(G), dim3(grid), dim3(64), 0, ctx->stream, G, (const double*)A->symp_vals, a.x, a.y, a.alpha, a.beta, a.dotw,
                           a.partials, a.done_flag, (int32_t*)nullptr, tl, nruns_pr);
      }
      MFEM_CHECK_LAUNCH();
    }
    if (a.part.part == 2 || (a.part.part == 0 && !tl.on)) {
      int go = 0;
      const int rc = mfem_dia_launch_outside(ctx, A, a, a.partials ? a.partials + np : nullptr, lo, hi, &go);
      if (rc) return rc;
      np += go;
      if (G.rim_units > 0) {  // the rim rows of the swept planes: no ghost column, but one launch with the other rows the sweep leaves out
        const int gr = (int)(G.rim_units < SYMP_RIM_GRID ? G.rim_units : SYMP_RIM_GRID);
        hipLaunchKernelGGL(k_symp_rim, dim3(gr), dim3(64), 0, ctx->stream, G, (const double*)A->symp_vals + (int64_t)G.NR * G.NPk * (G.p1 - G.p0) * sp_step(G.B, G.DC),
                           a.x, a.y, a.alpha, a.beta, a.dotw, a.partials ? a.partials + np : nullptr, a.done_flag);
        MFEM_CHECK_LAUNCH();
        np += gr;
      }
    }
  }
  if (a.n_partials && a.partials) *a.n_partials = np;
  return MFEM_OK;
}
