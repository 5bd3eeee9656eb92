// Which wave of the patch sweep (spmv_sym.hip: k_spmv_symp_const<B, DC, SCH>) sweeps which run, decided once per bind, and where the p . Ap partial sums of a
// product go.  Integer arithmetic alone, host + device, no HIP: tools/host_check_symp_sched.cpp replays it on the CPU (tests/test_symp_sched_decide.py).
//
// A run = one patch through the planes [nplanes seg / nseg, nplanes (seg + 1) / nseg) of the swept range (the cut: spt_nseg, symp_trim_decide.h), numbered
// run id = patch * nseg + seg: a function of the geometry alone.  In the constant form (symp_const_decide.h) a flagged step is ~450 instructions and an
// unflagged one ~2500, a wave has its SIMD to itself, and the launch ends when the slowest wave ends: equal counts of runs per wave (the identity schedule:
// equal XCD shares and spc_run) leave the waves that meet the never-flagged first / last patch column and row one or two slow runs behind the others.
//   * Partial sums per RUN (sps_per_run): the wave reduces its p . Ap sum at the end of every run and stores it at partials[run id]; the tail and rim units a
//     wave takes after its runs keep one sum per workgroup, behind the runs'.  The sums then do not depend on which wave swept what: every schedule gives the
//     same bytes, and the stored and the constant form of one geometry agree whatever the schedule.
//   * The schedule (sps_build, mode SPS_AUTO): XCD c -- the workgroups with blockIdx % 8 == c -- takes a contiguous range of patches in patch order, cut where the
//     prefix sum of the patch costs crosses c / 8 of the total (neighbouring patches still advance through the planes on one L2); inside the XCD the runs go,
//     costliest first, each to the wave with the least load so far (longest processing time first: makespan <= (4/3 - 1/(3 W)) x optimum).  Ties break by run
//     id, then by wave: the table is a pure function of its inputs.
//   * The table: int32 offset[grid + 1], then run[nruns] -- workgroup g sweeps run[offset[g]] .. run[offset[g + 1] - 1] in that order.  Rebuilt at every
//     bind from the step flags (they follow the values); its place in the layout's buffer is fixed (behind the flags), so captured cycles stay valid.
// The gate (sps_kind): the constant form with per-run sums only.  The stored form's steps all cost the same and the identity schedule is balanced there;
// it keeps the arithmetic form (no table) in either kernel.
#pragma once
#include <stdint.h>

#include "symp_const_decide.h"

// ---- the cost of a run, picoseconds: steps x their cost + a start (the first step has no history: nine low slots per row, the x ring, the requests).
// Measured per run with wall_clock64() stamps at run start and end (tools/symp_sched_probe.py on a build with -DSYMP_SCHED_CLOCKS; never
// in the shipped library) over the 3072 runs of a 512^3 product, B = 2, coded diagonal: the 468 never-flagged runs of 169 / 170 steps take 813 - 855 us
// (mean per segment), the 2604 wholly flagged ones 398 - 411 us; least squares over all runs gives CU = 4.96 / 4.97 us and CF = 2.35 / 2.40 us under the
// identity / the cost schedule, rounded here (profiles/r13_symp_sched_ab_512.txt).  Every run there has 169 or 170 steps, so a start cost cannot
// be told from the per-step costs: it is carried by them (1 / 170 of it each) and CS0 stays 0 until a geometry with runs of different lengths is measured.
// The 1.4 us per flagged step fitted to the launch time before the clocks existed was too low: a flagged step's ~450 instructions wait for its x loads.
#define SPS_CU_PS 4900000   // an unflagged step under CS = 1
#define SPS_CF_PS 2400000   // a flagged step
#define SPS_CS0_PS 0        // a run's start
__host__ __device__ constexpr int64_t sps_run_cost(int64_t unflagged, int64_t flagged) { return unflagged * SPS_CU_PS + flagged * SPS_CF_PS + SPS_CS0_PS; }

// ---- runs
__host__ __device__ constexpr int sps_run_id(int patch, int seg, int nseg) { return patch * nseg + seg; }
__host__ __device__ constexpr int sps_plane_lo(int nplanes, int seg, int nseg) { return (int)((int64_t)nplanes * seg / nseg); }  // first plane (from p0) of segment seg

// ---- partial sums.  Per run when the runs' sums, the workgroups' (tail and rim units) and the reserve for the launches that follow the sweep -- the boundary
// part of a split SpMV, or the rows outside the swept planes with bit 26 of the "ell" knob, and the rim launch -- fit one partial-sum array; else per
// workgroup, with the identity schedule, as before.  512^3 unsplit: 3072 + 768 + 0 <= 4096.
#define SPS_MAX_PARTIALS 4096   // (= MFEM_MAX_PARTIALS: spmv_sym.hip asserts it)
#define SPS_OUTSIDE_RESERVE 1280  // partial sums of the launches behind a sweep that does not take the other rows itself: 1024 + the rim launch's 256
__host__ __device__ constexpr bool sps_per_run(int64_t nruns, int64_t grid, int64_t reserve) { return nruns > 0 && nruns + grid + reserve <= SPS_MAX_PARTIALS; }
__host__ __device__ constexpr int sps_partials(int64_t nruns, int64_t grid, int64_t reserve) { return (int)(sps_per_run(nruns, grid, reserve) ? nruns + grid : grid); }
// doubles the table takes in the layout's buffer at the most (per-run sums bound its length)
#define SPS_TABLE_DOUBLES ((2 * SPS_MAX_PARTIALS + 2) / 2)

// ---- the knob (mfem_debug_set("symp_sched", mode | seed << 8, grid cap)) and the gate
enum { SPS_AUTO = 0, SPS_IDENTITY = 1, SPS_RANDOM = 2 };
// what a bind's products run: 0 = the arithmetic form (equal shares, spc_run; no table), else the table of that mode
__host__ __device__ constexpr int sps_kind(bool constant_form, bool per_run, int mode) {
  return !constant_form || !per_run || mode == SPS_IDENTITY ? 0 : mode == SPS_RANDOM ? SPS_RANDOM : 1;
}

// ---- the identity schedule: XCD c owns the patches [sps_eq_first(c), sps_eq_first(c + 1)), and in round rk wave jw of its W waves takes the run
// spc_run(W, jw, rk, rot) of its list (segment-major: run = seg * pcnt + patch - first) -- what the sweep computes without a table
__host__ __device__ constexpr int sps_eq_first(int NP, int c) { return c * (NP / 8) + (c < NP % 8 ? c : NP % 8); }
__host__ __device__ inline bool sps_identity_run(int NP, int NPk, int nseg, int W, int xcd, int jw, int rk, int& patch, int& seg) {
  const int first = sps_eq_first(NP, xcd), pcnt = sps_eq_first(NP, xcd + 1) - first;
  const int run = spc_run(W, jw, rk, spc_rot(NPk));
  if (run >= pcnt * nseg) return false;
  patch = first + run % pcnt;
  seg = run / pcnt;
  return true;
}
__host__ __device__ constexpr int sps_identity_rounds(int NP, int nseg, int W, int xcd) {
  return ((sps_eq_first(NP, xcd + 1) - sps_eq_first(NP, xcd)) * nseg + W - 1) / W;
}

struct SpsGeom {
  int NP, NPk;   // patches per plane, patch columns
  int nseg;      // runs per patch
  int nplanes;   // swept planes
  int grid;      // one-wave workgroups of the sweep: a multiple of 8, workgroup g on XCD g % 8 as wave g / 8 of W = grid / 8
};
__host__ __device__ constexpr int sps_nruns(const SpsGeom& g) { return g.NP * g.nseg; }
__host__ __device__ constexpr int sps_run_steps(const SpsGeom& g, int seg) { return sps_plane_lo(g.nplanes, seg + 1, g.nseg) - sps_plane_lo(g.nplanes, seg, g.nseg); }
// flagged steps of run (patch, seg) from the step flags, one byte per step [plane][patch]
__host__ __device__ inline int sps_run_flagged(const SpsGeom& g, const unsigned char* sflags, int patch, int seg) {
  int f = 0;
  for (int pl = sps_plane_lo(g.nplanes, seg, g.nseg); pl < sps_plane_lo(g.nplanes, seg + 1, g.nseg); ++pl) f += sflags[(int64_t)pl * g.NP + patch] != 0;
  return f;
}
__host__ __device__ inline int64_t sps_cost_of(const SpsGeom& g, const int32_t* flagged, int run) {
  const int steps = sps_run_steps(g, run % g.nseg);
  return sps_run_cost(steps - flagged[run], flagged[run]);
}

// ---- XCD shares by cost: first[0..8], first[c] = the first patch of XCD c -- the patch after the one at which the prefix sum of the patch costs reaches
// c / 8 of the total (a lattice of few patches may leave a share empty)
__host__ __device__ inline void sps_shares(const SpsGeom& g, const int32_t* flagged, int32_t* first) {
  int64_t tot = 0, acc = 0;
  for (int r = 0; r < sps_nruns(g); ++r) tot += sps_cost_of(g, flagged, r);
  int k = 1;
  first[0] = 0;
  for (int p = 0; p < g.NP; ++p) {
    for (int s = 0; s < g.nseg; ++s) acc += sps_cost_of(g, flagged, sps_run_id(p, s, g.nseg));
    while (k < 8 && acc * 8 >= tot * k) first[k++] = p + 1;
  }
  while (k <= 8) first[k++] = g.NP;
}
__host__ __device__ constexpr uint64_t sps_mix(uint64_t z) {  // splitmix64's finaliser: the pseudo-random assignment of SPS_RANDOM
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// a list is walked by descending key: the run's cost (ties keep the run order), SPS_RANDOM: a second pseudo-random number (a one-wave XCD still permutes)
__host__ __device__ inline uint64_t sps_list_key(const SpsGeom& g, const int32_t* flagged, int mode, uint64_t seed, int run) {
  return mode == SPS_RANDOM ? sps_mix(~seed * 0x9E3779B97F4A7C15ull + (uint64_t)run) : (uint64_t)sps_cost_of(g, flagged, run);
}

// ---- THE table.  mode: SPS_AUTO cost-cut shares + longest processing time first; SPS_IDENTITY equal shares + spc_run, as the arithmetic form walks them;
// SPS_RANDOM the cost-cut shares with run r on wave sps_mix(seed, r) % W of its XCD, in a pseudo-random order.  flagged[run id]: flagged steps of the run.
// Out: offset[grid + 1], run[nruns], first[9] (the shares), load[grid] (model cost of every workgroup's list, ps).  work: 2 * nruns + grid int32 of scratch.
__host__ __device__ inline void sps_build(const SpsGeom& g, const int32_t* flagged, int mode, uint64_t seed, int32_t* offset, int32_t* run, int32_t* first,
                                          int64_t* load, int32_t* work) {
  const int W = g.grid / 8, nruns = sps_nruns(g);
  int32_t* wave_of = work;        // run id -> workgroup
  int32_t* order = work + nruns;  // the runs of one XCD in assignment order
  int32_t* cursor = work + 2 * nruns;  // per workgroup: where its next run goes
  for (int w = 0; w < g.grid; ++w) load[w] = 0;
  for (int w = 0; w <= g.grid; ++w) offset[w] = 0;
  if (mode == SPS_IDENTITY) {
    for (int c = 0; c <= 8; ++c) first[c] = sps_eq_first(g.NP, c);
    int n = 0;
    for (int w = 0; w < g.grid; ++w) {  // (lists in workgroup order, each in round order)
      offset[w] = n;
      for (int rk = 0; rk < sps_identity_rounds(g.NP, g.nseg, W, w & 7); ++rk) {
        int patch = 0, seg = 0;
        if (!sps_identity_run(g.NP, g.NPk, g.nseg, W, w & 7, w >> 3, rk, patch, seg)) continue;
        run[n] = sps_run_id(patch, seg, g.nseg);
        load[w] += sps_cost_of(g, flagged, run[n]);
        ++n;
      }
    }
    offset[g.grid] = n;
    return;
  }
  sps_shares(g, flagged, first);
  for (int c = 0; c < 8; ++c) {
    const int r0 = first[c] * g.nseg, r1 = first[c + 1] * g.nseg, n = r1 - r0;  // the XCD's runs: a contiguous range of run ids
    if (mode == SPS_RANDOM) {
      for (int r = r0; r < r1; ++r) {
        const int w = 8 * (int)(sps_mix(seed * 0x9E3779B97F4A7C15ull + (uint64_t)r + 1) % (uint64_t)W) + c;
        wave_of[r] = w;
        load[w] += sps_cost_of(g, flagged, r);
      }
      continue;
    }
    // costliest first, ties by run id: a stable insertion into descending order (a share holds a few hundred runs)
    for (int i = 0; i < n; ++i) {
      const int r = r0 + i;
      const int64_t cr = sps_cost_of(g, flagged, r);
      int j = i;
      while (j > 0 && sps_cost_of(g, flagged, order[j - 1]) < cr) {
        order[j] = order[j - 1];
        --j;
      }
      order[j] = r;
    }
    for (int i = 0; i < n; ++i) {  // ... each to the least loaded wave, ties by wave
      int best = 0;
      for (int jw = 1; jw < W; ++jw)
        if (load[8 * jw + c] < load[8 * best + c]) best = jw;
      wave_of[order[i]] = 8 * best + c;
      load[8 * best + c] += sps_cost_of(g, flagged, order[i]);
    }
  }
  // the lists: per workgroup its runs in run order, then by descending key -- costliest first, ties by run id: the order they were given out in
  for (int r = 0; r < nruns; ++r) ++offset[wave_of[r] + 1];
  for (int w = 0; w < g.grid; ++w) {
    offset[w + 1] += offset[w];
    cursor[w] = offset[w];
  }
  for (int r = 0; r < nruns; ++r) run[cursor[wave_of[r]]++] = r;
  for (int w = 0; w < g.grid; ++w)
    for (int i = offset[w] + 1; i < offset[w + 1]; ++i) {
      const int r = run[i];
      const uint64_t kr = sps_list_key(g, flagged, mode, seed, r);
      int j = i;
      while (j > offset[w] && sps_list_key(g, flagged, mode, seed, run[j - 1]) < kr) {
        run[j] = run[j - 1];
        --j;
      }
      run[j] = r;
    }
}
// model makespan of a table: the largest workgroup load
__host__ __device__ inline int64_t sps_makespan(const SpsGeom& g, const int64_t* load) {
  int64_t m = 0;
  for (int w = 0; w < g.grid; ++w) m = load[w] > m ? load[w] : m;
  return m;
}
