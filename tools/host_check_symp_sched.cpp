// CPU replay of csrc/symp_sched_decide.h (tests/test_symp_sched_decide.py): the schedule of the constant form's runs, the XCD shares, the identity schedule
// against the sweep's own arithmetic, the model makespans and the partial-sum rule.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_symp_sched.cpp -o host_check_symp_sched && ./host_check_symp_sched
#include <cstdio>
#include <vector>

#include "symp_sched_decide.h"
#include "symp_trim_decide.h"

static int fails = 0;
#define CHECK(c, ...)            \
  do {                           \
    if (!(c)) {                  \
      ++fails;                   \
      printf("FAIL %s: ", #c);   \
      printf(__VA_ARGS__);       \
      printf("\n");              \
    }                            \
  } while (0)

struct Lattice {
  const char* name;
  int planes, m1, m2, p0, p1, B, grid_cap;  // lattice, swept planes [p0, p1), bands, cap on the grid (0: the resident slots of 256 CUs)
};
struct Table {
  std::vector<int32_t> offset, run;
  std::vector<int64_t> load;
  int32_t first[9];
};

// flags by spc_expected's predicate: whole patches with lines and points in [2, m - 3], planes in [2, planes - 3]
static void geometry(const Lattice& L, SpsGeom& g, std::vector<int32_t>& flagged) {
  const int ms1 = spt_ms1(L.m1, L.B), ms2 = spt_ms2(L.m2), NR = spt_rows(ms1, L.B), NPk = spt_cols(ms2), NP = NR * NPk, nplanes = L.p1 - L.p0;
  const int slots = sp_wg_per_cu(L.B) * 256;
  const int nseg = spt_nseg(NP, slots, nplanes);
  int64_t grid = 8 * (((int64_t)NP + 7) / 8) * nseg, cap = slots;
  if (L.grid_cap > 0 && cap > L.grid_cap) cap = L.grid_cap;
  cap &= ~(int64_t)7;
  if (grid > cap) grid = cap;
  if (grid < 8) grid = 8;
  g = SpsGeom{NP, NPk, nseg, nplanes, (int)grid};
  std::vector<unsigned char> fl((size_t)NP * nplanes, 0);
  const int Ll = SP_L * L.B;
  int64_t count = 0;
  for (int pl = 0; pl < nplanes; ++pl)
    for (int patch = 0; patch < NP; ++patch) {
      const int j0 = (patch / NPk) * Ll, k0 = (patch % NPk) * SP_W, p = L.p0 + pl;
      const bool f = j0 + Ll <= ms1 && j0 >= 2 && j0 + Ll - 1 <= L.m1 - 3 && k0 + SP_W <= ms2 && k0 >= 2 && k0 + SP_W - 1 <= L.m2 - 3 && p >= 2 && p <= L.planes - 3;
      fl[(size_t)pl * NP + patch] = f;
      count += f;
    }
  CHECK(count == spc_expected(L.planes, L.m1, L.m2, L.p0, L.p1, ms1, ms2, L.B), "%s: %lld flagged steps", L.name, (long long)count);
  flagged.assign((size_t)sps_nruns(g), 0);
  int64_t sum = 0;
  for (int patch = 0; patch < NP; ++patch)
    for (int s = 0; s < nseg; ++s) sum += flagged[(size_t)sps_run_id(patch, s, nseg)] = sps_run_flagged(g, fl.data(), patch, s);
  CHECK(sum == count, "%s: the runs hold %lld of %lld flagged steps", L.name, (long long)sum, (long long)count);
}
static Table build(const SpsGeom& g, const std::vector<int32_t>& flagged, int mode, uint64_t seed) {
  Table T;
  T.offset.assign((size_t)g.grid + 1, -1);
  T.run.assign((size_t)sps_nruns(g), -1);
  T.load.assign((size_t)g.grid, -1);
  std::vector<int32_t> work(2 * (size_t)sps_nruns(g) + g.grid);
  sps_build(g, flagged.data(), mode, seed, T.offset.data(), T.run.data(), T.first, T.load.data(), work.data());
  return T;
}
// a table is a schedule: every run once, every list inside its XCD's patch range, the ranges contiguous and covering, the loads the lists' costs
static void check_table(const char* name, const SpsGeom& g, const std::vector<int32_t>& flagged, const Table& T, int mode) {
  const int nruns = sps_nruns(g);
  CHECK(T.first[0] == 0 && T.first[8] == g.NP, "%s mode %d: shares [%d, %d)", name, mode, T.first[0], T.first[8]);
  for (int c = 0; c < 8; ++c) CHECK(T.first[c] <= T.first[c + 1], "%s mode %d: share %d", name, mode, c);
  CHECK(T.offset[0] == 0 && T.offset[(size_t)g.grid] == nruns, "%s mode %d: offsets %d .. %d", name, mode, T.offset[0], T.offset[(size_t)g.grid]);
  std::vector<int> seen((size_t)nruns, 0);
  for (int w = 0; w < g.grid; ++w) {
    CHECK(T.offset[(size_t)w] <= T.offset[(size_t)w + 1], "%s mode %d: offset %d", name, mode, w);
    int64_t load = 0;
    for (int i = T.offset[(size_t)w]; i < T.offset[(size_t)w + 1]; ++i) {
      const int r = T.run[(size_t)i];
      if (r < 0 || r >= nruns) {
        CHECK(false, "%s mode %d: entry %d = %d", name, mode, i, r);
        continue;
      }
      ++seen[(size_t)r];
      const int patch = r / g.nseg;
      CHECK(patch >= T.first[w & 7] && patch < T.first[(w & 7) + 1], "%s mode %d: workgroup %d (XCD %d) sweeps patch %d", name, mode, w, w & 7, patch);
      load += sps_cost_of(g, flagged.data(), r);
    }
    CHECK(load == T.load[(size_t)w], "%s mode %d: load of workgroup %d", name, mode, w);
  }
  for (int r = 0; r < nruns; ++r) CHECK(seen[(size_t)r] == 1, "%s mode %d: run %d taken %d times", name, mode, r, seen[(size_t)r]);
}

int main() {
  const Lattice lattices[] = {
      {"512^3", 513, 513, 513, 2, 511, 2, 0},          // 64 x 16 patches, 509 swept planes, 3 runs per patch, 96 waves per XCD
      {"256^3", 257, 257, 257, 2, 255, 1, 0},          // 64 x 8 patches, 253 planes, 7 runs per patch: too many for per-run sums
      {"(17, 33, 129) B2", 17, 33, 129, 2, 15, 2, 8},  // the GPU tests' fixtures under their grid cap of 8
      {"(17, 33, 129) B1", 17, 33, 129, 2, 15, 1, 8},
      {"(49, 33, 129) B2", 49, 33, 129, 2, 47, 2, 8},
      {"(49, 33, 129) B1", 49, 33, 129, 2, 47, 1, 8},
      {"(49, 33, 129) B2 uncapped", 49, 33, 129, 2, 47, 2, 0},
      {"(17, 65, 1089) B1", 17, 65, 1089, 2, 15, 1, 8},  // 16 x 34 patches on 8 workgroups: lists of more than 64 runs
  };
  for (const Lattice& L : lattices) {
    SpsGeom g{};
    std::vector<int32_t> flagged;
    geometry(L, g, flagged);
    const int W = g.grid / 8, nruns = sps_nruns(g);
    printf("%s: %d patches (%d columns) x %d runs, %d planes, grid %d\n", L.name, g.NP, g.NPk, g.nseg, g.nplanes, g.grid);
    const Table A = build(g, flagged, SPS_AUTO, 0), I = build(g, flagged, SPS_IDENTITY, 0), R1 = build(g, flagged, SPS_RANDOM, 1), R2 = build(g, flagged, SPS_RANDOM, 2);
    check_table(L.name, g, flagged, A, SPS_AUTO);
    check_table(L.name, g, flagged, I, SPS_IDENTITY);
    check_table(L.name, g, flagged, R1, SPS_RANDOM);
    check_table(L.name, g, flagged, R2, SPS_RANDOM);
    // a pure function of its inputs
    const Table A2 = build(g, flagged, SPS_AUTO, 0), R1b = build(g, flagged, SPS_RANDOM, 1);
    CHECK(A.offset == A2.offset && A.run == A2.run && A.load == A2.load, "%s: the table differs when built twice", L.name);
    CHECK(R1.offset == R1b.offset && R1.run == R1b.run, "%s: the seeded table differs when built twice", L.name);
    if (nruns > 8) CHECK(R1.run != R2.run || R1.offset != R2.offset, "%s: two seeds, one assignment", L.name);
    // the identity schedule is the sweep's arithmetic form (spmv_sym.hip), restated: XCD shares pc (+ 1 for the first NP % 8), round loop, spc_run
    {
      size_t n = 0;
      bool same = true;
      for (int w = 0; w < g.grid; ++w) {
        const int xcd = w & 7, jw = w >> 3, pc = g.NP / 8, prem = g.NP % 8, pcnt = pc + (xcd < prem ? 1 : 0), pfirst = xcd * pc + (xcd < prem ? xcd : prem);
        same = same && I.offset[(size_t)w] == (int)n;
        for (int rk = 0; W * rk < pcnt * g.nseg; ++rk) {
          const int run = spc_run(W, jw, rk, spc_rot(g.NPk));
          if (run >= pcnt * g.nseg) continue;
          const int patch = pfirst + run % pcnt, seg = run / pcnt;
          same = same && n < I.run.size() && I.run[n] == patch * g.nseg + seg;
          ++n;
        }
      }
      CHECK(same && (int)n == nruns, "%s: the identity table is not the sweep's arithmetic (%zu runs)", L.name, n);
    }
    // the model makespan of the schedule, per XCD, against the LPT bound (4/3 - 1/(3 W)) x max(mean load, costliest run) -- in integers, times 3 W^2
    for (int c = 0; c < 8; ++c) {
      int64_t total = 0, top = 0, span = 0;
      for (int r = A.first[c] * g.nseg; r < A.first[c + 1] * g.nseg; ++r) {
        const int64_t cr = sps_cost_of(g, flagged.data(), r);
        total += cr;
        top = cr > top ? cr : top;
      }
      for (int jw = 0; jw < W; ++jw) span = A.load[(size_t)(8 * jw + c)] > span ? A.load[(size_t)(8 * jw + c)] : span;
      const int64_t lower_w = total > top * W ? total : top * W;  // W x max(mean, costliest)
      // span <= (4 W - 1) / (3 W) x lower_w / W, in 128-bit integers (span x 3 W^2 passes 2^63 from a few thousand waves on)
      CHECK((__int128)span * 3 * W * W <= (__int128)(4 * W - 1) * lower_w, "%s XCD %d: makespan %lld, total %lld, costliest %lld, W %d", L.name, c, (long long)span,
            (long long)total, (long long)top, W);
    }
    const int64_t ma = sps_makespan(g, A.load.data()), mi = sps_makespan(g, I.load.data());
    int64_t total = 0;
    for (int r = 0; r < nruns; ++r) total += sps_cost_of(g, flagged.data(), r);
    printf("  model makespan: schedule %.4f ms, identity %.4f ms (ratio %.3f), perfect balance %.4f ms\n", (double)ma * 1e-9, (double)mi * 1e-9, (double)ma / (double)mi,
           (double)total / g.grid * 1e-9);
    if (L.planes == 513) {
      CHECK(g.NP == 1024 && g.NPk == 16 && g.nseg == 3 && g.nplanes == 509 && g.grid == 768, "the headline's geometry");
      // With the constants the issue fitted (CF = 1.4 us) the ratio was 0.61; the per-run clocks gave CF = 2.4 us (profiles/r13_symp_sched_ab_512.txt), and
      // with whole runs of 830 or 408 us the best any assignment can do above the mean load of 1.89 ms is five flagged runs, 2.04 ms: 0.83 of the identity
      // schedule's 2.48 ms is what the header yields, within 1 % of that optimum
      CHECK(ma * 1000 <= mi * 830, "512^3: schedule %lld ps against identity %lld ps", (long long)ma, (long long)mi);
      CHECK(ma * 100 <= (total / g.grid) * 110, "512^3: schedule %lld ps against perfect balance %lld ps", (long long)ma, (long long)(total / g.grid));
      CHECK(sps_per_run(nruns, g.grid, 0) && sps_partials(nruns, g.grid, 0) == 3072 + 768, "512^3 unsplit must fit");
      CHECK(!sps_per_run(nruns, g.grid, SPS_OUTSIDE_RESERVE) && sps_partials(nruns, g.grid, SPS_OUTSIDE_RESERVE) == 768, "512^3 with the launches behind it does not fit");
    }
    if (L.planes == 257) {
      CHECK(g.nseg == 7 && g.grid == 1792, "256^3: %d runs per patch, grid %d", g.nseg, g.grid);
      CHECK(!sps_per_run(nruns, g.grid, 0) && sps_partials(nruns, g.grid, 0) == g.grid, "256^3: 3584 runs + 1792 workgroups do not fit: per workgroup");
      CHECK(sps_kind(true, sps_per_run(nruns, g.grid, 0), SPS_AUTO) == 0, "256^3: no schedule without per-run sums");
    }
    if (L.grid_cap == 8) {
      CHECK(g.grid == 8 && nruns >= 16, "%s: %d runs on %d workgroups", L.name, nruns, g.grid);
      CHECK(sps_per_run(nruns, g.grid, 0) && sps_per_run(nruns, g.grid, SPS_OUTSIDE_RESERVE), "%s: per-run sums either way", L.name);
    }
    if (L.m2 == 1089) {
      int longest = 0;
      for (int w = 0; w < g.grid; ++w) longest = A.offset[(size_t)w + 1] - A.offset[(size_t)w] > longest ? A.offset[(size_t)w + 1] - A.offset[(size_t)w] : longest;
      CHECK(nruns == 544 && longest > 64, "%s: %d runs, longest list %d", L.name, nruns, longest);
    }
    if (L.planes == 49) CHECK(g.nseg >= 2, "%s: %d runs per patch", L.name, g.nseg);
  }
  // ---- the gate and the rule
  CHECK(sps_kind(false, true, SPS_AUTO) == 0 && sps_kind(false, true, SPS_RANDOM) == 0, "the stored form keeps the arithmetic form");
  CHECK(sps_kind(true, true, SPS_IDENTITY) == 0 && sps_kind(true, false, SPS_AUTO) == 0, "the identity mode; no per-run sums");
  CHECK(sps_kind(true, true, SPS_AUTO) == 1 && sps_kind(true, true, SPS_RANDOM) == SPS_RANDOM && sps_kind(true, true, 77) == 1, "modes");
  CHECK(!sps_per_run(0, 8, 0) && sps_per_run(4088, 8, 0) && !sps_per_run(4089, 8, 0), "the rule's ends");
  CHECK(sps_run_cost(0, 0) == SPS_CS0_PS && sps_run_cost(2, 3) == 2 * (int64_t)SPS_CU_PS + 3 * (int64_t)SPS_CF_PS + SPS_CS0_PS, "cost");
  CHECK(SPS_CU_PS > SPS_CF_PS && SPS_CF_PS > 0 && SPS_CS0_PS >= 0, "constants");
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
