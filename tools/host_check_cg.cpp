// CPU walk through the host decisions of the classic CG pass about its ring of search directions (csrc/cg_decide.h): the depth at its threshold and at
// the knob's bounds, the slots and the pending updates over whole passes, the length of a captured cycle.  The ring's bookkeeping is replayed against
// the per-iteration update it stands for: every iteration's update of x is applied exactly once, in iteration order, wherever the pass ends.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_cg.cpp -o tools/bin/host_check_cg && tools/bin/host_check_cg
#include <cstdio>
#include <vector>
#include "cg_decide.h"

static int bad = 0;
static void depth(int64_t nv, int knob, int want, const char* what) {
  const int got = cg_ring_depth(nv, knob);
  if (got != want) { printf("depth, %s (nv %lld, knob %d): %d, expected %d\n", what, (long long)nv, knob, got, want); ++bad; }
}

int main() {
  // automatic: 1 below 4e7 rows (256^3 = 16 974 593 points: m = 1), 8 from there on (512^3 = 135 005 697)
  depth(0, 0, 1, "empty");
  depth(16974593, 0, 1, "256^3");
  depth(39999999, 0, 1, "one below the threshold");
  depth(40000000, 0, 8, "the threshold");
  depth(135005697, 0, 8, "512^3");
  // the knob: 1 .. 16 force, everything else is automatic
  depth(135005697, 1, 1, "forced off on a large system");
  depth(100, 2, 2, "forced on a small system");
  depth(100, 16, 16, "upper bound");
  depth(100, 17, 1, "above the upper bound: automatic");
  depth(40000000, 17, 8, "above the upper bound: automatic, large");
  depth(100, -1, 1, "negative: automatic");
  depth(40000000, -1, 8, "negative: automatic, large");

  for (int m = 1; m <= CG_RING_MAX; ++m) {
    const int unit = cg_ring_unit(m);
    // the least common multiple of the slots' and the banks' periods
    int lcm = m;
    while (lcm % 2) lcm += m;
    if (unit != lcm) { printf("unit of depth %d: %d, expected %d\n", m, unit, lcm); ++bad; }
    // a pass of `iters` iterations, replayed: slot[k] = the iteration whose direction slot k holds; applied[j] = how often x got iteration j's update
    for (int iters = 0; iters <= 3 * m + 3; ++iters) {
      std::vector<int> slot(m, -1), applied(iters, 0);
      std::vector<int> order;
      for (int it = 0; it < iters; ++it) {
        const int s = cg_ring_slot(it, m);
        if (slot[s] >= 0 && !applied[slot[s]]) { printf("depth %d: iteration %d overwrites the pending direction of iteration %d\n", m, it, slot[s]); ++bad; }
        slot[s] = it;
        if (s == m - 1)  // flush position: the m - 1 earlier slots in order, then this iteration's
          for (int k = 0; k < m; ++k) { ++applied[slot[k]]; order.push_back(slot[k]); }
      }
      const int pending = cg_ring_pending(iters, m);
      for (int k = 0; k < pending; ++k) { ++applied[slot[k]]; order.push_back(slot[k]); }  // k_cg_xflush
      for (int j = 0; j < iters; ++j)
        if (applied[j] != 1 || order[j] != j) { printf("depth %d, %d iterations: update %d applied %d times, position %d\n", m, iters, j, applied[j], order[j]); ++bad; break; }
    }
  }
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
