// CPU walk through every branch of the two host decisions of mfem_solve's driver (csrc/solve_decide.h): what the workspace placement trial does with
// a candidate's time, and how the recheck of a tile solve on the caller's CSR values tightens the next pass.  The expected steps and factors are worked
// out here from the rules themselves (a candidate 5 % faster has found the fast kind; shrink = min(1/2, tol / 2 res) * min(tile_res / tol, 1), floor 1e-3).
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_solve.cpp -o tools/bin/host_check_solve && tools/bin/host_check_solve
#include <cmath>
#include <cstdio>
#include "solve_decide.h"

static int bad = 0;
static void trial(int tried, float ms, float best_ms, WsTrialStep want, const char* what) {
  const WsTrialStep got = ws_trial_decide(tried, ms, best_ms);
  if (got != want) { printf("trial, %s (tried %d, %.3f ms against %.3f ms): step %d, expected %d\n", what, tried, ms, best_ms, (int)got, (int)want); ++bad; }
}
static void recheck(double tile_res, double csr_res, double prev, double factor, bool stop, double want_factor, double want_prev, const char* what) {
  const double tol = 1e-8;
  const RecheckStep t = recheck_tighten(tol, tile_res, csr_res, prev, factor);
  if (t.stop != stop || !(t.tol_factor == want_factor) || !(t.prev_csr_res == want_prev)) {
    printf("recheck, %s: stop %d factor %.17g previous %.17g, expected %d %.17g %.17g\n", what, (int)t.stop, t.tol_factor, t.prev_csr_res, (int)stop, want_factor, want_prev);
    ++bad;
  }
}

int main() {
  trial(0, 8.0f, 0.0f, WS_ALLOC_FIRST, "first candidate");
  for (int tried = 1; tried <= 2; ++tried) {
    trial(tried, 7.0f, 8.0f, WS_KEEP, "clearly faster");  // 7.0 < 0.95 * 8.0 = 7.6
    trial(tried, 8.0f, 7.0f, WS_BACK, "clearly slower");  // 7.0 < 0.95 * 8.0
  }
  trial(1, 7.8f, 8.0f, WS_SWAP_ALLOC_NEXT, "alike, the current one better, a candidate left");  // 7.8 >= 7.6 and 8.0 >= 0.95 * 7.8 = 7.41
  trial(1, 8.0f, 7.8f, WS_ALLOC_NEXT, "alike, the alternative better, a candidate left");
  trial(1, 8.0f, 8.0f, WS_ALLOC_NEXT, "equal, a candidate left");
  trial(2, 7.8f, 8.0f, WS_KEEP, "alike, the current one better, last candidate");
  trial(2, 8.0f, 7.8f, WS_BACK, "alike, the alternative better, last candidate");
  trial(2, 8.0f, 8.0f, WS_KEEP, "equal, last candidate");
  trial(2, 0.95f * 8.0f, 8.0f, WS_KEEP, "exactly on the 5 % line: alike");  // (not strictly below it)

  const double tol = 1e-8;
  recheck(0.9e-8, 0.95e-8, -1.0, 1.0, false, 1.0, -1.0, "below the tolerance: nothing changes");
  recheck(0.9e-8, 0.95e-8, 1.2e-8, 0.25, false, 0.25, 1.2e-8, "below the tolerance after a tightened pass: nothing changes");
  // above: the residual 10 % over the tolerance, the tiles' 10 % under it -> (1/2) (tol / res) (tile_res / tol), about 0.409
  const double s1 = fmin(0.5, 0.5 * tol / 1.1e-8) * fmin(0.9e-8 / tol, 1.0);
  if (!(fabs(s1 - 0.45 / 1.1) < 1e-15)) { printf("recheck: the worked factor %.17g is not 0.45 / 1.1\n", s1); ++bad; }
  recheck(0.9e-8, 1.1e-8, -1.0, 1.0, false, s1, 1.1e-8, "above, first recheck");
  recheck(0.9e-8, 1.1e-8, 2.0e-8, 0.5, false, 0.5 * s1, 1.1e-8, "above with progress since the previous recheck: the factors compound");
  recheck(0.9e-8, 1.1e-8, 2.0e-8, 3.0, false, s1, 1.1e-8, "a factor above 1 counts as 1");
  recheck(0.9e-8, 1.85e-8, 2.0e-8, 0.5, true, 0.5, 2.0e-8, "above without progress (not below 0.9 of the previous): the passes end");
  recheck(0.9e-8, 0.9 * 2.0e-8, 2.0e-8, 0.5, true, 0.5, 2.0e-8, "exactly 0.9 of the previous: the passes end");
  recheck(1e-12, 1.1e-8, -1.0, 1.0, false, 1e-3, 1.1e-8, "the floor: (0.45 / 1.1) * 1e-4 is below 1e-3");
  recheck(0.9e-8, 1.1e-8, 2.0e-8, 2e-3, false, 1e-3, 1.1e-8, "the floor, by compounding");
  recheck(0.0, 1.1e-8, -1.0, 1.0, false, fmin(0.5, 0.5 * tol / 1.1e-8), 1.1e-8, "tile_res = 0: its margin drops out");
  recheck(0.9e-8, 4e-8, -1.0, 1.0, false, (0.5 * tol / 4e-8) * (0.9e-8 / tol), 4e-8, "far above: tol / 2 res, below the factor two");
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
