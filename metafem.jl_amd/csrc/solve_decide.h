// The two decisions of mfem_solve's driver (krylov.hip) that are host arithmetic alone: what the workspace placement trial does with a candidate's
// time, and how the recheck of a tile solve on the caller's CSR values tightens the next pass.  No HIP, no context: tools/host_check_solve.cpp walks
// every branch on the CPU.
#pragma once
#include <math.h>

// What the trial does after it has timed the current workspace candidate.  The driver performs it (mfem_ws_next_candidate / mfem_ws_decide).
enum WsTrialStep {
  WS_ALLOC_FIRST,      // first candidate: its time is the one to beat, it stays alive as the alternative; allocate a second and start over on it
  WS_KEEP,             // end of the trial: the current candidate stays
  WS_BACK,             // end of the trial: back to the alternative, start over on it
  WS_ALLOC_NEXT,       // alike: the current candidate is replaced by a new allocation, start over on it
  WS_SWAP_ALLOC_NEXT,  // alike, the current one a little better: it becomes the alternative (its time the one to beat) first, then as WS_ALLOC_NEXT
};
// The two speeds are 11 % apart: a candidate 5 % faster than another has found the fast kind.  Two alike (both fast, or both slow): one more
// candidate is tried (the current one freed first -- a new allocation does not come back to memory just freed, the probe's alternation).
static const float WS_FAST_KIND = 0.95f;
// tried: candidates allocated after the first (ctx->ws_try); ms: the current candidate's time; best_ms: the alternative's (unused while tried == 0)
static inline WsTrialStep ws_trial_decide(int tried, float ms, float best_ms) {
  if (tried == 0) return WS_ALLOC_FIRST;
  if (ms < WS_FAST_KIND * best_ms) return WS_KEEP;  // the current one is the fast kind
  if (best_ms < WS_FAST_KIND * ms) return WS_BACK;  // the alternative was: back to it
  if (tried < 2) return ms < best_ms ? WS_SWAP_ALLOC_NEXT : WS_ALLOC_NEXT;  // alike: the better of the two becomes the alternative, the other is replaced
  return ms <= best_ms ? WS_KEEP : WS_BACK;  // alike, and no further candidate: the faster of the two
}

// The recheck of a pass that the tiles' copy ended (tile_res below the tolerance) has recomputed the residual from the caller's CSR values: csr_res.  Below
// the tolerance too: nothing changes, the passes end converged.  Otherwise the two straddle the tolerance (they differ in the last digits: another
// summation order, the repaired rows): the next pass, which iterates on the tiles' copy, would find itself converged at once and the passes would run
// out with the caller's residual a hair above the tolerance (seen once in the 3-rank test's single-rank reference solve, round 5).  It iterates to a
// tighter tolerance instead: below the tiles' residual of this pass by the margin the caller's residual is above the tolerance, and at least a factor two.
//  the caller's residual can have a FLOOR above the tolerance -- a tight tolerance against the per-row symmetry gate of the tiles (LAT_SYM_GATE) --: the tiles' residual
// then keeps falling, the tightened tolerance compounds towards zero and every remaining pass burns its full maxiter.  If the caller's residual did not
// fall since the previous recheck that went on (prev_csr_res; <= 0: none yet), iterating on the tiles cannot help: the passes end, not converged.  The
// tightening is bounded.
struct RecheckStep {
  bool stop;            // end the passes here, not converged
  double tol_factor;    // of the next pass
  double prev_csr_res;  // for the next recheck
};
static inline RecheckStep recheck_tighten(double tol, double tile_res, double csr_res, double prev_csr_res, double tol_factor) {
  if (!(csr_res >= tol)) return {false, tol_factor, prev_csr_res};
  if (prev_csr_res > 0.0 && csr_res >= 0.9 * prev_csr_res) return {true, tol_factor, prev_csr_res};
  const double shrink = fmin(0.5, 0.5 * tol / csr_res) * (tile_res > 0.0 ? fmin(tile_res / tol, 1.0) : 1.0);
  return {false, fmax(fmin(tol_factor, 1.0) * shrink, 1e-3), csr_res};
}
