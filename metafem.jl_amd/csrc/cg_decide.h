// The host decisions of the classic CG pass (krylov_cg.hip: mfem_cg_pass) about its ring of search directions that are integer arithmetic alone:
// how deep the ring is, which iterations apply the pending updates of x, how many iterations one captured cycle holds.  No HIP, no context:
// tools/host_check_cg.cpp walks them on the CPU (tests/test_cg_ring_decide.py).
//
// The ring: iteration `it` of a pass keeps its direction p_it in slot it % m and writes p_(it+1) to slot (it + 1) % m.  x += alpha_it p_it is NOT
// applied per iteration: at a flush position, (it + 1) % m == 0 -- the iteration in the last slot --, k_cg_pupdate applies the m pending updates per element in iteration order, with the
// operation the per-iteration update uses (one fma per component) -- the stored x is bit for bit what m per-iteration updates leave.  m = 1 is the
// per-iteration update itself.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define CG_HD __host__ __device__
#else
#define CG_HD
#endif

static const int CG_RING_MAX = 16;                  // slots (and stored step lengths) at the most
static const int64_t CG_RING_MIN_ROWS = 40000000;   // from here on a vector is out of reach of the Infinity Cache (the nontemporal stores' threshold too)
static const int CG_RING_AUTO = 8;                  // depth from CG_RING_MIN_ROWS on: 7.125 vector streams per iteration on average instead of 8

// nv: padded vector length of the solve; knob: mfem_debug_set("cg_ring"): 0 = automatic, 1 .. CG_RING_MAX forces that depth (anything else: automatic)
static inline int cg_ring_depth(int64_t nv, int knob) {
  if (knob >= 1 && knob <= CG_RING_MAX) return knob;
  return nv >= CG_RING_MIN_ROWS ? CG_RING_AUTO : 1;
}
// slot of p_it
static inline int cg_ring_slot(int it, int m) { return it % m; }
// updates of x still pending after `iters` iterations of a pass: what k_cg_xflush applies when the pass ends there
CG_HD static inline int cg_ring_pending(int iters, int m) { return iters % m; }
// Iterations of one captured cycle: the kernel arguments repeat with the period of the slots (m) AND of the two scalar / flag banks (2) -- their least
// common multiple.  m = 1: the even / odd pair.  A cycle starts at it % unit == 0.
static inline int cg_ring_unit(int m) { return (m & 1) ? 2 * m : m; }
