// The host decisions of the matrix-free hex-27 ELASTICITY brick operator (brick_operator_elasticity_hex27.hip): three field-major unknowns per control
// point of an order-2 brick.  The ownership, the tiles, the segments, the work items and the fold are the thermal operator's, unchanged
// (brick_operator_hex27_decide.h: b27_volume, b27_item, b27_face_elements -- read its header comment first); this file adds the per-wave carve-up for
// six interpolated components, the number of waves a workgroup runs, the per-workgroup LDS, the rule predicate and the refusals.
// Plain integers in, plain structs out; no HIP, no context: tools/host_check_brick_operator_elasticity_hex27.cpp walks them on the CPU.
//
// The arrangement.  Carried over with NI = 6 the thermal carve-up needs, on the 3-point rule, 8000 B per wave, 52 488 B for the element vectors
// Fe[81 columns][81] and 6 808 B of decode words: 123 720 B with 8 waves, ONE workgroup per CU (163 840 B) where the thermal kernel has two.  No
// candidate brings two back -- Fe one field at a time saves 35 KB of the 124, a 4 x 4 tile 36 KB while R rises from (9/8)^2 to (5/4)^2 per plane, and
// even 5 waves take 99 720 B -- so the one resident workgroup is made larger instead: E27_WAVES_MAX = 12 waves (3 per SIMD, <= 168 VGPRs) take
// 155 720 B with the tile, and so R, unchanged.  The number of waves is a launch parameter (the kernel walks elements blockDim / 64 apart), so the
// 4-point rule, whose per-wave block is 16 640 B, runs with e27_waves(4) = 5 waves -- the fewest that cover the 17 x 17 control-point columns of the
// owner sums -- in 148 848 B.  (tools/host_check_brick_operator_elasticity_hex27.cpp asserts these figures.)
#pragma once
#include "brick_operator_hex27_decide.h"

#define E27_TE 8                   // elements per tile in j and in k (the thermal operator's: its work items are reused)
#define E27_LMIN 4                 // the shortest segment of the sweep (b27_volume)
#define E27_NI 6                   // components through the sum-factorised interpolation: x1, x2, x3, u1, u2, u3
#define E27_NF 3                   // fields
#define E27_NV (27 * E27_NF)       // entries of an element vector, field-major: [f][a]
#define E27_WAVES_MAX 12           // waves of a workgroup at the most: 3 per SIMD of the one workgroup a CU holds
#define E27_WAVES_MIN 5            // ... and at the least: 320 threads >= B27_NP^2 = 289 owner columns
#define E27_LDS_LIMIT (160 * 1024) // bytes of LDS of one gfx950 CU
#define E27_LDS_STATIC 128         // bytes of static LDS of the volume kernel beside its dynamic block (red[16]: the workgroup's dot sum)
static_assert(E27_TE == B27_TE && E27_LMIN == B27_LMIN, "the work items are b27_volume's and b27_item's");
static_assert(64 * E27_WAVES_MIN >= B27_NP * B27_NP, "a thread per owner column");

// ---- the per-wave block (doubles) ------------------------------------------------------------------------------------------------------------------
//   X [27][NI] | T1 [2][ng][9][NI]          both dead once stage 2 has run: stage 3 writes J -> Jinv [nq][9] | grad_xi u [nq][3][3] over them, and the
//                                           transposed stages VA [3][3][ng][ng][3] | WB [3][2][ng][9] over those
//   T2 [3][ng][ng][3][NI]; the flux [3][nq][3] overlays it
//   w det [nq]
constexpr int e27_n1(int ng) { return 18 * ng * E27_NI; }
constexpr int e27_n2(int ng) { return 9 * ng * ng * E27_NI; }
constexpr int e27_n3(int ng) { return 18 * ng * ng * ng; }              // J [q][3][3], then grad_xi u [q][f][m]
constexpr int e27_na(int ng) { return E27_NF * 9 * ng * ng; }           // VA[f][v][q0][q1][a2]
constexpr int e27_nb(int ng) { return E27_NF * 18 * ng; }               // WB[f][w][q0][a12]
constexpr int e27_ndec(int ng) { return e27_n1(ng) + e27_n2(ng) + e27_n3(ng) + e27_na(ng) + e27_nb(ng); }
constexpr int e27_w_t1() { return 27 * E27_NI; }
constexpr int e27_w_wb(int ng) { return b27_pad(e27_na(ng)); }
constexpr int e27_w_t2(int ng) { return b27_pad(b27_max(e27_w_t1() + e27_n1(ng), b27_max(e27_n3(ng), e27_w_wb(ng) + e27_nb(ng)))); }
constexpr int e27_w_d(int ng) { return e27_w_t2(ng) + b27_pad(b27_max(e27_n2(ng), 9 * ng * ng * ng)); }
constexpr int e27_w_size(int ng) { return e27_w_d(ng) + b27_pad(ng * ng * ng); }
// the workgroup's block: w [nq] | tab1 [2][ng][4] | decode words | Fe [B27_EH^2][81] | the per-wave blocks
constexpr int e27_off_tab1(int ng) { return b27_pad(ng * ng * ng); }
constexpr int e27_off_dec(int ng) { return e27_off_tab1(ng) + 8 * ng; }
constexpr int e27_off_fe(int ng) { return e27_off_dec(ng) + (b27_pad(e27_ndec(ng)) >> 1); }
constexpr int e27_off_waves(int ng) { return e27_off_fe(ng) + b27_pad(B27_EH * B27_EH * E27_NV); }
// (the DYNAMIC block: what a launch asks for; a CU must hold it plus E27_LDS_STATIC)
constexpr size_t e27_lds_bytes(int ng, int waves) { return sizeof(double) * ((size_t)e27_off_waves(ng) + (size_t)waves * e27_w_size(ng)); }
// the decode words keep an LDS offset in 12 bits (transposed stages) or 16 bits (interpolation stages)
constexpr bool e27_decode_fits(int ng) { return E27_NF * 3 * ng * ng * ng <= 4096 && e27_na(ng) <= 4096 && e27_w_t2(ng) + e27_n2(ng) <= 65536; }

// waves per workgroup of a rule: as many as fit, E27_WAVES_MAX at the most; 0: not even E27_WAVES_MIN fit
constexpr int e27_waves(int ng) {
  int w = E27_WAVES_MAX;
  while (w >= E27_WAVES_MIN && e27_lds_bytes(ng, w) + E27_LDS_STATIC > E27_LDS_LIMIT) --w;
  return w >= E27_WAVES_MIN ? w : 0;
}
// THE rule predicate: ng Gauss points per direction are served
constexpr bool e27_rule_known(int ng) { return ng >= 1 && ng <= 4; }
constexpr bool e27_rule_served(int ng) { return e27_rule_known(ng) && e27_waves(ng) > 0; }
static_assert(e27_decode_fits(1) && e27_decode_fits(2) && e27_decode_fits(3) && e27_decode_fits(4), "the decode words hold every known rule's offsets");
static_assert(e27_rule_served(1) && e27_rule_served(2) && e27_rule_served(3), "the rules with 1 to 3 Gauss points per direction are served");
static_assert(e27_waves(3) == E27_WAVES_MAX, "the flagship rule runs the full workgroup");
#define E27_THREADS_MAX (64 * E27_WAVES_MAX)

// ---- which bricks: order 2, the whole lattice on one rank, a rule whose LDS block fits ---------------------------------------------------------------
static inline const char* bop_e27_refusal(int itp_order, int plo, int phi, int m0, int ng) {
  if (itp_order != 2) return "an order-1 (hex-8) brick: the hex-27 elasticity operator covers order-2 bricks; a hex-8 brick takes mfem_brick_operator_create_elasticity";
  if (plo != 0 || phi != m0) return "a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank";
  if (!e27_rule_known(ng)) return "a Gauss rule outside 1 to 4 points per direction (itg_order 1 to 7): the hex-27 tables hold no such rule";
  if (!e27_rule_served(ng)) return "the 4-point Gauss rule (itg_order 6 to 7): the volume kernel's per-workgroup LDS block exceeds the 160 KB of a CU";
  return nullptr;
}
static inline const char* bop_e27_multigrid_refusal() {
  return "a hex-27 elasticity operator: a multigrid hierarchy for it does not exist yet";
}
// the face launch: penalty rows when tau and penalty_faces are set; the residual's launch also when traction_faces are
static inline bool bop_e27_face_launch(double tau, unsigned penalty, unsigned traction, bool residual) {
  return (tau != 0.0 && penalty != 0u) || (residual && traction != 0u);
}
