// The host decisions of the matrix-free hex-27 thermal brick operator (brick_operator_hex27.hip): the tile constants, the work items of the volume
// kernel (the box of control points an item owns, the elements it integrates), the fold onto the partial sums, the per-workgroup LDS and the refusals.
// Plain integers in, plain structs out; no HIP, no context: tools/host_check_brick_operator_hex27.cpp walks them on the CPU.
//
// Ownership.  The lattice has m = 2 ne + 1 control points per direction; element E covers the points 2E .. 2E + 2.  In j and k the elements are cut
// into tiles of B27_TE; tile t owns the points [2 B27_TE t, 2 B27_TE (t + 1)) and the LAST tile also the last point, so a tile owns at most
// B27_NP = 2 B27_TE + 1 lines.  Its lowest line is shared with the element below, so it integrates the one-element halo on the low side: B27_EH =
// B27_TE + 1 element columns.  Along i the sweep is cut into segments of L element planes under the same rule (a segment integrates the element plane
// below its first one only for the carry into its lowest control-point plane).  Every element adjacent to an owned point is integrated by the owner:
// no atomics, no colours.  The price is the redundancy R = elements integrated / elements of the brick: (9/8)^2 (L + 1) / L on a large brick, minus
// the halo that the first tile and the first segment do not have -- 1.277 at 128^3 with L = 32.
#pragma once
#include "brick_operator_decide.h"

#define B27_TE 8                   // elements per tile in j and in k
#define B27_EH (B27_TE + 1)        // element columns a tile integrates per direction (low-side halo)
#define B27_NP (2 * B27_TE + 1)    // control-point lines a tile owns per direction at the most (the last tile: + the last line)
#define B27_WAVES 8                // a wave per element; with <= 128 VGPRs two workgroups share a CU and fill each other's ragged last round and barriers
#define B27_THREADS (64 * B27_WAVES)
#define B27_LMAX 32                // element planes per segment ...
#define B27_LMIN 4                 // ... halved down to this while the items stay below B27_FILL
#define B27_FILL 1024
#define B27_NI 4                   // components through the sum-factorised interpolation: x1, x2, x3, T
#define B27_LDS_LIMIT (160 * 1024) // bytes of LDS of one gfx950 CU: what a workgroup may take (64 KB for the 3-point rule: two workgroups per CU; 113 KB for the 4-point rule: one)

struct B27Volume {
  int L, nseg, ntj, ntk;
  int64_t items;
  int rounds, grid;  // the fold (brick_operator_decide.h): workgroup b sweeps the items b, b + grid, ...
};
H8_HD B27Volume b27_volume(int ne0, int ne1, int ne2) {
  B27Volume V;
  V.ntj = (ne1 + B27_TE - 1) / B27_TE;
  V.ntk = (ne2 + B27_TE - 1) / B27_TE;
  V.L = B27_LMAX;
  while (V.L > B27_LMIN && (int64_t)V.ntj * V.ntk * ((ne0 + V.L - 1) / V.L) < B27_FILL) V.L >>= 1;
  V.nseg = (ne0 + V.L - 1) / V.L;
  V.items = (int64_t)V.ntj * V.ntk * V.nseg;
  V.rounds = (int)((V.items + BOP_VOLUME_PARTIALS - 1) / BOP_VOLUME_PARTIALS);
  V.grid = (int)((V.items + V.rounds - 1) / V.rounds);
  return V;
}
H8_HD int64_t b27_volume_grid(const B27Volume& V, bool want_partials) { return want_partials ? (int64_t)V.grid : V.items; }

// work item w: control points [i0, i1) x [j0, j1) x [k0, k1) owned, elements [I0, I1) x [J0, J1) x [K0, K1) integrated; (Jb, Kb) = the element column
// that slot 0 of the workgroup's 9 x 9 element-vector block stands for (B27_TE t - 1: outside the brick for the first tile)
struct B27Item {
  int i0, i1, j0, j1, k0, k1;
  int I0, I1, J0, J1, K0, K1;
  int Iown, Jb, Kb;  // Iown: first element plane whose two lower control-point planes the item writes (I0, or I0 + 1 behind a halo plane)
  int last_seg;      // the item also writes the brick's last control-point plane
};
H8_HD void b27_span(int t, int nt, int T, int ne, int& c0, int& c1, int& E0, int& E1) {
  c0 = 2 * T * t;
  c1 = t == nt - 1 ? 2 * ne + 1 : 2 * T * (t + 1);
  E0 = T * t - 1 < 0 ? 0 : T * t - 1;
  E1 = T * (t + 1) < ne ? T * (t + 1) : ne;
}
H8_HD B27Item b27_item(const B27Volume& V, int64_t w, int ne0, int ne1, int ne2) {
  B27Item it;
  const int tk = (int)(w % V.ntk), tj = (int)((w / V.ntk) % V.ntj), seg = (int)(w / ((int64_t)V.ntk * V.ntj));
  b27_span(tk, V.ntk, B27_TE, ne2, it.k0, it.k1, it.K0, it.K1);
  b27_span(tj, V.ntj, B27_TE, ne1, it.j0, it.j1, it.J0, it.J1);
  b27_span(seg, V.nseg, V.L, ne0, it.i0, it.i1, it.I0, it.I1);
  it.Iown = V.L * seg;
  it.Jb = B27_TE * tj - 1;
  it.Kb = B27_TE * tk - 1;
  it.last_seg = seg == V.nseg - 1;
  return it;
}

// ---- the per-wave block of the volume kernel (doubles), NI = B27_NI; the carve-up of k_hex27<false> without its source component ---------------------
//   X [27][NI] | T1 [2][ng][9][NI]                      both dead once stage 2 has run: stage 3 writes J -> Jinv [nq][9] | grad_xi T [nq][3] over them,
//                                                       and the transposed stages VA [3][ng][ng][3] | WB [2][ng][9] over those
//   T2 [3][ng][ng][3][NI]; the flux [nq][3] overlays it
//   w det [nq]
constexpr int b27_pad(int v) { return (v + 1) & ~1; }
constexpr int b27_max(int a, int b) { return a > b ? a : b; }
constexpr int b27_n1(int ng) { return 18 * ng * B27_NI; }
constexpr int b27_n2(int ng) { return 9 * ng * ng * B27_NI; }
constexpr int b27_n3(int ng) { return 12 * ng * ng * ng; }
constexpr int b27_na(int ng) { return 9 * ng * ng; }
constexpr int b27_nb(int ng) { return 18 * ng; }
constexpr int b27_ndec(int ng) { return b27_n1(ng) + b27_n2(ng) + b27_n3(ng) + b27_na(ng) + b27_nb(ng); }
constexpr int b27_w_t1() { return 27 * B27_NI; }
constexpr int b27_w_t2(int ng) { return b27_max(b27_w_t1() + b27_n1(ng), b27_max(b27_n3(ng), b27_pad(b27_na(ng)) + b27_nb(ng))); }
constexpr int b27_w_d(int ng) { return b27_w_t2(ng) + b27_max(b27_n2(ng), 3 * ng * ng * ng); }
constexpr int b27_w_size(int ng) { return b27_w_d(ng) + b27_pad(ng * ng * ng); }
// the workgroup's block: w [nq] | tab1 [2][ng][4] | decode words | Fe [B27_EH^2][27] | B27_WAVES per-wave blocks
constexpr int b27_off_tab1(int ng) { return b27_pad(ng * ng * ng); }
constexpr int b27_off_dec(int ng) { return b27_off_tab1(ng) + 8 * ng; }
constexpr int b27_off_fe(int ng) { return b27_off_dec(ng) + (b27_pad(b27_ndec(ng)) >> 1); }
constexpr int b27_off_waves(int ng) { return b27_off_fe(ng) + b27_pad(B27_EH * B27_EH * 27); }
constexpr size_t b27_lds_bytes(int ng) { return sizeof(double) * ((size_t)b27_off_waves(ng) + (size_t)B27_WAVES * b27_w_size(ng)); }

// ---- the face launch and the diagonal: the hex-8 operator's own decisions on the hex-27 lattice (bop_face_launch, bop_boundary_count, bop_face_grid,
// bop_diagonal_grid) ------------------------------------------------------------------------------------------------------------------------------------
// the <= 2 face elements along one tangential direction that contain lattice index t, low one first: element E[n], the point's local index c[n]
H8_HD int b27_face_elements(int t, int ne, int E[2], int c[2]) {
  int n = 0;
  if (t & 1) {
    E[n] = (t - 1) / 2; c[n] = 1; ++n;
  } else {
    if (t / 2 - 1 >= 0) { E[n] = t / 2 - 1; c[n] = 2; ++n; }
    if (t / 2 < ne) { E[n] = t / 2; c[n] = 0; ++n; }
  }
  return n;
}

// ---- which bricks: order 2, the whole lattice on one rank -----------------------------------------------------------------------------------------------
static inline const char* bop27_refusal(int itp_order, int plo, int phi, int m0) {
  if (itp_order != 2) return "an order-1 (hex-8) brick: the hex-27 operator covers order-2 bricks; a hex-8 brick takes mfem_brick_operator_create";
  if (plo != 0 || phi != m0) return "a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank";
  return nullptr;
}

// ---- the signed diagonal as a plane sweep (brick_operator_hex27_diagonal.hip: k_brick27_diagonal_sweep) ---------------------------------------------
// The product's skeleton -- b27_volume, b27_item, the 8 x 8 column tile, the segments, the low-side halo, the owner sum -- with the two apply stages
// replaced by the contraction of Ke_aa = sum_q w det (-k) |Jinv^T grad N_a|^2 = sum_q sum_(d <= e) H_de(q) dN_a/dxi_d dN_a/dxi_e, H_de = (-k w det)
// (2 - [d == e]) (Jinv Jinv^T)_de.  On the tensor basis dN_a/dxi_d dN_a/dxi_e is a product of three 1-D factors, one per direction r, of kind
// [r == d] + [r == e]: 0 = l^2, 1 = l l', 2 = l'^2 -- a 3 x ng x 3 table -- so the sum over q runs in three short stages over q2, q1, q0.
#define B27D_PAIRS 6  // (d, e): (0,0) (1,1) (2,2) (0,1) (0,2) (1,2)
H8_HD int b27d_pair_d(int p) { return p < 3 ? p : (p == 5 ? 1 : 0); }
H8_HD int b27d_pair_e(int p) { return p < 3 ? p : (p == 3 ? 1 : 2); }
H8_HD int b27d_kind(int p, int r) { return (b27d_pair_d(p) == r ? 1 : 0) + (b27d_pair_e(p) == r ? 1 : 0); }
constexpr int b27d_n3(int ng) { return 9 * ng * ng * ng; }               // J alone: no grad_xi T
constexpr int b27d_na(int ng) { return B27D_PAIRS * 3 * ng * ng; }       // VA[p][q0][q1][a2]
constexpr int b27d_nb(int ng) { return B27D_PAIRS * 9 * ng; }            // WB[p][q0][a12]
constexpr int b27d_ndec(int ng) { return b27_n1(ng) + b27_n2(ng) + b27d_n3(ng) + b27d_na(ng) + b27d_nb(ng); }
// per wave: the product's block (X | T1, then J over them, T2, w det); H[p][q] overlays T2 once J is inverted, VA | WB overlay J once H is formed
constexpr int b27d_w_wb(int ng) { return b27_pad(b27d_na(ng)); }
constexpr bool b27d_fits(int ng) {
  return B27D_PAIRS * ng * ng * ng <= b27_w_d(ng) - b27_w_t2(ng) && b27d_w_wb(ng) + b27d_nb(ng) <= b27_w_t2(ng);
}
static_assert(b27d_fits(1) && b27d_fits(2) && b27d_fits(3) && b27d_fits(4), "the diagonal's stages overlay the product's per-wave block");
// the workgroup's block: w [nq] | tab1 [2][ng][4] | tabp [3][ng][4] | decode words | Fe [B27_EH^2][27] | B27_WAVES per-wave blocks
constexpr int b27d_off_tab1(int ng) { return b27_pad(ng * ng * ng); }
constexpr int b27d_off_tabp(int ng) { return b27d_off_tab1(ng) + 8 * ng; }
constexpr int b27d_off_dec(int ng) { return b27d_off_tabp(ng) + 12 * ng; }
constexpr int b27d_off_fe(int ng) { return b27d_off_dec(ng) + (b27_pad(b27d_ndec(ng)) >> 1); }
constexpr int b27d_off_waves(int ng) { return b27d_off_fe(ng) + b27_pad(B27_EH * B27_EH * 27); }
constexpr size_t b27d_lds_bytes(int ng) { return sizeof(double) * ((size_t)b27d_off_waves(ng) + (size_t)B27_WAVES * b27_w_size(ng)); }
static_assert(b27d_lds_bytes(4) <= B27_LDS_LIMIT && 2 * b27d_lds_bytes(3) <= B27_LDS_LIMIT, "one workgroup per CU on the 4-point rule, two below it");
