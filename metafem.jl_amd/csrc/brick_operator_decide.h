// The host decisions of the matrix-free hex-8 brick operator (brick_operator.hip): which kernel form serves a Gauss rule, the work items of the
// volume kernel and how many workgroups share them, the face kernel's grid, how the partial sums of a product are split between the two launches, and
// which bricks the operator refuses.  Plain integers in, plain structs out; no HIP, no context: tools/host_check_brick_operator.cpp walks them on the
// CPU for every lattice up to 1025^3.  The tile constants, the sweep segments and the boundary enumeration are those of the fused residual
// (hex8_decide.h): the operator's volume kernels own the same control points as k_thermal_residual_sweep / k_thermal_residual.
#pragma once
#include "hex8_decide.h"

// A product leaves at most BOP_MAX_PARTIALS partial sums of dotw . y: the volume kernel's first, then the face kernel's increments (as the split SpMV
// does with np1 + np2).  The residual sweep's own grid is one workgroup per (tile, segment) -- 35 * 35 * 17 = 20 825 at 512^3, and 69 * 69 tiles alone
// exceed the cap at 1025^3, whatever the segment length --, so the operator FOLDS: a grid of at most BOP_VOLUME_PARTIALS workgroups, workgroup b
// sweeps the work items b, b + grid, b + 2 grid, ... in that order and adds their sums in that order.  The same bits on every run, no atomics.
// The grid is the smallest that keeps the rounds of the cap: every workgroup then sweeps `rounds` items or one fewer (at 512^3: 3471 workgroups of
// 6 items, not 3584 of 5 or 6).  A product that is asked for NO partial sums (mul!, the solvers' products without a dot) is not folded: one
// workgroup per item, the residual's own grid, balanced by the dispatcher (bop_volume_grid).
#define BOP_MAX_PARTIALS 4096  // (= MFEM_MAX_PARTIALS)
#define BOP_FACE_PARTIALS 512
#define BOP_VOLUME_PARTIALS (BOP_MAX_PARTIALS - BOP_FACE_PARTIALS)

// ---- which volume kernel: the sweep exists for the 2- and 3-point rules (itg_order 2-5), the 1- and 4-point rules take the 4 x 4 x 8 tiles ----------
enum BopKernel { BOP_SWEEP, BOP_TILES, BOP_POINTS };
H8_HD BopKernel bop_kernel(int ng) { return ng == 2 || ng == 3 ? BOP_SWEEP : BOP_TILES; }
// elasticity (brick_operator_elasticity.hip) follows ITS residual's choice: the sweep for the 2-point rule alone (the 3-point rule's three fields do
// not fit that form's registers: h8_elasticity_residual_kernel), a thread per control point (BOP_POINTS) for the 1-, 3- and 4-point rules
H8_HD BopKernel bop_elasticity_kernel(int ng) {
  return h8_elasticity_residual_kernel(h8_elasticity_knobs(0), ng) == H8_EL_RESIDUAL_SWEEP ? BOP_SWEEP : BOP_POINTS;
}

// ---- the volume launch ------------------------------------------------------------------------------------------------------------------------------
struct BopVolume {
  BopKernel kernel;
  int L;          // sweep: lattice planes per segment (h8_residual_sweep: 32, halved down to 4 on small grids); tiles: 0
  int64_t items;  // work items: (tile, segment) pairs of the sweep, 4 x 4 x 8 tiles of the tile form
  int rounds;     // items per workgroup at the most: ceil(items / BOP_VOLUME_PARTIALS)
  int grid;       // workgroups = partial sums of the volume kernel: ceil(items / rounds) <= BOP_VOLUME_PARTIALS
  int threads;
};
H8_HD BopVolume bop_volume(int ng, int m0, int m1, int m2) {
  BopVolume V;
  V.kernel = bop_kernel(ng);
  if (V.kernel == BOP_SWEEP) {
    const H8Sweep S = h8_residual_sweep(m1, m2, m0);
    V.L = S.L;
    V.items = S.grid;
    V.threads = SW_THREADS;
  } else {
    V.L = 0;
    V.items = h8_tile_grid(m0, m1, m2);
    V.threads = TT_THREADS;
  }
  V.rounds = (int)((V.items + BOP_VOLUME_PARTIALS - 1) / BOP_VOLUME_PARTIALS);
  V.grid = (int)((V.items + V.rounds - 1) / V.rounds);
  return V;
}
// The elasticity volume launch (three fields, n = 3 m0 m1 m2 unknowns; an item owns the three unknowns of each of its control points).  The sweep's
// items are the thermal sweep's; the point form's are the workgroups of k_elasticity_residual: H8_BLOCK consecutive control points each
// (bop_point_range), folded like the others.
H8_HD BopVolume bop_elasticity_volume(int ng, int m0, int m1, int m2) {
  BopVolume V;
  V.kernel = bop_elasticity_kernel(ng);
  if (V.kernel == BOP_SWEEP) {
    const H8Sweep S = h8_residual_sweep(m1, m2, m0);
    V.L = S.L;
    V.items = S.grid;
    V.threads = SW_THREADS;
  } else {
    V.L = 0;
    V.items = ((int64_t)m0 * m1 * m2 + H8_BLOCK - 1) / H8_BLOCK;
    V.threads = H8_BLOCK;
  }
  V.rounds = (int)((V.items + BOP_VOLUME_PARTIALS - 1) / BOP_VOLUME_PARTIALS);
  V.grid = (int)((V.items + V.rounds - 1) / V.rounds);
  return V;
}
// the control points [first, last) work item w of the point form owns
struct BopRange {
  int64_t first, last;
};
H8_HD BopRange bop_point_range(int64_t w, int64_t n_points) {
  BopRange r;
  r.first = w * H8_BLOCK;
  r.last = r.first + H8_BLOCK < n_points ? r.first + H8_BLOCK : n_points;
  return r;
}
// workgroups of the volume launch: the fold when the product leaves partial sums, one per item otherwise
H8_HD int64_t bop_volume_grid(const BopVolume& V, bool want_partials) { return want_partials ? (int64_t)V.grid : V.items; }
// the control points work item w of the sweep owns: [j0, j1) x [k0, k1) in the plane, planes [i0, i1)
struct BopBox {
  int i0, i1, j0, j1, k0, k1;
};
H8_HD BopBox bop_item_box(const BopVolume& V, int64_t w, int m0, int m1, int m2) {
  BopBox b;
  if (V.kernel == BOP_SWEEP) {  // (BOP_POINTS owns no box: bop_point_range)
    const H8SweepTile T = h8_sweep_tile((unsigned)w, m1, m2, 0, m0, V.L, SW_N, SW_N);
    b.i0 = T.i0; b.i1 = T.i1;
    b.j0 = T.tj0; b.j1 = T.tj0 + SW_N < m1 ? T.tj0 + SW_N : m1;
    b.k0 = T.tk0; b.k1 = T.tk0 + SW_N < m2 ? T.tk0 + SW_N : m2;
  } else {
    const H8TileOrigin T = h8_tile_origin(w, m1, m2, 0);
    b.i0 = T.ti; b.i1 = T.ti + TT_NI < m0 ? T.ti + TT_NI : m0;
    b.j0 = T.tj; b.j1 = T.tj + TT_NJ < m1 ? T.tj + TT_NJ : m1;
    b.k0 = T.tk; b.k1 = T.tk + TT_NK < m2 ? T.tk + TT_NK : m2;
  }
  return b;
}

// ---- the face launch: one kernel over the boundary control points (h8_boundary_point), each adding its own Robin and Nitsche terms -----------------
H8_HD bool bop_nitsche_on(double k, double h_penalty, uint32_t fixed_faces) { return fixed_faces != 0u && (h_penalty != 0.0 || k != 0.0); }  // (mfem_brick_nitsche_faces' own test)
H8_HD bool bop_face_launch(double k, double h, uint32_t robin_faces, double h_penalty, uint32_t fixed_faces) {
  return h8_robin_launch(h, robin_faces) || bop_nitsche_on(k, h_penalty, fixed_faces);
}
// boundary control points of the whole brick and the face kernel's grid (a thread strides over the points: at most BOP_FACE_PARTIALS workgroups)
H8_HD int64_t bop_boundary_count(int m0, int m1, int m2) { return h8_boundary_count(0, m0, m0 - 1, (int64_t)m1 * m2, m1, m2); }
H8_HD int bop_face_grid(int64_t boundary_count) {
  const int64_t g = (boundary_count + H8_BLOCK - 1) / H8_BLOCK;
  return (int)(g < 1 ? 1 : g > BOP_FACE_PARTIALS ? BOP_FACE_PARTIALS : g);
}
// launches of one product: 1, or 2 with face terms
H8_HD int bop_launches(double k, double h, uint32_t robin_faces, double h_penalty, uint32_t fixed_faces) {
  return bop_face_launch(k, h, robin_faces, h_penalty, fixed_faces) ? 2 : 1;
}
// elasticity: the penalty faces alone enter K (traction_faces and sig are the residual's load), under the residual's own launch test
H8_HD bool bop_elasticity_face_launch(double tau, uint32_t penalty_faces) { return h8_elasticity_faces_launch(tau, penalty_faces, 0u); }
H8_HD int bop_elasticity_launches(double tau, uint32_t penalty_faces) { return bop_elasticity_face_launch(tau, penalty_faces) ? 2 : 1; }
// the diagonal: a thread per control point (elasticity: of its three unknowns)
H8_HD int64_t bop_diagonal_grid(int64_t n) { return (n + H8_BLOCK - 1) / H8_BLOCK; }

// ---- which bricks: hex-8 (one thermal or three elasticity fields), the whole lattice on one rank ------------------------------------------------------------------------------------
// nullptr: taken; otherwise why not (MFEM_ERR_UNSUPPORTED at mfem_brick_operator_create)
static inline const char* bop_refusal(int itp_order, int plo, int phi, int m0) {
  if (itp_order != 1) return "an order-2 (hex-27) brick: the matrix-free brick operator covers hex-8 bricks";
  if (plo != 0 || phi != m0) return "a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank";
  return nullptr;
}
