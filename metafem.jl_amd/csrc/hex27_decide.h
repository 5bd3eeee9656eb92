// The host decisions of the hex-27 thermal assembly (assemble_hex27.hip and the kernels in hex27_gather.hip, hex27_direct.hip, hex27_rows.hip): the
// knob word, the element planes and colour counts of a slab, which of the six paths builds the matrix, the workspace of the scratch-free paths, the
// ring of the two-pass path, the grids, the schedule of the Robin-face launches and the dynamic LDS of k_hex27 (next to the macros the kernel lays
// its block out with).  No HIP, no context: tools/host_check_hex27.cpp walks them on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- tile constants the decisions share with the kernels ----------------------------------------------------------------------------------------
#define H27_WAVES 8                    // waves per workgroup of k_hex27 (they share the reference tables in LDS)
#define H27_THREADS (64 * H27_WAVES)
#define H27_NQP(nq) (((nq) + 3) & ~3)  // Gauss points padded to whole k-groups of the MFMA loop
#define G27_NODES 32                   // control points per workgroup of k_hex27_gather_lds
#define G27_ROW 126                    // up to 125 entries per row, padded
#define D27_WAVES 8
#define D27_NODES (8 * D27_WAVES)      // control points per block of k_hex27_direct
#define D27_THREADS (64 * D27_WAVES)
#define R27_THREADS 256
#define R27_MIN_PERCENT 30             // non-affine elements from which the row-owner kernel of general elements is taken
#define H27_MIXED_MAX_PERCENT 80       // ... up to which the per-element choice is (profiles/r05_hex27_mixed.txt -- at 75 % the choice takes 11.2 ms against 11.9 for the two-pass path, at 100 % 13.1 against 12.2)
static const size_t H27_SCRATCH_BUDGET = (size_t)16 << 30;  // bytes of workspace one assembly may take for element matrices or G_q

// ---- knob word (mfem_debug_set_hex27) -----------------------------------------------------------------------------------------------------------
struct H27Knobs {
  int variant;       // bits 0-1: 1 two-pass and the scratch-free paths in front of it (0 = default = 1), 2 FP64 atomics, 3 colour scatter
  int rows_min;      // bits 2-7: percentage of non-affine elements FROM which the row-owner kernel of general elements is taken (0 = R27_MIN_PERCENT)
  bool affine;       // bit 8 CLEAR: elements that are an affine image of the reference nodes take the constant-Jacobian shortcut
  bool direct;       // bit 9 CLEAR: the scratch-free assembly of all-affine meshes
  bool mixed;        // bit 10 CLEAR: the per-element choice (set: a mesh with a non-affine element takes the two-pass path whole)
  bool rows;         // bit 11 CLEAR: the row-owner kernel of general elements (k_hex27_rows_gq)
  int rows_ablate;   // bits 12-14: TIMING-ONLY ablations of k_hex27_rows_gq (wrong values): 1 no arithmetic, 2 no LDS additions, 4 no G_q loads
  int chunk_planes;  // bits 16-23: element planes per scratch chunk of the two-pass ring (0 = from the budget)
  int mixed_max;     // bits 24-30: percentage of non-affine elements UP TO which the per-element choice is taken (0 = H27_MIXED_MAX_PERCENT)
};
static inline H27Knobs h27_knobs(int word) {
  H27Knobs K;
  K.variant = (word & 3) == 0 ? 1 : (word & 3);
  K.rows_min = ((word >> 2) & 63) ? ((word >> 2) & 63) : R27_MIN_PERCENT;
  K.affine = !((word >> 8) & 1);
  K.direct = !((word >> 9) & 1);
  K.mixed = !((word >> 10) & 1);
  K.rows = !((word >> 11) & 1);
  K.rows_ablate = (word >> 12) & 7;
  K.chunk_planes = (word >> 16) & 255;
  K.mixed_max = ((word >> 24) & 127) ? ((word >> 24) & 127) : H27_MIXED_MAX_PERCENT;
  return K;
}

// ---- planes ---------------------------------------------------------------------------------------------------------------------------------------
// Element planes (dimension 0) that touch the owned control-point planes [plo, phi) of a slab.  Slabs start and end on element boundaries
// (mfem_brick_set_slab), so the first owned plane also needs the element plane below it.
static inline void hex27_element_planes(int plo, int phi, int ne0, int* elo, int* ehi) {
  *elo = plo / 2 - 1 < 0 ? 0 : plo / 2 - 1;
  *ehi = phi / 2 > ne0 ? ne0 : phi / 2;
}
// elements of one parity colour (0..7: (I&1) | (J&1)<<1 | (K&1)<<2) within the element planes [elo, ehi)
static inline int64_t hex27_colour_count(int ne1, int ne2, int colour, int elo, int ehi) {
  const int o0 = elo + (((colour & 1) - elo) & 1);
  const int64_t n0 = o0 < ehi ? (ehi - o0 + 1) >> 1 : 0, n1 = (ne1 - ((colour >> 1) & 1) + 1) >> 1, n2 = (ne2 - (colour >> 2) + 1) >> 1;
  return n0 * n1 * n2;
}
// slabs ([plo, phi) short of the m0 planes of the brick) are assembled by variant 1 only
static inline bool h27_slab_refused(const H27Knobs& K, int plo, int phi, int m0) { return !(plo == 0 && phi == m0) && K.variant != 1; }

// ---- which path -------------------------------------------------------------------------------------------------------------------------------------
// Is the count of non-affine elements needed at all?  (G0 of every element + the count: k_hex27_affine_g0 and one 4-byte read-back per assembly.  The
// row-owner kernels behind it keep control-point ids in 32 bits.)
static inline bool h27_needs_count(const H27Knobs& K, int64_t n_owned) { return K.variant == 1 && K.direct && K.affine && n_owned < ((int64_t)1 << 31); }

static inline size_t h27_gq_bytes(int ng, int64_t nel) { return sizeof(double) * 6 * (size_t)(ng * ng * ng) * (size_t)nel; }  // G_q of every element
static inline size_t h27_stored_bytes(int64_t n_stored) { return sizeof(double) * 729 * (size_t)n_stored; }                 // Ke of the non-affine ones

enum H27Path {
  H27_ATOMICS,   // every element's Ke added with FP64 atomics, one launch
  H27_COLOUR,    // colour-partitioned read-modify-write scatter, 8 launches
  H27_TWO_PASS,  // Ke -> a ring of element planes, row-owner gather
  H27_DIRECT,    // every element affine: rows from G0 and the reference integrals, no Ke stored
  H27_MIXED,     // the same with the non-affine elements' Ke in a compact scratch
  H27_ROWS       // mostly general elements: rows from per-element G_q
};
// nel elements in the assembled planes, n_stored of them non-affine (< 0: not counted, see h27_needs_count).  Mostly general elements with three
// Gauss points per direction go to the row owners of k_hex27_rows_gq; up to mixed_max percent the per-element choice is the faster one; beyond it, or
// with a scratch beyond the budget, the plain two-pass path (its gather streams every run with no arithmetic beside it; it rings over element planes).
// (budget: an argument so that the host check can stand on both sides of it; the library passes none.)
static inline H27Path h27_path(const H27Knobs& K, int ng, int64_t nel, int64_t n_stored, size_t budget = H27_SCRATCH_BUDGET) {
  if (K.variant == 2) return H27_ATOMICS;
  if (n_stored >= 0) {
    if (K.rows && ng == 3 && n_stored * 100 >= nel * (int64_t)K.rows_min && n_stored > 0 && h27_gq_bytes(ng, nel) <= budget && K.chunk_planes == 0)
      return H27_ROWS;
    if (n_stored == 0) return H27_DIRECT;
    if (K.mixed && n_stored * 100 <= nel * (int64_t)K.mixed_max && h27_stored_bytes(n_stored) <= budget) return H27_MIXED;
  }
  return K.variant == 1 ? H27_TWO_PASS : H27_COLOUR;
}

// ---- workspace of the direct, mixed and rows paths ------------------------------------------------------------------------------------------------------
// G0 [6 nel] | slot [nel] | elist [nel] (int32, each padded to 256 bytes) | the compact scratch of the non-affine elements' Ke from `head` on (its size
// is known once they are counted).  The rows path overwrites all of it with G_q.
struct H27Ws {
  size_t g_bytes, map_bytes;       // G0; one of the two int32 maps
  size_t slot, elist;              // byte offsets of the maps
  size_t count_bytes;              // what the count needs: G0 and both maps
  size_t head, stored_bytes;       // byte offset (256-byte aligned) and size of the stored Ke
  size_t gq_bytes;
};
static inline H27Ws h27_ws(int ng, int64_t nel, int64_t n_stored) {
  H27Ws W;
  W.g_bytes = sizeof(double) * 6 * (size_t)nel;
  W.map_bytes = (sizeof(int32_t) * (size_t)nel + 255) & ~(size_t)255;
  W.slot = W.g_bytes;
  W.elist = W.g_bytes + W.map_bytes;
  W.count_bytes = W.g_bytes + 2 * W.map_bytes;
  W.head = (W.count_bytes + 255) & ~(size_t)255;
  W.stored_bytes = h27_stored_bytes(n_stored > 0 ? n_stored : 0);
  W.gq_bytes = h27_gq_bytes(ng, nel);
  return W;
}

// ---- the ring of the two-pass path ---------------------------------------------------------------------------------------------------------------------
// The scratch is a ring of element planes (dimension 0): a chunk computes planes [a, b), b - a <= P, and gathers the control-point planes [2a, 2b) (the
// last chunk also 2b), which need element planes a-1 .. b-1 -- plane a-1 is still in a ring of P + 1 planes.
struct H27Ring {
  int P, ring;
  size_t plane_bytes;  // Ke of one element plane
};
static inline H27Ring h27_ring(int npl, int64_t plane_el, int chunk_planes, size_t budget = H27_SCRATCH_BUDGET) {
  H27Ring R;
  R.plane_bytes = sizeof(double) * 729 * (size_t)plane_el;
  int P = npl;
  if (chunk_planes > 0) P = chunk_planes;
  else if (R.plane_bytes * (size_t)npl > budget) P = (int)(budget / R.plane_bytes) - 1;
  if (P < 1) P = 1;
  if (P > npl) P = npl;
  R.P = P;
  R.ring = P >= npl ? npl : P + 1;
  return R;
}
// rows the chunk [a, b) of the element planes [.., ehi) gathers: control-point planes [2a, 2b) (the last chunk: up to phi), clipped to the owned planes
static inline void h27_chunk_rows(int a, int b, int ehi, int plo, int phi, int64_t plane_rows, int64_t* row_lo, int64_t* row_hi) {
  const int gp_lo = 2 * a < plo ? plo : 2 * a, gp_hi = b == ehi ? phi : 2 * b;
  *row_lo = (int64_t)(gp_lo - plo) * plane_rows;
  *row_hi = (int64_t)(gp_hi - plo) * plane_rows;
}

// ---- grids ----------------------------------------------------------------------------------------------------------------------------------------------
// persistent kernels: two workgroups per CU at most, each walking the blocks grid apart
static inline int h27_persistent_grid(int64_t nblocks, int num_cus) {
  const int64_t cap = (int64_t)num_cus * 2;
  return (int)(nblocks < cap ? nblocks : cap);
}
// k_hex27: a wave per element, H27_WAVES per workgroup
static inline int h27_wave_grid(int64_t nelem, int num_cus) { return h27_persistent_grid((nelem + H27_WAVES - 1) / H27_WAVES, num_cus); }
// k_hex27_direct: D27_NODES owned control points per block (78 KB of LDS per workgroup)
static inline int h27_direct_grid(int64_t n_owned, int num_cus) { return h27_persistent_grid((n_owned + D27_NODES - 1) / D27_NODES, num_cus); }
static inline unsigned h27_gather_grid(int64_t row_lo, int64_t row_hi) { return (unsigned)((row_hi - row_lo + G27_NODES - 1) / G27_NODES); }
// k_hex27_rows_gq: tiles of 4 x 4 x 4 control points that cover the owned planes (67 KB of LDS per workgroup)
struct H27RowsGrid {
  int T0lo, nT0, nT1, nT2, grid;
};
static inline H27RowsGrid h27_rows_grid(int plo, int phi, int m1, int m2, int num_cus) {
  H27RowsGrid G;
  G.T0lo = plo / 4;
  G.nT0 = (phi - 1) / 4 - G.T0lo + 1;
  G.nT1 = (m1 + 3) / 4;
  G.nT2 = (m2 + 3) / 4;
  G.grid = h27_persistent_grid((int64_t)G.nT0 * G.nT1 * G.nT2, num_cus);
  return G;
}

// ---- Robin faces --------------------------------------------------------------------------------------------------------------------------------------------
// One launch per (direction, side, colour of the face elements in their two tangential directions); the two opposite faces of a direction share no
// node and go into the same launch (side = -1) when both carry the condition.  robin: bit (id - 1) of face id, ids as in make_Brick (x: 5 / 3, y: 2 / 4,
// z: 1 / 6).  Colour classes without a face element are left out.
#define H27_FACE_BLOCK 256  // (= MFEM_BLOCK)
struct H27FaceLaunch {
  int nd, side, colour, n1, n2, grid;
};
static inline int h27_face_schedule(uint32_t robin, double h, const int ne[3], H27FaceLaunch out[24]) {
  int n = 0;
  if (h == 0.0 || robin == 0u) return 0;
  for (int nd = 0; nd < 3; ++nd) {
    const int id_lo = (nd == 0) ? 5 : (nd == 1) ? 2 : 1, id_hi = (nd == 0) ? 3 : (nd == 1) ? 4 : 6;
    const bool lo = robin & (1u << (id_lo - 1)), hi = robin & (1u << (id_hi - 1));
    const int t1 = (nd + 1) % 3, t2 = (nd + 2) % 3;
    for (int side = (lo && hi) ? -1 : 0; side < 2; ++side) {
      if (side >= 0 && ((lo && hi) || !(side ? hi : lo))) continue;
      for (int colour = 0; colour < 4; ++colour) {
        const int n1 = (ne[t1] - (colour & 1) + 1) >> 1, n2 = (ne[t2] - (colour >> 1) + 1) >> 1;
        if (n1 <= 0 || n2 <= 0) continue;
        const int64_t nthreads = (int64_t)n1 * n2 * 9 * (side < 0 ? 2 : 1);
        out[n++] = {nd, side, colour, n1, n2, (int)((nthreads + H27_FACE_BLOCK - 1) / H27_FACE_BLOCK)};
      }
    }
  }
  return n;
}

// ---- dynamic LDS of k_hex27 ---------------------------------------------------------------------------------------------------------------------------------
// mode: 0 residual, 1 matrix with colour scatter / atomics (row descriptors per wave), 2 matrix -> scratch.  NI = components pushed through the
// sum-factorised interpolation: 3 (x1, x2, x3) for the matrix, 5 (+ nodal T and nodal source s) for the residual.
// Per-wave carve-up (doubles), sized from ng / nq = ng^3 (even-padded):
//   X[27][NI] | T1 [2][ng][9][NI] (first stage)                         -- both dead once stage 2 has run, so
//   J -> Jinv [nq][9] | grad_xi T [nq][3] | s at the Gauss points [nq]  -- (written by stage 3) overlay them; the
//                                                                           residual's transposed stages reuse this space again
//   T2 [3][ng][ng][3][NI] (second stage); the residual's flux [nq][3] + source [nq] overlays it later
//   w det [nq] | int64 rowbase[27] + int32 info[27][8] (colour-scatter matrix variant only)
constexpr int h27_mode_ni(int mode) { return mode == 0 ? 5 : 3; }
constexpr int h27_pad(int v) { return (v + 1) & ~1; }
constexpr int h27_max(int a, int b) { return a > b ? a : b; }
constexpr int h27_n1(int ng, int NI) { return 18 * ng * NI; }
constexpr int h27_n2(int ng, int NI) { return 9 * ng * ng * NI; }
constexpr int h27_n3(int nq, int NI) { return (NI == 3 ? 9 : 13) * nq; }
constexpr int h27_na(int ng) { return 9 * ng * ng; }  // residual, transposed stage A: [3][ng][ng][3]
constexpr int h27_nb(int ng) { return 18 * ng; }      // residual, transposed stage B: [2][ng][9]
constexpr int h27_w_t1(int NI) { return h27_pad(27 * NI); }
constexpr int h27_w_t2(int ng, int nq, int NI) { return h27_max(h27_w_t1(NI) + h27_pad(h27_n1(ng, NI)), h27_pad(h27_n3(nq, NI))); }
constexpr int h27_w_d(int ng, int nq, int NI) { return h27_w_t2(ng, nq, NI) + h27_max(h27_pad(h27_n2(ng, NI)), 4 * h27_pad(nq)); }
constexpr int h27_w_info(int ng, int nq, int NI) { return h27_w_d(ng, nq, NI) + h27_pad(nq); }
constexpr int h27_w_size(int ng, int nq, int NI, bool with_info) { return h27_w_info(ng, nq, NI) + (with_info ? 27 + 27 * 4 + 1 : 0); }
// workgroup-shared decode table of the sum-factorised stages (int32 words)
constexpr int h27_ndec(int ng, int nq, int NI) { return h27_n1(ng, NI) + h27_n2(ng, NI) + h27_n3(nq, NI) + (NI == 3 ? 0 : h27_na(ng) + h27_nb(ng)); }
// the workgroup's block: dN [nqp + 1][3][27] (matrix) | w [nq] | tab1 [2][ng][4] | decode words | H27_WAVES per-wave blocks
constexpr size_t hex27_lds_bytes(int ng, int mode) {
  return sizeof(double) * ((size_t)(mode == 0 ? 0 : (H27_NQP(ng * ng * ng) + 1) * 81) + ((ng * ng * ng + 1) & ~1) + 8 * ng +
                           (h27_pad(h27_ndec(ng, ng * ng * ng, h27_mode_ni(mode))) >> 1) +
                           H27_WAVES * (size_t)h27_w_size(ng, ng * ng * ng, h27_mode_ni(mode), mode == 1));
}

// The same carve-up as k_hex27 spells it: macros over the kernel's own ng, nq and NI.  (Written through the functions above the kernel compiles to
// other instructions; tools/host_check_hex27.cpp expands both and checks that they agree for every ng, mode and wave.)
#define H27_N1 (18 * ng * NI)
#define H27_N2 (9 * ng * ng * NI)
#define H27_N3 ((NI == 3 ? 9 : 13) * nq)
#define H27_NA (9 * ng * ng)
#define H27_NB (18 * ng)
#define W_X 0
#define W_T1 h27_pad(27 * NI)
#define W_J 0
#define W_GX (9 * nq)
#define W_SV (12 * nq)
#define W_VA 0
#define W_WB h27_pad(H27_NA)
#define W_T2 h27_max(W_T1 + h27_pad(H27_N1), h27_pad(H27_N3))
#define W_G W_T2
#define W_D (W_T2 + h27_max(h27_pad(H27_N2), 4 * h27_pad(nq)))
#define W_INFO (W_D + h27_pad(nq))
#define W_SIZE(with_info) (W_INFO + ((with_info) ? 27 + 27 * 4 + 1 : 0))
#define H27_NDEC (H27_N1 + H27_N2 + H27_N3 + (NI == 3 ? 0 : H27_NA + H27_NB))
