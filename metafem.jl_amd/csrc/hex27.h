// What the files of the hex-27 thermal assembly share (assemble_hex27.hip: tables, k_hex27, the Robin faces, the residual and the driver;
// hex27_gather.hip: pass 2 of the two-pass ring; hex27_direct.hip: the scratch-free rows of affine / mixed meshes; hex27_rows.hip: the row owners of
// general elements): the reference tables, the kernel argument records, the row order of the scratch, and one launch function per kernel outside
// the driver's file.  The tile constants and every host decision: hex27_decide.h.
#pragma once
#include "brick.h"
#include "hex27_decide.h"

static_assert(H27_FACE_BLOCK == MFEM_BLOCK, "the face schedule sizes its grids for MFEM_BLOCK threads");

#define H27_MAXQ 64

struct Hex27Tables {        // device-global, filled once per ng
  double dN[H27_MAXQ][3][27];  // [q][m][a]: lanes that differ in a (or in (q, m)) read different LDS banks
  double N[H27_MAXQ][27];
  double w[H27_MAXQ];
  double tab1[2][4][4];       // 1-D Lagrange-2 values (k = 0) and derivatives (k = 1) at the ng Gauss points: [k][q][a], rows padded to 4
  double T1[4][3][4];         // affine elements: 1-D integrals over the ng Gauss points, [X][a][b] (rows padded to 4): X = 0: sum w l'_a l'_b, 1: sum w l_a l_b,
                              // 2: sum w l'_a l_b, 3: sum w l_a l'_b -- the reference integrals of Ke are products of three of them (tensor-product basis and quadrature)
  // face tables: 2-D Lagrange-2 on [0,1]^2 at ng x ng Gauss points, c = c1 + 3*c2
  double fN[16][9];
  double fdN[16][9][2];
  double fw[16];
};
// the device copy, filled for the ng of the last hex27_upload_tables (assemble_hex27.hip owns it)
const Hex27Tables* hex27_tables();
// the tables of ng Gauss points per direction, filled on the host (assemble_hex27.hip)
void hex27_fill_tables(int ng, Hex27Tables* h);

struct Hex27Args {
  BrickView B;
  const Hex27Tables* tab;
  double kcond;
  int affine_fast;   // matrix: elements whose 27 nodes are an affine image of the reference nodes (to round-off) take the constant-Jacobian shortcut
  int colour;        // 0..7: (I&1) | (J&1)<<1 | (K&1)<<2
  int nq, ng;
  int e_lo, e_cnt, ring;  // element planes [e_lo, e_lo + e_cnt) of dimension 0 this launch covers; scratch variant: plane I kept in ring slot I % ring
  // mixed meshes (round 5): pass 1 over a LIST of elements only -- elist[k] = index (I - e_lo, J, K) of the k-th non-affine element inside the planes
  // above, its Ke goes to scratch slot k; nullptr: every element of the planes
  const int32_t* elist;
  int64_t ecount;
};

struct Face27Args {
  BrickView B;
  const Hex27Tables* tab;
  double h, Tenv;
  int nd, side, colour, ng;
};

// Row order of an element's Ke in the scratch: dimension-2 index fastest (a = a0 + 3 a1 + 9 a2 -> a2 + 3 a1 + 9 a0).  The
// gather walks the control points with dimension 2 fastest, so the three rows an element gives to one wave are one
// contiguous 648-byte piece and the nine rows of a dimension-0 layer (1944 bytes) are used within a few workgroups of each
// other -- whole cache lines get used while they are resident.
__device__ __forceinline__ int scratch_row(int a) { return a / 9 + 3 * ((a / 3) % 3) + 9 * (a % 3); }

// hex27_gather.hip -- pass 2 of the two-pass path: the CSR rows [row_lo, row_hi) from the ring `ke` of element planes
int hex27_launch_gather(mfem_context_s* ctx, const BrickView& B, const double* ke, double* vals, int64_t row_lo, int64_t row_hi, int ring);
// hex27_direct.hip -- G0 of the elements of the planes [elo, elo + ecnt) -> g; *d_cnt (cleared here) counts the non-affine ones, slot / elist map them
// to and from their places in the compact scratch
int hex27_launch_g0(mfem_context_s* ctx, const BrickView& B, double kcond, int elo, int ecnt, double* g, int32_t* d_cnt, int32_t* slot, int32_t* elist);
// ... and every owned row from g (slot_of == nullptr: all elements affine; else the runs of element e with slot_of[e] >= 0 are read from ke)
int hex27_launch_direct(mfem_context_s* ctx, const BrickView& B, const double* g, double* vals, int elo, const int32_t* slot_of, const double* ke);
// hex27_rows.hip -- G_q of every element of the planes -> gq; every owned row from gq
int hex27_launch_gq(mfem_context_s* ctx, const BrickView& B, double kcond, int elo, int ecnt, double* gq);
int hex27_launch_rows(mfem_context_s* ctx, const BrickView& B, const double* gq, double* vals, int elo, int ecnt, int ablate);
