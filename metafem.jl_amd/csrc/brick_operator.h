// What the files of the matrix-free brick operator share: brick_operator.hip (the handle of every physics, the bind, every entry point, the ops table;
// no kernel) and one file of kernels and launchers per physics -- brick_operator_thermal.hip (hex-8 thermal), brick_operator_elasticity.hip (hex-8
// elasticity), brick_operator_hex27.hip with brick_operator_hex27_diagonal.hip (hex-27 thermal), brick_operator_elasticity_hex27.hip (hex-27 elasticity).
// The library is one code object per .hip file and a kernel is launched from the file that defines it, so the device functions here are inline copies
// per file; the hex-8 reference tables have ONE owner (bop_tables, brick_operator.hip).  Every physics hands over through launchers of one signature,
// declared below and gathered in the ops table of brick_operator.hip; what a physics IS (fields, parameter block, ...) is its row in
// brick_operator_physics.h.
#pragma once
#include "hex8_device.h"
#include "brick_operator_decide.h"
#include "operator.h"
#include "brick_operator_physics.h"

// Reference-cell tables in device memory, one IMMUTABLE copy per (device, rule), made when the first operator with that rule is created and kept for the
// life of the process.  The constant-memory tables of hex8_device.h are one mutable copy per file, re-uploaded whenever the rule changes: a solver cycle
// captured with one rule and replayed from the graph cache after a brick with another rule had been served would read the wrong tables, and an
// upload at launch is a synchronous copy inside a stream capture.  These kernels therefore take a pointer that never changes its contents, and nothing
// is uploaded at launch.
int bop_tables(int device, int ng, const H8Tables** out);  // brick_operator.hip

// hex8_geom and face_geom of hex8_device.h on those tables
__device__ __forceinline__ double bop_geom(const H8Tables* __restrict__ T, const double (&X)[8][3], int q, double (&g)[8][3]) {
  double J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < 8; ++b) s += T->dN[q][b][m] * X[b][i];
      J[i][m] = s;
    }
  const double det = J[0][0] * J[1][1] * J[2][2] - J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] +
                     J[0][1] * J[1][2] * J[2][0] + J[0][2] * J[1][0] * J[2][1] - J[0][2] * J[1][1] * J[2][0];
  const double id = 1.0 / det;
  double I[3][3];
  I[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
  I[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
  I[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) * id;
  I[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) * id;
  I[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
  I[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
  I[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
  I[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) * id;
  I[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) * id;
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int s = 0; s < 3; ++s) g[b][s] = T->dN[q][b][0] * I[0][s] + T->dN[q][b][1] * I[1][s] + T->dN[q][b][2] * I[2][s];
  return T->w[q] * det;
}
__device__ __forceinline__ double bop_face_weight(const H8Tables* __restrict__ T, const double (&Xf)[4][3], int q, bool low_face) {
  double t1[3], t2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a += T->fdN[q][c][0] * Xf[c][i];
      b += T->fdN[q][c][1] * Xf[c][i];
    }
    t1[i] = low_face ? -a : a;
    t2[i] = b;
  }
  const double r0 = t1[1] * t2[2] - t1[2] * t2[1];
  const double r1 = -t1[0] * t2[2] + t1[2] * t2[0];
  const double r2 = t1[0] * t2[1] - t1[1] * t2[0];
  return T->fw[q] * sqrt(r0 * r0 + r1 * r1 + r2 * r2);
}

enum { BOP_PHYSICS_THERMAL = 1, BOP_PHYSICS_ELASTICITY = 2, BOP_PHYSICS_HEX27 = 3, BOP_PHYSICS_ELASTICITY_HEX27 = 4 };  // (HEX27: thermal on an order-2 brick.  ELASTICITY_HEX27: elasticity on an order-2 brick; of its parameter block traction_faces and sig are read too, by the residual entry point.  What else a tag means: its row, bop_physics_row)
static_assert(BOP_PHYSICS_THERMAL == 1 && BOP_PHYSICS_ELASTICITY == 2 && BOP_PHYSICS_HEX27 == 3 && BOP_PHYSICS_ELASTICITY_HEX27 == BOP_PHYSICS_ROWS,
              "brick_operator_physics.h spells the tags out");
struct Hex27Tables;  // hex27.h
struct mfem_brick_operator_s {
  mfem_operator_head head;  // MFEM_OPERATOR_BRICK (operator.h)
  mfem_context_s* ctx;
  mfem_brick_s* brick;      // borrowed: coordinates are read live at every product
  int physics;              // BOP_PHYSICS_*: its row says which parameter block is set
  mfem_thermal_params thermal;
  mfem_elasticity_params elasticity;  // (traction_faces and sig are kept as sent and never read: they contribute nothing to K)
  const H8Tables* tables;   // bop_tables(ctx->device, brick->ng): immutable (hex-8 physics)
  const Hex27Tables* tables27;  // bop27_tables(ctx->device, brick->ng): immutable (BOP_PHYSICS_HEX27, BOP_PHYSICS_ELASTICITY_HEX27)
  int ng;                   // the brick's rule when the operator was created
  const double* seen_x0;    // the brick's first coordinate array at the last bind (a change starts a new epoch of the cycle-graph key)
  mfem_csr_s csr;           // pattern-less: what the Krylov loop holds in place of a matrix (n = fields x control points)
  struct mfem_brick_multigrid_s* mg;  // the multigrid hierarchy attached to a hex-8 thermal or elasticity or a hex-27 thermal operator (brick_multigrid.hip), or nullptr; destroyed with the operator
};
mfem_brick_operator_s* bop_from_handle(uint64_t handle);  // brick_operator.hip: nullptr unless the handle is a brick operator's
inline const BopPhysicsRow& bop_row(const mfem_brick_operator_s* op) { return *bop_physics_row(op->physics); }  // (bop_create admits no tag without a row)
// brick_operator.hip: the brick as it is NOW, refused (MFEM_ERR_UNSUPPORTED, "matrix-free brick operator: ...") when the physics no longer takes it, or
// MFEM_ERR_INVALID when its size or rule changed under the operator; what every launcher below is handed
int bop_view(const mfem_brick_operator_s* op, BrickView* B);
// diag K of a hex-8 thermal or elasticity or of a hex-27 thermal operator WITH its sign (d_i <- K_ii where K_ii != 0; a zero diagonal keeps the
// caller's preset -- hex-27: is written as 0, which is what the multigrid setup presets; elasticity: 3 x control points entries, field-major): what the
// multigrid setup reads the sign of K from
int bop_signed_diagonal(mfem_context_s* ctx, mfem_brick_operator_s* op, double* d);
void mfem_mg_release(struct mfem_brick_multigrid_s* mg);  // brick_multigrid.hip: frees a hierarchy (its operator is being destroyed, or it is destroyed on its own)

__device__ __forceinline__ double bop_scaled(const double* __restrict__ x, const double* __restrict__ dsc, int64_t i) {
  return dsc ? x[i] / dsc[i] : x[i];
}

// brick_operator_thermal.hip: the product and the diagonal of an operator with physics == BOP_PHYSICS_THERMAL, on the view its caller verified (bop_view).
// The launch contract is bop_launch's (stated at the top of that file); the three physics below follow it.
int bop_thermal_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                       double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag);
int bop_thermal_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);
int bop_thermal_signed_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);  // K_ii itself (bop_signed_diagonal)

// brick_operator_elasticity.hip: the same of an operator with physics == BOP_PHYSICS_ELASTICITY.
int bop_elasticity_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                          double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag);
int bop_elasticity_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);
int bop_elasticity_signed_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);  // K_ii itself (bop_signed_diagonal)

// brick_operator_hex27.hip: the product and the diagonal of an operator with physics == BOP_PHYSICS_HEX27 (thermal, order-2 brick) under the same
// contract; its immutable per-(device, rule) tables; bop27_prepare raises the volume kernel's dynamic-LDS limit (when an operator is created: never at
// a launch).
int bop27_tables(int device, int ng, const Hex27Tables** out);
int bop27_prepare(int ng);
int bop27_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                 double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag);
int bop27_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);
// brick_operator_hex27_diagonal.hip: K_ii itself for EVERY control point (a zero diagonal is written as 0), as a plane sweep on the product's skeleton
// (bop_signed_diagonal: the multigrid setup); bop27_diagonal_prepare raises that kernel's dynamic-LDS limit beside bop27_prepare
int bop27_signed_diagonal(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);
int bop27_diagonal_prepare(int ng);

// brick_operator_elasticity_hex27.hip: the product and the diagonal of an operator with physics == BOP_PHYSICS_ELASTICITY_HEX27 (three-field elasticity,
// order-2 brick) under the same contract, on bop27_tables' tables; bop_e27_prepare raises the volume kernel's dynamic-LDS limit (when an operator is
// created: never at a launch).  mfem_brick_operator_residual_elasticity is defined beside its kernels.
int bop_e27_prepare(int ng);
int bop_e27_launch(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, const double* x, const double* dsc, double* y, double alpha,
                   double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag);
int bop_e27_jacobi(mfem_context_s* ctx, const mfem_brick_operator_s* op, const BrickView& B, double* d);
