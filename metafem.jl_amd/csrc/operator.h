// The matrix-free operators as the solve driver (krylov.hip: mfem_solve_operator) and the product dispatch (spmv.hip) see them: one small
// interface, two kinds -- the unstructured-mesh operator (mesh_operator.hip) and the hex-8 brick operator (brick_operator.hip).  Every operator
// handle starts with a kind tag; the driver reads the tag, takes the kind's table and never looks further into the handle.
#pragma once
#include "common.h"

enum mfem_operator_kind : uint32_t { MFEM_OPERATOR_MESH = 0x4d4f504du /* "MPOM" */, MFEM_OPERATOR_BRICK = 0x4d4f5042u /* "BPOM" */ };
struct mfem_operator_head {
  uint32_t kind;  // mfem_operator_kind: the first member of mfem_mesh_operator_s and of mfem_brick_operator_s
};

struct mfem_operator_interface {
  mfem_context_s* (*ctx)(mfem_operator_head* op);
  mfem_csr_s* (*csr)(mfem_operator_head* op);                  // the internal pattern-less handle: n rows, nnz = 0
  size_t (*scratch_doubles)(const mfem_operator_head* op);     // what a product needs behind the solver's vectors (the brick operator: 0)
  // Binds the operator to its handle for a solve: products on csr(op) go to the operator from here on, with `scratch` and, if dsc != nullptr, the
  // column scaling x_j / dsc_j applied while x is read.  unbind releases it.
  // bind returns a status: what an operator has to verify before the driver may replay a cached cycle (which enters no launcher) is verified here.
  int (*bind)(mfem_operator_head* op, double* scratch, const double* dsc);
  void (*unbind)(mfem_operator_head* op);
  // d (preset by the caller) <- |K_ii| where row i has a non-zero diagonal: the guarded rule of jacobi.hip
  int (*jacobi)(mfem_context_s* ctx, mfem_operator_head* op, double* scratch, double* d);
  // y = alpha K x + beta y on the bound operator of A, under the contract of spmv_launch_inner (dot partials, done_flag)
  int (*launch)(mfem_context_s* ctx, mfem_csr_s* A, const double* x, double* y, double alpha, double beta, const double* dotw, double* partials,
                int* n_partials, const int32_t* done_flag);
};
const mfem_operator_interface* mfem_mesh_operator_interface();   // mesh_operator.hip
const mfem_operator_interface* mfem_brick_operator_interface();  // brick_operator.hip

// the table of a handle's kind; nullptr: no handle, or not an operator's
static inline const mfem_operator_interface* mfem_operator_interface_of(const mfem_operator_head* op) {
  if (!op) return nullptr;
  switch (op->kind) {
    case MFEM_OPERATOR_MESH: return mfem_mesh_operator_interface();
    case MFEM_OPERATOR_BRICK: return mfem_brick_operator_interface();
  }
  return nullptr;
}
