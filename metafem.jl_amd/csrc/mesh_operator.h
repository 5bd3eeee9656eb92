// The matrix-free mesh operator as the solve driver (krylov.hip) and the product dispatch (spmv.hip) see it; the handle, the kernels and their
// launches live in mesh_operator.hip, the host decisions in mesh_operator_decide.h.
#pragma once
#include "common.h"

struct mfem_mesh_operator_s;
mfem_mesh_operator_s* mfem_mesh_operator_from_handle(uint64_t handle);
mfem_context_s* mfem_mesh_operator_ctx(mfem_mesh_operator_s* op);
mfem_csr_s* mfem_mesh_operator_csr(mfem_mesh_operator_s* op);            // the internal pattern-less handle: n = n_fields * ncp, nnz = 0
size_t mfem_mesh_operator_scratch_doubles(const mfem_mesh_operator_s* op);
// Binds the operator to its handle for a solve: products on mfem_mesh_operator_csr(op) go to the operator from here on, with their element vectors
// in `scratch` and, if dsc != nullptr, the column scaling x_j / dsc_j applied while x is gathered.  unbind releases it.
void mfem_mesh_operator_bind(mfem_mesh_operator_s* op, double* scratch, const double* dsc);
void mfem_mesh_operator_unbind(mfem_mesh_operator_s* op);
// d (preset by the caller) <- |K_ii| where row i has adjacency and K_ii != 0: the guarded rule of jacobi.hip.  scratch as above.
int mfem_mesh_operator_jacobi(mfem_context_s* ctx, mfem_mesh_operator_s* op, double* scratch, double* d);
// y = alpha K x + beta y on the bound operator of A, under the contract of spmv_launch_inner (dot partials, done_flag)
int mfem_mesh_operator_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* x, double* y, double alpha, double beta, const double* dotw,
                              double* partials, int* n_partials, const int32_t* done_flag);
