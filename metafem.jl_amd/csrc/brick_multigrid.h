// What the solve driver (krylov.hip) and the multigrid CG pass (krylov_cg_mg.hip) see of the geometric multigrid hierarchy of a hex-8 thermal or
// elasticity brick operator (brick_multigrid.hip; the host decisions: brick_multigrid_decide.h).
#pragma once
#include "operator.h"

struct mfem_brick_multigrid_s;

// mfem_solve_operator with MFEM_PRECOND_MULTIGRID, in front of mop_solve_gate: MFEM_OK, or MFEM_ERR_UNSUPPORTED with the reason in mfem_last_error()
// (host only: nothing is launched, nothing is written)
int mfem_mg_solve_check(mfem_context_s* ctx, mfem_operator_head* op, const mfem_solve_options* o);
// the hierarchy attached to the operator; a default one is created and attached when there is none (before the solve takes its workspace; thermal
// only: the gate admits an elasticity or a hex-27 operator only with its own hierarchy attached)
int mfem_mg_attach_default(mfem_context_s* ctx, mfem_operator_head* op);
// the setup of the attached hierarchy, inside solve_ms (the operator is not bound yet)
int mfem_mg_setup_attached(mfem_context_s* ctx, mfem_operator_head* op);
// the hierarchy of the operator bound to A (mfem_cg_mg_pass); nullptr: none
mfem_brick_multigrid_s* mfem_mg_of(const mfem_csr_s* A);
// z = Cycle(0, r): enqueued on the context stream, no host synchronisation, no allocation; r is not changed
int mfem_mg_cycle(mfem_context_s* ctx, mfem_brick_multigrid_s* mg, const double* r, double* z);
// level-0 products of one cycle: 2 nu, or nu_c - 1 on a hierarchy of one level
int mfem_mg_level0_products(const mfem_brick_multigrid_s* mg);
