// The per-layout planning, binding, release and accounting of the solver layouts.  Internal to layout.hip, which chooses among them, and to the
// files that implement them (spmv_ell.hip with spmv_dia.hip, spmv_sym.hip; spmv_sell.hip with spmv_bsell.hip; spmv_lat27.hip with spmv_lat27_gather.hip; spmv_lat8.hip; the
// tiles' symmetry probe: sym_probe.hip): every other file goes through mfem_layout_* (common.h).  Accounting of the tiles: mfem_lat27_entries /
// _design_bytes and the lat8 twins, their release: mfem_lat_unbind (common.h).
#pragma once
#include "common.h"

int mfem_lat8_plan(mfem_context_s* ctx, mfem_csr_s* A);
bool mfem_lat8_for_method(const mfem_csr_s* A, bool is_cg);  // one-field matrices: only the solvers that work on A D^-1 (cg! keeps the bitwise patch sweep)
size_t mfem_lat8_bytes(const mfem_csr_s* A);
int mfem_lat8_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, double* scratch, bool allow_rem);
int mfem_lat27_plan(mfem_context_s* ctx, mfem_csr_s* A);
size_t mfem_lat27_bytes(const mfem_csr_s* A);
int mfem_lat27_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, double* scratch, bool allow_rem);
int mfem_sell_plan(mfem_context_s* ctx, mfem_csr_s* A);
size_t mfem_sell_vals_bytes(const mfem_csr_s* A);
int mfem_sell_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc);
void mfem_sell_unbind(mfem_csr_s* A);
void mfem_sell_free(mfem_csr_s* A);
int64_t mfem_sell_entries(const mfem_csr_s* A);       // matrix entries (8-byte values) one SpMV reads from memory
int64_t mfem_sell_design_bytes(const mfem_csr_s* A);  // bytes one SpMV moves by design
int mfem_ell_plan(mfem_context_s* ctx, mfem_csr_s* A);
size_t mfem_ell_vals_bytes(const mfem_csr_s* A);
int mfem_ell_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, const double* ssym);
bool mfem_dia_layout_planned(const mfem_csr_s* A);  // mfem_ell_bind would make the diagonal-slotted copy (mode 2)
void mfem_ell_unbind(mfem_csr_s* A);
void mfem_ell_free(mfem_csr_s* A);
int64_t mfem_ell_entries(const mfem_context_s* ctx, const mfem_csr_s* A, int32_t* sweep);  // modes 1 and 2; *sweep: 2 / 1 = the structure allows the patch / the tile sweep
int64_t mfem_ell_design_bytes(const mfem_context_s* ctx, const mfem_csr_s* A);
