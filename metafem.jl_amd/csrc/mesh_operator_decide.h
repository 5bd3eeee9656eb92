// The host decisions of the matrix-free mesh operator (mesh_operator.hip, mfem_solve_operator in krylov.hip) that are arithmetic alone: the terms of a
// part compiled, grouped and merged into the program the kernels read, the caps, the doubles of one wave's LDS block and the waves of a workgroup,
// where every part's element vectors lie in the scratch and where the scratch lies in the solve's workspace, and which solve options the operator
// accepts.  No HIP, no context: tools/host_check_mesh_operator.cpp and tools/host_check_mesh_operator_var.cpp walk them on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/metafem_mi355x.h"

#define MOP_MAX_TERMS 48     // constant terms of one part
#define MOP_MAX_VAR_TERMS 128  // variable terms of one part (coefficient arrays at the Gauss points)
#define MOP_MAX_FIELDS 8     // dual fields of one part, and base fields (sources) of one part
#define MOP_MAX_ENTRIES 128  // distinct (base field, base word, normal) monomials of one part, after merging per dual word, plus its variable terms
#define MOP_MAX_PARTS 8      // the elements + facet groups
#define MOP_MAX_NFIELDS 32   // fields of the system
static const size_t MOP_LDS_CAP = 64 * 1024;  // bytes of LDS one wave's block may take

// The terms of one part, compiled for the kernels (passed by value; read with wave-uniform or small indices).  y[f][a] of an item is
//   sum_q sum_{g of f} D^{grp_sd[g]} N_a(q) * w_q det_q * sum_{e of g} ent_coef[e] [n_{ent_nrm[e]}(q)] D^{ent_word[e]} x_{src_pos[ent_src[e]]}(q)
// The entries of group g are its constant ones, [grp_end[g - 1], grp_var[g]), then its variable ones, [grp_var[g], grp_end[g]), in the order the
// caller gave them and never merged: entry e of those takes its coefficient from the caller's array, term ent_nrm[e] (the slot), at [q, item].
struct OpProgram {
  int nsrc, ngroups, nfo, nent;
  int32_t src_pos[MOP_MAX_FIELDS];      // base field of source k
  int8_t grp_sd[MOP_MAX_TERMS];         // dual word of group g (groups sorted by dual field, then word)
  int16_t grp_end[MOP_MAX_TERMS];       // entries of group g: [grp_end[g - 1], grp_end[g])
  int8_t ent_src[MOP_MAX_ENTRIES];      // source
  int8_t ent_word[MOP_MAX_ENTRIES];     // base word
  int8_t ent_nrm[MOP_MAX_ENTRIES];      // -1, or j: times n_j
  double ent_coef[MOP_MAX_ENTRIES];
  int32_t fo_pos[MOP_MAX_FIELDS];       // dual field of output fo
  int8_t fo_g0[MOP_MAX_FIELDS + 1];     // groups of output fo: [fo_g0[fo], fo_g0[fo + 1])
  int16_t grp_var[MOP_MAX_TERMS];       // first variable entry of group g (== grp_end[g]: none); behind the fields of the constant program
  int32_t nvar;                         // variable entries of the part
};
static_assert(sizeof(OpProgram) < 2048, "OpProgram travels in the kernel arguments");

// Checks the caller's constant terms and variable terms (vterms: n_var of them, slot = position in the list) and compiles them into one program.
// MFEM_OK, MFEM_ERR_INVALID or MFEM_ERR_UNSUPPORTED; *why names the reason of a refusal.  With n_var == 0 the program is the constant one.
static inline int mop_compile_mixed(int dim, bool facet, int n_fields, int32_t n_terms, const mfem_operator_term* terms, int32_t n_var,
                                    const mfem_kval_term* vterms, OpProgram* P, const char** why) {
  static const char* none = "";
  *why = none;
  if (n_terms < 0 || (n_terms > 0 && !terms)) { *why = "terms missing"; return MFEM_ERR_INVALID; }
  if (n_var < 0 || (n_var > 0 && !vterms)) { *why = "variable terms missing"; return MFEM_ERR_INVALID; }
  if (n_terms > MOP_MAX_TERMS) { *why = "more than 48 terms in one part"; return MFEM_ERR_UNSUPPORTED; }
  memset(P, 0, sizeof(*P));
  for (int i = 0; i < n_var; ++i) {  // (checked before the cap: a list with a bad word is invalid however long it is)
    const mfem_kval_term& T = vterms[i];
    if (T.dual_sd < 0 || T.dual_sd > dim || T.base_sd < 0 || T.base_sd > dim) { *why = "term words: 0 = value, 1 + j = d/dx_j"; return MFEM_ERR_INVALID; }
    if (T.block < 0 || T.block >= n_fields * n_fields) { *why = "term block out of range"; return MFEM_ERR_INVALID; }
  }
  if (n_var > MOP_MAX_VAR_TERMS) { *why = "more than 128 variable terms in one part"; return MFEM_ERR_UNSUPPORTED; }
  for (int i = 0; i < n_terms; ++i) {
    const mfem_operator_term& T = terms[i];
    if (T.dual_sd < 0 || T.dual_sd > dim || T.base_sd < 0 || T.base_sd > dim) { *why = "term words: 0 = value, 1 + j = d/dx_j"; return MFEM_ERR_INVALID; }
    if (T.block < 0 || T.block >= n_fields * n_fields) { *why = "term block out of range"; return MFEM_ERR_INVALID; }
    if (!(T.coef == T.coef)) { *why = "term coefficient is not a number"; return MFEM_ERR_INVALID; }
    for (int j = 0; j < 3; ++j) {
      if (!(T.normal_coef[j] == T.normal_coef[j])) { *why = "term coefficient is not a number"; return MFEM_ERR_INVALID; }
      if (T.normal_coef[j] != 0.0 && (!facet || j >= dim)) { *why = "normal_coef must be 0 on elements and beyond the dimension"; return MFEM_ERR_INVALID; }
    }
  }
  // groups = distinct (dual field, dual word), sorted by field then word (stable: the terms of a group keep their order, the constant ones first)
  const int n_all = n_terms + n_var;
  int order[MOP_MAX_TERMS + MOP_MAX_VAR_TERMS];
  for (int i = 0; i < n_all; ++i) order[i] = i;
  auto blk = [&](int i) { return i < n_terms ? terms[i].block : vterms[i - n_terms].block; };
  auto dsd = [&](int i) { return i < n_terms ? terms[i].dual_sd : vterms[i - n_terms].dual_sd; };
  auto bsd = [&](int i) { return i < n_terms ? terms[i].base_sd : vterms[i - n_terms].base_sd; };
  auto dpos = [&](int i) { return blk(i) / n_fields; };
  for (int i = 1; i < n_all; ++i)
    for (int j = i; j > 0; --j) {
      const int a = order[j - 1], b = order[j];
      if (dpos(a) < dpos(b) || (dpos(a) == dpos(b) && dsd(a) <= dsd(b))) break;
      order[j - 1] = b;
      order[j] = a;
    }
  int nent = 0;
  for (int ii = 0; ii < n_all; ++ii) {
    const int it = order[ii];
    const int dp = blk(it) / n_fields, bp = blk(it) % n_fields;
    const bool new_field = ii == 0 || dp != dpos(order[ii - 1]);
    if (new_field || dsd(it) != dsd(order[ii - 1])) {
      if (new_field) {
        if (P->nfo == MOP_MAX_FIELDS) { *why = "more than 8 dual fields in one part"; return MFEM_ERR_UNSUPPORTED; }
        P->fo_pos[P->nfo] = dp;
        P->fo_g0[P->nfo] = (int8_t)P->ngroups;
        ++P->nfo;
      }
      P->grp_sd[P->ngroups] = (int8_t)dsd(it);
      P->grp_var[P->ngroups] = (int16_t)nent;
      ++P->ngroups;
    }
    const int g = P->ngroups - 1;
    int s = 0;
    while (s < P->nsrc && P->src_pos[s] != bp) ++s;
    if (s == P->nsrc) {
      if (P->nsrc == MOP_MAX_FIELDS) { *why = "more than 8 base fields in one part"; return MFEM_ERR_UNSUPPORTED; }
      P->src_pos[P->nsrc++] = bp;
    }
    const int g_begin = g ? P->grp_end[g - 1] : 0;
    if (it >= n_terms) {  // a variable term: an entry of its own behind the constant ones of its dual word
      if (nent == MOP_MAX_ENTRIES) { *why = "more than 128 entries (distinct constant monomials plus variable terms) in one part"; return MFEM_ERR_UNSUPPORTED; }
      P->ent_src[nent] = (int8_t)s;
      P->ent_word[nent] = (int8_t)bsd(it);
      P->ent_nrm[nent] = (int8_t)(it - n_terms);  // the slot
      P->ent_coef[nent] = 0.0;
      ++nent;
      ++P->nvar;
      P->grp_end[g] = (int16_t)nent;
      continue;
    }
    const mfem_operator_term& T = terms[it];
    for (int j = -1; j < 3; ++j) {
      const double c = j < 0 ? T.coef : T.normal_coef[j];
      if (c == 0.0) continue;
      int e = g_begin;
      while (e < nent && !(P->ent_src[e] == s && P->ent_word[e] == T.base_sd && P->ent_nrm[e] == j)) ++e;  // (equal monomials of a dual word merge)
      if (e == nent) {
        if (nent == MOP_MAX_ENTRIES) { *why = "more than 128 distinct (field, word, normal) monomials in one part"; return MFEM_ERR_UNSUPPORTED; }
        P->ent_src[e] = (int8_t)s;
        P->ent_word[e] = (int8_t)T.base_sd;
        P->ent_nrm[e] = (int8_t)j;
        P->ent_coef[e] = 0.0;
        ++nent;
      }
      P->ent_coef[e] += c;
    }
    P->grp_end[g] = (int16_t)nent;
    P->grp_var[g] = (int16_t)nent;
  }
  P->fo_g0[P->nfo] = (int8_t)P->ngroups;
  P->nent = nent;
  return MFEM_OK;
}
static inline int mop_compile(int dim, bool facet, int n_fields, int32_t n_terms, const mfem_operator_term* terms, OpProgram* P, const char** why) {
  return mop_compile_mixed(dim, facet, n_fields, n_terms, terms, 0, nullptr, P, why);
}

// One wave's LDS block of the product kernel: w det, J^-1, node coordinates, (facets) normals, the nodal values of the sources, their words at the
// Gauss points, the weighted dual words, the dual words pulled back to the reference derivatives.  The diagonal kernel takes the geometry alone.
static inline size_t mop_geo_doubles(int dim, int itg, int itp, bool facet) {
  return (size_t)itg * (1 + dim * dim) + (size_t)itp * dim + (facet ? (size_t)itg * dim : 0);
}
static inline size_t mop_wave_doubles(int dim, int itg, int itp, bool facet, int nsrc, int nfo, int ngroups) {
  return mop_geo_doubles(dim, itg, itp, facet) + (size_t)nsrc * itp + (size_t)(nsrc + nfo) * itg * (1 + dim) + (size_t)ngroups * itg;
}
// Waves of a workgroup (4, 2 or 1: as many blocks as fit the cap); 0 = one wave's block does not fit: MFEM_ERR_UNSUPPORTED at the set / add call.
static inline int mop_waves(size_t per_wave_doubles) {
  const size_t bytes = per_wave_doubles * sizeof(double);
  if (bytes > MOP_LDS_CAP) return 0;
  int wv = 4;
  while (wv > 1 && bytes * wv > MOP_LDS_CAP) wv >>= 1;
  return wv;
}

// The element-major scratch: part p holds n_items[p] * itp * nfo[p] doubles, the parts in the order they were added.  offsets[p] in doubles; returns the total.
static inline size_t mop_scratch_layout(int n_parts, const int64_t* n_items, const int* nfo, int itp, size_t* offsets) {
  size_t total = 0;
  for (int p = 0; p < n_parts; ++p) {
    if (offsets) offsets[p] = total;
    total += (size_t)n_items[p] * (size_t)itp * (size_t)nfo[p];
  }
  return total;
}

// The workspace of mfem_solve_operator: x, b, d, 1 / d and the work vectors (nv doubles each, nv a multiple of 32), the scratch right behind them,
// then gmres!'s block at the next multiple of 256 bytes.  No layout copy, no copy of a matrix.
struct OpWorkspace {
  size_t vec_bytes, scratch_offset, gm_offset, total;
};
static inline OpWorkspace mop_workspace(int64_t nv, int nwork, size_t scratch_doubles, size_t gmres_bytes) {
  OpWorkspace W;
  W.vec_bytes = (size_t)nv * sizeof(double);
  W.scratch_offset = W.vec_bytes * (size_t)(4 + nwork);
  W.total = W.scratch_offset + scratch_doubles * sizeof(double);
  W.gm_offset = (W.total + 255) / 256 * 256;
  if (gmres_bytes) W.total = W.gm_offset + gmres_bytes;
  return W;
}

// Which solve options the operator takes (method / precond / left_precond already inside their enums).  What needs columns or rows of K or a product
// with A' is MFEM_ERR_UNSUPPORTED; what asks to write into a matrix that does not exist, or for more than one rank, is MFEM_ERR_INVALID.
static inline int mop_solve_gate(int method, int precond, int left_precond, int scale_in_place, bool has_comm, const char** why) {
  *why = "";
  if (method == MFEM_SOLVER_LSQR) { *why = "lsqr! needs products with A': not on a matrix-free operator"; return MFEM_ERR_UNSUPPORTED; }
  if (precond == MFEM_PRECOND_JACOBI_RIGHT_COLNORM) { *why = "the column-norm scaling needs the columns of K: not on a matrix-free operator"; return MFEM_ERR_UNSUPPORTED; }
  if (left_precond != MFEM_LEFT_NONE) { *why = "a left preconditioner needs the rows of K: not on a matrix-free operator"; return MFEM_ERR_UNSUPPORTED; }
  if (scale_in_place) { *why = "scale_in_place: a matrix-free operator has no values to scale"; return MFEM_ERR_INVALID; }
  if (has_comm) { *why = "the matrix-free operator runs on one rank only: no communicator may be attached"; return MFEM_ERR_INVALID; }
  return MFEM_OK;
}
