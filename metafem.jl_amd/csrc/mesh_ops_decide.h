// The host decisions of the table-free mesh operators (mesh_ops.hip) that are arithmetic alone: the doubles of one wave's LDS block per operator
// (the kernels lay their blocks out with the same functions), whether a launch fits, how many waves share a workgroup, and which slots of the
// physical table the gradient operator keeps.  No HIP, no context: tools/host_check_mesh_ops.cpp walks them on the CPU.
#pragma once
#include <stddef.h>
#if defined(__HIPCC__)
#define MO_HD __host__ __device__
#else
#define MO_HD
#endif

static const size_t MO_LDS_CAP = 64 * 1024;  // bytes of LDS one workgroup (at least one wave) may take

// J^-1, w det, node coordinates (and on facets the normals) of one item
MO_HD static inline size_t mo_geo_doubles(int dim, int itg, int itp, bool facet) {
  return (size_t)itg * (1 + dim * dim) + (size_t)itp * dim + (facet ? (size_t)itg * dim : 0);
}
// var: + the nodal values of nsrc sources and every word of them at the Gauss points
MO_HD static inline size_t mo_var_doubles(int dim, int itg, int itp, bool facet, int nsrc) {
  return mo_geo_doubles(dim, itg, itp, facet) + (size_t)nsrc * itp + (size_t)nsrc * itg * (1 + dim);
}
// res: + the dual words of nfo output fields pulled back to the reference derivatives
MO_HD static inline size_t mo_res_doubles(int dim, int itg, int itp, bool facet, int nfo) {
  return mo_geo_doubles(dim, itg, itp, facet) + (size_t)nfo * itg * (1 + dim);
}
// kval: + ns slots of the physical table and the weighted coefficients of n_terms terms
MO_HD static inline size_t mo_kval_doubles(int dim, int itg, int itp, bool facet, int ns, int n_terms) {
  return mo_geo_doubles(dim, itg, itp, facet) + (size_t)itg * itp * ns + (size_t)n_terms * itg;
}

// What all seven entry points refuse together, so that a group of a domain takes one path: an item's physical table itg * itp * (1 + dim) beyond the cap.
static inline bool mo_table_fits(int dim, int itg, int itp) { return sizeof(double) * (size_t)itg * itp * (1 + dim) <= MO_LDS_CAP; }
// Waves of a workgroup (4, 2 or 1: as many blocks as fit the cap), 0 = one wave's block does not fit.
static inline int mo_waves(size_t per_wave_bytes) {
  if (per_wave_bytes > MO_LDS_CAP) return 0;
  int wv = 4;
  while (wv > 1 && per_wave_bytes * wv > MO_LDS_CAP) wv >>= 1;
  return wv;
}
// Table slots of the gradient operator from the smallest / largest word of its terms: 0 values + gradients, 1 gradients only, 2 values only
static inline int mo_kval_mode(int smin, int smax) { return smax == 0 ? 2 : smin >= 1 ? 1 : 0; }
static inline int mo_kval_slots(int mode, int dim) { return mode == 2 ? 1 : mode == 1 ? dim : 1 + dim; }
static inline int mo_kval_first_slot(int mode) { return mode == 1 ? 1 : 0; }
