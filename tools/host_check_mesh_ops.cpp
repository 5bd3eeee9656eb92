// CPU walk through the host decisions of the table-free mesh operators (csrc/mesh_ops_decide.h): the doubles of one wave's LDS block for the
// element families of the examples, whether a launch fits the 64 KB cap and how many waves share a workgroup, and the table slots of the
// gradient operator.  The expected sizes are worked out here from the layouts themselves (mesh_ops.hip: wd [itg], J^-1 [itg][dim^2],
// X [itp][dim], normals [itg][dim] on facets, then the operator's own arrays).
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_mesh_ops.cpp -o tools/bin/host_check_mesh_ops && tools/bin/host_check_mesh_ops
#include <cstdio>
#include "mesh_ops_decide.h"

static int bad = 0;
static void eq(size_t got, size_t want, const char* what) {
  if (got != want) { printf("%s: %zu, expected %zu\n", what, got, want); ++bad; }
}

int main() {
  // hex-20, 27 Gauss points: 27 * 10 + 60 = 330 doubles of geometry; facets (9 points on a face, all 20 host nodes): 9 * 10 + 60 + 27 = 177
  eq(mo_geo_doubles(3, 27, 20, false), 330, "geometry, hex-20 elements");
  eq(mo_geo_doubles(3, 9, 20, true), 177, "geometry, hex-20 facets");
  eq(mo_geo_doubles(2, 9, 8, false), 9 * 5 + 16, "geometry, quad-8 elements");
  // var, 3 sources: + 3 * 20 nodal values + 3 * 27 * 4 words
  eq(mo_var_doubles(3, 27, 20, false, 3), 330 + 60 + 324, "var, hex-20, 3 sources");
  // res, 3 dual fields: + 3 * 27 * 4
  eq(mo_res_doubles(3, 27, 20, false, 3), 330 + 324, "res, hex-20, 3 fields");
  // kval, gradients only (3 slots), 48 terms: + 27 * 20 * 3 + 48 * 27 = 1620 + 1296: 25 968 bytes -> two waves per workgroup
  eq(mo_kval_doubles(3, 27, 20, false, 3, 48), 330 + 1620 + 1296, "kval, hex-20, gradients, 48 terms");
  eq((size_t)mo_waves(8 * mo_kval_doubles(3, 27, 20, false, 3, 48)), 2, "waves, hex-20 kval with 48 terms");
  // hex-27 with every slot and 48 terms: (27 * 10 + 81) + 27 * 27 * 4 + 48 * 27 = 4563 doubles = 36 504 bytes -> one wave
  eq(mo_kval_doubles(3, 27, 27, false, 4, 48), 351 + 2916 + 1296, "kval, hex-27, all slots, 48 terms");
  eq((size_t)mo_waves(8 * mo_kval_doubles(3, 27, 27, false, 4, 48)), 1, "waves, hex-27 kval with 48 terms");
  // the cap: exactly 64 KB fits one wave, one byte more does not; 16 KB fits four, 16 KB + 8 two
  eq((size_t)mo_waves(MO_LDS_CAP), 1, "waves at the cap");
  eq((size_t)mo_waves(MO_LDS_CAP + 8), 0, "waves beyond the cap");
  eq((size_t)mo_waves(MO_LDS_CAP / 4), 4, "waves at a quarter of the cap");
  eq((size_t)mo_waves(MO_LDS_CAP / 4 + 8), 2, "waves just above a quarter");
  eq((size_t)mo_waves(MO_LDS_CAP / 2 + 8), 1, "waves just above a half");
  eq((size_t)mo_waves(8), 4, "a tiny block");
  // the table every entry point refuses together: itg * itp * (1 + dim) doubles beyond 64 KB (64 x 32 x 4 = 8192 doubles is the last that fits)
  eq(mo_table_fits(3, 64, 32), 1, "table of exactly 64 KB");
  eq(mo_table_fits(3, 64, 33), 0, "table beyond 64 KB");
  eq(mo_table_fits(3, 64, 64), 0, "table of 128 KB");
  eq(mo_table_fits(3, 27, 20), 1, "hex-20 table");
  eq(mo_table_fits(2, 9, 8), 1, "quad-8 table");
  // table slots of the gradient operator
  eq((size_t)mo_kval_mode(0, 0), 2, "values only");
  eq((size_t)mo_kval_mode(1, 3), 1, "gradients only");
  eq((size_t)mo_kval_mode(0, 3), 0, "values and gradients");
  eq((size_t)mo_kval_mode(0, 1), 0, "a value against a gradient");
  for (int dim = 2; dim <= 3; ++dim) {
    eq((size_t)mo_kval_slots(2, dim), 1, "slots, values only");
    eq((size_t)mo_kval_slots(1, dim), (size_t)dim, "slots, gradients only");
    eq((size_t)mo_kval_slots(0, dim), (size_t)(1 + dim), "slots, everything");
  }
  eq((size_t)mo_kval_first_slot(1), 1, "first slot, gradients only");
  eq((size_t)mo_kval_first_slot(0), 0, "first slot, everything");
  eq((size_t)mo_kval_first_slot(2), 0, "first slot, values only");
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
