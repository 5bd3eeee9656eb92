// CPU walk through the physics rows of the matrix-free brick operator (csrc/brick_operator_physics.h):
//   1. every tag 1 to 4 has exactly one row -- its own --, the tags 0 and 5 (and everything around them) have none;
//   2. fields and interpolation order per row: (1, 1), (3, 1), (1, 2), (3, 2);
//   3. the parameter block a row reads is the block its accepted set-params entry point writes;
//   4. the multigrid entry point of each row: create, create_elasticity, create_hex27, none -- the nonsymmetric entry point is no row's own --, and
//      every value is a valid index of the create entry points' tables or BOP_MG_NONE;
//   5. the signed diagonal: yes, yes, yes, no -- and a physics whose hierarchy can be built has one (the multigrid setup reads the sign of K from it);
//   6. every row has a name, and no two rows share one (the names stand in messages).
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_operator_physics.cpp -o host_check_brick_operator_physics
#include <cstdio>
#include <cstring>
#include "brick_operator_physics.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

int main() {
  static_assert(BOP_PHYSICS_ROWS == 4 && BOP_MG_ENTRIES == 4 && BOP_MG_NONE < 0, "the tables of brick_operator.hip and brick_multigrid.hip are sized by these");
  const int fields[4] = {1, 3, 1, 3}, order[4] = {1, 1, 2, 2};
  const int multigrid[4] = {BOP_MG_CREATE, BOP_MG_CREATE_ELASTICITY, BOP_MG_CREATE_HEX27, BOP_MG_NONE};
  const bool signed_diagonal[4] = {true, true, true, false};
  for (int tag = -3; tag <= 12; ++tag) {
    const BopPhysicsRow* r = bop_physics_row(tag);
    CHECK((r != nullptr) == (tag >= 1 && tag <= 4), "tag %d: a row exactly for the tags 1 to 4", tag);
    if (!r) continue;
    int same = 0;
    for (int other = 1; other <= 4; ++other) same += bop_physics_row(other) == r;
    CHECK(r->tag == tag && same == 1, "tag %d: its own row, once", tag);
    CHECK(r->fields == fields[tag - 1] && r->order == order[tag - 1], "tag %d: %d fields, order %d", tag, r->fields, r->order);
    CHECK(r->block == bop_set_params_block(r->set_params), "tag %d: reads block %d, its set-params entry point writes block %d", tag, (int)r->block,
          (int)bop_set_params_block(r->set_params));
    CHECK((r->block == BOP_BLOCK_ELASTICITY) == (r->fields == 3), "tag %d: three fields are the elasticity block's", tag);
    CHECK(r->multigrid == multigrid[tag - 1] && r->multigrid != BOP_MG_CREATE_NONSYMMETRIC && (r->multigrid == BOP_MG_NONE || (r->multigrid >= 0 && r->multigrid < BOP_MG_ENTRIES)),
          "tag %d: multigrid entry point %d", tag, r->multigrid);
    CHECK(r->signed_diagonal == signed_diagonal[tag - 1] && (r->multigrid == BOP_MG_NONE || r->signed_diagonal), "tag %d: the signed diagonal", tag);
    CHECK(r->name && strlen(r->name) > 0, "tag %d: a name", tag);
    for (int other = 1; other < tag; ++other) CHECK(strcmp(bop_physics_row(other)->name, r->name) != 0, "tags %d and %d share a name", other, tag);
    printf("tag %d: %s, %d field(s), order %d, block %d, set-params %d, multigrid %d, signed diagonal %d\n", tag, r->name, r->fields, r->order, (int)r->block,
           (int)r->set_params, r->multigrid, (int)r->signed_diagonal);
  }
  CHECK(bop_set_params_block(BOP_SET_PARAMS) == BOP_BLOCK_THERMAL && bop_set_params_block(BOP_SET_ELASTICITY_PARAMS) == BOP_BLOCK_ELASTICITY, "what the two entry points write");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
