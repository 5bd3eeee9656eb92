// The physics of the matrix-free brick operator as host data: one row per BOP_PHYSICS_* tag (the enum: brick_operator.h, which includes this header and
// asserts the tag numbers spelled out here), read wherever the handle's files and brick_multigrid.hip used to test the tag.  Plain C++, no HIP, no
// context: tools/host_check_brick_operator_physics.cpp walks the rows on the CPU.  What a row cannot hold -- the launchers, which are functions of the
// .hip files -- is the ops table of brick_operator.hip, indexed by the same tag.  A new physics is a row here, an entry there and a file of kernels.
#pragma once

enum BopBlock { BOP_BLOCK_THERMAL, BOP_BLOCK_ELASTICITY };  // which parameter block of the handle a row reads: .thermal or .elasticity
enum BopSetParams { BOP_SET_PARAMS, BOP_SET_ELASTICITY_PARAMS };  // mfem_brick_operator_set_params, mfem_brick_operator_set_elasticity_params
static inline BopBlock bop_set_params_block(BopSetParams entry) { return entry == BOP_SET_PARAMS ? BOP_BLOCK_THERMAL : BOP_BLOCK_ELASTICITY; }  // the block it writes
// the mfem_brick_multigrid_create* entry points, in the order of brick_multigrid.hip's tables
enum { BOP_MG_NONE = -1, BOP_MG_CREATE, BOP_MG_CREATE_NONSYMMETRIC, BOP_MG_CREATE_ELASTICITY, BOP_MG_CREATE_HEX27, BOP_MG_ENTRIES };

struct BopPhysicsRow {
  int tag;                  // BOP_PHYSICS_*
  int fields;               // per control point: the handle has n = fields x control points unknowns, field-major
  int order;                // interpolation order of the brick: 1 (hex-8), 2 (hex-27)
  BopBlock block;
  BopSetParams set_params;  // the one set-params entry point the operator accepts (the other answers MFEM_ERR_INVALID)
  int multigrid;            // the entry point that builds its hierarchy (BOP_MG_CREATE also stands for _NONSYMMETRIC), or BOP_MG_NONE
  bool signed_diagonal;     // bop_signed_diagonal exists (the multigrid setup reads the sign of K from it)
  const char* name;
};
#define BOP_PHYSICS_ROWS 4
// nullptr: not a physics tag
static inline const BopPhysicsRow* bop_physics_row(int tag) {
  static const BopPhysicsRow rows[BOP_PHYSICS_ROWS] = {
      {1, 1, 1, BOP_BLOCK_THERMAL, BOP_SET_PARAMS, BOP_MG_CREATE, true, "hex-8 thermal"},
      {2, 3, 1, BOP_BLOCK_ELASTICITY, BOP_SET_ELASTICITY_PARAMS, BOP_MG_CREATE_ELASTICITY, true, "hex-8 elasticity"},
      {3, 1, 2, BOP_BLOCK_THERMAL, BOP_SET_PARAMS, BOP_MG_CREATE_HEX27, true, "hex-27 thermal"},
      {4, 3, 2, BOP_BLOCK_ELASTICITY, BOP_SET_ELASTICITY_PARAMS, BOP_MG_NONE, false, "hex-27 elasticity"},
  };
  for (const BopPhysicsRow& r : rows)
    if (r.tag == tag) return &r;
  return nullptr;
}
