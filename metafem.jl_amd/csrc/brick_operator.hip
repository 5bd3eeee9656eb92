// The handle of the matrix-free brick operator, for EVERY physics: the immutable hex-8 tables (bop_tables), create and destroy, the bind, the operator
// interface of the solve driver, and every extern "C" entry point but the elasticity residual.  No kernel lives here.  What differs between the physics
// is decided in two tables and nowhere else: the rows of brick_operator_physics.h (fields, parameter block, set-params entry point -- host data) and
// the ops table below (refusal, prepare, launch, jacobi, signed diagonal -- functions of the file that defines the kernels, which launches them):
//   hex-8 thermal: brick_operator_thermal.hip; hex-8 elasticity: brick_operator_elasticity.hip; hex-27 thermal: brick_operator_hex27.hip and, for the signed
//   diagonal, brick_operator_hex27_diagonal.hip; hex-27 elasticity: brick_operator_elasticity_hex27.hip (which defines the elasticity residual entry point)
// What has to hold before a cached cycle is replayed (the brick still whole, its arrays where the cycle expects them) is verified when the operator is
// bound (bop_view), not in the launcher a replay never enters; the tables the kernels read are immutable per rule (brick_operator.h): no upload at a launch.
// Contract of a launch (bop_launch: spmv_launch_inner's), the same for every physics: the product kernels leave at once when done_flag[0] is set, launch
// without a host sync or an allocation (capturable in the solve's cycle graphs), and leave the partial sums of dotw . y of the final y: the volume
// kernel's workgroup sums first, the face kernel's increments behind them.  Then the grids are capped (brick_operator_decide.h): a workgroup FOLDS the
// work items b, b + grid, ... in that order; a product without partial sums launches one workgroup per item, as the residual does.  No atomics.
#include "hex8_device.h"
#include "blas1.h"
#include "brick_operator.h"
#include "brick_operator_hex27_decide.h"
#include "brick_operator_elasticity_hex27_decide.h"
static_assert(BOP_MAX_PARTIALS == MFEM_MAX_PARTIALS, "brick_operator_decide.h spells the cap out");

static std::atomic<long long> g_brick_operator_count{0};
extern "C" int64_t mfem_debug_brick_operator_count(void) { return g_brick_operator_count; }

// the one owner of the immutable per-rule tables (brick_operator.h says why they exist)
#define BOP_MAX_DEVICES 64
int bop_tables(int device, int ng, const H8Tables** out) {
  static std::mutex mu;
  static H8Tables* tables[BOP_MAX_DEVICES][H8_MAX_NG];
  MFEM_REQUIRE(device >= 0 && device < BOP_MAX_DEVICES && ng >= 1 && ng <= H8_MAX_NG, "device or Gauss rule out of range");
  std::lock_guard<std::mutex> lk(mu);
  if (!tables[device][ng - 1]) {
    static H8Tables host;  // (guarded by mu)
    h8_reference_tables(ng, &host);
    DevBuf<H8Tables> buf;
    MFEM_CHECK_HIP(buf.alloc(1));
    MFEM_CHECK_HIP(hipMemcpy(buf, &host, sizeof(host), hipMemcpyHostToDevice));
    tables[device][ng - 1] = buf.release();
  }
  *out = tables[device][ng - 1];
  return MFEM_OK;
}

mfem_brick_operator_s* bop_from_handle(uint64_t handle) {
  mfem_operator_head* h = (mfem_operator_head*)(uintptr_t)handle;
  return h && h->kind == MFEM_OPERATOR_BRICK ? (mfem_brick_operator_s*)h : nullptr;
}

// ---- the ops table: what a physics does, beside its row ----------------------------------------------------------------------------------------------
struct BopOps {
  const char* (*refusal)(const mfem_brick_s*);                    // nullptr: the brick is taken; otherwise why not (MFEM_ERR_UNSUPPORTED)
  int (*prepare)(int device, int ng, mfem_brick_operator_s* op);  // once per operator, never at a launch: the rule's tables, the dynamic-LDS limits
  decltype(&bop_thermal_launch) launch;                           // (the one signature of brick_operator.h's launchers)
  decltype(&bop_thermal_jacobi) jacobi, signed_diagonal;          // signed_diagonal == nullptr: the physics has none
};
static const char* bop_refusal_hex8(const mfem_brick_s* m) { return bop_refusal(m->p, m->plo, m->phi, m->m[0]); }
static const char* bop_refusal_hex27(const mfem_brick_s* m) { return bop27_refusal(m->p, m->plo, m->phi, m->m[0]); }
static const char* bop_refusal_e27(const mfem_brick_s* m) { return bop_e27_refusal(m->p, m->plo, m->phi, m->m[0], m->ng); }
static int bop_prepare_hex8(int device, int ng, mfem_brick_operator_s* op) { return bop_tables(device, ng, &op->tables); }
static int bop_prepare_hex27(int device, int ng, mfem_brick_operator_s* op) {
  int rc = bop27_tables(device, ng, &op->tables27);
  if (!rc) rc = bop27_prepare(ng);
  if (!rc) rc = bop27_diagonal_prepare(ng);
  return rc;
}
static int bop_prepare_e27(int device, int ng, mfem_brick_operator_s* op) {
  const int rc = bop27_tables(device, ng, &op->tables27);
  return rc ? rc : bop_e27_prepare(ng);
}
static const BopOps& bop_ops(const mfem_brick_operator_s* op) {  // (a function-local table, for the reason given at mfem_brick_operator_interface)
  static const BopOps ops[BOP_PHYSICS_ROWS + 1] = {
      {},
      /* BOP_PHYSICS_THERMAL */ {bop_refusal_hex8, bop_prepare_hex8, bop_thermal_launch, bop_thermal_jacobi, bop_thermal_signed_diagonal},
      /* BOP_PHYSICS_ELASTICITY */ {bop_refusal_hex8, bop_prepare_hex8, bop_elasticity_launch, bop_elasticity_jacobi, bop_elasticity_signed_diagonal},
      /* BOP_PHYSICS_HEX27 */ {bop_refusal_hex27, bop_prepare_hex27, bop27_launch, bop27_jacobi, bop27_signed_diagonal},
      /* BOP_PHYSICS_ELASTICITY_HEX27 */ {bop_refusal_e27, bop_prepare_e27, bop_e27_launch, bop_e27_jacobi, nullptr},
  };
  return ops[op->physics];
}

static int bop_refuse(int rc, const char* why) {
  mfem_set_error("matrix-free brick operator: %s", why);
  return rc;
}

// The brick as it is NOW (a caller may move coordinates between solves; a slab set after the operator was created is refused here).  Host only:
// nothing is uploaded.  Called when the operator is bound -- before the driver can replay a cached cycle -- and again at every launch.
int bop_view(const mfem_brick_operator_s* op, BrickView* B) {
  const mfem_brick_s* m = op->brick;
  const char* why = bop_ops(op).refusal(m);
  if (why) return bop_refuse(MFEM_ERR_UNSUPPORTED, why);
  const int fields = bop_row(op).fields;
  MFEM_REQUIRE(fields * m->n_owned == op->csr.n, "the brick changed size under the operator");
  MFEM_REQUIRE(m->ng == op->ng, "the brick's Gauss rule changed under the operator");
  *B = mfem_brick_view(m, fields);
  return MFEM_OK;
}

static int bop_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* x, double* y, double alpha, double beta, const double* dotw, double* partials,
                      int* n_partials, const int32_t* done_flag) {
  mfem_brick_operator_s* op = A->op && A->op->kind == MFEM_OPERATOR_BRICK ? (mfem_brick_operator_s*)A->op : nullptr;
  MFEM_REQUIRE(op, "the operator is not bound");
  BrickView B;
  int rc = bop_view(op, &B);
  if (rc) return rc;
  rc = bop_ops(op).launch(ctx, op, B, x, A->op_dsc, y, alpha, beta, dotw, partials, n_partials, done_flag);  // (kernels are launched from the file that defines them)
  if (rc) return rc;
  if (!ctx->probe_active) ++g_brick_operator_count;
  return MFEM_OK;
}

static int bop_jacobi(mfem_context_s* ctx, mfem_brick_operator_s* op, double* d) {
  BrickView B;
  const int rc = bop_view(op, &B);
  return rc ? rc : bop_ops(op).jacobi(ctx, op, B, d);
}
int bop_signed_diagonal(mfem_context_s* ctx, mfem_brick_operator_s* op, double* d) {
  const auto signed_diagonal = bop_ops(op).signed_diagonal;
  MFEM_REQUIRE(bop_row(op).signed_diagonal && signed_diagonal, "the signed diagonal exists for the brick operators");
  BrickView B;
  const int rc = bop_view(op, &B);
  return rc ? rc : signed_diagonal(ctx, op, B, d);
}

static int bop_bind(mfem_brick_operator_s* op, const double* dsc) {
  BrickView B;
  const int rc = bop_view(op, &B);  // (a slab set since the last solve is refused here, not by a launch that a cached cycle would skip)
  if (rc) return rc;
  if (B.X0 != op->seen_x0) {  // (the brick's arrays moved: no cached cycle may replay the old pointers)
    op->seen_x0 = B.X0;
    ++op->csr.op_epoch;
  }
  op->csr.op = &op->head;
  op->csr.op_scratch = nullptr;
  op->csr.op_dsc = dsc;
  return MFEM_OK;
}
static void bop_unbind(mfem_brick_operator_s* op) {
  op->csr.op = nullptr;
  op->csr.op_scratch = nullptr;
  op->csr.op_dsc = nullptr;
}

// what the solve driver and the product dispatch hold of this kind (operator.h)
static mfem_brick_operator_s* as_brick(mfem_operator_head* h) { return (mfem_brick_operator_s*)h; }
static mfem_context_s* bop_if_ctx(mfem_operator_head* h) { return as_brick(h)->ctx; }
static mfem_csr_s* bop_if_csr(mfem_operator_head* h) { return &as_brick(h)->csr; }
static size_t bop_if_scratch(const mfem_operator_head*) { return 0; }  // no element-vector scratch: the workspace is the solver's vectors only
static int bop_if_bind(mfem_operator_head* h, double*, const double* dsc) { return bop_bind(as_brick(h), dsc); }
static void bop_if_unbind(mfem_operator_head* h) { bop_unbind(as_brick(h)); }
static int bop_if_jacobi(mfem_context_s* ctx, mfem_operator_head* h, double*, double* d) { return bop_jacobi(ctx, as_brick(h), d); }
const mfem_operator_interface* mfem_brick_operator_interface() {  // (a function-local table: a const global of a .hip file is emitted for the device too)
  static const mfem_operator_interface I = {bop_if_ctx, bop_if_csr, bop_if_scratch, bop_if_bind, bop_if_unbind, bop_if_jacobi, bop_launch};
  return &I;
}

// what every physics does to create an operator: the refusals, the rule's tables and LDS limits (the one upload of a rule: here, never at a launch),
// the handle -- filled on the stack, allocated once nothing can refuse any more
static int bop_create(mfem_context ctx, mfem_brick m, int physics, const void* p, uint64_t* out) {
  MFEM_REQUIRE(out, "null out");
  *out = 0;
  MFEM_REQUIRE(ctx && m && p, "null argument");
  MFEM_REQUIRE(m->ctx == ctx, "the brick was created on another context");
  mfem_brick_operator_s seed;
  memset(&seed, 0, sizeof(seed));
  seed.head.kind = MFEM_OPERATOR_BRICK;
  seed.ng = m->ng;
  seed.ctx = ctx;
  seed.brick = m;
  seed.physics = physics;
  const char* why = bop_ops(&seed).refusal(m);
  if (why) return bop_refuse(MFEM_ERR_UNSUPPORTED, why);
  const int rct = bop_ops(&seed).prepare(ctx->device, m->ng, &seed);
  if (rct) return rct;
  const BopPhysicsRow& row = bop_row(&seed);
  if (row.block == BOP_BLOCK_ELASTICITY) seed.elasticity = *(const mfem_elasticity_params*)p;
  else seed.thermal = *(const mfem_thermal_params*)p;
  seed.csr.ctx = ctx;
  seed.csr.n = row.fields * m->n_owned;  // field-major unknowns (brick_xindex)
  seed.csr.rowptr_bits = 64;
  mfem_host_alloc_probe();
  mfem_brick_operator_s* op = new mfem_brick_operator_s(seed);
  op->csr.serial = mfem_next_csr_serial();
  *out = (uint64_t)(uintptr_t)op;
  return MFEM_OK;
}
extern "C" int mfem_brick_operator_create(mfem_context ctx, mfem_brick m, const mfem_thermal_params* p, uint64_t* out) try {
  return bop_create(ctx, m, BOP_PHYSICS_THERMAL, p, out);
} MFEM_API_CATCH("mfem_brick_operator_create")
extern "C" int mfem_brick_operator_create_elasticity(mfem_context ctx, mfem_brick m, const mfem_elasticity_params* p, uint64_t* out) try {
  return bop_create(ctx, m, BOP_PHYSICS_ELASTICITY, p, out);
} MFEM_API_CATCH("mfem_brick_operator_create_elasticity")
extern "C" int mfem_brick_operator_create_elasticity_hex27(mfem_context ctx, mfem_brick m, const mfem_elasticity_params* p, uint64_t* out) try {
  return bop_create(ctx, m, BOP_PHYSICS_ELASTICITY_HEX27, p, out);
} MFEM_API_CATCH("mfem_brick_operator_create_elasticity_hex27")
extern "C" int mfem_brick_operator_create_hex27(mfem_context ctx, mfem_brick m, const mfem_thermal_params* p, uint64_t* out) try {
  return bop_create(ctx, m, BOP_PHYSICS_HEX27, p, out);
} MFEM_API_CATCH("mfem_brick_operator_create_hex27")

// a set-params call of the other physics answers MFEM_ERR_INVALID and changes nothing
static int bop_set_params(uint64_t handle, const void* p, BopSetParams entry) {
  mfem_brick_operator_s* op = bop_from_handle(handle);
  MFEM_REQUIRE(op && p, "null argument, or not a brick operator's handle");
  MFEM_REQUIRE(bop_row(op).set_params == entry, "the operator was created for the other physics (thermal: mfem_brick_operator_set_params, elasticity: mfem_brick_operator_set_elasticity_params)");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  if (bop_set_params_block(entry) == BOP_BLOCK_ELASTICITY) op->elasticity = *(const mfem_elasticity_params*)p;
  else op->thermal = *(const mfem_thermal_params*)p;
  ++op->csr.op_epoch;  // (a captured cycle bakes the parameters in)
  return MFEM_OK;
}
extern "C" int mfem_brick_operator_set_params(uint64_t handle, const mfem_thermal_params* p) try {
  return bop_set_params(handle, p, BOP_SET_PARAMS);
} MFEM_API_CATCH("mfem_brick_operator_set_params")
extern "C" int mfem_brick_operator_set_elasticity_params(uint64_t handle, const mfem_elasticity_params* p) try {
  return bop_set_params(handle, p, BOP_SET_ELASTICITY_PARAMS);
} MFEM_API_CATCH("mfem_brick_operator_set_elasticity_params")

extern "C" int mfem_brick_operator_destroy(uint64_t handle) try {
  if (!handle) return MFEM_OK;
  mfem_brick_operator_s* op = bop_from_handle(handle);
  MFEM_REQUIRE(op, "not a brick operator's handle");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  if (op->ctx && mfem_context_alive(op->ctx)) {
    (void)hipStreamSynchronize(op->ctx->stream);
    mfem_graphs_invalidate(op->ctx);  // (a cached cycle holds the brick's arrays and the parameters)
  }
  if (op->mg) mfem_mg_release(op->mg);  // (one hierarchy per operator, destroyed with it)
  op->head.kind = 0;
  delete op;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_brick_operator_destroy")

static int bop_standalone(mfem_context ctx, uint64_t handle, mfem_brick_operator_s** out) {
  mfem_brick_operator_s* op = bop_from_handle(handle);
  MFEM_REQUIRE(ctx && op, "null handle, or not a brick operator's");
  MFEM_REQUIRE(op->ctx == ctx, "the operator was created on another context");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  *out = op;
  return MFEM_OK;
}

extern "C" int mfem_brick_operator_apply(mfem_context ctx, uint64_t handle, const double* x, double* y, double alpha, double beta) try {
  mfem_brick_operator_s* op = nullptr;
  const int rc = bop_standalone(ctx, handle, &op);
  if (rc) return rc;
  MFEM_REQUIRE(x && y, "null vector");
  const int rcb = bop_bind(op, nullptr);
  if (rcb) return rcb;
  struct Release { mfem_brick_operator_s* op; ~Release() { bop_unbind(op); } } release{op};
  return mfem_spmv_launch(ctx, &op->csr, nullptr, x, y, alpha, beta, nullptr, nullptr, nullptr, nullptr);
} MFEM_API_CATCH("mfem_brick_operator_apply")

extern "C" int mfem_debug_brick_operator_apply_dot(mfem_context ctx, uint64_t handle, const double* x, double* y, double alpha, double beta, const double* dotw,
                                                   double* partials, int32_t* n_partials) try {
  mfem_brick_operator_s* op = nullptr;
  const int rc = bop_standalone(ctx, handle, &op);
  if (rc) return rc;
  MFEM_REQUIRE(x && y && dotw && partials && n_partials, "null argument");
  const int rcb = bop_bind(op, nullptr);
  if (rcb) return rcb;
  struct Release { mfem_brick_operator_s* op; ~Release() { bop_unbind(op); } } release{op};
  int np = 0;
  const int rcl = bop_launch(ctx, &op->csr, x, y, alpha, beta, dotw, partials, &np, nullptr);
  *n_partials = np;
  return rcl;
} MFEM_API_CATCH("mfem_debug_brick_operator_apply_dot")

extern "C" int mfem_debug_brick_operator_signed_diagonal(mfem_context ctx, uint64_t handle, double* d) try {
  mfem_brick_operator_s* op = nullptr;
  const int rc = bop_standalone(ctx, handle, &op);
  if (rc) return rc;
  MFEM_REQUIRE(d, "null vector");
  return bop_signed_diagonal(ctx, op, d);
} MFEM_API_CATCH("mfem_debug_brick_operator_signed_diagonal")

extern "C" int mfem_brick_operator_diagonal(mfem_context ctx, uint64_t handle, double* d) try {
  mfem_brick_operator_s* op = nullptr;
  const int rc = bop_standalone(ctx, handle, &op);
  if (rc) return rc;
  MFEM_REQUIRE(d, "null vector");
  return bop_jacobi(ctx, op, d);
} MFEM_API_CATCH("mfem_brick_operator_diagonal")
