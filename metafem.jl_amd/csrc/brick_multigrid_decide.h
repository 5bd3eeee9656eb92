// The host decisions of the geometric multigrid preconditioner on hex-8 thermal and elasticity bricks (brick_multigrid.hip, krylov_cg_mg.hip) that are arithmetic
// alone: the level plan, the options' defaults and their refusals, the Chebyshev coefficients, the grids and tiles of the transfer kernels, how many
// vectors a level owns, the device bytes of a hierarchy, the products of a cycle and of a pass, and which solves take the preconditioner.  Plain
// integers in, plain structs out; no HIP, no context: tools/host_check_brick_multigrid.cpp walks them on the CPU (the field-aware forms at the end:
// tools/host_check_brick_multigrid_elasticity.cpp; the hex-27 forms behind them: tools/host_check_brick_multigrid_hex27.cpp; the nonsymmetric
// hierarchy's gate and the products of gmres! with the cycle last: tools/host_check_brick_multigrid_nonsym.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/metafem_mi355x.h"

#define MG_MAX_LEVELS 12  // (= MFEM_MG_MAX_LEVELS)
static_assert(MG_MAX_LEVELS == MFEM_MG_MAX_LEVELS, "the header spells the cap out");

// ---- the options: a zero field takes the default -----------------------------------------------------------------------------------------------------
#define MG_DEFAULT_SMOOTHER_DEGREE 2
#define MG_DEFAULT_COARSE_DEGREE 32
#define MG_DEFAULT_SMOOTHING_RANGE 4.0
#define MG_DEFAULT_COARSE_RANGE 300.0
#define MG_DEFAULT_EIG_STEPS 20
#define MG_MIN_EIG_STEPS 10
#define MG_MAX_DEGREE 4096
#define MG_EIG_SAFETY 1.1  // hi = 1.1 x the estimate of lambda_max(D^-1 A)
#define MG_EIG_SEED 0x4d47u  // the start vector of the estimate: mfem_rand(MG_EIG_SEED, level)

struct MgOptions {
  int nu, nu_c, eig_steps, max_levels;
  double range_s, range_c;
};
// nullptr: taken (*out filled); otherwise what is wrong (MFEM_ERR_INVALID)
static inline const char* mg_options(const mfem_multigrid_options* o, MgOptions* out) {
  MgOptions r{MG_DEFAULT_SMOOTHER_DEGREE, MG_DEFAULT_COARSE_DEGREE, MG_DEFAULT_EIG_STEPS, MG_MAX_LEVELS, MG_DEFAULT_SMOOTHING_RANGE, MG_DEFAULT_COARSE_RANGE};
  if (o) {
    if (o->smoother_degree < 0 || o->smoother_degree > MG_MAX_DEGREE) return "smoother_degree must be in 1 .. 4096 (0: the default, 2)";
    if (o->coarse_degree < 0 || o->coarse_degree > MG_MAX_DEGREE) return "coarse_degree must be in 1 .. 4096 (0: the default, 32)";
    if (o->smoothing_range != 0.0 && !(o->smoothing_range > 1.0)) return "smoothing_range must be > 1 (0: the default, 4)";
    if (o->coarse_range != 0.0 && !(o->coarse_range > 1.0)) return "coarse_range must be > 1 (0: the default, 300)";
    if (o->eig_steps != 0 && (o->eig_steps < MG_MIN_EIG_STEPS || o->eig_steps > MG_MAX_DEGREE)) return "eig_steps must be in 10 .. 4096 (0: the default, 20)";
    if (o->max_levels < 0 || o->max_levels > MG_MAX_LEVELS) return "max_levels must be in 1 .. 12 (0: the default, 12)";
    if (o->smoother_degree) r.nu = o->smoother_degree;
    if (o->coarse_degree) r.nu_c = o->coarse_degree;
    if (o->smoothing_range != 0.0) r.range_s = o->smoothing_range;
    if (o->coarse_range != 0.0) r.range_c = o->coarse_range;
    if (o->eig_steps) r.eig_steps = o->eig_steps;
    if (o->max_levels) r.max_levels = o->max_levels;
  }
  *out = r;
  return nullptr;
}

// ---- the level plan: level 0 is the caller's brick; level l + 1 exists while all three element counts of level l are even and each half is >= 2 ----
struct MgPlan {
  int nlev;
  int ne[MG_MAX_LEVELS][3];
};
static inline MgPlan mg_plan(int nx, int ny, int nz, int max_levels) {
  MgPlan P;
  P.nlev = 1;
  P.ne[0][0] = nx; P.ne[0][1] = ny; P.ne[0][2] = nz;
  if (max_levels < 1 || max_levels > MG_MAX_LEVELS) max_levels = MG_MAX_LEVELS;
  while (P.nlev < max_levels) {
    const int* e = P.ne[P.nlev - 1];
    if ((e[0] | e[1] | e[2]) & 1) break;
    if (e[0] / 2 < 2 || e[1] / 2 < 2 || e[2] / 2 < 2) break;
    for (int d = 0; d < 3; ++d) P.ne[P.nlev][d] = e[d] / 2;
    ++P.nlev;
  }
  return P;
}
static inline int64_t mg_points(const int* ne) { return (int64_t)(ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1); }

// ---- the transfer kernels: a thread per lattice point of the lattice the kernel WRITES (restriction: the coarse one; prolongation and the injection
// of the coordinates: the fine resp. the coarse one), lanes along k, the fastest index: a workgroup owns MG_TILE_J lattice lines x MG_TILE_K points
// of one lattice plane ------------------------------------------------------------------------------------------------------------------------------
#define MG_TILE_K 64
#define MG_TILE_J 4
#define MG_TILE_THREADS (MG_TILE_K * MG_TILE_J)
#define MG_RESTRICT_TILE_K MG_TILE_K   // (coarse points)
#define MG_RESTRICT_TILE_J MG_TILE_J
#define MG_PROLONG_TILE_K MG_TILE_K    // (fine points)
#define MG_PROLONG_TILE_J MG_TILE_J
struct MgGrid {
  unsigned gx, gy, gz;  // tiles along k, tiles along j, planes
};
static inline MgGrid mg_transfer_grid(int m0, int m1, int m2) {
  MgGrid g;
  g.gx = (unsigned)((m2 + MG_TILE_K - 1) / MG_TILE_K);
  g.gy = (unsigned)((m1 + MG_TILE_J - 1) / MG_TILE_J);
  g.gz = (unsigned)m0;
  return g;
}
// the point thread t of workgroup (bx, by, bz) owns; false: none (past the end of a line or of the plane)
static inline bool mg_tile_point(unsigned bx, unsigned by, unsigned bz, int t, int m1, int m2, int* i, int* j, int* k) {
  *i = (int)bz;
  *j = (int)by * MG_TILE_J + t / MG_TILE_K;
  *k = (int)bx * MG_TILE_K + t % MG_TILE_K;
  return *j < m1 && *k < m2;
}
// a launch's grid dimensions y and z hold at most 65535 workgroups
static inline bool mg_grid_ok(const MgGrid& g) { return g.gx >= 1 && g.gy >= 1 && g.gz >= 1 && g.gy <= 65535u && g.gz <= 65535u; }

// ---- vectors and bytes ------------------------------------------------------------------------------------------------------------------------------
// Level 0 works on the caller's r and z and owns three scratch vectors (1 / |diag|, the carried residual, the Chebyshev direction); a coarse level owns
// five (its right-hand side and its iterate besides).  Every vector is padded to a multiple of 32 doubles.  A coarse level also owns its brick: three
// coordinate arrays and the per-dimension lattice tables of mfem_brick_create (two int32 and one int64 entry per lattice index, one more int64).
#define MG_FINE_VECTORS 3
#define MG_COARSE_VECTORS 5
#define MG_FLAG_BYTES 16
static inline int64_t mg_padded(int64_t n) { return (n + 31) / 32 * 32; }
static inline int mg_level_vectors(int level) { return level == 0 ? MG_FINE_VECTORS : MG_COARSE_VECTORS; }
static inline int64_t mg_level_bytes(int level, const int* ne) {
  const int64_t n = mg_points(ne);
  int64_t b = (int64_t)mg_level_vectors(level) * mg_padded(n) * 8;
  if (level > 0) {
    b += 3 * (n > 0 ? n : 1) * 8;
    for (int d = 0; d < 3; ++d) b += (int64_t)(ne[d] + 1) * 16 + 8;
  }
  return b;
}
static inline int64_t mg_bytes(const MgPlan& P) {
  int64_t b = MG_FLAG_BYTES;
  for (int l = 0; l < P.nlev; ++l) b += mg_level_bytes(l, P.ne[l]);
  return b;
}

// ---- products: 2 nu per cycle on every level but the coarsest, nu_c - 1 there; a pass of cg! with the cycle runs one A p per iteration, one cycle per
// iteration (the first before iteration 1, none after the last) and the restart wrapper's true residual ------------------------------------------------
static inline int mg_cycle_products(int level, int nlev, int nu, int nu_c) { return level == nlev - 1 ? nu_c - 1 : 2 * nu; }
static inline int64_t mg_pass_products(int x0, int it, int nlev, int nu, int nu_c) {
  return it >= 1 ? (int64_t)x0 + it + (int64_t)mg_cycle_products(0, nlev, nu, nu_c) * it + 1 : (int64_t)x0 + 1;
}
// vector streams the library's own kernels move per cycle on a level, the products' own traffic apart:
//   below the coarsest: first step from a zero start 5 (b, 1/d -> d, z, r), every further step 6 (r, 1/d, d, z -> d, z), the restriction's read of r 1,
//   the prolongation 3 (z -> z, d; the coarse iterate counts on its own level), the first step after it 5 (r, 1/d, z -> d, z):
//   2 * (5 + 6 (nu - 1)) + 1 + 3 = 12 nu + 2 (26 at nu = 2)
//   on the coarsest: 5 + 6 (nu_c - 1), or 4 when nu_c == 1 (no copy of b is needed); a level that is restricted to also takes the write of its b, and
//   one that is prolongated from the read of its z
static inline int mg_cycle_streams(int level, int nlev, int nu, int nu_c) {
  int s = 0;
  if (level == nlev - 1) s = nu_c == 1 ? 4 : 5 + 6 * (nu_c - 1);
  else s = 12 * nu + 2;
  if (level > 0) s += 2;
  return s;
}

// ---- Chebyshev polynomial smoother in D^-1 A on [lo, hi]: step k adds d_k = c1_k d_(k-1) + c2_k D^-1 r to z ------------------------------------------
struct MgCheb {
  double theta, delta, sigma, rho;  // rho: of the step last taken
};
static inline MgCheb mg_cheb_start(double lo, double hi, double* c1, double* c2) {
  MgCheb C;
  C.theta = (hi + lo) / 2.0;
  C.delta = (hi - lo) / 2.0;
  C.sigma = C.theta / C.delta;
  C.rho = 1.0 / C.sigma;
  *c1 = 0.0;
  *c2 = 1.0 / C.theta;
  return C;
}
static inline void mg_cheb_next(MgCheb* C, double* c1, double* c2) {
  const double rho = 1.0 / (2.0 * C->sigma - C->rho);
  *c1 = rho * C->rho;
  *c2 = 2.0 * rho / C->delta;
  C->rho = rho;
}

// ---- which solves take MFEM_PRECOND_MULTIGRID: nullptr, or what is missing (MFEM_ERR_UNSUPPORTED, nothing launched, nothing written) ---------------
static inline const char* mg_solve_refusal(bool brick_operator, bool thermal_hex8, int method, int left_precond, bool has_comm, bool nitsche_on) {
  if (!brick_operator) return "the multigrid preconditioner needs a hex-8 thermal brick operator (mfem_brick_operator_create): this handle is not one";
  if (!thermal_hex8) return "the multigrid preconditioner covers the hex-8 thermal brick operator: elasticity and hex-27 operators are not covered";
  if (method != MFEM_SOLVER_CG) return "the multigrid preconditioner needs MFEM_SOLVER_CG: the cycle is a symmetric operator, the other methods are not offered it";
  if (left_precond != MFEM_LEFT_NONE) return "the multigrid preconditioner takes no left preconditioner";
  if (has_comm) return "the multigrid preconditioner runs on one rank: no communicator may be attached";
  if (nitsche_on) return "the multigrid preconditioner needs a symmetric K: a Nitsche (fixed_faces) term is active";
  return nullptr;
}

// ---- the field-aware forms: a hierarchy of `fields` field-major fields per lattice point (1: thermal, 3: elasticity) ----------------------------------
// A level vector holds fields x points entries, field f at [f * points, (f + 1) * points); the VECTOR is padded to 32 doubles, not each field.  The
// transfer kernels keep their grids (a thread per lattice point, which loops over the fields); coordinates are three arrays whatever the fields.
#define MG_ELASTICITY_FIELDS 3
static inline int64_t mg_field_offset(int field, int64_t points) { return (int64_t)field * points; }
static inline int64_t mg_level_entries(int fields, const int* ne) { return (int64_t)fields * mg_points(ne); }
static inline int64_t mg_level_bytes_fields(int level, const int* ne, int fields) {
  const int64_t n = mg_points(ne);
  int64_t b = (int64_t)mg_level_vectors(level) * mg_padded((int64_t)fields * n) * 8;
  if (level > 0) {
    b += 3 * (n > 0 ? n : 1) * 8;
    for (int d = 0; d < 3; ++d) b += (int64_t)(ne[d] + 1) * 16 + 8;
  }
  return b;
}
static inline int64_t mg_bytes_fields(const MgPlan& P, int fields) {
  int64_t b = MG_FLAG_BYTES;
  for (int l = 0; l < P.nlev; ++l) b += mg_level_bytes_fields(l, P.ne[l], fields);
  return b;
}
// bytes the library's own kernels move per cycle on a level: mg_cycle_streams (unchanged) level vectors of fields x points doubles
static inline int64_t mg_cycle_stream_bytes(int level, int nlev, int nu, int nu_c, int fields, const int* ne) {
  return (int64_t)mg_cycle_streams(level, nlev, nu, nu_c) * 8 * mg_level_entries(fields, ne);
}
// an elasticity K without a penalty face keeps the rigid-body modes: the coarsest level's Chebyshev interval does not cover a singular operator
static inline const char* mg_elasticity_refusal(double tau, uint32_t penalty_faces) {
  if (tau == 0.0) return "tau == 0: without the penalty K keeps the rigid-body modes and is singular";
  if ((penalty_faces & 0x3Fu) == 0u) return "penalty_faces == 0: without a penalty face K keeps the rigid-body modes and is singular";
  return nullptr;
}
// mg_solve_refusal with the hex-8 elasticity operator admitted when a hierarchy of mfem_brick_multigrid_create_elasticity is attached to it (that
// hierarchy is the opt-in: no default one is created); every other row answers as mg_solve_refusal does
static inline const char* mg_solve_refusal_fields(bool brick_operator, bool thermal_hex8, bool elasticity_hex8, bool hierarchy_attached, int method,
                                                  int left_precond, bool has_comm, bool nitsche_on) {
  if (!brick_operator || !elasticity_hex8 || thermal_hex8) return mg_solve_refusal(brick_operator, thermal_hex8, method, left_precond, has_comm, nitsche_on);
  if (!hierarchy_attached)
    return "the multigrid preconditioner runs on a hex-8 elasticity brick operator only with a hierarchy attached: create one with "
           "mfem_brick_multigrid_create_elasticity (no default hierarchy is made for elasticity)";
  return mg_solve_refusal(true, true, method, left_precond, has_comm, false);
}

// ---- the hex-27 thermal hierarchy (mfem_brick_multigrid_create_hex27): p-coarsening once, then the h-hierarchy above -----------------------------------
// Level 0 is the caller's hex-27 brick of (nx, ny, nz) elements on the lattice (2 nx + 1, 2 ny + 1, 2 nz + 1); level 1 -- whenever max_levels >= 2, for
// any element counts >= 1 -- is a library-owned hex-8 brick with the SAME element counts, lengths and rule on the lattice (nx + 1, ny + 1, nz + 1), so
// mf = 2 mc - 1 as between two hex-8 levels: the trilinear P of k_mg_prolong<1> is the embedding Q1 in Q2 on the same mesh, k_mg_restrict<1> its
// transpose, and k_mg_inject takes the hex-27 corner nodes (the even lattice points) as the hex-8 coordinates.  From level 1 on mg_plan's halving rule.
// MgPlan.ne holds ELEMENT counts on every level: ne[0] == ne[1] on such a plan, and the lattice of level 0 is mg_lattice_hex27's.
static inline MgPlan mg_plan_hex27(int nx, int ny, int nz, int max_levels) {
  if (max_levels < 1 || max_levels > MG_MAX_LEVELS) max_levels = MG_MAX_LEVELS;
  MgPlan P;
  P.nlev = 1;
  P.ne[0][0] = nx; P.ne[0][1] = ny; P.ne[0][2] = nz;
  if (max_levels < 2) return P;
  const MgPlan H = mg_plan(nx, ny, nz, max_levels - 1);  // the hex-8 brick of the same elements and what lies below it
  for (int l = 0; l < H.nlev; ++l)
    for (int d = 0; d < 3; ++d) P.ne[1 + l][d] = H.ne[l][d];
  P.nlev = 1 + H.nlev;
  return P;
}
// lattice points per direction of a level: 2 ne + 1 on the hex-27 level 0, ne + 1 on every hex-8 level
static inline int mg_lattice_hex27(int level, int ne) { return level == 0 ? 2 * ne + 1 : ne + 1; }
static inline int64_t mg_points_hex27(int level, const int* ne) {
  return (int64_t)mg_lattice_hex27(level, ne[0]) * mg_lattice_hex27(level, ne[1]) * mg_lattice_hex27(level, ne[2]);
}
// the bytes of a level that knows the level-0 lattice: level 0 owns its three scratch vectors of (2 nx + 1)(2 ny + 1)(2 nz + 1) entries, a hex-8 level
// what mg_level_bytes counts
static inline int64_t mg_level_bytes_hex27(int level, const int* ne) {
  if (level > 0) return mg_level_bytes(level, ne);
  return (int64_t)mg_level_vectors(0) * mg_padded(mg_points_hex27(0, ne)) * 8;
}
static inline int64_t mg_bytes_hex27(const MgPlan& P) {
  int64_t b = MG_FLAG_BYTES;
  for (int l = 0; l < P.nlev; ++l) b += mg_level_bytes_hex27(l, P.ne[l]);
  return b;
}
static inline int64_t mg_cycle_stream_bytes_hex27(int level, int nlev, int nu, int nu_c, const int* ne) {
  return (int64_t)mg_cycle_streams(level, nlev, nu, nu_c) * 8 * mg_points_hex27(level, ne);
}
// what the hex-27 hierarchy refuses beside the thermal rows (create, every setup, the solve gate): a rule with fewer than 3 Gauss points per direction
#define MG_HEX27_MIN_NG 3
static inline const char* mg_hex27_refusal(int ng, bool nitsche_on) {
  if (nitsche_on) return "a Nitsche (fixed_faces) term is active: K is not symmetric";
  if (ng < MG_HEX27_MIN_NG)
    return "a rule with fewer than 3 Gauss points per direction (itg_order < 4): the under-integrated order-2 K keeps near-null modes that the "
           "hex-8 coarse space does not hold";
  return nullptr;
}
// mg_solve_refusal_fields with the hex-27 thermal operator admitted when a hierarchy of mfem_brick_multigrid_create_hex27 is attached to it (the
// hierarchy is the opt-in: no default one is created); every other row answers as mg_solve_refusal_fields does
static inline const char* mg_solve_refusal_hex27(bool brick_operator, bool thermal_hex8, bool elasticity_hex8, bool thermal_hex27, bool hierarchy_attached,
                                                 int method, int left_precond, bool has_comm, bool nitsche_on) {
  if (!brick_operator || !thermal_hex27 || thermal_hex8 || elasticity_hex8)
    return mg_solve_refusal_fields(brick_operator, thermal_hex8, elasticity_hex8, hierarchy_attached, method, left_precond, has_comm, nitsche_on);
  if (!hierarchy_attached)
    return "the multigrid preconditioner runs on a hex-27 thermal brick operator only with a hierarchy attached: create one with "
           "mfem_brick_multigrid_create_hex27 (no default hierarchy is made for hex-27)";
  return mg_solve_refusal(true, true, method, left_precond, has_comm, nitsche_on);
}

// ---- the nonsymmetric thermal hierarchy (mfem_brick_multigrid_create_nonsymmetric) and gmres! with the cycle (krylov_gmres_mg.hip) ---------------------
// A hierarchy created by that entry point is the hex-8 thermal one, marked: its setups run with a Nitsche (fixed_faces) term active too -- the level
// products carry the Nitsche rows and the signed diagonal has them; every other refusal of a setup stays.  The fixed Chebyshev V-cycle is then a fixed
// linear operator that is not symmetric: a right preconditioner for restarted GMRES, not for cg!.
// mg_solve_refusal_hex27 with MFEM_SOLVER_GMRES admitted on a hex-8 thermal operator when a NONSYMMETRIC hierarchy is attached to it (that hierarchy
// is the opt-in: no default one is made), with no left preconditioner and no communicator; the Nitsche term may be on or off.  Every other row answers
// as mg_solve_refusal_hex27 does: cg! with an active Nitsche term is refused whatever is attached, cg! on a nonsymmetric hierarchy whose Nitsche
// term is off runs as on a plain one, gmres! on an elasticity, hex-27 or mesh operator is answered by those operators' rows.
static inline const char* mg_solve_refusal_nonsym(bool brick_operator, bool thermal_hex8, bool elasticity_hex8, bool thermal_hex27, bool hierarchy_attached,
                                                  bool hierarchy_nonsymmetric, int method, int left_precond, bool has_comm, bool nitsche_on) {
  if (method != MFEM_SOLVER_GMRES || !brick_operator || !thermal_hex8 || elasticity_hex8 || thermal_hex27)
    return mg_solve_refusal_hex27(brick_operator, thermal_hex8, elasticity_hex8, thermal_hex27, hierarchy_attached, method, left_precond, has_comm, nitsche_on);
  if (!hierarchy_attached)
    return "gmres! takes the multigrid preconditioner on a hex-8 thermal brick operator only with a nonsymmetric hierarchy attached: create one with "
           "mfem_brick_multigrid_create_nonsymmetric (no default hierarchy is made for gmres!)";
  if (!hierarchy_nonsymmetric)
    return "gmres! takes the multigrid preconditioner only from a nonsymmetric hierarchy: the attached one is of mfem_brick_multigrid_create; destroy it "
           "and create one with mfem_brick_multigrid_create_nonsymmetric";
  return mg_solve_refusal(true, true, MFEM_SOLVER_CG, left_precond, has_comm, false);  // (the left preconditioner's and the communicator's rows)
}
// whether a setup refuses an active Nitsche term: a plain thermal hierarchy does, a nonsymmetric one does not
static inline bool mg_setup_refuses_nitsche(bool hierarchy_nonsymmetric, bool nitsche_on) { return nitsche_on && !hierarchy_nonsymmetric; }

// Level-0 products of a pass of gmres! with the cycle (mfem_solve_stats.spmv_count; the restart wrapper adds its true residual's): x0 for the start
// residual as mfem_pass_residual counts it (0 from a zero start), then per restart of width k: k cycles and k products A z for the Arnoldi steps, one
// more cycle for x += Cycle(Q y) and the true residual -- k (1 + c) + c + 1 with c = mg_cycle_products(0, ...).  Summed over the restarts of a pass of
// `it` steps: it (1 + c) + restarts (c + 1); cycles = it + restarts.  A restart ends at width s, at the step that stops, or at an exact breakdown.
#define MG_GMRES_DEFAULT_S 20
#define MG_GMRES_MAX_S 32
static inline int64_t mg_gmres_cycles(int it, int restarts) { return (int64_t)it + restarts; }
static inline int64_t mg_gmres_restart_products(int width, int c) { return (int64_t)width * (1 + c) + c + 1; }
static inline int64_t mg_gmres_pass_products(int x0, int it, int restarts, int nlev, int nu, int nu_c) {
  const int c = mg_cycle_products(0, nlev, nu, nu_c);
  return (int64_t)x0 + (int64_t)it * (1 + c) + (int64_t)restarts * (c + 1);
}
// restarts of a pass that takes `it` steps without a convergence stop or a breakdown in between (fixed_iterations, or maxiter reached): ceil(it / s)
static inline int mg_gmres_full_restarts(int it, int s) { return it <= 0 ? 0 : (it + s - 1) / s; }
