// CPU walk through the host decisions of the geometric multigrid preconditioner on hex-8 thermal bricks (csrc/brick_multigrid_decide.h):
//   1. the level plan of every (nx, ny, nz) up to 64^3 and of 512^3, 768^3, 1000^3, 1024^3: level l + 1 exists while all three counts of level l are
//      even and each half is >= 2, at most 12 levels, max_levels honoured; a digest of all plans and byte totals is printed for the Python
//      restatement (tests/test_brick_multigrid_host.py);
//   2. the transfer kernels' grids: every lattice point is owned by exactly one thread of one workgroup, none lies outside the lattice, the grid
//      dimensions fit a launch -- point by point on small lattices, through the axis extents on the large ones;
//   3. the bytes of a hierarchy against the closed form, the vectors per level, the products of a cycle and of a pass, the streams' bound 12 nu + 4;
//   4. the options' defaults and refusals, the Chebyshev coefficients against the three-term recurrence, the solve gate.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_multigrid.cpp -o tools/bin/host_check_brick_multigrid && tools/bin/host_check_brick_multigrid
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "brick_multigrid_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

static void check_plan(int nx, int ny, int nz, int max_levels) {
  const MgPlan P = mg_plan(nx, ny, nz, max_levels);
  const int cap = (max_levels >= 1 && max_levels <= MG_MAX_LEVELS) ? max_levels : MG_MAX_LEVELS;
  CHECK(P.nlev >= 1 && P.nlev <= cap, "%d x %d x %d (max %d): %d levels", nx, ny, nz, max_levels, P.nlev);
  CHECK(P.ne[0][0] == nx && P.ne[0][1] == ny && P.ne[0][2] == nz, "%d x %d x %d: level 0", nx, ny, nz);
  for (int l = 1; l < P.nlev; ++l)
    for (int d = 0; d < 3; ++d) {
      CHECK(P.ne[l - 1][d] % 2 == 0 && P.ne[l][d] == P.ne[l - 1][d] / 2 && P.ne[l][d] >= 2, "%d x %d x %d: level %d, dim %d", nx, ny, nz, l, d);
      CHECK(2 * (P.ne[l][d] + 1) - 1 == P.ne[l - 1][d] + 1, "%d x %d x %d: level %d: the fine lattice has 2 mc - 1 points", nx, ny, nz, l);
    }
  const int* e = P.ne[P.nlev - 1];
  const bool could = e[0] % 2 == 0 && e[1] % 2 == 0 && e[2] % 2 == 0 && e[0] / 2 >= 2 && e[1] / 2 >= 2 && e[2] / 2 >= 2;
  CHECK(!could || P.nlev == cap, "%d x %d x %d: the plan stops early", nx, ny, nz);
}

// every point of an m0 x m1 x m2 lattice is owned by exactly one thread
static void check_grid_points(int m0, int m1, int m2) {
  const MgGrid g = mg_transfer_grid(m0, m1, m2);
  CHECK(mg_grid_ok(g), "%d x %d x %d: grid", m0, m1, m2);
  std::vector<unsigned char> seen((size_t)m0 * m1 * m2, 0);
  long long outside = 0;
  for (unsigned bz = 0; bz < g.gz; ++bz)
    for (unsigned by = 0; by < g.gy; ++by)
      for (unsigned bx = 0; bx < g.gx; ++bx)
        for (int t = 0; t < MG_TILE_THREADS; ++t) {
          int i, j, k;
          if (!mg_tile_point(bx, by, bz, t, m1, m2, &i, &j, &k)) continue;
          if (i < 0 || i >= m0 || j < 0 || j >= m1 || k < 0 || k >= m2) { ++outside; continue; }
          ++seen[((size_t)i * m1 + j) * m2 + k];
        }
  long long wrong = 0;
  for (unsigned char c : seen) wrong += c != 1;
  CHECK(outside == 0 && wrong == 0, "%d x %d x %d: %lld points outside, %lld not owned exactly once", m0, m1, m2, outside, wrong);
}
// the same through the extents: tiles along k cover [0, m2) without overlap, tiles along j cover [0, m1), planes [0, m0)
static void check_grid_extents(int m0, int m1, int m2) {
  const MgGrid g = mg_transfer_grid(m0, m1, m2);
  CHECK(mg_grid_ok(g), "%d x %d x %d: grid", m0, m1, m2);
  CHECK((long long)(g.gx - 1) * MG_TILE_K < m2 && (long long)g.gx * MG_TILE_K >= m2, "%d x %d x %d: tiles along k", m0, m1, m2);
  CHECK((long long)(g.gy - 1) * MG_TILE_J < m1 && (long long)g.gy * MG_TILE_J >= m1, "%d x %d x %d: tiles along j", m0, m1, m2);
  CHECK((int)g.gz == m0, "%d x %d x %d: planes", m0, m1, m2);
}

int main() {
  // 1. plans; the digest
  unsigned long long digest = 0, count = 0;
  for (int nx = 1; nx <= 64; ++nx)
    for (int ny = 1; ny <= 64; ++ny)
      for (int nz = 1; nz <= 64; ++nz) {
        check_plan(nx, ny, nz, 0);
        const MgPlan P = mg_plan(nx, ny, nz, 0);
        digest = digest * 1000003ull + (unsigned long long)P.nlev * 1315423911ull + (unsigned long long)mg_bytes(P);
        ++count;
      }
  printf("PLANS %llu %llu\n", count, digest);
  const int big[4] = {512, 768, 1000, 1024};
  for (int b = 0; b < 4; ++b) {
    for (int ml = 0; ml <= 13; ++ml) check_plan(big[b], big[b], big[b], ml);
    const MgPlan P = mg_plan(big[b], big[b], big[b], 0);
    printf("PLAN %d %d %lld", big[b], P.nlev, (long long)mg_bytes(P));
    for (int l = 0; l < P.nlev; ++l) printf(" %d", P.ne[l][0]);
    printf("\n");
    // 2b. the grids of every level of the large bricks
    for (int l = 0; l < P.nlev; ++l) check_grid_extents(P.ne[l][0] + 1, P.ne[l][1] + 1, P.ne[l][2] + 1);
  }
  for (int ml = 1; ml <= 5; ++ml) CHECK(mg_plan(64, 64, 64, ml).nlev == ml, "max_levels %d", ml);
  CHECK(mg_plan(64, 64, 64, 0).nlev == 6 && mg_plan(16, 24, 12, 0).nlev == 3 && mg_plan(6, 10, 14, 0).nlev == 2 && mg_plan(9, 14, 15, 0).nlev == 1 &&
        mg_plan(4, 4, 4, 0).nlev == 2 && mg_plan(2, 2, 2, 0).nlev == 1 && mg_plan(1024, 1024, 1024, 0).nlev == 10, "known plans");
  // 2a. grids point by point: around the tile in both directions
  const int ks[] = {1, 2, MG_TILE_K - 1, MG_TILE_K, MG_TILE_K + 1, 2 * MG_TILE_K, 2 * MG_TILE_K + 1, 129};
  const int js[] = {1, 2, MG_TILE_J - 1, MG_TILE_J, MG_TILE_J + 1, 2 * MG_TILE_J + 1, 17};
  for (int k : ks)
    for (int j : js)
      for (int i : {1, 2, 5}) check_grid_points(i, j, k);
  check_grid_extents(1025, 1025, 1025);
  check_grid_extents(65535, 3, 3);
  CHECK(!mg_grid_ok(mg_transfer_grid(65536, 3, 3)), "a lattice with more planes than a grid dimension holds is refused");
  // 3. bytes, vectors, products, streams
  {
    const MgPlan P = mg_plan(16, 24, 12, 0);
    int64_t want = MG_FLAG_BYTES;
    for (int l = 0; l < P.nlev; ++l) {
      const int64_t n = (int64_t)(P.ne[l][0] + 1) * (P.ne[l][1] + 1) * (P.ne[l][2] + 1);
      want += (l ? 5 : 3) * ((n + 31) / 32 * 32) * 8;
      if (l) want += 3 * n * 8 + 16 * (P.ne[l][0] + 1 + P.ne[l][1] + 1 + P.ne[l][2] + 1) + 24;
    }
    CHECK(mg_bytes(P) == want, "bytes of 16 x 24 x 12: %lld, closed form %lld", (long long)mg_bytes(P), (long long)want);
    CHECK(mg_level_vectors(0) == 3 && mg_level_vectors(1) == 5, "vectors per level");
  }
  for (int nu = 1; nu <= 6; ++nu)
    for (int nlev = 1; nlev <= 5; ++nlev) {
      for (int l = 0; l < nlev; ++l) {
        CHECK(mg_cycle_products(l, nlev, nu, 32) == (l == nlev - 1 ? 31 : 2 * nu), "products of level %d of %d", l, nlev);
        if (l < nlev - 1) CHECK(mg_cycle_streams(l, nlev, nu, 32) <= 12 * nu + 4, "streams of level %d of %d at nu = %d", l, nlev, nu);
      }
      CHECK(mg_pass_products(1, 7, nlev, nu, 32) == 1 + 7 + (nlev == 1 ? 31 : 2 * nu) * 7 + 1 && mg_pass_products(0, 0, nlev, nu, 32) == 1, "products of a pass");
    }
  CHECK(mg_cycle_streams(0, 3, 2, 32) == 26, "a level below the coarsest moves 26 streams at nu = 2");
  // 4. options, Chebyshev, gate
  {
    MgOptions o;
    CHECK(mg_options(nullptr, &o) == nullptr && o.nu == 2 && o.nu_c == 32 && o.range_s == 4.0 && o.range_c == 300.0 && o.eig_steps == 20 && o.max_levels == 12, "defaults");
    mfem_multigrid_options in;
    memset(&in, 0, sizeof(in));
    CHECK(mg_options(&in, &o) == nullptr && o.nu == 2 && o.eig_steps == 20, "zero fields take the defaults");
    in.smoother_degree = 3; in.coarse_degree = 8; in.smoothing_range = 5.0; in.coarse_range = 100.0; in.eig_steps = 12; in.max_levels = 2;
    CHECK(mg_options(&in, &o) == nullptr && o.nu == 3 && o.nu_c == 8 && o.range_s == 5.0 && o.range_c == 100.0 && o.eig_steps == 12 && o.max_levels == 2, "given fields");
    in.eig_steps = 9;
    CHECK(mg_options(&in, &o) != nullptr, "fewer than 10 power steps are refused");
    in.eig_steps = 0; in.smoothing_range = 1.0;
    CHECK(mg_options(&in, &o) != nullptr, "a range of 1 is refused");
    in.smoothing_range = 0.0; in.max_levels = 13;
    CHECK(mg_options(&in, &o) != nullptr, "13 levels are refused");
    in.max_levels = 0; in.smoother_degree = -1;
    CHECK(mg_options(&in, &o) != nullptr, "a negative degree is refused");
  }
  {  // the coefficients reproduce the Chebyshev residual polynomial: on a scalar problem a x = 1 the error after nu steps is T_nu((theta - a) / delta) / T_nu(sigma)
    const double lo = 0.4, hi = 1.65;
    for (int nu = 1; nu <= 8; ++nu)
      for (double a : {0.4, 0.7, 1.0, 1.3, 1.65}) {
        double c1, c2, z = 0.0, d = 0.0, r = 1.0;
        MgCheb C = mg_cheb_start(lo, hi, &c1, &c2);
        for (int k = 0; k < nu; ++k) {
          if (k) { r -= a * d; mg_cheb_next(&C, &c1, &c2); }
          d = c1 * d + c2 * r;
          z += d;
        }
        auto T = [](int n, double x) { double t0 = 1.0, t1 = x; if (n == 0) return t0; for (int i = 1; i < n; ++i) { const double t2 = 2.0 * x * t1 - t0; t0 = t1; t1 = t2; } return t1; };
        const double theta = (hi + lo) / 2.0, delta = (hi - lo) / 2.0;
        const double want = T(nu, (theta - a) / delta) / T(nu, theta / delta);
        CHECK(std::fabs((1.0 - a * z) - want) <= 1e-13, "Chebyshev residual at a = %g after %d steps: %g, want %g", a, nu, 1.0 - a * z, want);
      }
  }
  CHECK(mg_solve_refusal(true, true, MFEM_SOLVER_CG, MFEM_LEFT_NONE, false, false) == nullptr, "the admitted solve");
  CHECK(mg_solve_refusal(false, false, MFEM_SOLVER_CG, 0, false, false) && mg_solve_refusal(true, false, MFEM_SOLVER_CG, 0, false, false) &&
        mg_solve_refusal(true, true, MFEM_SOLVER_IDRS, 0, false, false) && mg_solve_refusal(true, true, MFEM_SOLVER_CG, MFEM_LEFT_JACOBI_DIAG, false, false) &&
        mg_solve_refusal(true, true, MFEM_SOLVER_CG, 0, true, false) && mg_solve_refusal(true, true, MFEM_SOLVER_CG, 0, false, true), "every refusal has a reason");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
