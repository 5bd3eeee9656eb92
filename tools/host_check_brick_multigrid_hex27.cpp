// CPU walk through the host decisions that the hex-27 thermal hierarchy (mfem_brick_multigrid_create_hex27) adds to csrc/brick_multigrid_decide.h:
//   1. the level plan: level 0 the hex-27 brick, level 1 a hex-8 brick of the SAME element counts whenever max_levels >= 2, then mg_plan's halving
//      rule -- (1,1,1), (2,1,3), (8,12,6), (16,16,16), (3,5,7), max_levels 1 and 2, and every brick up to 20^3 against mg_plan shifted by one level;
//   2. the level-0 lattice (2 ne + 1), mf = 2 mc - 1 between levels 0 and 1 as between every other pair, and the bytes against the closed form (a
//      digest of every plan up to 20^3 for the Python restatement, tests/test_brick_multigrid_hex27_host.py, and 128^3 line by line);
//   3. every refusal string: ng < 3, Nitsche, no hierarchy attached (it names the entry point and says hex-27), the other gate rows;
//   4. that mg_plan, mg_solve_refusal and mg_solve_refusal_fields answer as before.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_multigrid_hex27.cpp -o tools/bin/host_check_brick_multigrid_hex27
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "brick_multigrid_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

static int64_t closed_form(const MgPlan& P) {
  int64_t want = 16;
  for (int l = 0; l < P.nlev; ++l) {
    const int* e = P.ne[l];
    const int64_t pts = l ? (int64_t)(e[0] + 1) * (e[1] + 1) * (e[2] + 1) : (int64_t)(2 * e[0] + 1) * (2 * e[1] + 1) * (2 * e[2] + 1);
    want += (l ? 5 : 3) * ((pts + 31) / 32 * 32) * 8;
    if (l) want += 3 * pts * 8 + 16 * ((int64_t)e[0] + 1 + e[1] + 1 + e[2] + 1) + 24;
  }
  return want;
}

static bool plan_is(const MgPlan& P, std::initializer_list<std::initializer_list<int>> want) {
  if (P.nlev != (int)want.size()) return false;
  int l = 0;
  for (const auto& lv : want) {
    int d = 0;
    for (int v : lv) {
      if (P.ne[l][d] != v) return false;
      ++d;
    }
    ++l;
  }
  return true;
}

int main() {
  // 1. the plans of the issue's table
  CHECK(plan_is(mg_plan_hex27(1, 1, 1, 0), {{1, 1, 1}, {1, 1, 1}}), "1x1x1: 27 -> 1^3");
  CHECK(plan_is(mg_plan_hex27(2, 1, 3, 0), {{2, 1, 3}, {2, 1, 3}}), "2x1x3: 27 -> 2x1x3");
  CHECK(plan_is(mg_plan_hex27(8, 12, 6, 0), {{8, 12, 6}, {8, 12, 6}, {4, 6, 3}}), "8x12x6: 27 -> 8x12x6 -> 4x6x3");
  CHECK(plan_is(mg_plan_hex27(16, 16, 16, 0), {{16, 16, 16}, {16, 16, 16}, {8, 8, 8}, {4, 4, 4}, {2, 2, 2}}), "16^3: 27 -> 16^3 -> ... -> 2^3");
  CHECK(plan_is(mg_plan_hex27(3, 5, 7, 0), {{3, 5, 7}, {3, 5, 7}}), "3x5x7: 27 -> 3x5x7");
  CHECK(plan_is(mg_plan_hex27(8, 8, 8, 0), {{8, 8, 8}, {8, 8, 8}, {4, 4, 4}, {2, 2, 2}}), "8^3");
  CHECK(plan_is(mg_plan_hex27(4, 4, 4, 0), {{4, 4, 4}, {4, 4, 4}, {2, 2, 2}}), "4^3");
  CHECK(plan_is(mg_plan_hex27(6, 6, 6, 0), {{6, 6, 6}, {6, 6, 6}, {3, 3, 3}}), "6^3");
  CHECK(plan_is(mg_plan_hex27(16, 16, 16, 1), {{16, 16, 16}}), "max_levels 1: the hex-27 level alone");
  CHECK(plan_is(mg_plan_hex27(16, 16, 16, 2), {{16, 16, 16}, {16, 16, 16}}), "max_levels 2: p-coarsening alone");
  CHECK(plan_is(mg_plan_hex27(16, 16, 16, 3), {{16, 16, 16}, {16, 16, 16}, {8, 8, 8}}), "max_levels 3");
  CHECK(plan_is(mg_plan_hex27(1, 1, 1, 1), {{1, 1, 1}}) && plan_is(mg_plan_hex27(1, 1, 1, 2), {{1, 1, 1}, {1, 1, 1}}), "1^3 with max_levels 1 and 2");
  CHECK(mg_plan_hex27(1024, 1024, 1024, 0).nlev == 11 && mg_plan_hex27(4096, 4096, 4096, 0).nlev == MG_MAX_LEVELS, "the cap of 12 levels holds");
  // 2. every brick up to 20^3: the plan is mg_plan shifted by one level; lattices; bytes; the digest
  unsigned long long digest = 0, count = 0;
  for (int nx = 1; nx <= 20; ++nx)
    for (int ny = 1; ny <= 20; ++ny)
      for (int nz = 1; nz <= 20; ++nz)
        for (int ml : {0, 1, 2, 3}) {
          const MgPlan P = mg_plan_hex27(nx, ny, nz, ml);
          const MgPlan H = mg_plan(nx, ny, nz, ml == 0 ? MG_MAX_LEVELS - 1 : (ml >= 2 ? ml - 1 : 1));
          CHECK(P.ne[0][0] == nx && P.ne[0][1] == ny && P.ne[0][2] == nz, "level 0 is the caller's brick");
          if (ml == 1) {
            CHECK(P.nlev == 1, "max_levels 1");
          } else {
            CHECK(P.nlev == 1 + H.nlev, "%d x %d x %d (%d): %d levels, the hex-8 plan has %d", nx, ny, nz, ml, P.nlev, H.nlev);
            for (int l = 0; l < H.nlev && l + 1 < P.nlev; ++l)
              for (int d = 0; d < 3; ++d) CHECK(P.ne[l + 1][d] == H.ne[l][d], "level %d is the hex-8 plan's level %d", l + 1, l);
          }
          CHECK(ml == 0 || P.nlev <= ml, "max_levels caps the plan");
          for (int l = 0; l < P.nlev; ++l) {
            for (int d = 0; d < 3; ++d) {
              const int m = mg_lattice_hex27(l, P.ne[l][d]);
              CHECK(m == (l ? P.ne[l][d] + 1 : 2 * P.ne[l][d] + 1), "lattice of level %d", l);
              if (l + 1 < P.nlev) CHECK(m == 2 * mg_lattice_hex27(l + 1, P.ne[l + 1][d]) - 1, "mf = 2 mc - 1 between levels %d and %d", l, l + 1);
            }
            int64_t pts = 1;
            for (int d = 0; d < 3; ++d) pts *= mg_lattice_hex27(l, P.ne[l][d]);
            CHECK(mg_points_hex27(l, P.ne[l]) == pts, "points of level %d", l);
            if (l) CHECK(mg_points_hex27(l, P.ne[l]) == mg_points(P.ne[l]) && mg_level_bytes_hex27(l, P.ne[l]) == mg_level_bytes(l, P.ne[l]), "a hex-8 level");
          }
          const int64_t b = mg_bytes_hex27(P);
          CHECK(b == closed_form(P), "%d x %d x %d (%d): bytes %lld, closed form %lld", nx, ny, nz, ml, (long long)b, (long long)closed_form(P));
          if (ml == 0) {
            digest = digest * 1000003ull + (unsigned long long)P.nlev * 1315423911ull + (unsigned long long)b;
            ++count;
          }
        }
  printf("PLANS27 %llu %llu\n", count, digest);
  {
    const MgPlan P = mg_plan_hex27(128, 128, 128, 0);
    CHECK(P.nlev == 8 && mg_points_hex27(0, P.ne[0]) == 257ll * 257 * 257 && mg_bytes_hex27(P) == closed_form(P), "128^3");
    printf("PLAN27 128 %d %lld\n", P.nlev, (long long)mg_bytes_hex27(P));
    const int ne[3] = {8, 6, 4};
    CHECK(mg_cycle_stream_bytes_hex27(0, 3, 2, 32, ne) == 26ll * 8 * 17 * 13 * 9, "stream bytes of level 0");
    CHECK(mg_cycle_stream_bytes_hex27(1, 3, 2, 32, ne) == 28ll * 8 * 9 * 7 * 5, "stream bytes of level 1");
  }
  // 3. the refusals
  const int CG = MFEM_SOLVER_CG, NONE = MFEM_LEFT_NONE;
  {
    CHECK(!mg_hex27_refusal(3, false) && !mg_hex27_refusal(4, false), "3 and 4 Gauss points per direction are taken");
    const char* w1 = mg_hex27_refusal(1, false);
    const char* w2 = mg_hex27_refusal(2, false);
    CHECK(w1 && w2 && !strcmp(w1, w2), "1 and 2 points are refused alike");
    CHECK(w2 && strstr(w2, "fewer than 3 Gauss points") && strstr(w2, "itg_order < 4") && strstr(w2, "near-null modes") && strstr(w2, "hex-8 coarse space"),
          "the ng < 3 refusal says why");
    const char* wn = mg_hex27_refusal(3, true);
    CHECK(wn && strstr(wn, "Nitsche"), "a Nitsche term is refused");
    CHECK(mg_hex27_refusal(2, true) && strstr(mg_hex27_refusal(2, true), "Nitsche"), "Nitsche is named first");
    const char* none = mg_solve_refusal_hex27(true, false, false, true, false, CG, NONE, false, false);
    CHECK(none && strstr(none, "hex-27") && strstr(none, "mfem_brick_multigrid_create_hex27"), "no hierarchy attached: hex-27 and the entry point are named");
    CHECK(!mg_solve_refusal_hex27(true, false, false, true, true, CG, NONE, false, false), "attached: admitted");
    const char* w;
    w = mg_solve_refusal_hex27(true, false, false, true, true, MFEM_SOLVER_IDRS, NONE, false, false);
    CHECK(w && strstr(w, "MFEM_SOLVER_CG"), "the method");
    w = mg_solve_refusal_hex27(true, false, false, true, true, CG, MFEM_LEFT_JACOBI_DIAG, false, false);
    CHECK(w && strstr(w, "left"), "a left preconditioner");
    w = mg_solve_refusal_hex27(true, false, false, true, true, CG, NONE, true, false);
    CHECK(w && strstr(w, "communicator"), "a communicator");
    w = mg_solve_refusal_hex27(true, false, false, true, true, CG, NONE, false, true);
    CHECK(w && strstr(w, "Nitsche"), "a Nitsche term in the gate");
  }
  // 4. the gate's truth table; every row without a hex-27 operator answers as before, in the same words
  for (int brick = 0; brick <= 1; ++brick)
    for (int kind = 0; kind <= 3; ++kind)  // 0: none of the three, 1: hex-8 thermal, 2: hex-8 elasticity, 3: hex-27 thermal
      for (int attached = 0; attached <= 1; ++attached)
        for (int method : {MFEM_SOLVER_CG, MFEM_SOLVER_IDRS})
          for (int left : {MFEM_LEFT_NONE, MFEM_LEFT_JACOBI_DIAG})
            for (int comm = 0; comm <= 1; ++comm)
              for (int nitsche = 0; nitsche <= 1; ++nitsche) {
                const bool thermal = kind == 1, elast = kind == 2, h27 = kind == 3;
                if ((!brick && kind) || (nitsche && !(thermal || h27))) continue;  // (rows no operator produces)
                const char* why = mg_solve_refusal_hex27(brick, thermal, elast, h27, attached, method, left, comm, nitsche);
                const bool plain = method == CG && left == NONE && !comm && !nitsche;
                const bool admitted = brick && plain && (thermal || ((elast || h27) && attached));
                CHECK((why == nullptr) == admitted, "gate row %d %d %d %d %d %d %d", brick, kind, attached, method, left, comm, nitsche);
                if (!h27) {
                  const char* old = mg_solve_refusal_fields(brick, thermal, elast, attached, method, left, comm, nitsche);
                  CHECK(why == old || (why && old && !strcmp(why, old)), "the rows without a hex-27 operator are unchanged");
                }
              }
  {  // the functions from before this hierarchy
    CHECK(plan_is(mg_plan(16, 24, 12, 0), {{16, 24, 12}, {8, 12, 6}, {4, 6, 3}}) && plan_is(mg_plan(9, 14, 15, 0), {{9, 14, 15}}) &&
          plan_is(mg_plan(32, 32, 32, 2), {{32, 32, 32}, {16, 16, 16}}) && mg_plan(4, 4, 4, 0).nlev == 2 && mg_plan(2, 2, 2, 0).nlev == 1, "mg_plan answers as before");
    const char* a = mg_solve_refusal(true, false, CG, NONE, false, false);
    CHECK(a && !strcmp(a, "the multigrid preconditioner covers the hex-8 thermal brick operator: elasticity and hex-27 operators are not covered"),
          "mg_solve_refusal keeps its words");
    CHECK(!mg_solve_refusal(true, true, CG, NONE, false, false) && mg_solve_refusal(false, false, CG, NONE, false, false), "mg_solve_refusal's rows");
    const char* b = mg_solve_refusal_fields(true, false, false, false, CG, NONE, false, false);
    CHECK(b && !strcmp(a, b), "mg_solve_refusal_fields answers a hex-27 operator as before");
    const char* c = mg_solve_refusal_fields(true, false, true, false, CG, NONE, false, false);
    CHECK(c && strstr(c, "mfem_brick_multigrid_create_elasticity") && !mg_solve_refusal_fields(true, false, true, true, CG, NONE, false, false),
          "mg_solve_refusal_fields' elasticity rows");
    const int ne[3] = {8, 8, 8};
    CHECK(mg_level_bytes(0, ne) == 3 * 736 * 8 && mg_points(ne) == 729, "mg_level_bytes and mg_points are unchanged");
  }
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
