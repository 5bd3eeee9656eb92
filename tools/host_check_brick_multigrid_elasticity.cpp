// CPU walk through the field-aware host decisions of the geometric multigrid preconditioner (csrc/brick_multigrid_decide.h) that the hex-8
// elasticity hierarchy (mfem_brick_multigrid_create_elasticity) adds beside the thermal ones:
//   1. the bytes of a 3-field hierarchy against the closed form, for every plan up to 32^3 (a digest for the Python restatement,
//      tests/test_brick_multigrid_elasticity_host.py) and for 128^3, 256^3, 512^3 line by line; with fields = 1 they are mg_bytes;
//   2. the field offsets and the padding: field f of a level vector starts at f * points, the fields tile [0, fields * points) without a gap, the
//      vector -- not each field -- is padded to 32 doubles, and the pad is shorter than 32;
//   3. the streams per cycle: mg_cycle_streams is unchanged, the bytes are streams x 8 x fields x points;
//   4. the truth table of the solve gate with "elasticity operator" and "hierarchy attached" as inputs, and the refusal of a singular K.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_multigrid_elasticity.cpp -o tools/bin/host_check_brick_multigrid_elasticity
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "brick_multigrid_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

static int64_t closed_form(const MgPlan& P, int fields) {
  int64_t want = 16;
  for (int l = 0; l < P.nlev; ++l) {
    const int64_t pts = (int64_t)(P.ne[l][0] + 1) * (P.ne[l][1] + 1) * (P.ne[l][2] + 1);
    want += (l ? 5 : 3) * ((fields * pts + 31) / 32 * 32) * 8;
    if (l) want += 3 * pts * 8 + 16 * ((int64_t)P.ne[l][0] + 1 + P.ne[l][1] + 1 + P.ne[l][2] + 1) + 24;
  }
  return want;
}

static void check_fields(const MgPlan& P) {
  for (int l = 0; l < P.nlev; ++l) {
    const int64_t pts = mg_points(P.ne[l]);
    for (int fields : {1, MG_ELASTICITY_FIELDS}) {
      const int64_t n = mg_level_entries(fields, P.ne[l]), npad = mg_padded(n);
      CHECK(n == fields * pts, "entries of level %d", l);
      CHECK(npad % 32 == 0 && npad >= n && npad - n < 32, "the vector is padded to 32 doubles: %lld -> %lld", (long long)n, (long long)npad);
      for (int f = 0; f < fields; ++f) {
        CHECK(mg_field_offset(f, pts) == f * pts, "field %d starts at f * points", f);
        CHECK(mg_field_offset(f, pts) + pts <= n, "field %d ends inside the vector", f);
        if (f) CHECK(mg_field_offset(f, pts) == mg_field_offset(f - 1, pts) + pts, "fields %d and %d are adjacent: no pad between fields", f - 1, f);
      }
    }
  }
}

int main() {
  // 1. bytes: every plan up to 32^3, the digest
  unsigned long long digest = 0, count = 0;
  for (int nx = 1; nx <= 32; ++nx)
    for (int ny = 1; ny <= 32; ++ny)
      for (int nz = 1; nz <= 32; ++nz) {
        const MgPlan P = mg_plan(nx, ny, nz, 0);
        const int64_t b3 = mg_bytes_fields(P, MG_ELASTICITY_FIELDS);
        CHECK(b3 == closed_form(P, 3), "%d x %d x %d: bytes of the 3-field hierarchy %lld, closed form %lld", nx, ny, nz, (long long)b3, (long long)closed_form(P, 3));
        CHECK(mg_bytes_fields(P, 1) == mg_bytes(P), "%d x %d x %d: one field is the thermal hierarchy", nx, ny, nz);
        CHECK(b3 >= mg_bytes(P) && b3 <= 3 * mg_bytes(P), "%d x %d x %d: between one and three thermal hierarchies", nx, ny, nz);
        for (int l = 0; l < P.nlev; ++l) CHECK(mg_level_bytes_fields(l, P.ne[l], 1) == mg_level_bytes(l, P.ne[l]), "level %d with one field", l);
        if (nx <= 12 && ny <= 12) check_fields(P);
        digest = digest * 1000003ull + (unsigned long long)P.nlev * 1315423911ull + (unsigned long long)b3;
        ++count;
      }
  printf("PLANS3 %llu %llu\n", count, digest);
  const int big[3] = {128, 256, 512};
  for (int b = 0; b < 3; ++b) {
    const MgPlan P = mg_plan(big[b], big[b], big[b], 0);
    const int64_t b3 = mg_bytes_fields(P, MG_ELASTICITY_FIELDS);
    CHECK(b3 == closed_form(P, 3), "%d^3: bytes", big[b]);
    check_fields(P);
    printf("PLAN3 %d %d %lld\n", big[b], P.nlev, (long long)b3);
  }
  {  // an odd point count: 3 x 5^3 = 375 entries pad to 384 as a whole (each field padded on its own would take 3 x 128 = 384 too; 3 x 3^3 = 81 -> 96, not 3 x 32)
    const int ne4[3] = {4, 4, 4}, ne2[3] = {2, 2, 2};
    CHECK(mg_padded(mg_level_entries(3, ne4)) == 384 && mg_padded(mg_level_entries(3, ne2)) == 96, "the vector is padded, not each field");
    CHECK(mg_field_offset(1, 27) == 27 && mg_field_offset(2, 27) == 54, "field offsets on 3^3 points");
  }
  // 3. streams
  for (int nu = 1; nu <= 4; ++nu)
    for (int nlev = 1; nlev <= 4; ++nlev)
      for (int l = 0; l < nlev; ++l) {
        const int ne[3] = {8, 6, 4};
        const int s = mg_cycle_streams(l, nlev, nu, 32);
        CHECK(mg_cycle_stream_bytes(l, nlev, nu, 32, 3, ne) == (int64_t)s * 8 * 3 * 9 * 7 * 5, "stream bytes, 3 fields");
        CHECK(mg_cycle_stream_bytes(l, nlev, nu, 32, 1, ne) == (int64_t)s * 8 * 9 * 7 * 5, "stream bytes, 1 field");
      }
  CHECK(mg_cycle_streams(0, 3, 2, 32) == 26, "a level below the coarsest still moves 26 streams at nu = 2");
  // 4. the gate's truth table
  const int CG = MFEM_SOLVER_CG, NONE = MFEM_LEFT_NONE;
  for (int brick = 0; brick <= 1; ++brick)
    for (int thermal = 0; thermal <= 1; ++thermal)
      for (int elast = 0; elast <= 1; ++elast)
        for (int attached = 0; attached <= 1; ++attached)
          for (int method : {MFEM_SOLVER_CG, MFEM_SOLVER_IDRS})
            for (int left : {MFEM_LEFT_NONE, MFEM_LEFT_JACOBI_DIAG})
              for (int comm = 0; comm <= 1; ++comm)
                for (int nitsche = 0; nitsche <= 1; ++nitsche) {
                  if ((thermal && elast) || (!brick && (thermal || elast)) || (nitsche && !thermal)) continue;  // (rows no operator produces)
                  const char* why = mg_solve_refusal_fields(brick, thermal, elast, attached, method, left, comm, nitsche);
                  const bool plain = method == CG && left == NONE && !comm && !nitsche;
                  const bool admitted = brick && plain && (thermal || (elast && attached));
                  CHECK((why == nullptr) == admitted, "gate row %d %d %d %d %d %d %d %d", brick, thermal, elast, attached, method, left, comm, nitsche);
                  if (!elast) {  // every row without an elasticity operator answers as before, in the same words
                    const char* old = mg_solve_refusal(brick, thermal, method, left, comm, nitsche);
                    CHECK(why == old || (why && old && !strcmp(why, old)), "the thermal rows are unchanged");
                  }
                }
  {
    const char* why = mg_solve_refusal_fields(true, false, true, false, CG, NONE, false, false);
    CHECK(why && strstr(why, "elasticity") && strstr(why, "mfem_brick_multigrid_create_elasticity"), "no hierarchy attached: the message names the entry point");
    CHECK(mg_solve_refusal_fields(true, false, true, true, MFEM_SOLVER_IDRS, NONE, false, false) &&
          strstr(mg_solve_refusal_fields(true, false, true, true, MFEM_SOLVER_IDRS, NONE, false, false), "MFEM_SOLVER_CG"), "idrs on an attached hierarchy");
    const char* h27 = mg_solve_refusal_fields(true, false, false, false, CG, NONE, false, false);
    CHECK(h27 && strstr(h27, "hex-27"), "a hex-27 operator keeps its message");
  }
  CHECK(mg_elasticity_refusal(0.0, 0x10) && mg_elasticity_refusal(1000.0, 0) && mg_elasticity_refusal(1000.0, 0x40) && !mg_elasticity_refusal(1000.0, 0x10) &&
        !mg_elasticity_refusal(-1.0, 0x21), "a K without a penalty face is refused");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
