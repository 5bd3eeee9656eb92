// CPU walk of csrc/symp_const_decide.h (tests/test_symp_const_decide.py): the gate of the constant form, the rotation of the runs among the waves and the entry accounting.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_symp_const.cpp -o host_check_symp_const && ./host_check_symp_const
#include <cstdio>
#include <vector>

#include "symp_const_decide.h"
#include "symp_trim_decide.h"

static int fails = 0;
#define CHECK(c, ...)            \
  do {                           \
    if (!(c)) {                  \
      ++fails;                   \
      printf("FAIL %s: ", #c);   \
      printf(__VA_ARGS__);       \
      printf("\n");              \
    }                            \
  } while (0)

int main() {
  // ---- the gate: flagged / steps >= 2 c / (c + g), never without a flagged step; walked against the rational form
  {
    const int64_t c = spc_cost_ps(), g = SPC_GAIN_PS;
    CHECK(g > 0 && c >= 0, "c %lld g %lld", (long long)c, (long long)g);
    const int64_t steps[] = {1, 7, 16, 208, 1000, 523264};
    for (int64_t T : steps)
      for (int64_t f = 0; f <= T; f += (T > 2000 ? T / 997 : 1)) {
        const bool want = f > 0 && (double)f / (double)T >= 2.0 * (double)c / (double)(c + g) - 1e-15;
        const bool got = spc_gate(f, T);
        // (the double form may differ from the integer one only on the boundary itself)
        if (f * (c + g) != 2 * c * T) CHECK(got == want, "gate(%lld, %lld) = %d", (long long)f, (long long)T, (int)got);
      }
    CHECK(!spc_gate(0, 100) && !spc_gate(0, 0) && spc_gate(100, 100), "ends");
    // the benchmark: 62 x 14 of 1024 patches in the 509 swept planes
    CHECK(spc_gate((int64_t)62 * 14 * 509, (int64_t)1024 * 509), "the headline's share must pass");
    // the decision: no constant form without usable flags; the knob's two bits; an invalid reference row
    CHECK(spc_form(false, true, 10, 10, false, true) == 0, "no usable flags");
    CHECK(spc_form(true, true, 10, 10, true, false) == 0 && spc_form(true, true, 10, 10, true, true) == 0, "forced stored");
    CHECK(spc_form(true, false, 0, 10, false, true) == 1, "forced constant");
    CHECK(spc_form(true, false, 10, 10, false, false) == 0 && spc_form(true, true, 0, 10, false, false) == 0 && spc_form(true, true, 10, 10, false, false) == 1, "by the gate");
  }
  // ---- runs and waves: every run of a round is taken exactly once; at the headline (96 waves per XCD, 128 patches x 3 runs, 16 patch columns) no wave
  // meets the first or last patch column in more than one of its four rounds, where the unrotated order gives a wave the same column four times
  {
    const int Ws[] = {96, 96, 7, 24, 1}, Rts[] = {384, 100, 30, 24, 5}, NPks[] = {16, 16, 5, 3, 2};
    for (int c = 0; c < 5; ++c) {
      const int W = Ws[c], Rt = Rts[c], rot = spc_rot(NPks[c]);
      std::vector<int> seen((size_t)Rt, 0);
      for (int jw = 0; jw < W; ++jw)
        for (int rk = 0; W * rk < Rt; ++rk) {
          const int run = spc_run(W, jw, rk, rot);
          CHECK(run >= W * rk && run < W * rk + W, "W %d jw %d rk %d: run %d outside its round", W, jw, rk, run);
          if (run < Rt) ++seen[(size_t)run];
        }
      for (int r = 0; r < Rt; ++r) CHECK(seen[(size_t)r] == 1, "W %d Rt %d: run %d taken %d times", W, Rt, r, seen[(size_t)r]);
    }
    CHECK(spc_rot(16) == 4, "rot %d", spc_rot(16));
    for (int jw = 0; jw < 96; ++jw) {
      int rim = 0, rim0 = 0;
      for (int rk = 0; rk < 4; ++rk) {
        const int col = (spc_run(96, jw, rk, spc_rot(16)) % 128) % 16, col0 = (spc_run(96, jw, rk, 0) % 128) % 16;
        rim += col == 0 || col == 15;
        rim0 += col0 == 0 || col0 == 15;
      }
      CHECK(rim <= 1 && (rim0 == 0 || rim0 == 4), "wave %d: %d rim-column runs (unrotated %d)", jw, rim, rim0);
    }
  }
  // ---- accounting, by hand: a whole step reads per lane pair 14 slots of two rows and the edge block
  CHECK(spc_saved_entries(1) == 28 * 64 + 318 && spc_saved_entries(2) == 28 * 128 + 354, "%lld %lld", (long long)spc_saved_entries(1), (long long)spc_saved_entries(2));
  CHECK(spc_saved_codes(1) == 128 && spc_saved_codes(2) == 256, "codes");
  CHECK(spc_saved_entries(2) == sp_eoff(2, 0) + sp_ne(2) && spc_saved_entries(2) - spc_saved_codes(2) == sp_eoff(2, 1) + sp_ne(2), "the main part's slots");
  CHECK(spc_flag_doubles(0) == 0 && spc_flag_doubles(1) == 1 && spc_flag_doubles(8) == 1 && spc_flag_doubles(9) == 2, "flag doubles");
  // ---- the tests' fixture: lattice (17, 33, 129), swept planes [2, 15)
  {
    const int planes = 17, m1 = 33, m2 = 129, p0 = 2, p1 = 15;
    for (int B = 1; B <= 2; ++B)
      for (int trim = 0; trim <= 1; ++trim) {
        const int ms1 = spt_ms1(m1, B, trim != 0), ms2 = spt_ms2(m2, trim != 0);
        const int64_t got = spc_expected(planes, m1, m2, p0, p1, ms1, ms2, B);
        const int64_t want = (B == 1 ? 6 : 2) * 2 * 13;  // patch rows 4..27 / 8..23, patch columns 32..95, planes 2..14
        CHECK(got == want, "B %d trim %d: %lld, by hand %lld", B, trim, (long long)got, (long long)want);
        const int64_t steps = (int64_t)spt_rows(ms1, B) * spt_cols(ms2) * (p1 - p0);
        CHECK(got > 0 && got < steps, "B %d trim %d", B, trim);
        // entries of a bind in the constant form against the stored form, stored diagonal: flagged x (28 x 64 B + ne) fewer, one byte per step more
        const int64_t fewer = got * spc_saved_entries(B) - spc_flag_doubles(steps);
        CHECK(fewer == want * (B == 1 ? 2110 : 3938) - (steps + 7) / 8, "B %d trim %d: %lld", B, trim, (long long)fewer);
      }
  }
  // the headline lattice: 513^3, swept planes [2, 511), B = 2 trimmed: 62 x 14 of 1024 patches in every swept plane
  CHECK(spc_expected(513, 513, 513, 2, 511, 512, 512, 2) == (int64_t)62 * 14 * 509, "%lld", (long long)spc_expected(513, 513, 513, 2, 511, 512, 512, 2));
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
