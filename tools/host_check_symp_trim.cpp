// CPU walk of csrc/symp_trim_decide.h (tests/test_symp_trim_decide.py): swept extents, the rim's enumeration and the run count of the trimmed patch sweep.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_symp_trim.cpp -o host_check_symp_trim && ./host_check_symp_trim
#include <cstdio>
#include <vector>

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
  const int sizes[] = {8, 9, 12, 16, 17, 32, 33, 34, 35, 64, 65, 513};
  for (int B = 1; B <= SP_BMAX; ++B)
    for (int m1 : sizes)
      for (int m2 : sizes) {
        const int ms1 = spt_ms1(m1, B), ms2 = spt_ms2(m2), L = SP_L * B;
        const int NR = spt_rows(ms1, B), NPk = spt_cols(ms2), nrim = spt_rim(m1, m2, ms1, ms2);
        // the rule: a direction is trimmed exactly when its remainder is narrow and a whole patch is left; a trimmed extent is whole patches
        const bool tj = m1 % L >= 1 && m1 % L <= SPT_MAX_LINES && m1 / L >= 1, tk = m2 % SP_W >= 1 && m2 % SP_W <= SPT_MAX_POINTS && m2 / SP_W >= 1;
        CHECK(ms1 == (tj ? m1 - m1 % L : m1) && ms2 == (tk ? m2 - m2 % SP_W : m2), "B %d m1 %d m2 %d -> %d %d", B, m1, m2, ms1, ms2);
        CHECK(ms1 >= 1 && ms2 >= 1 && NR >= 1 && NPk >= 1 && ms1 <= m1 && ms2 <= m2, "B %d m1 %d m2 %d: a direction trimmed to nothing", B, m1, m2);
        CHECK(!tj || NR * L == ms1, "B %d m1 %d", B, m1);
        CHECK(!tk || NPk * SP_W == ms2, "m2 %d", m2);
        CHECK(spt_ms1(m1, B, false) == m1 && spt_ms2(m2, false) == m2, "the untrimmed form");
        // patches and rim rows tile the plane exactly once; the corner rows are counted once, in the line rim
        std::vector<int> cover((size_t)m1 * m2, 0), seen((size_t)(nrim > 0 ? nrim : 1), 0);
        for (int pr = 0; pr < NR; ++pr)
          for (int pc = 0; pc < NPk; ++pc)
            for (int l = 0; l < L; ++l)
              for (int c = 0; c < SP_W; ++c) {
                const int j = pr * L + l, k = pc * SP_W + c;
                if (j < m1 && k < m2) {  // lane validity follows the lattice, not the swept extents
                  CHECK(j < ms1 && k < ms2, "B %d m1 %d m2 %d: patch cell (%d, %d) outside the swept extents", B, m1, m2, j, k);
                  ++cover[(size_t)j * m2 + k];
                }
              }
        int count = 0;
        for (int j = 0; j < m1; ++j)
          for (int k = 0; k < m2; ++k) {
            const int idx = spt_rim_index(j, k, m2, ms1, ms2);
            CHECK((idx < 0) == (j < ms1 && k < ms2), "B %d m1 %d m2 %d (%d, %d): idx %d", B, m1, m2, j, k, idx);
            if (idx < 0) continue;
            ++count;
            ++cover[(size_t)j * m2 + k];
            CHECK(idx < nrim, "B %d m1 %d m2 %d (%d, %d): idx %d of %d", B, m1, m2, j, k, idx, nrim);
            if (idx >= nrim) continue;
            ++seen[idx];
            int jb = -1, kb = -1;
            spt_rim_row(idx, m2, ms1, ms2, jb, kb);
            CHECK(jb == j && kb == k, "B %d m1 %d m2 %d (%d, %d) -> %d -> (%d, %d)", B, m1, m2, j, k, idx, jb, kb);
            // column rim first, then the line rim; the corner belongs to the line rim
            CHECK((idx >= spt_rim_cols(ms1, m2, ms2)) == (j >= ms1), "B %d m1 %d m2 %d (%d, %d): idx %d", B, m1, m2, j, k, idx);
          }
        CHECK(count == nrim, "B %d m1 %d m2 %d: %d rim rows, spt_rim %d", B, m1, m2, count, nrim);
        for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1, "B %d m1 %d m2 %d: row %zu covered %d times", B, m1, m2, i, cover[i]);
        for (int i = 0; i < nrim; ++i) {
          CHECK(seen[i] == 1, "B %d m1 %d m2 %d: rim index %d used %d times", B, m1, m2, i, seen[i]);
          int j = -1, k = -1;
          spt_rim_row(i, m2, ms1, ms2, j, k);
          CHECK(j >= 0 && j < m1 && k >= 0 && k < m2 && spt_rim_index(j, k, m2, ms1, ms2) == i, "B %d m1 %d m2 %d: rim index %d -> (%d, %d)", B, m1, m2, i, j, k);
        }
        // consecutive lines of the column rim are adjacent in the enumeration
        if (ms2 < m2 && ms1 > 1) CHECK(spt_rim_index(1, ms2, m2, ms1, ms2) == spt_rim_index(0, m2 - 1, m2, ms1, ms2) + 1, "B %d m1 %d m2 %d", B, m1, m2);
      }
  // the headline: 513 x 513 at B = 2 -- 64 x 16 whole patches and 512 + 513 rim rows per plane; 3 runs per patch fill 768 slots in four whole rounds
  {
    const int ms1 = spt_ms1(513, 2), ms2 = spt_ms2(513);
    CHECK(ms1 == 512 && ms2 == 512, "%d %d", ms1, ms2);
    CHECK(spt_rows(ms1, 2) * spt_cols(ms2) == 1024, "%d patches", spt_rows(ms1, 2) * spt_cols(ms2));
    CHECK(spt_rim(513, 513, ms1, ms2) == 1025, "%d rim rows", spt_rim(513, 513, ms1, ms2));
    CHECK(spt_rows(513, 2) * spt_cols(513) == 1105, "untrimmed: %d patches", spt_rows(513, 2) * spt_cols(513));
    CHECK(spt_nseg(1024, 768, 511) == 3, "nseg %d", spt_nseg(1024, 768, 511));
    CHECK(spt_nseg(1105, 768, 511) == 2, "untrimmed nseg %d", spt_nseg(1105, 768, 511));
    CHECK(spt_units((int64_t)1025 * 511) == 8184 && SPT_UNIT_DOUBLES == 1728, "units");
  }
  // 257 x 257 at B = 1 (256^3): 585 -> 512 patches
  CHECK(spt_rows(spt_ms1(257, 1), 1) * spt_cols(spt_ms2(257)) == 512 && spt_rows(257, 1) * spt_cols(257) == 585, "256^3");
  // what stays swept: a 3-point or 4-line remainder, and a lattice smaller than one patch
  CHECK(spt_ms2(35) == 35 && spt_ms2(34) == 32 && spt_ms1(12, 2) == 12 && spt_ms1(12, 1) == 12 && spt_ms1(5, 2) == 5 && spt_ms1(5, 1) == 4 && spt_ms2(3) == 3 && spt_ms2(1) == 1, "limits");
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
