// CPU replay of the mirror-table bookkeeping of the wave-private patch sweep (csrc/spmv_symp.h, k_spmv_symp in spmv_sym.hip) on a small
// lattice with a symmetric 27-point operator, for both forms (one band of four lines per patch, two bands): for every patch, plane, band, lane,
// row and lower slot the value the kernel would read from its LDS tables (interior cells written from the upper slots of the source rows --
// band 0's slots 24..26 held back until the plane's last band has read --, halo cells from the edge block, run starts from the row's
// own slots) must be the row's own entry; edge-block cells must be distinct halo cells, interior cells distinct non-halo cells; the placement of
// the patch-major copy (band-major main and low parts, edge block behind the bands) must give every (row, slot) a place of its own inside its step.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_symp.cpp -o tools/bin/host_check_symp && tools/bin/host_check_symp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
#include "spmv_symp.h"

static int m1, m2;
static int64_t PL;
// symmetric operator on the lattice: entry (r, c) for lattice neighbours, 0 where the neighbour does not exist
static bool coords(int64_t r, int& i, int& j, int& k) {
  i = (int)(r / PL);
  j = (int)((r % PL) / m2);
  k = (int)(r % m2);
  return true;
}
static double entry(int64_t r, int s) {  // slot s = (di, dj, dk) of row r
  int i, j, k;
  coords(r, i, j, k);
  const int di = s / 9 - 1, dj = (s / 3) % 3 - 1, dk = s % 3 - 1;
  const int jj = j + dj, kk = k + dk;
  if (jj < 0 || jj >= m1 || kk < 0 || kk >= m2) return 0.0;  // structurally absent
  const int64_t c = r + di * PL + dj * m2 + dk;
  const int64_t a = r < c ? r : c, b = r < c ? c : r;
  return 1.0 + (double)((a * 1315423911LL + b * 2654435761LL) % 1000003) / 7.0;  // symmetric in (r, c)
}

static int check_form(const int B) {
  int bad = 0;
  const int L = SP_L * B, NE = sp_ne(B), EPAD = sp_epad(B), TAB = sp_tab(B), BT = SP_L * SP_LS;
  // ---- static checks
  if (B == 1 && (NE != 318 || EPAD != 320 || TAB != 2196 || sp_main(1) != 14 * 128 + 320 || sp_low(1) != 13 * 128 || sp_xn(1) != 6 * 34)) { printf("one band: the geometry changed\n"); ++bad; }
  if (B == 2 && (NE != 354 || EPAD != 384 || TAB != 4068 || sp_main(2) != 14 * 256 + 384 || sp_xn(2) != 10 * 34)) { printf("two bands: geometry\n"); ++bad; }
  std::set<int> halo;
  for (int e = 0; e < EPAD; ++e) {
    int s, line, col, cell;
    if (!sp_edge(e, s, line, col, cell, B)) {
      if (e < NE) { printf("edge %d not decoded\n", e); ++bad; }
      continue;
    }
    if (cell < sp_tbase(s, B) || cell >= sp_tbase(s, B) + sp_tsize(s, B)) { printf("edge %d: cell outside table %d\n", e, s); ++bad; }
    if (!halo.insert(cell).second) { printf("edge %d: cell %d filled twice\n", e, cell); ++bad; }
    if (line < 0 || line >= L || col < 0 || col >= SP_W) { printf("edge %d: referencing row outside the patch\n", e); ++bad; }
  }
  {  // sp_edge_of is the inverse of sp_edge: every (slot, line, col) owns at most one entry, all NE entries are owned
    int owned = 0;
    for (int s = 0; s < 13; ++s)
      for (int line = 0; line < L; ++line)
        for (int col = 0; col < SP_W; ++col) {
          const int e = sp_edge_of(s, line, col, B);
          if (e < 0) continue;
          ++owned;
          int s2, l2, c2, cell2;
          if (e >= NE || !sp_edge(e, s2, l2, c2, cell2, B) || s2 != s || l2 != line || c2 != col) {
            printf("sp_edge_of(%d, %d, %d) = %d does not decode back\n", s, line, col, e);
            ++bad;
          }
        }
    if (owned != NE) { printf("sp_edge_of owns %d entries, NE = %d\n", owned, NE); ++bad; }
  }
  if ((int)halo.size() != NE) { printf("edge block has %zu cells, NE = %d\n", halo.size(), NE); ++bad; }
  for (int s = 0; s < 13; ++s)
    for (int b = 0; b < B; ++b)
      for (int lane = 0; lane < 64; ++lane) {
        const int lj = lane / SP_PW, pk = lane % SP_PW, lb = b * BT + lj * SP_LS + 2 * pk;
        const int w = sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb;  // the two interior cells the lane writes
        if (halo.count(w) || halo.count(w + 1)) { printf("slot %d lane %d: interior cell is a halo cell\n", s, lane); ++bad; }
        if (w + 1 >= sp_tbase(s, B) + sp_tsize(s, B)) { printf("slot %d lane %d: interior cell outside its table\n", s, lane); ++bad; }
      }
  {  // placement inside a step: (band, slot, line, column) and the edge entries each get a place of their own; main and low parts are filled exactly
    std::vector<int> main_(sp_main(B), 0), low_(sp_low(B), 0);
    for (int b = 0; b < B; ++b)
      for (int sl = 0; sl < 27; ++sl)
        for (int line = 0; line < SP_L; ++line)
          for (int col = 0; col < SP_W; ++col) {
            if (sl < 13) ++low_[b * 13 * SP_ROWS + sl * SP_ROWS + line * SP_W + col];
            else ++main_[b * 14 * SP_ROWS + (sl - 13) * SP_ROWS + line * SP_W + col];
          }
    for (int e = 0; e < EPAD; ++e) ++main_[B * 14 * SP_ROWS + e];
    for (int v : main_) if (v != 1) { printf("main part: a place written %d times\n", v); ++bad; break; }
    for (int v : low_) if (v != 1) { printf("low part: a place written %d times\n", v); ++bad; break; }
  }
  // ---- replay on lattices with partial patches in both directions (lines: band 1 empty, one line in band 1, a half-full band, 8 + 8 + 1)
  const int cases[6][3] = {{5, 9, 70}, {4, 4, 33}, {6, 13, 32}, {5, 5, 3}, {5, 12, 34}, {5, 17, 65}};
  for (auto& cs : cases) {
    const int m0 = cs[0];
    m1 = cs[1];
    m2 = cs[2];
    PL = (int64_t)m1 * m2;
    const int NR = (m1 + L - 1) / L, NPk = (m2 + SP_W - 1) / SP_W;
    for (int patch = 0; patch < NR * NPk; ++patch) {
      const int j0 = (patch / NPk) * L, k0 = (patch % NPk) * SP_W;
      int nb = 1;
      for (int b = 1; b < B; ++b) if (j0 + SP_L * b < m1) nb = b + 1;  // bands with a valid line: the others are skipped
      std::vector<double> tab(TAB + 2, NAN);
      for (int start = 1; start <= 2; ++start) {  // run starts at plane 1 and at plane 2
        std::fill(tab.begin(), tab.end(), NAN);
        bool have_hist = false;
        for (int p = start; p < m0 - 1; ++p) {
          auto rowof = [&](int b, int lane, int h, bool& valid) -> int64_t {
            const int j = j0 + SP_L * b + (lane / SP_PW), k = k0 + 2 * (lane % SP_PW) + h;
            valid = j < m1 && k < m2;
            return (int64_t)p * PL + (int64_t)j * m2 + k;
          };
          if (!have_hist)  // run start: own previous-plane slots to where the mirror reads look
            for (int b = 0; b < nb; ++b)
              for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 9; ++s)
                  for (int h = 0; h < 2; ++h) {
                    bool v;
                    const int64_t r = rowof(b, lane, h, v);
                    const int lb = b * BT + (lane / SP_PW) * SP_LS + 2 * (lane % SP_PW);
                    tab[sp_tbase(s, B) + (sp_dj(s) + sp_adj(s)) * SP_LS + sp_dk(s) + 2 + lb + h] = v ? entry(r, s) : 0.0;
                  }
          double keep[3][64][2];
          for (int b = 0; b < nb; ++b) {
            const bool lastb = b + 1 >= nb;
            // phase B: +z / +y slots of this band's rows; with band 0 the edge block of the step
            for (int lane = 0; lane < 64; ++lane)
              for (int s = 9; s < 13; ++s)
                for (int h = 0; h < 2; ++h) {
                  bool v;
                  const int64_t r = rowof(b, lane, h, v);
                  const int lb = b * BT + (lane / SP_PW) * SP_LS + 2 * (lane % SP_PW);
                  tab[sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb + h] = v ? entry(r, 26 - s) : 0.0;
                }
            if (b == 0)
              for (int e = 0; e < NE; ++e) {
                int s, line, col, cell;
                sp_edge(e, s, line, col, cell, B);
                const bool v = j0 + line < m1 && k0 + col < m2;
                tab[cell] = v ? entry((int64_t)p * PL + (int64_t)(j0 + line) * m2 + k0 + col, s) : 0.0;
              }
            // phase C: every lower slot of every valid row read through the tables
            for (int lane = 0; lane < 64; ++lane)
              for (int s = 0; s < 13; ++s)
                for (int h = 0; h < 2; ++h) {
                  bool v;
                  const int64_t r = rowof(b, lane, h, v);
                  if (!v) continue;
                  const int lb = b * BT + (lane / SP_PW) * SP_LS + 2 * (lane % SP_PW);
                  const double got = tab[sp_tbase(s, B) + (sp_dj(s) + sp_adj(s)) * SP_LS + sp_dk(s) + 2 + lb + h];
                  const double want = entry(r, s);
                  if (!(got == want)) {
                    if (bad < 10) printf("bands %d lattice %dx%dx%d patch %d plane %d band %d lane %d row %d slot %d: table %.6f, entry %.6f\n", B, m0, m1, m2, patch, p, b, lane, h, s, got, want);
                    ++bad;
                  }
                  // the edge entry the row owns is the one the copy's placement gives it
                  if (s < 13) {
                    const int e = sp_edge_of(s, SP_L * b + lane / SP_PW, 2 * (lane % SP_PW) + h, B);
                    const int gl = SP_L * b + lane / SP_PW + sp_dj(s), gc = 2 * (lane % SP_PW) + h + sp_dk(s);
                    const bool inside = gl >= 0 && gl < L && gc >= 0 && gc < SP_W;
                    if ((e >= 0) == inside) { if (bad < 10) printf("bands %d: slot %d line %d: edge ownership\n", B, s, gl); ++bad; }
                  }
                }
            // phase D: next-plane slots into the previous-plane tables; slots 24..26 of a band that is not the last wait in keep
            for (int lane = 0; lane < 64; ++lane)
              for (int s = 0; s < 9; ++s)
                for (int h = 0; h < 2; ++h) {
                  bool v;
                  const int64_t r = rowof(b, lane, h, v);
                  const int lb = b * BT + (lane / SP_PW) * SP_LS + 2 * (lane % SP_PW);
                  const double val = v ? entry(r, 26 - s) : 0.0;
                  if (s < 3 && !lastb) { keep[s][lane][h] = val; continue; }
                  tab[sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb + h] = val;
                  if (s < 3 && b > 0) tab[sp_tbase(s, B) + sp_adj(s) * SP_LS + 2 + lb - BT + h] = keep[s][lane][h];
                }
          }
          have_hist = true;
        }
      }
    }
  }
  return bad;
}

int main() {
  int bad = 0;
  for (int B = 1; B <= SP_BMAX; ++B) bad += check_form(B);
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
