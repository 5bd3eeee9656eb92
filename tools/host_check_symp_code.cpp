// CPU check of the coded-diagonal form of the patch-major copy's main part (csrc/spmv_symp.h; k_symp_fill<RP, true, true> writes it, k_spmv_symp<MODE, B, 1>
// reads it): for B = 1 and B = 2 the 13 slots 14..26 of every band, the edge block and the code bytes tile the main part exactly, every piece starts on a
// 16-byte boundary (steps included: the main part's size is a multiple of two doubles), the default form reproduces the stored form's constants, and the
// code <-> double round trip is exact for every code the gate admits.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_symp_code.cpp -o tools/bin/host_check_symp_code && tools/bin/host_check_symp_code
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "spmv_symp.h"

static int check_form(const int B) {
  int bad = 0;
  // ---- the default form is the stored form, unchanged
  if (sp_main(B) != 14 * SP_ROWS * B + sp_epad(B) || sp_main(B, 0) != sp_main(B) || sp_step(B) != sp_main(B) + 13 * SP_ROWS * B || sp_nslots() != 14 ||
      sp_eoff(B) != 14 * SP_ROWS * B || sp_cpad(B) != 0 || sp_coff(B) != sp_main(B)) { printf("bands %d: the stored form changed\n", B); ++bad; }
  if (B == 1 && (sp_tab(1) != 2196 || sp_ne(1) != 318 || SP_MAIN != 14 * 128 + 320 || SP_STEP != SP_MAIN + SP_LOW || sp_main(1, 1) != 13 * 128 + 320 + 16)) { printf("one band: constants\n"); ++bad; }
  if (B == 2 && (sp_tab(2) != 4068 || sp_ne(2) != 354 || sp_main(2) != 3968 || sp_main(2, 1) != 3744)) { printf("two bands: constants\n"); ++bad; }
  // ---- coded form: bytes of the main part, each written exactly once
  const int DC = 1, MB = sp_main(B, DC) * 8;
  std::vector<int> bytes((size_t)MB, 0);
  auto piece = [&](long long off_bytes, int len_bytes, const char* what) {
    if (off_bytes % 16 != 0) { printf("bands %d: %s at byte %lld is not 16-byte aligned\n", B, what, off_bytes); ++bad; }
    for (int i = 0; i < len_bytes; ++i) {
      if (off_bytes + i >= MB) { printf("bands %d: %s leaves the main part\n", B, what); ++bad; return; }
      ++bytes[(size_t)(off_bytes + i)];
    }
  };
  for (int b = 0; b < B; ++b)
    for (int sl = 14; sl < 27; ++sl)  // what the fill writes and the sweep's request() loads: slot sl of band b, SP_ROWS doubles
      piece(8LL * (b * sp_nslots(DC) * SP_ROWS + (sl - (27 - sp_nslots(DC))) * SP_ROWS), 8 * SP_ROWS, "slot");
  piece(8LL * sp_eoff(B, DC), 8 * sp_epad(B), "edge block");
  for (int b = 0; b < B; ++b) piece(8LL * sp_coff(B, DC) + b * SP_ROWS, SP_ROWS, "code bytes of a band");  // byte = row of the band (line * SP_W + column)
  for (int v : bytes) if (v != 1) { printf("bands %d: a byte of the coded main part is written %d times\n", B, v); ++bad; break; }
  if ((sp_main(B, DC) * 8) % 16 != 0 || (sp_low(B) * 8) % 16 != 0) { printf("bands %d: the next step is not 16-byte aligned\n", B); ++bad; }
  // the lane's two codes are one aligned 2-byte load: lane <-> rows 2 lane, 2 lane + 1 of the band
  for (int b = 0; b < B; ++b)
    for (int lane = 0; lane < 64; ++lane) {
      const int lj = lane / SP_PW, pk = lane % SP_PW, row = lj * SP_W + 2 * pk;
      if (row != 2 * lane || (b * SP_ROWS + row) % 2 != 0) { printf("bands %d lane %d: code pair\n", B, lane); ++bad; }
    }
  return bad;
}

static int check_codes() {
  int bad = 0;
  const double one = 1.0;
  long long ob;
  memcpy(&ob, &one, 8);
  if (ob != SP_ONE_BITS) { printf("bits(1.0)\n"); ++bad; }
  double prev = 0.0;
  for (int code = -SP_CODE_MAX; code <= SP_CODE_MAX; ++code) {
    const double v = sp_diag_value(code);
    int back = 1000;
    if (!sp_diag_code(v, back) || back != code) { printf("code %d -> %.17g -> %d\n", code, v, back); ++bad; }
    long long vb;
    memcpy(&vb, &v, 8);
    if (vb - ob != code) { printf("code %d: bits\n", code); ++bad; }
    if (code > -SP_CODE_MAX && !(v > prev && v == std::nextafter(prev, 2.0))) { printf("code %d: not the next double\n", code); ++bad; }  // (across the binade boundary at 1.0 too)
    prev = v;
  }
  if (sp_diag_value(0) != 1.0 || sp_diag_value(1) != 1.0 + std::numeric_limits<double>::epsilon() || sp_diag_value(-1) != 1.0 - std::numeric_limits<double>::epsilon() / 2) { printf("codes 0, +-1\n"); ++bad; }
  // the unit -1.0 (a negative definite matrix): the same codes count magnitudes, a value of the other sign has none
  const long long neg = sp_unit_bits(1);
  if (sp_diag_value(0, neg) != -1.0 || sp_unit_bits(0) != SP_ONE_BITS) { printf("unit -1.0\n"); ++bad; }
  for (int code = -SP_CODE_MAX; code <= SP_CODE_MAX; ++code) {
    const double v = sp_diag_value(code, neg);
    int back = 1000, other = 0;
    if (v != -sp_diag_value(code) || !sp_diag_code(v, back, neg) || back != code) { printf("unit -1.0: code %d -> %.17g -> %d\n", code, v, back); ++bad; }
    if (sp_diag_code(v, other) || sp_diag_code(-v, other, neg)) { printf("unit: %.17g has a code from the other unit\n", v); ++bad; }
  }
  // what the gate refuses
  const double refused[] = {0.0, -0.0, -1.0, 2.0, 0.5, sp_diag_value(SP_CODE_MAX + 1), sp_diag_value(-SP_CODE_MAX - 1), std::numeric_limits<double>::infinity(),
                            -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), -std::numeric_limits<double>::quiet_NaN(), 1e-310};
  for (double v : refused) {
    int c = 0;
    if (sp_diag_code(v, c)) { printf("%.17g got the code %d\n", v, c); ++bad; }
    if (v != -1.0 && sp_diag_code(v, c, neg)) { printf("%.17g got the code %d from -1.0\n", v, c); ++bad; }
  }
  return bad;
}

int main() {
  int bad = check_codes();
  for (int B = 1; B <= SP_BMAX; ++B) bad += check_form(B);
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
