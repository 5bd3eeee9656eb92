// CPU walk through the decisions csrc/mesh_operator_decide.h takes for the VARIABLE terms of the matrix-free mesh operator (mop_compile_mixed):
// constant and variable term lists compiled into one program (the constant entries of a dual word first, then its variable ones in the order given,
// each with its slot), variable entries never merged, the caps, the refusals, and that a constant-only list compiles to the program it always
// compiled to (field by field against values written out by hand, and entry by entry as the prefix of a mixed program).
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_mesh_operator_var.cpp -o tools/bin/host_check_mesh_operator_var && tools/bin/host_check_mesh_operator_var
#include <cstdio>
#include <vector>
#include "mesh_operator_decide.h"

static int bad = 0;
static void eq(long long got, long long want, const char* what) {
  if (got != want) { printf("%s: %lld, expected %lld\n", what, got, want); ++bad; }
}
static void feq(double got, double want, const char* what) {
  if (got != want) { printf("%s: %.17g, expected %.17g\n", what, got, want); ++bad; }
}
static void ok(bool cond, const char* what) {
  if (!cond) { printf("FAILED: %s\n", what); ++bad; }
}

static mfem_operator_term term(int ds, int bs, int block, double c, double n0 = 0.0, double n1 = 0.0, double n2 = 0.0) {
  mfem_operator_term t;
  t.dual_sd = ds; t.base_sd = bs; t.block = block; t.reserved = 0; t.coef = c;
  t.normal_coef[0] = n0; t.normal_coef[1] = n1; t.normal_coef[2] = n2;
  return t;
}
static mfem_kval_term vterm(int ds, int bs, int block) {
  mfem_kval_term t;
  t.dual_sd = ds; t.base_sd = bs; t.block = block; t.reserved = 0;
  return t;
}

int main() {
  OpProgram P, Q;
  const char* why = "";
  {  // a constant-only list: every field of the program, by hand (two fields given field 1 first, one merge)
    std::vector<mfem_operator_term> t = {term(1, 2, 1 * 2 + 0, 3.0), term(1, 1, 1 * 2 + 1, 2.0), term(2, 1, 0 * 2 + 1, 5.0), term(1, 1, 0 * 2 + 0, 1.0),
                                         term(1, 2, 1 * 2 + 0, 0.5)};
    eq(mop_compile_mixed(2, false, 2, (int)t.size(), t.data(), 0, nullptr, &P, &why), MFEM_OK, "constant list compiles");
    eq(P.nsrc, 2, "nsrc"); eq(P.ngroups, 3, "ngroups"); eq(P.nfo, 2, "nfo"); eq(P.nent, 4, "nent"); eq(P.nvar, 0, "no variable entries");
    const int src_pos[2] = {0, 1}, grp_sd[3] = {1, 2, 1}, grp_end[3] = {1, 2, 4}, fo_g0[3] = {0, 2, 3};
    const int ent_src[4] = {0, 1, 0, 1}, ent_word[4] = {1, 1, 2, 1};
    const double ent_coef[4] = {1.0, 5.0, 3.5, 2.0};
    for (int i = 0; i < 2; ++i) { eq(P.src_pos[i], src_pos[i], "src_pos"); eq(P.fo_pos[i], i, "fo_pos"); }
    for (int g = 0; g < 3; ++g) {
      eq(P.grp_sd[g], grp_sd[g], "grp_sd");
      eq(P.grp_end[g], grp_end[g], "grp_end");
      eq(P.grp_var[g], grp_end[g], "a group without variable terms: grp_var == grp_end");
      eq(P.fo_g0[g], fo_g0[g], "fo_g0");
    }
    for (int e = 0; e < 4; ++e) {
      eq(P.ent_src[e], ent_src[e], "ent_src"); eq(P.ent_word[e], ent_word[e], "ent_word"); eq(P.ent_nrm[e], -1, "ent_nrm");
      feq(P.ent_coef[e], ent_coef[e], "ent_coef");
    }
    eq(mop_compile(2, false, 2, (int)t.size(), t.data(), &Q, &why), MFEM_OK, "mop_compile");
    ok(memcmp(&P, &Q, sizeof(P)) == 0, "mop_compile is the mixed compiler without variable terms");
  }
  {  // mixed: thermal constants on a word, variable terms on the same and on another word; unsorted; two equal variable terms stay two
    std::vector<mfem_operator_term> c = {term(1, 1, 0, -0.6), term(0, 0, 0, -0.7), term(2, 2, 0, -0.6), term(0, 0, 0, -4.0)};
    std::vector<mfem_kval_term> v = {vterm(2, 1, 0), vterm(0, 0, 0), vterm(3, 3, 0), vterm(0, 0, 0), vterm(2, 2, 0)};
    eq(mop_compile_mixed(3, false, 1, (int)c.size(), c.data(), (int)v.size(), v.data(), &P, &why), MFEM_OK, "mixed list compiles");
    eq(P.ngroups, 4, "words 0, 1, 2 and the variable-only word 3");
    eq(P.nent, 3 + 5, "three constant monomials (one merge), five variable entries: none merged");
    eq(P.nvar, 5, "nvar");
    const int grp_var[4] = {1, 4, 5, 7}, grp_end[4] = {3, 4, 7, 8};
    for (int g = 0; g < 4; ++g) {
      eq(P.grp_sd[g], g, "groups ordered by word");
      eq(P.grp_var[g], grp_var[g], "grp_var");
      eq(P.grp_end[g], grp_end[g], "grp_end");
    }
    feq(P.ent_coef[0], -4.7, "the constant entries are merged as before");
    eq(P.ent_nrm[1], 1, "word 0: slot 1 first ..."); eq(P.ent_nrm[2], 3, "... then slot 3: the order given, the equal term not merged");
    eq(P.ent_nrm[5], 0, "word 2: slot 0"); eq(P.ent_word[5], 1, "its base word");
    eq(P.ent_nrm[6], 4, "word 2: slot 4"); eq(P.ent_word[6], 2, "its base word");
    eq(P.ent_nrm[7], 2, "word 3: slot 2");
    eq(P.fo_g0[1], 4, "one dual field, four groups");
    // the constant entries of every dual word are the entries of the constant-only program, in its order
    eq(mop_compile(3, false, 1, (int)c.size(), c.data(), &Q, &why), MFEM_OK, "constant part alone");
    for (int g = 0; g < Q.ngroups; ++g) {
      const int q0 = g ? Q.grp_end[g - 1] : 0, p0 = g ? P.grp_end[g - 1] : 0;
      eq(P.grp_var[g] - p0, Q.grp_end[g] - q0, "constant entries of the word");
      for (int k = 0; k < Q.grp_end[g] - q0; ++k) {
        eq(P.ent_src[p0 + k], Q.ent_src[q0 + k], "constant prefix: source"); eq(P.ent_word[p0 + k], Q.ent_word[q0 + k], "constant prefix: word");
        eq(P.ent_nrm[p0 + k], Q.ent_nrm[q0 + k], "constant prefix: normal"); feq(P.ent_coef[p0 + k], Q.ent_coef[q0 + k], "constant prefix: coefficient");
      }
    }
  }
  {  // variable terms alone, on a field the constant terms do not touch; sources in order of first use; off-diagonal blocks
    std::vector<mfem_operator_term> c = {term(0, 0, 0, 1.0)};
    std::vector<mfem_kval_term> v = {vterm(1, 0, 2 * 3 + 1), vterm(0, 2, 2 * 3 + 0)};
    eq(mop_compile_mixed(2, true, 3, 1, c.data(), 2, v.data(), &P, &why), MFEM_OK, "facet part, variable terms on dual field 2");
    eq(P.nfo, 2, "dual fields 0 and 2"); eq(P.fo_pos[1], 2, "the second is field 2");
    eq(P.nsrc, 2, "base fields 0 and 1"); eq(P.src_pos[1], 1, "source 1 is field 1");
    eq(P.ngroups, 3, "(0, word 0), (2, word 0), (2, word 1)");
    eq(P.grp_var[1], 1, "a variable-only word: grp_var == its first entry"); eq(P.grp_end[1], 2, "one entry");
    eq(P.ent_nrm[1], 1, "slot 1 sorts before slot 0: word 0 of field 2"); eq(P.ent_src[1], 0, "on base field 0");
    eq(P.ent_nrm[2], 0, "slot 0"); eq(P.ent_src[2], 1, "on base field 1");
    eq(mop_compile_mixed(2, false, 3, 0, nullptr, 2, v.data(), &P, &why), MFEM_OK, "no constant terms at all");
    eq(P.nent, 2, "two entries"); eq(P.nvar, 2, "both variable"); eq(P.grp_var[0], 0, "the first word starts variable");
  }
  {  // the Neo-Hookean element part: 81 variable terms under 9 dual words, 3 sources
    std::vector<mfem_kval_term> v;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k)
          for (int l = 0; l < 3; ++l) v.push_back(vterm(1 + j, 1 + l, i * 3 + k));
    eq(mop_compile_mixed(3, false, 3, 0, nullptr, 81, v.data(), &P, &why), MFEM_OK, "Neo-Hookean compiles");
    eq(P.ngroups, 9, "9 dual words"); eq(P.nent, 81, "81 entries"); eq(P.nsrc, 3, "3 sources"); eq(P.nfo, 3, "3 dual fields");
    for (int g = 0; g < 9; ++g) eq(P.grp_end[g] - P.grp_var[g], 9, "9 variable entries per dual word");
    eq(mop_waves(mop_wave_doubles(3, 27, 20, false, P.nsrc, P.nfo, P.ngroups)), 4, "hex-20: the LDS block does not grow, four waves");
  }
  {  // caps and refusals
    std::vector<mfem_kval_term> many(129, vterm(0, 0, 0));
    eq(mop_compile_mixed(3, false, 1, 0, nullptr, 128, many.data(), &P, &why), MFEM_OK, "128 variable terms");
    eq(P.nent, 128, "... are 128 entries");
    eq(mop_compile_mixed(3, false, 1, 0, nullptr, 129, many.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "129 variable terms");
    ok(why[0] != 0, "a refusal names its reason");
    std::vector<mfem_operator_term> c = {term(0, 0, 0, 1.0)};
    eq(mop_compile_mixed(3, false, 1, 1, c.data(), 127, many.data(), &P, &why), MFEM_OK, "1 constant + 127 variable entries");
    eq(mop_compile_mixed(3, false, 1, 1, c.data(), 128, many.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "1 constant + 128 variable entries: 129");
    std::vector<mfem_operator_term> c2 = {term(0, 0, 0, 1.0), term(0, 0, 0, 2.0)};
    eq(mop_compile_mixed(3, false, 1, 2, c2.data(), 127, many.data(), &P, &why), MFEM_OK, "merged constants count once");
    std::vector<mfem_kval_term> nine, nine_base;
    for (int f = 0; f < 9; ++f) { nine.push_back(vterm(0, 0, f * 9 + f)); nine_base.push_back(vterm(0, 0, f)); }
    eq(mop_compile_mixed(3, false, 9, 0, nullptr, 9, nine.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "9 dual fields");
    eq(mop_compile_mixed(3, false, 9, 0, nullptr, 8, nine.data(), &P, &why), MFEM_OK, "8 dual fields");
    eq(mop_compile_mixed(3, false, 9, 0, nullptr, 9, nine_base.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "9 base fields");
    std::vector<mfem_kval_term> b = {vterm(0, 0, 4)};
    eq(mop_compile_mixed(3, false, 2, 0, nullptr, 1, b.data(), &P, &why), MFEM_ERR_INVALID, "block out of range");
    b[0] = vterm(0, 0, -1);
    eq(mop_compile_mixed(3, false, 2, 0, nullptr, 1, b.data(), &P, &why), MFEM_ERR_INVALID, "negative block");
    b[0] = vterm(4, 0, 0);
    eq(mop_compile_mixed(3, false, 2, 0, nullptr, 1, b.data(), &P, &why), MFEM_ERR_INVALID, "dual word out of range");
    b[0] = vterm(0, 3, 0);
    eq(mop_compile_mixed(2, false, 2, 0, nullptr, 1, b.data(), &P, &why), MFEM_ERR_INVALID, "base word out of range in 2-D");
    eq(mop_compile_mixed(3, false, 1, 0, nullptr, 1, nullptr, &P, &why), MFEM_ERR_INVALID, "variable terms missing");
    eq(mop_compile_mixed(3, false, 1, 0, nullptr, -1, nullptr, &P, &why), MFEM_ERR_INVALID, "negative count");
    eq(mop_compile_mixed(3, false, 1, 0, nullptr, 0, nullptr, &P, &why), MFEM_OK, "nothing at all: an empty part");
    eq(P.nfo, 0, "an empty part has no output");
  }
  if (bad) {
    printf("%d check(s) failed\n", bad);
    return 1;
  }
  printf("OK\n");
  return 0;
}
