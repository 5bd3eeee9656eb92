// CPU walk through the host decisions of the matrix-free mesh operator (csrc/mesh_operator_decide.h): the term compilation (equal monomials
// merged, groups ordered by dual field then word, normal parts as monomials of their own, refusals and caps), the LDS block of a wave and the
// waves of a workgroup for the element families of the examples, the scratch and workspace layout, and the gate of the solve options.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_mesh_operator.cpp -o tools/bin/host_check_mesh_operator && tools/bin/host_check_mesh_operator
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

int main() {
  OpProgram P;
  const char* why = "";
  {  // thermal: -k (grad, grad) - alpha (T, T), the mass term given twice (merged), in scrambled order
    std::vector<mfem_operator_term> t = {term(2, 2, 0, -0.6), term(0, 0, 0, -0.7), term(3, 3, 0, -0.6), term(1, 1, 0, -0.6), term(0, 0, 0, -4.0)};
    eq(mop_compile(3, false, 1, (int)t.size(), t.data(), &P, &why), MFEM_OK, "thermal compiles");
    eq(P.nfo, 1, "thermal: one dual field");
    eq(P.nsrc, 1, "thermal: one source");
    eq(P.ngroups, 4, "thermal: four dual words");
    eq(P.nent, 4, "thermal: the two mass terms merged");
    for (int g = 0; g < 4; ++g) eq(P.grp_sd[g], g, "thermal: groups ordered by word");
    feq(P.ent_coef[0], -4.7, "thermal: merged coefficient");
    eq(P.grp_end[0], 1, "thermal: the value group holds one entry");
    eq(P.fo_g0[0], 0, "thermal: first group");
    eq(P.fo_g0[1], 4, "thermal: group count of the field");
  }
  {  // two fields given field 1 first: groups sorted by dual field, sources in order of first use, an off-diagonal block
    std::vector<mfem_operator_term> t = {term(1, 2, 1 * 2 + 0, 3.0), term(1, 1, 1 * 2 + 1, 2.0), term(2, 1, 0 * 2 + 1, 5.0), term(1, 1, 0 * 2 + 0, 1.0)};
    eq(mop_compile(2, false, 2, (int)t.size(), t.data(), &P, &why), MFEM_OK, "two fields compile");
    eq(P.nfo, 2, "two dual fields");
    eq(P.fo_pos[0], 0, "dual field 0 first");
    eq(P.fo_pos[1], 1, "dual field 1 second");
    eq(P.ngroups, 3, "groups (0, 1), (0, 2), (1, 1)");
    eq(P.grp_sd[0], 1, "group 0 word");
    eq(P.grp_sd[1], 2, "group 1 word");
    eq(P.grp_sd[2], 1, "group 2 word");
    eq(P.fo_g0[1], 2, "field 1 starts at group 2");
    eq(P.nsrc, 2, "two sources");
    eq(P.src_pos[0], 0, "source of the first sorted term");
    eq(P.grp_end[2], 4, "field 1's word holds two entries (base fields 0 and 1 do not merge)");
  }
  {  // facets: the normal parts are monomials of their own; on elements they are refused
    std::vector<mfem_operator_term> t = {term(0, 0, 0, -1000.0), term(0, 1, 0, 0.0, 0.6), term(0, 2, 0, 0.0, 0.0, 0.6), term(0, 1, 0, 0.5, 0.25)};
    eq(mop_compile(2, true, 1, (int)t.size(), t.data(), &P, &why), MFEM_OK, "Nitsche facet compiles");
    eq(P.ngroups, 1, "one dual word");
    eq(P.nent, 4, "(T), (T_x n_0), (T_y n_1), (T_x)");
    feq(P.ent_coef[1], 0.85, "normal monomial merged");
    eq(P.ent_nrm[1], 0, "its normal component");
    eq(mop_compile(2, false, 1, (int)t.size(), t.data(), &P, &why), MFEM_ERR_INVALID, "normal_coef on elements is invalid");
    std::vector<mfem_operator_term> z = {term(0, 0, 0, 1.0, 0.0, 0.0, 2.0)};
    eq(mop_compile(2, true, 1, 1, z.data(), &P, &why), MFEM_ERR_INVALID, "n_2 in 2-D is invalid");
  }
  {  // refusals and caps
    std::vector<mfem_operator_term> t = {term(0, 0, 4, 1.0)};
    eq(mop_compile(3, false, 2, 1, t.data(), &P, &why), MFEM_ERR_INVALID, "block out of range");
    t[0] = term(4, 0, 0, 1.0);
    eq(mop_compile(3, false, 2, 1, t.data(), &P, &why), MFEM_ERR_INVALID, "dual word out of range");
    t[0] = term(0, 3, 0, 1.0);
    eq(mop_compile(2, false, 2, 1, t.data(), &P, &why), MFEM_ERR_INVALID, "base word out of range in 2-D");
    eq(mop_compile(3, false, 1, 1, nullptr, &P, &why), MFEM_ERR_INVALID, "terms missing");
    eq(mop_compile(3, false, 1, 0, nullptr, &P, &why), MFEM_OK, "no terms: an empty part");
    eq(P.nfo, 0, "an empty part has no output");
    std::vector<mfem_operator_term> many(49, term(0, 0, 0, 1.0));
    eq(mop_compile(3, false, 1, 49, many.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "49 terms");
    eq(mop_compile(3, false, 1, 48, many.data(), &P, &why), MFEM_OK, "48 terms");
    eq(P.nent, 1, "48 equal terms merge into one monomial");
    feq(P.ent_coef[0], 48.0, "their sum");
    std::vector<mfem_operator_term> nine;
    for (int f = 0; f < 9; ++f) nine.push_back(term(0, 0, f * 9 + f, 1.0));
    eq(mop_compile(3, false, 9, 9, nine.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "9 dual fields");
    eq(mop_compile(3, false, 9, 8, nine.data(), &P, &why), MFEM_OK, "8 dual fields");
    std::vector<mfem_operator_term> nine_base;
    for (int f = 0; f < 9; ++f) nine_base.push_back(term(0, 0, f, 1.0));
    eq(mop_compile(3, false, 9, 9, nine_base.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "9 base fields");
    std::vector<mfem_operator_term> wide;  // 48 terms x 4 monomials each, all distinct: beyond 128 entries
    for (int i = 0; i < 48; ++i) wide.push_back(term(i % 4, (i / 4) % 4, (i / 16) * 8 + (i / 16), 1.0, 1.0, 1.0, 1.0));
    eq(mop_compile(3, true, 8, 48, wide.data(), &P, &why), MFEM_ERR_UNSUPPORTED, "more than 128 monomials");
    ok(why[0] != 0, "a refusal names its reason");
  }
  {  // LDS blocks: hex-20 (27 points, 20 nodes) elasticity = 3 sources, 3 outputs, 12 dual words; the residual's formula with the fields as sources
    const size_t d = mop_wave_doubles(3, 27, 20, false, 3, 3, 12);
    eq((long long)d, 27 * 10 + 60 + 60 + 6 * 27 * 4 + 12 * 27, "hex-20 elasticity doubles");
    eq(mop_waves(d), 4, "hex-20 elasticity: four waves per workgroup");
    eq(mop_waves(mop_wave_doubles(3, 125, 27, false, 3, 3, 12)), 1, "hex-27 with 125 points, elasticity: one wave");
    eq(mop_waves(mop_wave_doubles(3, 343, 64, false, 8, 8, 32)), 0, "a block beyond 64 KB is refused");
    eq((long long)mop_geo_doubles(2, 9, 8, true), 9 * 5 + 16 + 18, "quad-8 facet geometry");
    eq(mop_waves(MOP_LDS_CAP / 8), 1, "exactly the cap: one wave");
    eq(mop_waves(MOP_LDS_CAP / 8 + 1), 0, "one double more: none");
  }
  {  // scratch: parts in the order they were added; the solve's workspace: vectors, scratch right behind, gmres!'s block aligned
    const int64_t items[3] = {36, 10, 0};
    const int nfo[3] = {3, 1, 2};
    size_t off[3];
    eq((long long)mop_scratch_layout(3, items, nfo, 20, off), 36 * 20 * 3 + 10 * 20, "scratch doubles");
    eq((long long)off[0], 0, "elements first");
    eq((long long)off[1], 36 * 20 * 3, "first facet part behind them");
    eq((long long)off[2], 36 * 20 * 3 + 200, "an empty part takes nothing");
    const OpWorkspace W = mop_workspace(96, 3, 2360, 0);
    eq((long long)W.scratch_offset, 96 * 8 * 7, "scratch behind x, b, d, 1 / d and three work vectors");
    eq((long long)W.total, 96 * 8 * 7 + 2360 * 8, "cg!: vectors + scratch, nothing else");
    const OpWorkspace G = mop_workspace(96, 22, 2361, 1000);
    eq((long long)(G.gm_offset % 256), 0, "gmres!'s block is aligned");
    ok(G.gm_offset >= G.scratch_offset + 2361 * 8, "... and behind the scratch");
    eq((long long)G.total, (long long)G.gm_offset + 1000, "... and counted");
  }
  {  // the gate of the solve options
    for (int m = MFEM_SOLVER_CG; m <= MFEM_SOLVER_LSQR; ++m)
      for (int pr = 0; pr <= 2; ++pr)
        for (int pl = 0; pl <= 2; ++pl)
          for (int sip = 0; sip <= 1; ++sip)
            for (int comm = 0; comm <= 1; ++comm) {
              const int got = mop_solve_gate(m, pr, pl, sip, comm != 0, &why);
              const bool unsup = m == MFEM_SOLVER_LSQR || pr == MFEM_PRECOND_JACOBI_RIGHT_COLNORM || pl != MFEM_LEFT_NONE;
              const int want = unsup ? MFEM_ERR_UNSUPPORTED : (sip || comm) ? MFEM_ERR_INVALID : MFEM_OK;
              eq(got, want, "solve gate");
              ok((got == MFEM_OK) == (why[0] == 0), "a refusal names its reason, an acceptance none");
            }
  }
  if (bad) {
    printf("%d check(s) failed\n", bad);
    return 1;
  }
  printf("OK\n");
  return 0;
}
