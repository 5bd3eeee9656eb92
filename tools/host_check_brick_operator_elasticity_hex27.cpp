// CPU walk through the host decisions of the matrix-free hex-27 ELASTICITY brick operator (csrc/brick_operator_elasticity_hex27_decide.h; the work
// items are csrc/brick_operator_hex27_decide.h's, walked here again because the new kernel depends on them):
//   1. ownership: the work items put every control point into exactly one item, point by point, on every lattice from 1^3 to 5^3 elements and on
//      shapes around the tile and segment edges;
//   2. adjacency: every element adjacent to a point an item owns is integrated by the item, its column lies inside the B27_EH^2 element-vector block,
//      and a tile owns at most B27_NP x B27_NP columns -- one thread each of the smallest workgroup (E27_WAVES_MIN waves);
//   3. the LDS block: per rule, the waves e27_waves(ng) a workgroup runs, its bytes within the 160 KB of a gfx950 CU, the shared parts and the per-wave
//      overlays in order and without overlap, the decode words' fields wide enough; the rule predicate e27_rule_served;
//   4. the redundancy R = elements integrated / elements of the brick, printed for the cubes: 1.277 at 128^3, as the thermal operator's (same items);
//   5. the diagonal formula of k_brick27e_diagonal, -sum_q w det [mu |g|^2 + (lambda + mu) g_f^2], against element matrices built from unit vectors
//      through the product's own stress form, on distorted elements;
//   6. the refusals and their messages.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_operator_elasticity_hex27.cpp -o host_check_brick_operator_elasticity_hex27
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "brick_operator_elasticity_hex27_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

// ---- 1. + 2. + 4. ------------------------------------------------------------------------------------------------------------------------------------
static double walk(int ne0, int ne1, int ne2, bool mark, bool print) {
  const int m0 = 2 * ne0 + 1, m1 = 2 * ne1 + 1, m2 = 2 * ne2 + 1;
  const B27Volume V = b27_volume(ne0, ne1, ne2);
  std::vector<unsigned char> seen(mark ? (size_t)m0 * m1 * m2 : 0, 0);
  long long integrated = 0, volume = 0;
  for (int64_t w = 0; w < V.items; ++w) {
    const B27Item b = b27_item(V, w, ne0, ne1, ne2);
    const bool in = b.i0 >= 0 && b.i0 < b.i1 && b.i1 <= m0 && b.j0 >= 0 && b.j0 < b.j1 && b.j1 <= m1 && b.k0 >= 0 && b.k0 < b.k1 && b.k1 <= m2;
    CHECK(in, "%d x %d x %d elements, item %lld: an empty box or one outside the lattice", ne0, ne1, ne2, (long long)w);
    if (!in) continue;
    volume += (long long)(b.i1 - b.i0) * (b.j1 - b.j0) * (b.k1 - b.k0);
    integrated += (long long)(b.I1 - b.I0) * (b.J1 - b.J0) * (b.K1 - b.K0);
    CHECK(b.j1 - b.j0 <= B27_NP && b.k1 - b.k0 <= B27_NP && (b.j1 - b.j0) * (b.k1 - b.k0) <= 64 * E27_WAVES_MIN, "item %lld: more columns than threads", (long long)w);
    CHECK(b.J0 - b.Jb >= 0 && b.J1 - 1 - b.Jb < B27_EH && b.K0 - b.Kb >= 0 && b.K1 - 1 - b.Kb < B27_EH, "item %lld: an element column outside the block", (long long)w);
    CHECK(2 * b.Iown == b.i0 && b.Iown >= b.I0 && b.Iown <= b.I0 + 1 && b.Iown < b.I1, "item %lld: first written plane", (long long)w);
    CHECK(b.last_seg == (b.i1 == m0) && (b.last_seg ? b.i1 == 2 * b.I1 + 1 : b.i1 == 2 * b.I1), "item %lld: last plane", (long long)w);
    if (!mark) continue;
    long long miss = 0;
    for (int i = b.i0; i < b.i1; ++i)
      for (int j = b.j0; j < b.j1; ++j)
        for (int k = b.k0; k < b.k1; ++k) {
          ++seen[((size_t)i * m1 + j) * m2 + k];
          int E[3][2], c[3][2];
          const int n0 = b27_face_elements(i, ne0, E[0], c[0]), n1 = b27_face_elements(j, ne1, E[1], c[1]), n2 = b27_face_elements(k, ne2, E[2], c[2]);
          for (int a = 0; a < n0; ++a) miss += !(E[0][a] >= b.I0 && E[0][a] < b.I1);
          for (int a = 0; a < n1; ++a) miss += !(E[1][a] >= b.J0 && E[1][a] < b.J1);
          for (int a = 0; a < n2; ++a) miss += !(E[2][a] >= b.K0 && E[2][a] < b.K1);
        }
    CHECK(miss == 0, "%d x %d x %d elements, item %lld: %lld adjacent elements not integrated", ne0, ne1, ne2, (long long)w, miss);
  }
  if (mark) {
    long long wrong = 0;
    for (unsigned char c : seen) wrong += c != 1;
    CHECK(wrong == 0, "%d x %d x %d elements: %lld control points not owned exactly once", ne0, ne1, ne2, wrong);
  }
  CHECK(volume == (long long)m0 * m1 * m2, "%d x %d x %d elements: the boxes hold %lld points", ne0, ne1, ne2, volume);
  CHECK(V.grid >= 1 && V.grid <= BOP_VOLUME_PARTIALS && b27_volume_grid(V, true) == V.grid && b27_volume_grid(V, false) == V.items, "%d x %d x %d: the fold", ne0, ne1, ne2);
  const double R = (double)integrated / ((double)ne0 * ne1 * ne2);
  if (print) printf("R(%d x %d x %d elements) = %.4f  (L = %d, %lld items, grid %d in %d rounds)\n", ne0, ne1, ne2, R, V.L, (long long)V.items, V.grid, V.rounds);
  return R;
}

// ---- 3. the LDS block --------------------------------------------------------------------------------------------------------------------------------
static void lds(int ng) {
  const int nq = ng * ng * ng, waves = e27_waves(ng);
  CHECK(e27_rule_served(ng) == (waves > 0) && e27_decode_fits(ng), "ng %d: the predicate", ng);
  printf("LDS(ng = %d): %d waves, %zu bytes (per wave %zu, shared %zu); 8 waves: %zu, 12 waves: %zu\n", ng, waves, waves ? e27_lds_bytes(ng, waves) : (size_t)0,
         sizeof(double) * e27_w_size(ng), sizeof(double) * e27_off_waves(ng), e27_lds_bytes(ng, 8), e27_lds_bytes(ng, 12));
  if (!waves) return;
  CHECK(waves >= E27_WAVES_MIN && waves <= E27_WAVES_MAX && e27_lds_bytes(ng, waves) + E27_LDS_STATIC <= E27_LDS_LIMIT, "ng %d: %d waves", ng, waves);
  CHECK(waves == E27_WAVES_MAX || e27_lds_bytes(ng, waves + 1) + E27_LDS_STATIC > E27_LDS_LIMIT, "ng %d: as many waves as fit", ng);
  // shared: w | tab1 | decode | Fe | waves, in order, each as large as its contents
  CHECK(e27_off_tab1(ng) >= nq && e27_off_dec(ng) - e27_off_tab1(ng) >= 8 * ng && 2 * (e27_off_fe(ng) - e27_off_dec(ng)) >= e27_ndec(ng) &&
            e27_off_waves(ng) - e27_off_fe(ng) >= B27_EH * B27_EH * E27_NV, "ng %d: the shared block", ng);
  // per wave: X | T1 below T2; J | grad_xi u over them; VA | WB over those; T2 and the flux below w det; w det inside the block
  CHECK(27 * E27_NI == e27_w_t1() && e27_w_t1() + e27_n1(ng) <= e27_w_t2(ng), "ng %d: X | T1", ng);
  CHECK(e27_n3(ng) == 18 * nq && e27_n3(ng) <= e27_w_t2(ng), "ng %d: J | grad_xi u", ng);
  CHECK(e27_na(ng) <= e27_w_wb(ng) && e27_w_wb(ng) + e27_nb(ng) <= e27_w_t2(ng), "ng %d: VA | WB", ng);
  CHECK(e27_n2(ng) <= e27_w_d(ng) - e27_w_t2(ng) && E27_NF * 3 * nq <= e27_w_d(ng) - e27_w_t2(ng), "ng %d: T2 / flux", ng);
  CHECK(e27_w_d(ng) + nq <= e27_w_size(ng) && (e27_w_size(ng) & 1) == 0, "ng %d: w det", ng);
  // decode words: 16-bit operand offsets and table rows of the interpolation stages, 12-bit offsets of the transposed ones
  CHECK(e27_w_t2(ng) + e27_n2(ng) < (1 << 16) && 4 * 2 * ng < (1 << 15), "ng %d: interpolation fields", ng);
  CHECK(E27_NF * 3 * nq <= (1 << 12) && e27_na(ng) <= (1 << 12), "ng %d: transposed fields", ng);
}

// ---- 5. the diagonal formula --------------------------------------------------------------------------------------------------------------------------
static const double GP[4][4] = {{0.0, 0, 0, 0}, {-0.57735026918962576451, 0.57735026918962576451, 0, 0}, {-0.77459666924148337704, 0.0, 0.77459666924148337704, 0},
                                {-0.86113631159405257522, -0.33998104358485626480, 0.33998104358485626480, 0.86113631159405257522}};
static const double GW[4][4] = {{2.0, 0, 0, 0}, {1.0, 1.0, 0, 0}, {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0, 0},
                                {0.34785484513745385737, 0.65214515486254614263, 0.65214515486254614263, 0.34785484513745385737}};
static void lag2(double x, double* L, double* dL) {
  L[0] = 2.0 * (x - 0.5) * (x - 1.0); L[1] = -4.0 * x * (x - 1.0); L[2] = 2.0 * x * (x - 0.5);
  dL[0] = 4.0 * x - 3.0; dL[1] = -8.0 * x + 4.0; dL[2] = 4.0 * x - 1.0;
}
struct Quad {
  double wd, g[27][3];
};
static Quad quad_point(const double X[27][3], int ng, int q) {
  const int q0 = q % ng, q1 = (q / ng) % ng, q2 = q / (ng * ng);
  double L[3][3], dL[3][3];
  lag2(GP[ng - 1][q0] / 2 + 0.5, L[0], dL[0]);
  lag2(GP[ng - 1][q1] / 2 + 0.5, L[1], dL[1]);
  lag2(GP[ng - 1][q2] / 2 + 0.5, L[2], dL[2]);
  double dn[27][3], J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int b = 0; b < 27; ++b) {
    const int b0 = b % 3, b1 = (b / 3) % 3, b2 = b / 9;
    dn[b][0] = dL[0][b0] * L[1][b1] * L[2][b2];
    dn[b][1] = L[0][b0] * dL[1][b1] * L[2][b2];
    dn[b][2] = L[0][b0] * L[1][b1] * dL[2][b2];
    for (int i = 0; i < 3; ++i)
      for (int m = 0; m < 3; ++m) J[i][m] += dn[b][m] * X[b][i];
  }
  const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
  double Iv[3][3];
  Iv[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) / det; Iv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det; Iv[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) / det;
  Iv[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) / det; Iv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det; Iv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
  Iv[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) / det; Iv[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) / det; Iv[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) / det;
  Quad Q;
  Q.wd = GW[ng - 1][q0] * GW[ng - 1][q1] * GW[ng - 1][q2] / 8 * det;
  for (int b = 0; b < 27; ++b)
    for (int s = 0; s < 3; ++s) Q.g[b][s] = dn[b][0] * Iv[0][s] + dn[b][1] * Iv[1][s] + dn[b][2] * Iv[2][s];
  return Q;
}
// fe[f][a] = -sum_q w det sigma_fj(u) d_jN_a, the way the product integrates it: grad u at the Gauss point, the stress, then the test gradients
static void element_vector(const double X[27][3], int ng, double lam, double mu, const double u[3][27], double fe[3][27]) {
  for (int f = 0; f < 3; ++f)
    for (int a = 0; a < 27; ++a) fe[f][a] = 0.0;
  for (int q = 0; q < ng * ng * ng; ++q) {
    const Quad Q = quad_point(X, ng, q);
    double du[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int b = 0; b < 27; ++b)
      for (int f = 0; f < 3; ++f)
        for (int s = 0; s < 3; ++s) du[f][s] += u[f][b] * Q.g[b][s];
    const double tr = du[0][0] + du[1][1] + du[2][2];
    for (int f = 0; f < 3; ++f)
      for (int a = 0; a < 27; ++a) {
        double acc = 0.0;
        for (int s = 0; s < 3; ++s) acc += (mu * (du[f][s] + du[s][f]) + (f == s ? lam * tr : 0.0)) * Q.g[a][s];
        fe[f][a] -= Q.wd * acc;
      }
  }
}
static void diagonal(int ng) {
  const double lam = 0.5769, mu = 0.3846;
  double X[27][3];
  for (int b = 0; b < 27; ++b) {  // a smoothly distorted element
    const double u = 0.5 * (b % 3), v = 0.5 * ((b / 3) % 3), w = 0.5 * (b / 9);
    X[b][0] = 1.3 * u + 0.06 * sin(2.1 * v + 0.4) * cos(1.7 * w);
    X[b][1] = 0.9 * v + 0.05 * sin(1.9 * w + 0.3) * cos(2.3 * u);
    X[b][2] = 1.1 * w + 0.04 * sin(2.2 * u + 0.2) * cos(1.3 * v);
  }
  double worst = 0.0, scale = 0.0, asym = 0.0;
  for (int f = 0; f < 3; ++f)
    for (int a = 0; a < 27; ++a) {
      double u[3][27] = {{0}}, fe[3][27];
      u[f][a] = 1.0;
      element_vector(X, ng, lam, mu, u, fe);
      double formula = 0.0;
      for (int q = 0; q < ng * ng * ng; ++q) {
        const Quad Q = quad_point(X, ng, q);
        const double g2 = Q.g[a][0] * Q.g[a][0] + Q.g[a][1] * Q.g[a][1] + Q.g[a][2] * Q.g[a][2];
        formula -= Q.wd * (mu * g2 + (lam + mu) * Q.g[a][f] * Q.g[a][f]);
      }
      worst = fmax(worst, fabs(formula - fe[f][a]));
      scale = fmax(scale, fabs(fe[f][a]));
      // Ke is symmetric: column (f, a) of it, read at row (0, 0), equals row (0, 0) applied to e_(f, a)
      double u0[3][27] = {{0}}, fe0[3][27];
      u0[0][0] = 1.0;
      element_vector(X, ng, lam, mu, u0, fe0);
      asym = fmax(asym, fabs(fe0[f][a] - fe[0][0]));
    }
  CHECK(scale > 0.0 && worst <= 1e-13 * scale, "ng %d: diagonal formula off by %.3e of %.3e", ng, worst, scale);
  CHECK(asym <= 1e-13 * scale, "ng %d: Ke asymmetric by %.3e", ng, asym);
}

int main() {
  static_assert(E27_TE == B27_TE && E27_NV == 81 && E27_NI == 6, "the constants the kernel is written for");
  for (int a = 1; a <= 5; ++a)
    for (int b = 1; b <= 5; ++b)
      for (int c = 1; c <= 5; ++c) walk(a, b, c, true, false);
  const int edge[][3] = {{9, 9, 9}, {8, 8, 8}, {7, 16, 17}, {33, 9, 1}, {65, 7, 9}, {1, 40, 41}, {4, 24, 25}, {5, 1, 64}, {17, 15, 23}, {1, 473, 473}};
  for (const auto& e : edge) walk(e[0], e[1], e[2], true, false);
  {  // the fold test's brick: more items than partial sums
    const B27Volume V = b27_volume(1, 473, 473);
    CHECK(V.items == 3600 && V.items > BOP_VOLUME_PARTIALS && V.rounds == 2 && V.grid == 1800, "1 x 473 x 473: %lld items, grid %d", (long long)V.items, V.grid);
  }
  const int big[][3] = {{16, 16, 16}, {32, 32, 32}, {64, 64, 64}, {128, 128, 128}, {256, 256, 256}};
  for (const auto& e : big) {
    const double R = walk(e[0], e[1], e[2], false, true);
    if (e[0] >= 128) CHECK(R <= 1.3, "R at %d^3 = %.4f", e[0], R);
    if (e[0] == 128) CHECK(fabs(R - 1.277) < 5e-4, "R at 128^3 = %.4f, stated as 1.277", R);
  }
  for (int ng = 1; ng <= 4; ++ng) lds(ng);
  CHECK(e27_waves(1) == 12 && e27_waves(2) == 12 && e27_waves(3) == 12 && e27_waves(4) == 5, "the waves per rule the documents state");
  CHECK(e27_lds_bytes(3, 12) == 155720 && e27_lds_bytes(3, 8) == 123720 && e27_lds_bytes(4, 5) == 148848, "the bytes the documents state");
  CHECK(E27_LDS_LIMIT == 160 * 1024 && 2 * e27_lds_bytes(3, E27_WAVES_MIN) > E27_LDS_LIMIT, "no arrangement of this carve-up holds two workgroups per CU on the 3-point rule");
  for (int ng = 1; ng <= 4; ++ng) diagonal(ng);
  // 6. the refusals
  CHECK(bop_e27_refusal(2, 0, 9, 9, 3) == nullptr && bop_e27_refusal(2, 0, 9, 9, 1) == nullptr && bop_e27_refusal(2, 0, 9, 9, 2) == nullptr, "a whole hex-27 brick is taken");
  CHECK((bop_e27_refusal(2, 0, 9, 9, 4) == nullptr) == e27_rule_served(4), "the 4-point rule follows the predicate");
  const char* r8 = bop_e27_refusal(1, 0, 9, 9, 3);
  CHECK(r8 && strstr(r8, "hex-8") && strstr(r8, "mfem_brick_operator_create_elasticity"), "hex-8");
  CHECK(bop_e27_refusal(2, 2, 9, 9, 3) && strstr(bop_e27_refusal(2, 2, 9, 9, 3), "slab") && bop_e27_refusal(2, 0, 8, 9, 3), "slab");
  CHECK(strcmp(bop_e27_refusal(2, 2, 9, 9, 3), bop_refusal(1, 2, 9, 9)) == 0, "the existing slab message");
  CHECK(bop_e27_refusal(2, 0, 9, 9, 5) && strstr(bop_e27_refusal(2, 0, 9, 9, 5), "outside 1 to 4 points") && bop_e27_refusal(2, 0, 9, 9, 0) &&
            strstr(bop_e27_refusal(2, 0, 9, 9, 0), "outside 1 to 4 points"), "an unknown rule is named as such, not as the 4-point rule");
  CHECK(!e27_rule_served(0) && !e27_rule_served(5) && E27_LDS_STATIC == 16 * sizeof(double), "unknown rules; the static bytes");
  CHECK(strstr(bop_e27_multigrid_refusal(), "does not exist yet"), "the multigrid refusal");
  CHECK(bop_e27_face_launch(1.0, 1u, 0u, false) && !bop_e27_face_launch(0.0, 1u, 4u, false) && bop_e27_face_launch(0.0, 0u, 4u, true) && !bop_e27_face_launch(1.0, 0u, 0u, true),
        "the face launch");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
