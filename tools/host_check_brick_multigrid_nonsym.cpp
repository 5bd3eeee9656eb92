// CPU walk through the host decisions that the nonsymmetric thermal hierarchy (mfem_brick_multigrid_create_nonsymmetric) and gmres! with the V-cycle
// (csrc/krylov_gmres_mg.hip) add to csrc/brick_multigrid_decide.h:
//   1. the gate mg_solve_refusal_nonsym: every row with a method other than MFEM_SOLVER_GMRES, and every GMRES row that is not a hex-8 thermal brick
//      operator, answers as mg_solve_refusal_hex27 does, in the same words; MFEM_SOLVER_GMRES on a hex-8 thermal operator is admitted exactly when a
//      nonsymmetric hierarchy is attached, with no left preconditioner and no communicator, the Nitsche term on or off; the new refusals name the
//      entry point.  One line per row ("GATE ...") for the Python restatement, tests/test_brick_multigrid_nonsym_host.py;
//   2. which setups refuse a Nitsche term;
//   3. the products of a pass: a host model of the pass's loop (restart lengths s = 1 .. 32, a stop at any step, several restarts) summed restart by
//      restart against the closed form mg_gmres_pass_products, cycles = iterations + restarts, and the lines of the issue's example.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_brick_multigrid_nonsym.cpp -o tools/bin/host_check_brick_multigrid_nonsym
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "brick_multigrid_decide.h"

static long long cases = 0, bad = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (++bad <= 20) { printf(__VA_ARGS__); printf(": %s\n", #cond); } } } while (0)

static bool same(const char* a, const char* b) { return a == b || (a && b && !strcmp(a, b)); }

// the loop of mfem_gmres_mg_pass on the host: `stop_at` (1-based, counted over the whole pass; 0: never) is the step whose estimate meets the
// tolerance, after which the true residual converges; the cap ends the pass as well.  Counts products and cycles as the pass's launches do.
struct Model {
  long long it = 0, restarts = 0, cycles = 0, products = 0, by_restarts = 0;  // (by_restarts: the sum of mg_gmres_restart_products)
};
static Model run_model(int x0, int s, int maxiter, int stop_at, int c) {
  Model M;
  M.products = x0;
  bool done = maxiter <= 0 || stop_at < 0;  // (stop_at < 0: the start has converged)
  while (!done) {
    int width = 0;
    bool stopped = false;
    for (int kk = 1; kk <= s; ++kk) {
      ++M.cycles; M.products += c;  // z = Cycle(Q_k)
      ++M.products;                 // w = A z
      ++M.it;
      width = kk;
      if (M.it == stop_at || M.it >= maxiter) { stopped = true; break; }
    }
    ++M.cycles; M.products += c;  // z = Cycle(Q y)
    ++M.products;                 // r = b - A x
    ++M.restarts;
    M.by_restarts += mg_gmres_restart_products(width, c);
    done = stopped;  // (a restart of s steps without a stop: the true residual has not converged in this model)
  }
  return M;
}

int main() {
  const int CG = MFEM_SOLVER_CG, GM = MFEM_SOLVER_GMRES, NONE = MFEM_LEFT_NONE;
  // 1. the gate
  for (int brick = 0; brick <= 1; ++brick)
    for (int kind = 0; kind <= 3; ++kind)  // 0: none of the three, 1: hex-8 thermal, 2: hex-8 elasticity, 3: hex-27 thermal
      for (int attached = 0; attached <= 1; ++attached)
        for (int nonsym = 0; nonsym <= 1; ++nonsym)
          for (int method : {MFEM_SOLVER_CG, MFEM_SOLVER_BICGSTABL_GS,MFEM_SOLVER_IDRS, MFEM_SOLVER_GMRES, MFEM_SOLVER_TFQMR})
            for (int left : {MFEM_LEFT_NONE, MFEM_LEFT_JACOBI_DIAG})
              for (int comm = 0; comm <= 1; ++comm)
                for (int nitsche = 0; nitsche <= 1; ++nitsche) {
                  const bool thermal = kind == 1, elast = kind == 2, h27 = kind == 3;
                  if ((!brick && kind) || (nitsche && !(thermal || h27)) || (nonsym && !(attached && thermal))) continue;  // (rows no operator produces)
                  const char* why = mg_solve_refusal_nonsym(brick, thermal, elast, h27, attached, nonsym, method, left, comm, nitsche);
                  const char* old = mg_solve_refusal_hex27(brick, thermal, elast, h27, attached, method, left, comm, nitsche);
                  const bool new_row = method == GM && brick && thermal;
                  if (!new_row) {
                    CHECK(same(why, old), "row %d %d %d %d %d %d %d %d answers as before", brick, kind, attached, nonsym, method, left, comm, nitsche);
                  } else {
                    const bool admitted = attached && nonsym && left == NONE && !comm;
                    CHECK((why == nullptr) == admitted, "gmres row %d %d %d %d %d %d", attached, nonsym, method, left, comm, nitsche);
                    CHECK(old && strstr(old, "MFEM_SOLVER_CG"), "before: gmres! was refused for the method");
                    if (why && !(attached && nonsym)) CHECK(strstr(why, "mfem_brick_multigrid_create_nonsymmetric"), "the refusal names the entry point");
                    if (why && attached && nonsym && left != NONE) CHECK(strstr(why, "left"), "a left preconditioner");
                    if (why && attached && nonsym && left == NONE && comm) CHECK(strstr(why, "communicator"), "a communicator");
                  }
                  printf("GATE %d %d %d %d %d %d %d %d %d\n", brick, kind, attached, nonsym, method, left, comm, nitsche, why == nullptr ? 1 : 0);
                }
  {
    const char* w = mg_solve_refusal_nonsym(true, true, false, false, true, true, CG, NONE, false, true);
    CHECK(w && strstr(w, "Nitsche"), "cg! with an active Nitsche term is refused whatever is attached");
    CHECK(!mg_solve_refusal_nonsym(true, true, false, false, true, true, CG, NONE, false, false), "cg! on a nonsymmetric hierarchy, Nitsche off: admitted");
    CHECK(!mg_solve_refusal_nonsym(true, true, false, false, true, true, GM, NONE, false, true), "gmres!, Nitsche on: admitted");
    CHECK(!mg_solve_refusal_nonsym(true, true, false, false, true, true, GM, NONE, false, false), "gmres!, Nitsche off: admitted");
    w = mg_solve_refusal_nonsym(true, true, false, false, false, false, GM, NONE, false, true);
    CHECK(w && strstr(w, "no default hierarchy"), "without a hierarchy: no default one is made");
    w = mg_solve_refusal_nonsym(true, true, false, false, true, false, GM, NONE, false, false);
    CHECK(w && strstr(w, "destroy it") && strstr(w, "mfem_brick_multigrid_create_nonsymmetric"), "a plain hierarchy: destroy it first");
    w = mg_solve_refusal_nonsym(true, true, false, false, true, true, MFEM_SOLVER_IDRS, NONE, false, true);
    CHECK(w && strstr(w, "MFEM_SOLVER_CG"), "idrs! as before");
    w = mg_solve_refusal_nonsym(true, false, true, false, true, false, GM, NONE, false, false);
    CHECK(w && strstr(w, "MFEM_SOLVER_CG"), "gmres! on an elasticity operator as before");
    w = mg_solve_refusal_nonsym(false, false, false, false, false, false, GM, NONE, false, false);
    CHECK(w && strstr(w, "brick operator"), "gmres! on a mesh operator as before");
  }
  // 2. the setups
  CHECK(mg_setup_refuses_nitsche(false, true) && !mg_setup_refuses_nitsche(true, true) && !mg_setup_refuses_nitsche(false, false) &&
        !mg_setup_refuses_nitsche(true, false), "only a plain hierarchy's setup refuses an active Nitsche term");
  // 3. the products
  CHECK(MG_GMRES_DEFAULT_S == 20 && MG_GMRES_MAX_S == 32, "the restart lengths");
  for (int nlev : {1, 3})
    for (int nu : {2, 3})
      for (int nu_c : {8, 32}) {
        const int c = mg_cycle_products(0, nlev, nu, nu_c);
        CHECK(c == (nlev == 1 ? nu_c - 1 : 2 * nu), "a cycle's level-0 products");
        for (int x0 = 0; x0 <= 1; ++x0)
          for (int s = 1; s <= MG_GMRES_MAX_S; ++s)
            for (int maxiter : {0, 1, 7, 40})
              for (int stop_at : {-1, 0, 1, 3, 4, 5, 9, 21}) {
                const Model M = run_model(x0, s, maxiter, stop_at, c);
                CHECK(M.products == mg_gmres_pass_products(x0, (int)M.it, (int)M.restarts, nlev, nu, nu_c), "pass products s %d maxiter %d stop %d", s, maxiter, stop_at);
                CHECK(M.products == x0 + M.by_restarts, "the pass is the sum of its restarts: k (1 + c) + c + 1 each");
                CHECK(M.cycles == mg_gmres_cycles((int)M.it, (int)M.restarts), "cycles = iterations + restarts");
                if (stop_at == 0 && maxiter > 0) {
                  CHECK(M.it == maxiter && M.restarts == mg_gmres_full_restarts(maxiter, s), "a run to the cap: %d steps in ceil(it / s) restarts", maxiter);
                }
                if (stop_at < 0 || maxiter == 0) CHECK(M.it == 0 && M.cycles == 0 && M.products == x0, "a converged start: no cycle");
              }
      }
  CHECK(mg_gmres_restart_products(8, 4) == 8 * 5 + 4 + 1, "one restart of width 8 at nu = 2: 45 products");
  CHECK(mg_gmres_pass_products(0, 8, 1, 4, 2, 32) == 45 && mg_gmres_pass_products(1, 8, 1, 4, 2, 32) == 46, "a converged run of 8 steps");
  CHECK(mg_gmres_pass_products(0, 7, 2, 4, 2, 32) == 7 * 5 + 2 * 5, "fixed: 7 steps at s = 4, two restarts");
  CHECK(mg_gmres_pass_products(0, 9, 3, 4, 3, 8) == 9 * 7 + 3 * 7, "nu = 3");
  CHECK(mg_gmres_pass_products(0, 6, 1, 1, 2, 8) == 6 * 8 + 8, "one level: c = nu_c - 1");
  CHECK(mg_pass_products(0, 5, 3, 2, 32) == 5 + 4 * 5 + 1, "cg!'s formula is unchanged");
  printf("%lld checks, %lld failed\n", cases, bad);
  if (bad) return 1;
  printf("OK\n");
  return 0;
}
