// CPU walk through the host decisions of the direct row assembly (csrc/mesh_direct_decide.h): the batch cuts and task lists of the inspector on
// a synthetic hex-8 lattice (element order shuffled in blocks, so that owners differ from element order) and on a triangle fan of valence 32,
// under several budgets; the refusals; and the LDS block of a workgroup for the element families of the examples.
//   g++ -O2 -std=c++17 -I metafem.jl_amd/csrc tools/host_check_mesh_direct.cpp -o tools/bin/host_check_mesh_direct && tools/bin/host_check_mesh_direct
#include <cstdio>
#include <numeric>
#include <set>
#include "mesh_direct_decide.h"

static int bad = 0;
static void eq(long long got, long long want, const char* what) {
  if (got != want) { printf("%s: %lld, expected %lld\n", what, got, want); ++bad; }
}
static void ok(bool cond, const char* what) {
  if (!cond) { printf("FAILED: %s\n", what); ++bad; }
}

struct Mesh {
  int itp;
  int64_t nel, ncp;
  std::vector<int32_t> cp;  // [nel][itp]
  std::vector<int64_t> adj_ptr;
  std::vector<int32_t> adj, L;
};

// adjacency (element * itp + local id per control point, ascending) and the coupled control points per row
static void finish(Mesh& m) {
  m.adj_ptr.assign((size_t)m.ncp + 1, 0);
  for (int32_t c : m.cp) ++m.adj_ptr[(size_t)c + 1];
  for (int64_t i = 0; i < m.ncp; ++i) m.adj_ptr[(size_t)i + 1] += m.adj_ptr[(size_t)i];
  m.adj.resize(m.cp.size());
  std::vector<int64_t> at(m.adj_ptr.begin(), m.adj_ptr.end() - 1);
  for (size_t ea = 0; ea < m.cp.size(); ++ea) m.adj[(size_t)at[(size_t)m.cp[ea]]++] = (int32_t)ea;
  m.L.resize((size_t)m.ncp);
  for (int64_t i = 0; i < m.ncp; ++i) {
    std::set<int32_t> nb;
    for (int64_t j = m.adj_ptr[(size_t)i]; j < m.adj_ptr[(size_t)i + 1]; ++j) {
      const int64_t el = m.adj[(size_t)j] / m.itp;
      for (int b = 0; b < m.itp; ++b) nb.insert(m.cp[(size_t)(el * m.itp + b)]);
    }
    m.L[(size_t)i] = (int32_t)nb.size();
  }
}

static Mesh lattice(int n) {  // n^3 hex-8 elements, visited in blocks of 4 taken in a scrambled order
  Mesh m;
  m.itp = 8;
  m.nel = (int64_t)n * n * n;
  m.ncp = (int64_t)(n + 1) * (n + 1) * (n + 1);
  const int64_t nblk = (m.nel + 3) / 4;
  std::vector<int64_t> order;
  for (int64_t k = 0; k < nblk; ++k) {
    const int64_t blk = (k * 7 + 3) % nblk;  // (7 and nblk coprime for the sizes below)
    for (int64_t e = blk * 4; e < blk * 4 + 4 && e < m.nel; ++e) order.push_back(e);
  }
  for (int64_t e : order) {
    const int x = (int)(e % n), y = (int)(e / n % n), z = (int)(e / ((int64_t)n * n));
    for (int c = 0; c < 8; ++c)
      m.cp.push_back((int32_t)((x + (c & 1)) + (n + 1) * ((y + (c >> 1 & 1)) + (n + 1) * (z + (c >> 2)))));
  }
  finish(m);
  return m;
}

static Mesh fan(int valence) {  // triangles around control point 0
  Mesh m;
  m.itp = 3;
  m.nel = valence;
  m.ncp = valence + 1;
  for (int e = 0; e < valence; ++e) {
    m.cp.push_back(1 + e);
    m.cp.push_back(0);
    m.cp.push_back(1 + (e + 1) % valence);
  }
  finish(m);
  return m;
}

static void walk(const Mesh& m, int nf, int64_t budget, const char* name) {
  MdPlan P;
  const int rc = md_plan_build(m.itp, m.nel, m.ncp, nf, m.adj_ptr.data(), m.adj.data(), m.L.data(), budget, &P);
  eq(rc, MD_OK, name);
  if (rc != MD_OK) return;
  const size_t nbatch = P.batch_node.size() - 1;
  eq((long long)P.task.size(), (long long)m.nel * m.itp, "tasks = nel * itp");
  eq(P.batch_task.back(), (long long)m.nel * m.itp, "the batches span the tasks");
  eq(P.batch_node.back(), (long long)m.ncp, "the batches span the control points");
  std::vector<int> seen(m.adj.size(), 0), node_seen((size_t)m.ncp, 0);
  int64_t runs = 0, max_batch = 0;
  for (size_t b = 0; b < nbatch; ++b) {
    int64_t doubles = 0;
    std::vector<int64_t> off_of((size_t)m.ncp, -1);
    for (int64_t k = P.batch_node[b]; k < P.batch_node[b + 1]; ++k) {
      const int32_t i = P.node[(size_t)k];
      ++node_seen[(size_t)i];
      eq(P.node_off[(size_t)k], doubles, "rows of a batch are packed");
      eq(P.node_L[(size_t)k], m.L[(size_t)i], "columns per segment");
      off_of[(size_t)i] = doubles;
      doubles += md_cp_doubles(nf, m.L[(size_t)i]);
      if (k > P.batch_node[b] || b > 0) {  // stable owner order
        const int32_t p = P.node[(size_t)k - 1];
        const int64_t oi = m.adj[(size_t)m.adj_ptr[(size_t)i]] / m.itp, op = m.adj[(size_t)m.adj_ptr[(size_t)p]] / m.itp;
        ok(op < oi || (op == oi && p < i), "control points in stable owner order");
      }
    }
    ok(doubles <= budget, "a batch within the budget");
    ok(P.batch_node[b + 1] > P.batch_node[b], "no empty batch");
    max_batch = std::max(max_batch, doubles);
    std::vector<int64_t> last_j((size_t)m.ncp, -1);
    for (int64_t t = P.batch_task[b]; t < P.batch_task[b + 1]; ++t) {
      const MdTask& k = P.task[(size_t)t];
      ++seen[(size_t)k.j];
      eq(k.ea, m.adj[(size_t)k.j], "a task carries its adjacency entry");
      const int32_t i = m.cp[(size_t)k.ea];
      eq(k.off, off_of[(size_t)i], "a task points at its control point's rows (and the control point is in the batch)");
      eq(k.L, m.L[(size_t)i], "a task carries its row's segment length");
      if (t > P.batch_task[b]) ok(P.task[(size_t)t - 1].ea / m.itp <= k.ea / m.itp, "tasks of a batch ascend in element");
      if (t == P.batch_task[b] || P.task[(size_t)t - 1].ea / m.itp != k.ea / m.itp) ++runs;
      ok(last_j[(size_t)i] < k.j, "the entries of a control point stay in adjacency order");
      last_j[(size_t)i] = k.j;
    }
  }
  for (int s : seen) eq(s, 1, "every adjacency entry in exactly one task");
  for (int s : node_seen) eq(s, 1, "every control point in exactly one batch");
  eq(P.runs, runs, "geometry evaluations");
  eq(P.max_batch, max_batch, "largest batch");
  ok(P.runs >= m.nel, "every element is evaluated at least once");
}

int main() {
  {
    const Mesh m = lattice(6);
    int64_t max_cp1 = 0;
    for (int32_t l : m.L) max_cp1 = std::max<int64_t>(max_cp1, l);
    eq(max_cp1, 27, "hex-8 lattice: an interior control point couples 27");
    for (int nf = 1; nf <= 4; ++nf)
      for (int64_t budget : {md_cp_doubles(nf, 27), md_budget(0), md_budget(1 << 30)}) walk(m, nf, std::max(budget, md_cp_doubles(nf, 27)), "hex-8 lattice");
    // the smallest budget splits the control points of one owner over batches; the largest holds several owners in a batch
    MdPlan P;
    eq(md_plan_build(m.itp, m.nel, m.ncp, 3, m.adj_ptr.data(), m.adj.data(), m.L.data(), md_cp_doubles(3, 27), &P), MD_OK, "smallest budget");
    ok(P.split_owners > 0, "smallest budget: an owner is split");
    eq(md_plan_build(m.itp, m.nel, m.ncp, 3, m.adj_ptr.data(), m.adj.data(), m.L.data(), md_budget(1 << 30), &P), MD_OK, "largest budget");
    ok(P.max_owners >= 2, "largest budget: several owners in a batch");
    eq(P.budget, (long long)(MD_LDS_CAP / 8), "the knob is capped");
    // the refusals
    eq(md_plan_build(m.itp, m.nel, m.ncp, 3, m.adj_ptr.data(), m.adj.data(), m.L.data(), md_cp_doubles(3, 27) - 1, &P), MD_REFUSE_BUDGET,
       "one control point beyond the budget");
    eq(md_plan_build(m.itp, m.nel, m.ncp, 5, m.adj_ptr.data(), m.adj.data(), m.L.data(), 1 << 20, &P), MD_REFUSE_FIELDS, "five fields");
    Mesh c = m;
    c.cp[1] = c.cp[0];  // element 0 collapsed: lists a control point twice
    finish(c);
    eq(md_plan_build(c.itp, c.nel, c.ncp, 1, c.adj_ptr.data(), c.adj.data(), c.L.data(), 1 << 20, &P), MD_REFUSE_REPEATED, "a collapsed element");
  }
  {
    const Mesh m = fan(32);
    eq(m.adj_ptr[1] - m.adj_ptr[0], 32, "fan: valence 32");
    eq(m.L[0], 33, "fan: the centre couples every control point");
    for (int nf = 1; nf <= 4; ++nf)
      for (int64_t budget : {md_cp_doubles(nf, 33), md_budget(0), md_budget(1 << 30)}) walk(m, nf, std::max(budget, md_cp_doubles(nf, 33)), "fan");
    MdPlan P;
    eq(md_plan_build(m.itp, m.nel, m.ncp, 2, m.adj_ptr.data(), m.adj.data(), m.L.data(), md_cp_doubles(2, 33) - 1, &P), MD_REFUSE_BUDGET,
       "fan: the centre beyond the budget");
  }
  // ---- the LDS block: (family, dim, itg, itp), every table slot, three fields with all nine blocks, the default budget
  struct Fam { const char* name; int dim, itg, itp; };
  const Fam fams[] = {{"quad-8", 2, 9, 8}, {"tet-10", 3, 14, 10}, {"hex-8", 3, 8, 8}, {"hex-20", 3, 27, 20}, {"hex-27", 3, 27, 27}};
  for (const Fam& f : fams) {
    const int ns = 1 + f.dim, nm = ns * ns, nb = 9;
    const int wv = md_waves(f.dim, f.itg, f.itp, ns, nb, nm, MD_DEFAULT_BUDGET);
    ok(wv >= 1, f.name);
    ok(md_lds_bytes(f.dim, f.itg, f.itp, ns, nb, nm, MD_DEFAULT_BUDGET, wv) <= MD_LDS_CAP, "the block is within the cap");
    ok(wv == 4 || md_lds_bytes(f.dim, f.itg, f.itp, ns, nb, nm, MD_DEFAULT_BUDGET, wv * 2) > MD_LDS_CAP, "as many waves as fit");
    const int64_t fit = md_fit_budget(f.dim, f.itg, f.itp, ns, nb, nm);
    ok(md_lds_bytes(f.dim, f.itg, f.itp, ns, nb, nm, fit, 1) == MD_LDS_CAP, "the fitting budget fills the cap");
    eq(md_waves(f.dim, f.itg, f.itp, ns, nb, nm, fit + 1), 0, "one double more does not fit");
  }
  // hex-20, every slot, nine blocks: 27 * 20 * 4 = 2160 doubles of reference table + 144 coefficients; per wave 2160 + 270 + 60 + the budget
  eq((long long)md_shared_doubles(3, 27, 20, 9, 16), 2304, "hex-20 shared doubles");
  eq((long long)md_wave_doubles(3, 27, 20, 4, 2048), 2160 + 270 + 60 + 2048, "hex-20 doubles per wave");
  eq(md_waves(3, 27, 20, 4, 9, 16, 2048), 2, "hex-20 three fields: two waves in 96 KB");
  eq(md_waves(3, 27, 20, 4, 1, 4, 2048), 2, "hex-20 thermal: two waves");
  eq(md_waves(3, 14, 10, 4, 9, 16, 2048), 4, "tet-10: four waves");
  // hex-27 with 64 Gauss points and every slot: the reference table and one physical table are 2 * 55 KB
  ok(md_fit_budget(3, 64, 27, 4, 9, 16) < 0, "hex-27 with 64 points: the tables alone exceed the cap");
  printf(bad ? "FAIL (%d)\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
