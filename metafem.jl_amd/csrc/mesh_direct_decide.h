// The host decisions of the direct row assembly on unstructured meshes (mesh_direct.hip): the per-wave budget of staged rows, how the control
// points are cut into batches and their adjacency entries into tasks, the doubles of a workgroup's LDS block (the kernel lays its block out with
// the same functions), waves per workgroup, and the refusals.  No HIP, no context: tools/host_check_mesh_direct.cpp walks them on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

static const size_t MD_LDS_CAP = 96 * 1024;       // bytes of LDS one workgroup may take: the cap of the staged k_mesh_assemble (two workgroups per CU at hex-20)
// doubles of staged rows per wave unless mfem_debug_set("mesh_direct_budget") says otherwise.  Measured at 96^3 hex-20 / 64^3 tet-10 elasticity with
// 1024 / 2048 / 4096 / 8192: 150 / 113 / 138 / 198 ms and 36 / 50 / 51 / 80 ms -- the resident waves decide, not the geometry evaluations saved.
static const int64_t MD_DEFAULT_BUDGET = 2048;
static const int MD_MAX_RUN = 64;                 // tasks of one element a wave takes in one go (a lane holds one)

// One adjacency entry j = (node i <- element el, local id a) of a batch: the wave adds row a of el's element matrix into the rows of node i,
// staged from double `off` of the wave's block with L columns per field segment.
struct alignas(16) MdTask {
  int32_t j, ea, off, L;
};

enum { MD_OK = 0, MD_REFUSE_FIELDS, MD_REFUSE_REPEATED, MD_REFUSE_BUDGET, MD_REFUSE_LDS };

struct MdPlan {
  int64_t budget = 0;                 // doubles of staged rows per wave the cuts were made for
  int64_t max_cp = 0;                 // n_fields^2 * L of the largest control point
  std::vector<int32_t> node;          // control points in stable owner order
  std::vector<int32_t> node_off;      // first staged double of node[k] inside its batch
  std::vector<int32_t> node_L;        // its columns per field segment
  std::vector<int64_t> batch_node;    // [nbatch + 1] into node
  std::vector<int64_t> batch_task;    // [nbatch + 1] into task
  std::vector<MdTask> task;           // sorted by element inside a batch, adjacency order inside a control point
  // statistics
  int64_t max_batch = 0;              // largest batch in doubles
  int64_t max_runs = 0;               // most geometry evaluations (element runs) of one batch
  int64_t runs = 0;                   // geometry evaluations in total
  int64_t split_owners = 0;           // owner elements whose nodes went to two or more batches
  int64_t max_owners = 0;             // most owner elements with a node in one batch
};

// doubles one control point stages: the rows of its n_fields fields, n_fields segments of L columns each
static inline int64_t md_cp_doubles(int nf, int64_t L) { return (int64_t)nf * nf * L; }

// The budget in doubles from the knob (bytes; 0 = default): never above the cap.
static inline int64_t md_budget(int64_t knob_bytes) {
  int64_t b = knob_bytes > 0 ? knob_bytes / 8 : MD_DEFAULT_BUDGET;
  const int64_t cap = (int64_t)(MD_LDS_CAP / 8);
  return b > cap ? cap : b;
}

// LDS of a workgroup: the reference table and the coefficient rows once, then per wave the physical table, w det, J^-1, X and the staged rows.
static inline size_t md_shared_doubles(int dim, int itg, int itp, int nb, int nm) { return (size_t)itg * itp * (1 + dim) + (size_t)nb * nm; }
static inline size_t md_geo_doubles(int dim, int itg, int itp, int ns) {
  return (size_t)itg * itp * ns + (size_t)itg * (1 + dim * dim) + (size_t)itp * dim;
}
static inline size_t md_wave_doubles(int dim, int itg, int itp, int ns, int64_t budget) { return md_geo_doubles(dim, itg, itp, ns) + (size_t)budget; }
static inline size_t md_lds_bytes(int dim, int itg, int itp, int ns, int nb, int nm, int64_t budget, int waves) {
  return sizeof(double) * (md_shared_doubles(dim, itg, itp, nb, nm) + (size_t)waves * md_wave_doubles(dim, itg, itp, ns, budget));
}
// Largest budget one wave can stage beside its tables (<= 0: not even the tables fit).
static inline int64_t md_fit_budget(int dim, int itg, int itp, int ns, int nb, int nm) {
  return (int64_t)(MD_LDS_CAP / 8) - (int64_t)md_shared_doubles(dim, itg, itp, nb, nm) - (int64_t)md_geo_doubles(dim, itg, itp, ns);
}
// Waves of a workgroup (4, 2 or 1), 0 = one wave's block does not fit the cap.
static inline int md_waves(int dim, int itg, int itp, int ns, int nb, int nm, int64_t budget) {
  int wv = 4;
  while (wv > 1 && md_lds_bytes(dim, itg, itp, ns, nb, nm, budget, wv) > MD_LDS_CAP) wv >>= 1;
  return md_lds_bytes(dim, itg, itp, ns, nb, nm, budget, wv) <= MD_LDS_CAP ? wv : 0;
}

// The inspector.  adj_ptr [ncp + 1], adj [adj_ptr[ncp]] = element * itp + local id, ascending per control point; L[i] = columns per field
// segment of the rows of control point i.  owner(i) = adj[adj_ptr[i]] / itp (control points no element lists go last: their rows are written
// as zeros).  Returns MD_OK or the refusal.
static inline int md_plan_build(int itp, int64_t nel, int64_t ncp, int nf, const int64_t* adj_ptr, const int32_t* adj, const int32_t* L,
                                int64_t budget, MdPlan* P) {
  *P = MdPlan();
  P->budget = budget;
  if (nf > 4) return MD_REFUSE_FIELDS;
  for (int64_t i = 0; i < ncp; ++i) {
    for (int64_t j = adj_ptr[i] + 1; j < adj_ptr[i + 1]; ++j)
      if (adj[j] / itp == adj[j - 1] / itp) return MD_REFUSE_REPEATED;  // (sorted: an element that lists i twice shows as neighbours)
    const int64_t need = md_cp_doubles(nf, L[i]);
    P->max_cp = need > P->max_cp ? need : P->max_cp;
  }
  if (P->max_cp > budget) return MD_REFUSE_BUDGET;
  // stable owner order: a counting sort over the owners
  std::vector<int64_t> first((size_t)nel + 2, 0);
  auto owner = [&](int64_t i) { return adj_ptr[i + 1] > adj_ptr[i] ? (int64_t)(adj[adj_ptr[i]] / itp) : nel; };
  for (int64_t i = 0; i < ncp; ++i) ++first[(size_t)owner(i) + 1];
  for (int64_t e = 0; e <= nel; ++e) first[(size_t)e + 1] += first[(size_t)e];
  P->node.resize((size_t)ncp);
  {
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (int64_t i = 0; i < ncp; ++i) P->node[(size_t)at[(size_t)owner(i)]++] = (int32_t)i;
  }
  P->node_off.resize((size_t)ncp);
  P->node_L.resize((size_t)ncp);
  P->task.reserve((size_t)adj_ptr[ncp]);
  P->batch_node.push_back(0);
  P->batch_task.push_back(0);
  int64_t cur = 0, owners_here = 0, last_owner = -1, prev_batch_last_owner = -1, last_split = -1;
  auto close = [&](int64_t k_end) {
    const size_t t0 = (size_t)P->batch_task.back();
    std::stable_sort(P->task.begin() + (std::ptrdiff_t)t0, P->task.end(),
                     [itp](const MdTask& x, const MdTask& y) { return x.ea / itp < y.ea / itp; });
    int64_t runs = 0, len = 0;
    for (size_t t = t0; t < P->task.size(); ++t) {  // a run: up to MD_MAX_RUN consecutive tasks of one element (what the kernel takes in one go)
      if (t == t0 || P->task[t].ea / itp != P->task[t - 1].ea / itp || len == MD_MAX_RUN) { ++runs; len = 0; }
      ++len;
    }
    P->runs += runs;
    P->max_runs = runs > P->max_runs ? runs : P->max_runs;
    P->max_batch = cur > P->max_batch ? cur : P->max_batch;
    P->max_owners = owners_here > P->max_owners ? owners_here : P->max_owners;
    P->batch_node.push_back(k_end);
    P->batch_task.push_back((int64_t)P->task.size());
    prev_batch_last_owner = last_owner;
    cur = 0;
    owners_here = 0;
  };
  for (int64_t k = 0; k < ncp; ++k) {
    const int64_t i = P->node[(size_t)k], need = md_cp_doubles(nf, L[i]);
    if (cur + need > budget) close(k);
    const int64_t o = owner(i);
    if (owners_here == 0 || o != last_owner) {
      ++owners_here;
      if (owners_here == 1 && o == prev_batch_last_owner && o != last_split) {  // the owner of the batch before goes on here
        ++P->split_owners;
        last_split = o;
      }
    }
    last_owner = o;
    P->node_off[(size_t)k] = (int32_t)cur;
    P->node_L[(size_t)k] = L[i];
    for (int64_t j = adj_ptr[i]; j < adj_ptr[i + 1]; ++j) P->task.push_back(MdTask{(int32_t)j, adj[j], (int32_t)cur, L[i]});
    cur += need;
  }
  if (ncp > 0) close(ncp);
  return MD_OK;
}
