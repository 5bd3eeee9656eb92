// Direct row assembly of constant-coefficient bilinear forms on UNSTRUCTURED classical meshes: the row-owner result of assemble_mesh.hip
// (mfem_mesh_assemble_elements_rows: no atomics, a fixed summation order) without the element-major scratch between its two passes.
//   A WAVE owns a batch of control points that share elements (the plan: mesh_direct_decide.h).  Its tasks are the adjacency entries
//   j = (node i <- element el, local id a) of those control points, sorted by element.  For every run of tasks with the same element the wave
//     1. gathers the element's coordinates, builds J, det, J^-1 and the physical table T[q][a][s] in LDS (mg_geometry / mg_table, as
//        k_mesh_assemble does: the reference table is staged once per workgroup);
//     2. forms ONLY the rows a of the element matrix that its tasks name -- a lane per (task, b): M_ab[c] = sum_q w_q det_q T[q][a][s] T[q][b][s'],
//        block value = sum_c C[k][c] M_ab[c] with the coefficient rows of TermMatrix / Cs --
//     3. and adds them into the batch's rows, staged in the wave's LDS block, at  off + (fd * nf + fb) * L + ranks[j * itp + b]  (what the
//        gather of the two-pass form computes).  Within a run the lanes hit distinct positions (an element lists a control point once); the
//        runs go in sequence.
//   When the batch is done its rows leave as whole-wave stores (overwrite: set, else added).
// Every (element, a) row is computed exactly once over the grid; geometry is recomputed once per (batch, adjacent element); no element
// matrix and no partial row goes to global memory.  The bits of one contribution (el, a, b, block) depend on (itg, itp, n_fields) alone: a
// lane runs the whole Gauss-point sum in q order, the Jacobian sum is split over two lane groups iff 2 * itg <= 64.  The additions into a K
// entry keep the adjacency order of its control point -- the result is identical bit for bit under every budget.
#include <atomic>
#include <memory>
#include "mesh_geometry.h"
#include "mesh_direct_decide.h"

int64_t g_mesh_direct_budget = 0;  // mfem_debug_set("mesh_direct_budget", bytes): staged rows per wave (0 = MD_DEFAULT_BUDGET doubles); read when a plan is created
static std::atomic<long long> g_mesh_direct_count{0};
extern "C" int64_t mfem_debug_mesh_direct_count(void) { return g_mesh_direct_count; }

struct MdDev {
  int64_t nbatch;
  const int64_t* batch_node;  // [nbatch + 1]
  const int64_t* batch_task;  // [nbatch + 1]
  const int32_t* batch_doubles;  // [nbatch] staged doubles of the batch
  const int32_t* node;        // control points in owner order
  const int32_t* node_off;    // first staged double
  const int32_t* node_L;      // columns per field segment
  const MdTask* task;
};
struct MdBlocks {
  int nb, nf;
  int32_t fd[16], fb[16];  // dual / base field of block k (run k of the term list)
};

struct mfem_mesh_direct_plan_s {
  mfem_context_s* ctx;
  int itp, nf;
  int64_t nel, ncp;
  mfem_csr_s* A;
  const uint16_t* ranks;
  std::vector<int64_t> adj_ptr;  // host copies: a smaller budget (an element table that leaves less LDS) cuts the batches again
  std::vector<int32_t> adj, L;
  MdPlan P;
  void* dev[7];
  size_t dev_bytes;
  int64_t waves_per_trip, waves_per_wg, lds_bytes;  // of the last launch
};

template <int DIM, int S0, int NS, bool DIAGT>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_direct(MeshItems V, ConstTerms T, MdDev P, MdBlocks B, const uint16_t* __restrict__ ranks,
                                                              const void* __restrict__ rowptr, int rp64, int cbase, double* __restrict__ K,
                                                              int set, int budget) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  constexpr int NM = DIAGT ? NS : NS * NS;  // products kept per pair
  const size_t ref_doubles = (size_t)itg * itp * (1 + DIM), coef_doubles = (size_t)B.nb * NM;
  const size_t per_wave = (size_t)itg * itp * NS + (size_t)itg * (1 + DIM * DIM) + (size_t)itp * DIM + (size_t)budget;
  double* Rs = lds;                                            // [1 + DIM][itp][itg]: the reference table
  double* Cs = lds + ref_doubles;                              // [nb][NM]: block k = sum_c Cs[k][c] M[c]
  double* Tt = lds + ref_doubles + coef_doubles + (size_t)w * per_wave;  // [itg][itp][NS]
  double* wd = Tt + (size_t)itg * itp * NS;                    // [itg]
  double* Ji = wd + itg;                                       // [itg][DIM * DIM]
  double* X = Ji + (size_t)itg * DIM * DIM;                    // [itp][DIM]
  double* St = X + (size_t)itp * DIM;                          // [budget]: the rows of the batch
  for (int i = threadIdx.x; i < (int)ref_doubles; i += blockDim.x) Rs[i] = V.ref[i];
  for (int c = threadIdx.x; c < (int)coef_doubles; c += blockDim.x) {  // terms in list order: a fixed sum
    const int k = c / NM, m = c - k * NM;
    double sum = 0.0;
    int run = -1;
    for (int i = 0; i < T.n; ++i) {
      if (i == 0 || T.block[i] != T.block[i - 1]) ++run;
      const int sel = DIAGT ? T.ds[i] - S0 : (T.ds[i] - S0) * NS + (T.bs[i] - S0);
      if (run == k && sel == m) sum += T.coef[i];
    }
    Cs[c] = sum;
  }
  __syncthreads();  // (the only workgroup barrier: every wave reaches it)
  const bool split_j = 2 * itg <= 64;  // (from itg alone: the bits of the geometry do not depend on the plan)
  const int nfnf = B.nf * B.nf;
  for (int64_t bt = (int64_t)blockIdx.x * nw + w; bt < P.nbatch; bt += (int64_t)gridDim.x * nw) {
    const int64_t n0 = P.batch_node[bt], n1 = P.batch_node[bt + 1];
    const int64_t t0 = P.batch_task[bt], t1 = P.batch_task[bt + 1];
    int used = P.batch_doubles[bt];
    used = used < budget ? used : budget;
    for (int i = lane; i < used; i += 64) St[i] = 0.0;
    __builtin_amdgcn_wave_barrier();
    for (int64_t t = t0; t < t1;) {
      // the next run: the leading tasks of one element, a lane each
      MdTask tk{0, 0, 0, 0};
      if (t + lane < t1) tk = P.task[t + lane];
      const int el = __builtin_amdgcn_readfirstlane(tk.ea) / itp;
      const unsigned long long same = __ballot(t + lane < t1 && tk.ea / itp == el);
      const int m = ~same == 0ull ? 64 : __builtin_ctzll(~same);  // (>= 1: lane 0 holds task t)
      const int32_t* cpe = V.cp + (int64_t)itp * el;
      for (int i = lane; i < itp * DIM; i += 64) {
        const int a = i / DIM, d = i - a * DIM;
        X[i] = V.coords[((int64_t)cpe[a] - V.base) + (int64_t)d * V.ncp];
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      mg_geometry<DIM>(V, Rs, X, 0, lane, itg, split_j, Ji, wd, nullptr);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      mg_table<DIM, S0, NS>(Rs, Ji, Tt, itg, itp, lane, itg * itp);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      // ---- (task, b) pairs over the lanes
      const int work = m * itp;
      for (int u0 = 0; u0 < work; u0 += 64) {
        const int u = u0 + lane;
        const bool on = u < work;
        const int ti = on ? u / itp : 0, b = on ? u - ti * itp : 0;
        const int tj = __shfl(tk.j, ti), tea = __shfl(tk.ea, ti), toff = __shfl(tk.off, ti), tL = __shfl(tk.L, ti);
        const int a = tea - el * itp;
        double M[NM];
#pragma unroll
        for (int c = 0; c < NM; ++c) M[c] = 0.0;
        {
          const double* ta = Tt + a * NS;
          const double* tb = Tt + b * NS;
          const int qs = itp * NS;
#pragma unroll 3
          for (int q = 0; q < itg; ++q) {
            const double wq_ = wd[q];
            double va[NS], vb[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
              va[s] = ta[q * qs + s];
              vb[s] = tb[q * qs + s] * wq_;
            }
            if (DIAGT) {
#pragma unroll
              for (int s = 0; s < NS; ++s) M[s] += va[s] * vb[s];
            } else {
#pragma unroll
              for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int u_ = 0; u_ < NS; ++u_) M[s * NS + u_] += va[s] * vb[u_];
            }
          }
        }
        const int rk = on ? (int)ranks[(int64_t)tj * itp + b] : 0;
        const bool put = on && rk < tL && toff + nfnf * tL <= budget;  // (a plan and ranks of one pattern always pass)
        for (int k = 0; k < B.nb; ++k) {
          double sum = 0.0;
#pragma unroll
          for (int c = 0; c < NM; ++c) sum += Cs[k * NM + c] * M[c];
          if (put) St[toff + (B.fd[k] * B.nf + B.fb[k]) * tL + rk] += sum;
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      t += m;
    }
    // ---- the rows leave as whole waves
    for (int64_t k = n0; k < n1; ++k) {
      const int64_t node = P.node[k];
      const int off = P.node_off[k], len = B.nf * P.node_L[k];
      if (off + B.nf * len > budget) continue;
      for (int fd = 0; fd < B.nf; ++fd) {
        const int64_t r = (int64_t)fd * V.ncp + node;
        const int64_t lo = (rp64 ? ((const int64_t*)rowptr)[r] : (int64_t)((const int32_t*)rowptr)[r]) - cbase;
        const double* src = St + off + fd * len;
        if (set) for (int i = lane; i < len; i += 64) K[lo + i] = src[i];
        else for (int i = lane; i < len; i += 64) K[lo + i] += src[i];
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
  }
}

static void md_free_dev(mfem_mesh_direct_plan_s* p) {
  for (void*& d : p->dev) {
    if (d) (void)hipFree(d);
    d = nullptr;
  }
  p->dev_bytes = 0;
}

// cuts the batches for `budget` doubles per wave and puts the plan on the device (MD_OK or the refusal of md_plan_build)
static int md_plan_device(mfem_mesh_direct_plan_s* p, int64_t budget, int* refusal) {
  *refusal = md_plan_build(p->itp, p->nel, p->ncp, p->nf, p->adj_ptr.data(), p->adj.data(), p->L.data(), budget, &p->P);
  if (*refusal != MD_OK) return MFEM_OK;
  MFEM_CHECK_HIP(hipStreamSynchronize(p->ctx->stream));  // (a launch on the old arrays may be in flight)
  md_free_dev(p);
  const MdPlan& P = p->P;
  const size_t nbatch = P.batch_node.size() - 1;
  std::vector<int32_t> doubles(nbatch);
  for (size_t b = 0; b < nbatch; ++b) {
    const size_t last = (size_t)P.batch_node[b + 1] - 1;
    doubles[b] = P.node_off[last] + (int32_t)md_cp_doubles(p->nf, P.node_L[last]);
  }
  const void* src[7] = {P.batch_node.data(), P.batch_task.data(), doubles.data(), P.node.data(), P.node_off.data(), P.node_L.data(), P.task.data()};
  const size_t bytes[7] = {sizeof(int64_t) * (nbatch + 1), sizeof(int64_t) * (nbatch + 1), sizeof(int32_t) * nbatch, sizeof(int32_t) * P.node.size(),
                           sizeof(int32_t) * P.node.size(), sizeof(int32_t) * P.node.size(), sizeof(MdTask) * P.task.size()};
  for (int i = 0; i < 7; ++i) {
    MFEM_CHECK_HIP(hipMalloc(&p->dev[i], bytes[i] > 0 ? bytes[i] : 16));
    if (bytes[i] > 0) MFEM_CHECK_HIP(hipMemcpy(p->dev[i], src[i], bytes[i], hipMemcpyHostToDevice));
    p->dev_bytes += bytes[i];
  }
  std::vector<MdTask>().swap(p->P.task);  // (the device holds them; the statistics stay)
  return MFEM_OK;
}

static int md_refuse(int refusal, const mfem_mesh_direct_plan_s* p) {
  switch (refusal) {
    case MD_REFUSE_FIELDS:
      mfem_set_error("%d fields: the direct row assembly takes 1..4; use mfem_mesh_assemble_elements_rows", p->nf);
      break;
    case MD_REFUSE_REPEATED:
      mfem_set_error("an element lists the same control point twice: the direct row assembly adds at distinct positions per element -- use "
                     "mfem_mesh_assemble_elements_rows (which sends such a mesh on to mfem_mesh_assemble_elements)");
      break;
    case MD_REFUSE_BUDGET:
      mfem_set_error("the rows of one control point take %lld doubles, the budget of a wave is %lld: use mfem_mesh_assemble_elements_rows",
                     (long long)p->P.max_cp, (long long)p->P.budget);
      break;
    default:
      mfem_set_error("the direct row assembly does not take this mesh: use mfem_mesh_assemble_elements_rows");
  }
  return MFEM_ERR_UNSUPPORTED;
}

extern "C" int mfem_mesh_direct_plan_create(mfem_context ctx, int32_t itp, int64_t nel, int64_t ncp, int32_t n_fields, mfem_csr A,
                                            const int64_t* adj_ptr, const int32_t* adj, const int32_t* controlpoint_IDs, int32_t index_base,
                                            const uint16_t* ranks, uint64_t* out) try {
  MFEM_REQUIRE(out, "null out");
  *out = 0;
  MFEM_REQUIRE(ctx && A && adj_ptr && adj && controlpoint_IDs && ranks, "null argument");
  MFEM_REQUIRE(itp > 0 && nel > 0 && ncp > 0 && n_fields >= 1, "bad sizes");
  MFEM_REQUIRE(index_base == 0 || index_base == 1, "index_base must be 0 or 1");
  if (n_fields > 4) {
    mfem_set_error("%d fields: the direct row assembly takes 1..4; use mfem_mesh_assemble_elements_rows", n_fields);
    return MFEM_ERR_UNSUPPORTED;
  }
  MFEM_REQUIRE(A->n == (int64_t)n_fields * ncp, "pattern rows != n_fields * ncp");
  MFEM_REQUIRE(nel * (int64_t)itp < ((int64_t)1 << 31), "nel * itp must fit 31 bits (adjacency entries are 32-bit)");
  std::unique_ptr<mfem_mesh_direct_plan_s> p(new mfem_mesh_direct_plan_s());
  p->ctx = ctx;
  p->itp = itp;
  p->nf = n_fields;
  p->nel = nel;
  p->ncp = ncp;
  p->A = A;
  p->ranks = ranks;
  for (void*& d : p->dev) d = nullptr;
  p->dev_bytes = 0;
  p->waves_per_trip = p->waves_per_wg = p->lds_bytes = 0;
  // the inspector runs on the host: adjacency and row lengths come back once per pattern
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  p->adj_ptr.resize((size_t)ncp + 1);
  MFEM_CHECK_HIP(hipMemcpy(p->adj_ptr.data(), adj_ptr, sizeof(int64_t) * ((size_t)ncp + 1), hipMemcpyDeviceToHost));
  MFEM_REQUIRE(p->adj_ptr[0] == 0 && p->adj_ptr[(size_t)ncp] == nel * (int64_t)itp, "adj_ptr must span the nel * itp adjacency entries");
  for (int64_t i = 0; i < ncp; ++i) MFEM_REQUIRE(p->adj_ptr[(size_t)i] <= p->adj_ptr[(size_t)i + 1], "adj_ptr must ascend");
  p->adj.resize((size_t)(nel * itp));
  MFEM_CHECK_HIP(hipMemcpy(p->adj.data(), adj, sizeof(int32_t) * p->adj.size(), hipMemcpyDeviceToHost));
  for (int32_t ea : p->adj) MFEM_REQUIRE(ea >= 0 && ea < nel * (int64_t)itp, "adjacency entry out of range");
  {
    const int64_t nrows = (int64_t)n_fields * ncp;
    std::vector<int64_t> rp((size_t)nrows + 1);
    if (A->rowptr_bits == 64) {
      MFEM_CHECK_HIP(hipMemcpy(rp.data(), A->rowptr, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
    } else {
      std::vector<int32_t> rp32(rp.size());
      MFEM_CHECK_HIP(hipMemcpy(rp32.data(), A->rowptr, sizeof(int32_t) * rp32.size(), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < rp.size(); ++i) rp[i] = rp32[i];
    }
    p->L.resize((size_t)ncp);
    for (int64_t i = 0; i < ncp; ++i) {
      const int64_t len = rp[(size_t)i + 1] - rp[(size_t)i];
      MFEM_REQUIRE(len >= 0 && len % n_fields == 0 && len / n_fields < 65536, "a row of the pattern is not n_fields segments of < 65536 columns");
      for (int fd = 1; fd < n_fields; ++fd)
        MFEM_REQUIRE(rp[(size_t)(fd * ncp + i) + 1] - rp[(size_t)(fd * ncp + i)] == len, "the rows of a control point's fields differ in length");
      p->L[(size_t)i] = (int32_t)(len / n_fields);
    }
  }
  int refusal = MD_OK;
  int rc = md_plan_device(p.get(), md_budget(g_mesh_direct_budget), &refusal);
  if (rc) { md_free_dev(p.get()); return rc; }
  if (refusal != MD_OK) return md_refuse(refusal, p.get());
  *out = (uint64_t)(uintptr_t)p.release();
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_direct_plan_create")

extern "C" int mfem_mesh_direct_plan_destroy(uint64_t handle) try {
  mfem_mesh_direct_plan_s* plan = (mfem_mesh_direct_plan_s*)(uintptr_t)handle;
  if (!plan) return MFEM_OK;
  (void)hipStreamSynchronize(plan->ctx->stream);
  md_free_dev(plan);
  delete plan;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_direct_plan_destroy")

extern "C" int mfem_mesh_direct_plan_stats(uint64_t handle, mfem_mesh_direct_stats* out) try {
  mfem_mesh_direct_plan_s* plan = (mfem_mesh_direct_plan_s*)(uintptr_t)handle;
  MFEM_REQUIRE(plan && out, "null argument");
  const MdPlan& P = plan->P;
  out->batches = (int64_t)P.batch_node.size() - 1;
  out->tasks = P.batch_task.back();
  out->max_batch_doubles = P.max_batch;
  out->max_batch_elements = P.max_runs;
  out->geometry_evaluations = P.runs;
  out->device_bytes = (int64_t)plan->dev_bytes;
  out->waves_per_trip = plan->waves_per_trip;
  out->max_control_point_doubles = P.max_cp;
  out->budget_doubles = P.budget;
  out->waves_per_workgroup = plan->waves_per_wg;
  out->lds_bytes = plan->lds_bytes;
  out->split_owners = P.split_owners;
  out->max_batch_owners = P.max_owners;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_direct_plan_stats")

extern "C" int mfem_mesh_assemble_elements_direct(mfem_context ctx, int32_t dim, int32_t itg, int32_t itp, int64_t nel, int64_t ncp,
                                                  const double* ref_itp_vals, const double* itg_weight, const double* coords,
                                                  const int32_t* controlpoint_IDs, int32_t index_base, int32_t n_terms,
                                                  const mfem_const_term* terms, int32_t n_fields, mfem_csr A, uint64_t handle,
                                                  double* K_val, int32_t overwrite) try {
  mfem_mesh_direct_plan_s* plan = (mfem_mesh_direct_plan_s*)(uintptr_t)handle;
  MFEM_REQUIRE(ctx && A, "null handle");
  MFEM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  MFEM_REQUIRE(itg > 0 && itp > 0 && nel > 0 && ncp > 0, "bad sizes");
  MFEM_REQUIRE(n_fields >= 1, "n_fields must be >= 1");
  if (n_fields > 4) {
    mfem_set_error("%d fields: the direct row assembly takes 1..4; use mfem_mesh_assemble_elements_rows", n_fields);
    return MFEM_ERR_UNSUPPORTED;
  }
  MFEM_REQUIRE(plan, "null plan");
  MFEM_REQUIRE(plan->ctx == ctx && plan->A == A && plan->itp == itp && plan->nel == nel && plan->ncp == ncp && plan->nf == n_fields,
               "the plan was made for another context, pattern or mesh");
  MFEM_REQUIRE(index_base == 0 || index_base == 1, "index_base must be 0 or 1");
  MFEM_REQUIRE(ref_itp_vals && itg_weight && coords && controlpoint_IDs && K_val, "null array");
  ConstTerms T;
  int rc = ma_terms(n_terms, terms, dim, &T);
  if (rc) return rc;
  MdBlocks B;
  memset(&B, 0, sizeof(B));
  B.nf = n_fields;
  int smin = 1 << 30, smax = -1;
  bool diag = true;  // every term pairs a word with itself
  for (int i = 0; i < T.n; ++i) {
    smin = std::min(smin, std::min(T.ds[i], T.bs[i]));
    smax = std::max(smax, std::max(T.ds[i], T.bs[i]));
    diag = diag && T.ds[i] == T.bs[i];
    if (i > 0 && T.block[i] == T.block[i - 1]) continue;
    MFEM_REQUIRE(T.block[i] < n_fields * n_fields, "block out of range");
    B.fd[B.nb] = T.block[i] / n_fields;
    B.fb[B.nb] = T.block[i] % n_fields;
    ++B.nb;
  }
  const int mode = smax == 0 ? 2 : smin >= 1 ? 1 : 0;  // values only | gradients only | everything
  const int NS = mode == 2 ? 1 : mode == 1 ? dim : 1 + dim, NM = diag ? NS : NS * NS;
  // the wave's block: the tables of an element beside the staged rows.  Less room than the plan's budget: the batches are cut again, once.
  const int64_t fit = md_fit_budget(dim, itg, itp, NS, B.nb, NM);
  if (fit < plan->P.max_cp) {
    mfem_set_error("element tables of %zu bytes and the rows of one control point (%lld doubles) exceed the %zu bytes of LDS of a wave of the direct "
                   "row assembly; use mfem_mesh_assemble_elements_rows",
                   sizeof(double) * (md_shared_doubles(dim, itg, itp, B.nb, NM) + md_geo_doubles(dim, itg, itp, NS)), (long long)plan->P.max_cp,
                   MD_LDS_CAP);
    return MFEM_ERR_UNSUPPORTED;
  }
  if (plan->P.budget > fit) {
    int refusal = MD_OK;
    rc = md_plan_device(plan, fit, &refusal);
    if (rc) return rc;
    if (refusal != MD_OK) return md_refuse(refusal, plan);
  }
  const int64_t budget = plan->P.budget;
  const int waves = md_waves(dim, itg, itp, NS, B.nb, NM, budget);
  MFEM_REQUIRE(waves > 0, "the wave block does not fit");
  const size_t ldsb = md_lds_bytes(dim, itg, itp, NS, B.nb, NM, budget, waves);
  const int64_t nbatch = (int64_t)plan->P.batch_node.size() - 1;
  const int per_cu = (int)(160 * 1024 / ldsb);  // persistent: what is resident (LDS-bound: 160 KB per CU)
  const int64_t cap = (int64_t)ctx->num_cus * (per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu);
  int64_t grid = (nbatch + waves - 1) / waves;
  if (grid > cap) grid = cap;
  plan->waves_per_trip = grid * waves;
  plan->waves_per_wg = waves;
  plan->lds_bytes = (int64_t)ldsb;
  MdDev P{nbatch, (const int64_t*)plan->dev[0], (const int64_t*)plan->dev[1], (const int32_t*)plan->dev[2], (const int32_t*)plan->dev[3],
          (const int32_t*)plan->dev[4], (const int32_t*)plan->dev[5], (const MdTask*)plan->dev[6]};
  MeshItems V{itg, itp, ncp, ref_itp_vals, 0, itg_weight, 0, nullptr, 0, coords, controlpoint_IDs, nullptr, nullptr, nullptr, index_base};
#define MD_LAUNCH(D, S0, NSS, DG)                                                                                                      \
  do {                                                                                                                                 \
    if (ldsb > 64 * 1024)                                                                                                              \
      MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mesh_direct<D, S0, NSS, DG>),                               \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb));                                     \
    hipLaunchKernelGGL((k_mesh_direct<D, S0, NSS, DG>), dim3((unsigned)grid), dim3(64 * waves), ldsb, ctx->stream, V, T, P, B, plan->ranks, \
                       A->rowptr, A->rowptr_bits == 64 ? 1 : 0, A->index_base, K_val, overwrite ? 1 : 0, (int)budget);                \
  } while (0)
#define MD_MODE(D, DG)                              \
  do {                                              \
    if (mode == 2) MD_LAUNCH(D, 0, 1, DG);          \
    else if (mode == 1) MD_LAUNCH(D, 1, D, DG);     \
    else MD_LAUNCH(D, 0, 1 + D, DG);                \
  } while (0)
  if (dim == 2) { if (diag) MD_MODE(2, true); else MD_MODE(2, false); }
  else { if (diag) MD_MODE(3, true); else MD_MODE(3, false); }
#undef MD_MODE
#undef MD_LAUNCH
  MFEM_CHECK_LAUNCH();
  ++g_mesh_direct_count;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_assemble_elements_direct")
