// The S3 operators (_Var_Basic, _Res_Basic, _Kval_Basic; solver/06_FEM_Kernel.jl:1-79) on UNSTRUCTURED classical meshes with geometry on the fly:
// what mfem_op_var_batch / mfem_op_res_batch / mfem_op_kval_batch (ops.hip) compute from the stored per-element physical table
// integral_vals[itg, itp, 1 + dim, nel] of update_BasicElements / update_BasicBoundary, computed straight from coordinates, connectivity and the
// reference tables.  A WAVE owns a work unit (an element or a boundary facet); mesh_geometry.h gives J, det, J^-1 (facets: surface det, normals).
//   var   the words of nodal arrays at the Gauss points, contracted on the REFERENCE table and pushed forward with J^-1 (k_mesh_residual step 3);
//   res   element vectors per dual field, the coefficient pulled back with J^-1 and contracted on the reference table -> element-major scratch ->
//         one lane per (field, control point) sums its adjacency list in ascending order (no atomics, bitwise reproducible);
//   kval  the physical table T[q][a][s] in the wave's LDS block (the pair loop needs both sides at every Gauss point, as k_mesh_assemble) with
//         the item's weighted coefficients vals_t[q] w_q det_q staged beside it; per node pair and sparse block
//         sum_{t in block} sum_q vals_t[q] T[q][a][dsd_t] T[q][b][bsd_t]  -> slot table (colour batches / FP64 atomics) or the element-major
//         scratch of the row-owner gather (assemble_mesh.hip: mfem_mesh_gather_launch).
// `vals` holds the COEFFICIENT only: the weight w_q det_q (the surface det on facets) is multiplied in here; no weight array exists on this path.
#include "mesh_geometry.h"
#include "mesh_ops_decide.h"

#define MO_MAX_FIELDS 8  // dual fields of one res launch

static std::atomic<long long> g_mesh_ops_count{0};
extern "C" int64_t mfem_debug_mesh_ops_count(void) { return g_mesh_ops_count; }

// The terms compiled for the kernels (built on the host per launch, passed by value).
struct VarProgram {
  int n, nsrc;
  const double* src_x[MFEM_MAX_BATCH_TERMS];  // distinct (array, shift) sources of the words
  int64_t src_shift[MFEM_MAX_BATCH_TERMS];
  int8_t term_src[MFEM_MAX_BATCH_TERMS], term_sd[MFEM_MAX_BATCH_TERMS];
};
struct ResOpProgram {
  int n, nfo;
  int64_t fo_shift[MO_MAX_FIELDS];  // cpID_shift of output field fo
  int8_t fo_t0[MO_MAX_FIELDS + 1];  // terms of output field fo: [fo_t0[fo], fo_t0[fo + 1])
  int8_t sd[MFEM_MAX_BATCH_TERMS];
};
struct KvalProgram {
  int n;
  int8_t ds[MFEM_MAX_BATCH_TERMS], bs[MFEM_MAX_BATCH_TERMS];  // table slots relative to S0
  int32_t block[MFEM_MAX_BATCH_TERMS];
};

__device__ __forceinline__ void mo_sync() {  // the wave's LDS writes are visible to its lanes
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
}

// The item of work unit t, its node coordinates and its geometry (phase 1) in the wave's block: wd [itg], Ji [itg][DIM * DIM], X [itp][DIM],
// Nq [itg][DIM] (facets; filled when want_normals).
template <int DIM>
__device__ __forceinline__ void mo_item(const MeshItems& V, int64_t t, int lane, double* wd, double* Ji, double* X, double* Nq, bool want_normals,
                                        int64_t& h, int64_t& el, const double*& R) {
  h = V.order ? (int64_t)V.order[t] - V.base : t;
  el = V.host_el ? (int64_t)V.host_el[h] - V.base : h;
  const int f = V.eindex ? V.eindex[h] - V.base : 0;
  R = V.ref + (int64_t)f * V.ref_stride;
  const int32_t* cpe = V.cp + (int64_t)V.itp * el;
  for (int i = lane; i < V.itp * DIM; i += 64) {
    const int a = i / DIM, d = i - a * DIM;
    X[i] = V.coords[((int64_t)cpe[a] - V.base) + (int64_t)d * V.ncp];
  }
  mo_sync();
  mg_geometry<DIM>(V, R, X, f, lane, V.itg, false, Ji, wd, want_normals ? Nq : nullptr);
  mo_sync();
}

// ---- var ----------------------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_var(MeshItems V, VarProgram P, double* __restrict__ targets, double* __restrict__ normals,
                                                           int64_t n_items) {
  extern __shared__ double lds[];
  constexpr int NC = 1 + DIM;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  const bool facet = V.eindex != nullptr;
  double* wd = lds + (size_t)w * mo_var_doubles(DIM, itg, itp, facet, P.nsrc);
  double* Ji = wd + itg;
  double* X = Ji + (size_t)itg * DIM * DIM;
  double* Nq = X + (size_t)itp * DIM;
  double* Un = Nq + (facet ? (size_t)itg * DIM : 0);  // [nsrc][itp]
  double* Vs = Un + (size_t)P.nsrc * itp;             // [nsrc][itg][NC]
  const int64_t t = (int64_t)blockIdx.x * nw + w;
  if (t >= n_items) return;  // (no workgroup barrier below)
  int64_t h, el;
  const double* R;
  {
    const int64_t h0 = V.order ? (int64_t)V.order[t] - V.base : t;
    const int64_t el0 = V.host_el ? (int64_t)V.host_el[h0] - V.base : h0;
    const int32_t* cpe = V.cp + (int64_t)itp * el0;
    for (int i = lane; i < P.nsrc * itp; i += 64) {
      const int k = i / itp, a = i - k * itp;
      Un[i] = P.src_x[k][P.src_shift[k] + ((int64_t)cpe[a] - V.base)];
    }
  }
  mo_item<DIM>(V, t, lane, wd, Ji, X, Nq, facet && normals, h, el, R);
  // every word of every source (lane <-> (source, q)): value and reference gradient, pushed forward with J^-1
  for (int i = lane; i < P.nsrc * itg; i += 64) {
    const int k = i / itg, q = i - k * itg;
    const double* u = Un + (size_t)k * itp;
    double v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = 0.0;
    for (int a = 0; a < itp; ++a) {
      const double ua = u[a];
#pragma unroll
      for (int c = 0; c < NC; ++c) v[c] += R[q + itg * (a + itp * c)] * ua;
    }
    double* o = Vs + (size_t)i * NC;
    o[0] = v[0];
#pragma unroll
    for (int s = 0; s < DIM; ++s) {
      double g = 0.0;
#pragma unroll
      for (int m = 0; m < DIM; ++m) g += v[1 + m] * Ji[q * DIM * DIM + m * DIM + s];
      o[1 + s] = g;
    }
  }
  mo_sync();
  for (int i = lane; i < P.n * itg; i += 64) {  // targets[term][q, unit]: unit-stride over q
    const int tt = i / itg, q = i - tt * itg;
    targets[((int64_t)tt * n_items + t) * itg + q] = Vs[((size_t)P.term_src[tt] * itg + q) * NC + P.term_sd[tt]];
  }
  if (facet && normals)
    for (int i = lane; i < itg * DIM; i += 64) {  // normal_directions[itg, dim, n_facets]
      const int d = i / itg, q = i - d * itg;
      normals[q + (int64_t)itg * (d + (int64_t)DIM * h)] = Nq[q * DIM + d];
    }
}

// ---- res ----------------------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_res(MeshItems V, ResOpProgram P, const double* __restrict__ vals, double* __restrict__ S,
                                                           int64_t n_items) {
  extern __shared__ double lds[];
  constexpr int NC = 1 + DIM;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  const bool facet = V.eindex != nullptr;
  double* wd = lds + (size_t)w * mo_res_doubles(DIM, itg, itp, facet, P.nfo);
  double* Ji = wd + itg;
  double* X = Ji + (size_t)itg * DIM * DIM;
  double* Nq = X + (size_t)itp * DIM;
  double* E = Nq + (facet ? (size_t)itg * DIM : 0);  // [nfo][itg][NC]: the dual words pulled back to the reference derivatives
  const int64_t t = (int64_t)blockIdx.x * nw + w;
  if (t >= n_items) return;
  int64_t h, el;
  const double* R;
  mo_item<DIM>(V, t, lane, wd, Ji, X, Nq, false, h, el, R);
  for (int i = lane; i < P.nfo * itg; i += 64) {  // lane <-> (output field, q)
    const int fo = i / itg, q = i - fo * itg;
    double d[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) d[c] = 0.0;
    for (int tt = P.fo_t0[fo]; tt < P.fo_t0[fo + 1]; ++tt) {
      const double v = vals[((int64_t)tt * n_items + t) * itg + q];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (P.sd[tt] == c) d[c] += v;
    }
    const double wq = wd[q];
    double* o = E + (size_t)i * NC;
    o[0] = d[0] * wq;
#pragma unroll
    for (int m = 0; m < DIM; ++m) {
      double e = 0.0;
#pragma unroll
      for (int s = 0; s < DIM; ++s) e += Ji[q * DIM * DIM + m * DIM + s] * d[1 + s];
      o[1 + m] = e * wq;
    }
  }
  mo_sync();
  for (int i = lane; i < P.nfo * itp; i += 64) {  // element vector (lane <-> (output field, node)) -> scratch of ITEM h
    const int fo = i / itp, a = i - fo * itp;
    const double* ef = E + (size_t)fo * itg * NC;
    double r = 0.0;
    for (int q = 0; q < itg; ++q) {
#pragma unroll
      for (int c = 0; c < NC; ++c) r += R[q + itg * (a + itp * c)] * ef[q * NC + c];
    }
    S[(h * P.nfo + fo) * itp + a] = r;
  }
}

// Pass 2: lane <-> (output field, control point); adjacency entries (item * itp + local node) in ascending order.
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_res_gather(int itp, int64_t ncp, ResOpProgram P, const int64_t* __restrict__ adj_ptr,
                                                                  const int32_t* __restrict__ adj, const double* __restrict__ S,
                                                                  double* __restrict__ residue) {
  const int nfo = P.nfo;
  const int64_t total = (int64_t)nfo * ncp;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int fo = (int)(i / ncp);
    const int64_t node = i - (int64_t)fo * ncp;
    const int64_t j0 = adj_ptr[node], j1 = adj_ptr[node + 1];
    double sum = 0.0;
    for (int64_t j = j0; j < j1; ++j) {
      const int32_t ea = adj[j];
      const int64_t it = ea / itp;
      const int a = ea - (int)it * itp;
      sum += S[(it * nfo + fo) * itp + a];
    }
    if (j1 > j0) residue[P.fo_shift[fo] + node] += sum;
  }
}

// ---- kval ---------------------------------------------------------------------------------------------------------------------------------
// S0 / NS: the table slots the terms use, OUT: 0 colour batches / 1 FP64 atomics through the slot table, 2 element-major scratch (k_mesh_assemble).
template <int DIM, int S0, int NS, int OUT>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_kval(MeshItems V, KvalProgram P, const double* __restrict__ vals, int64_t n_units,
                                                            const int32_t* __restrict__ slots, int64_t block_stride, double* __restrict__ K,
                                                            int64_t t0, int64_t t1, int nb) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  const bool facet = V.eindex != nullptr;
  double* wd = lds + (size_t)w * mo_kval_doubles(DIM, itg, itp, facet, NS, P.n);
  double* Ji = wd + itg;
  double* X = Ji + (size_t)itg * DIM * DIM;
  double* Nq = X + (size_t)itp * DIM;
  double* Tt = Nq + (facet ? (size_t)itg * DIM : 0);  // [itg][itp][NS]
  double* Vt = Tt + (size_t)itg * itp * NS;           // [n][itg]: vals_t[q] w_q det_q of this item
  const int64_t t = t0 + (int64_t)blockIdx.x * nw + w;
  if (t >= t1) return;
  int64_t h, el;
  const double* R;
  mo_item<DIM>(V, t, lane, wd, Ji, X, Nq, false, h, el, R);
  mg_table<DIM, S0, NS>(R, Ji, Tt, itg, itp, lane, itg * itp);
  for (int i = lane; i < P.n * itg; i += 64) {
    const int tt = i / itg, q = i - tt * itg;
    Vt[i] = vals[((int64_t)tt * n_units + t) * itg + q] * wd[q];
  }
  mo_sync();
  const int npair = itp * itp, qs = itp * NS;
  for (int p = lane; p < npair; p += 64) {
    // slot table order: a fastest; scratch order: b fastest (the lanes' stores are unit-stride)
    const int a = OUT == 2 ? p / itp : p % itp, b = OUT == 2 ? p % itp : p / itp;
    const double* ta0 = Tt + a * NS;
    const double* tb0 = Tt + b * NS;
    int i = 0, krun = 0;
    while (i < P.n) {  // runs of terms with the same sparse block (wave-uniform): one accumulate per run
      const int block = P.block[i];
      double sum = 0.0;
      for (; i < P.n && P.block[i] == block; ++i) {
        const double* ta = ta0 + P.ds[i];
        const double* tb = tb0 + P.bs[i];
        const double* v = Vt + i * itg;
        double s = 0.0;
#pragma unroll 3
        for (int q = 0; q < itg; ++q) s += v[q] * ta[q * qs] * tb[q * qs];
        sum += s;
      }
      if (OUT == 2) {
        K[(((int64_t)h * itp + a) * nb + krun) * itp + b] = sum;
      } else {
        double* dst = K + ((int64_t)slots[block * block_stride + (int64_t)npair * el + p] - V.base);
        if (OUT == 1) atomicAdd(dst, sum); else *dst += sum;
      }
      ++krun;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
static int mo_check_table(int dim, int itg, int itp) {
  if (!mo_table_fits(dim, itg, itp)) {
    mfem_set_error("an element table of %zu bytes: the table-free mesh operators take up to 64 KB; use mfem_op_* on the stored tables",
                   sizeof(double) * (size_t)itg * itp * (1 + dim));
    return MFEM_ERR_UNSUPPORTED;
  }
  return MFEM_OK;
}
static int mo_check_waves(size_t per_wave_bytes, const char* what, int* waves) {
  *waves = mo_waves(per_wave_bytes);
  if (*waves == 0) {
    mfem_set_error("%s: %zu bytes of LDS per wave, more than 64 KB; use mfem_op_* on the stored tables", what, per_wave_bytes);
    return MFEM_ERR_UNSUPPORTED;
  }
  return MFEM_OK;
}
static int mo_mesh_args(mfem_context_s* ctx, int dim, int itg, int itp, int64_t n_hosts, int64_t ncp, int index_base) {
  MFEM_REQUIRE(ctx, "null ctx");
  MFEM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  MFEM_REQUIRE(itg > 0 && itp > 0 && n_hosts >= 0 && ncp > 0, "bad sizes");
  MFEM_REQUIRE(index_base == 0 || index_base == 1, "index_base must be 0 or 1");
  return MFEM_OK;
}
static MeshItems mo_elements(int itg, int itp, int64_t ncp, const double* ref, const double* w, const double* coords, const int32_t* cp,
                             const int32_t* order, int base) {
  return MeshItems{itg, itp, ncp, ref, 0, w, 0, nullptr, 0, coords, cp, nullptr, nullptr, order, base};
}
static MeshItems mo_facets(int dim, int itg_b, int itp, int64_t ncp, const double* bref, const double* bw, const double* btan, const double* coords,
                           const int32_t* cp, const int32_t* element_ID, const int32_t* element_eindex, const int32_t* order, int base) {
  const int64_t rs = (int64_t)itg_b * itp * (1 + dim), ts = (int64_t)itg_b * dim * (dim - 1);
  return MeshItems{itg_b, itp, ncp, bref, rs, bw, (int64_t)itg_b, btan, ts, coords, cp, element_ID, element_eindex, order, base};
}

static int mo_var(mfem_context_s* ctx, int dim, const MeshItems& V, int64_t n_items, int32_t n_terms, const mfem_var_term* terms, double* targets,
                  double* normals) {
  const bool facet = V.eindex != nullptr;
  const int min_terms = facet && normals ? 0 : 1;  // (facets may be asked for their normals alone)
  MFEM_REQUIRE(n_terms >= min_terms && n_terms <= MFEM_MAX_BATCH_TERMS, "n_terms must be 1..MFEM_MAX_BATCH_TERMS");
  MFEM_REQUIRE(n_terms == 0 || (terms && targets), "null array");
  VarProgram P;
  memset(&P, 0, sizeof(P));
  P.n = n_terms;
  for (int i = 0; i < n_terms; ++i) {
    MFEM_REQUIRE(terms[i].sd >= 0 && terms[i].sd <= dim && terms[i].x, "sd out of range or null x");
    MFEM_REQUIRE(terms[i].cpID_shift >= 0, "negative cpID_shift");
    int s = 0;
    while (s < P.nsrc && !(P.src_x[s] == terms[i].x && P.src_shift[s] == terms[i].cpID_shift)) ++s;
    if (s == P.nsrc) {
      P.src_x[s] = terms[i].x;
      P.src_shift[s] = terms[i].cpID_shift;
      ++P.nsrc;
    }
    P.term_src[i] = (int8_t)s;
    P.term_sd[i] = (int8_t)terms[i].sd;
  }
  int rc = mo_check_table(dim, V.itg, V.itp);
  if (rc) return rc;
  int waves;
  const size_t per_wave = sizeof(double) * mo_var_doubles(dim, V.itg, V.itp, facet, P.nsrc);
  rc = mo_check_waves(per_wave, "words of the sources at the Gauss points", &waves);
  if (rc) return rc;
  if (n_items == 0) return MFEM_OK;
  const int64_t grid = (n_items + waves - 1) / waves;
  MFEM_REQUIRE(grid < (1ll << 31), "too many items for one launch");
  if (dim == 2)
    hipLaunchKernelGGL(k_mesh_var<2>, dim3((unsigned)grid), dim3(64 * waves), per_wave * waves, ctx->stream, V, P, targets, normals, n_items);
  else
    hipLaunchKernelGGL(k_mesh_var<3>, dim3((unsigned)grid), dim3(64 * waves), per_wave * waves, ctx->stream, V, P, targets, normals, n_items);
  MFEM_CHECK_LAUNCH();
  ++g_mesh_ops_count;
  return MFEM_OK;
}

static int mo_res(mfem_context_s* ctx, int dim, const MeshItems& V, int64_t n_items, int32_t n_terms, const mfem_res_term* terms,
                  const double* vals, const int64_t* adj_ptr, const int32_t* adj, double* residue) {
  const bool facet = V.eindex != nullptr;
  MFEM_REQUIRE(n_terms > 0 && n_terms <= MFEM_MAX_BATCH_TERMS, "n_terms must be 1..MFEM_MAX_BATCH_TERMS");
  MFEM_REQUIRE(terms && vals && adj_ptr && adj && residue, "null array");
  ResOpProgram P;
  memset(&P, 0, sizeof(P));
  P.n = n_terms;
  int nfo = 0;
  for (int i = 0; i < n_terms; ++i) {
    MFEM_REQUIRE(terms[i].dual_sd >= 0 && terms[i].dual_sd <= dim, "sd out of range");
    MFEM_REQUIRE(terms[i].cpID_shift >= 0 && (i == 0 || terms[i].cpID_shift >= terms[i - 1].cpID_shift), "terms must be sorted by cpID_shift");
    P.sd[i] = (int8_t)terms[i].dual_sd;
    if (i == 0 || terms[i].cpID_shift != terms[i - 1].cpID_shift) {
      if (nfo < MO_MAX_FIELDS) {
        P.fo_shift[nfo] = terms[i].cpID_shift;
        P.fo_t0[nfo] = (int8_t)i;
      }
      ++nfo;
    }
  }
  if (nfo > MO_MAX_FIELDS) {
    mfem_set_error("%d dual fields in one launch: the table-free mesh residual operator takes up to %d", nfo, MO_MAX_FIELDS);
    return MFEM_ERR_UNSUPPORTED;
  }
  P.nfo = nfo;
  P.fo_t0[nfo] = (int8_t)n_terms;
  int rc = mo_check_table(dim, V.itg, V.itp);
  if (rc) return rc;
  int waves;
  const size_t per_wave = sizeof(double) * mo_res_doubles(dim, V.itg, V.itp, facet, nfo);
  rc = mo_check_waves(per_wave, "dual words at the Gauss points", &waves);
  if (rc) return rc;
  if (n_items == 0) return MFEM_OK;
  rc = mfem_ws_reserve(ctx, sizeof(double) * (size_t)n_items * V.itp * nfo);
  if (rc) return rc;
  double* S = (double*)ctx->ws;
  const int64_t grid = (n_items + waves - 1) / waves;
  MFEM_REQUIRE(grid < (1ll << 31), "too many items for one launch");
  if (dim == 2)
    hipLaunchKernelGGL(k_mesh_res<2>, dim3((unsigned)grid), dim3(64 * waves), per_wave * waves, ctx->stream, V, P, vals, S, n_items);
  else
    hipLaunchKernelGGL(k_mesh_res<3>, dim3((unsigned)grid), dim3(64 * waves), per_wave * waves, ctx->stream, V, P, vals, S, n_items);
  MFEM_CHECK_LAUNCH();
  const int ggrid = mfem_grid_for((int64_t)nfo * V.ncp, MFEM_BLOCK, ctx->num_cus * 16);
  hipLaunchKernelGGL(k_mesh_res_gather, dim3(ggrid), dim3(MFEM_BLOCK), 0, ctx->stream, V.itp, V.ncp, P, adj_ptr, adj, S, residue);
  MFEM_CHECK_LAUNCH();
  ++g_mesh_ops_count;
  return MFEM_OK;
}

// Validates the terms and compiles them; *mode: 0 values + gradients, 1 gradients only, 2 values only (the table slots in LDS).
static int mo_kval_terms(int dim, int32_t n_terms, const mfem_kval_term* terms, const double* vals, KvalProgram* P, int* mode) {
  MFEM_REQUIRE(n_terms > 0 && n_terms <= MFEM_MAX_BATCH_TERMS, "n_terms must be 1..MFEM_MAX_BATCH_TERMS");
  MFEM_REQUIRE(terms && vals, "null array");
  int smin = 1 << 30, smax = -1;
  for (int i = 0; i < n_terms; ++i) {
    MFEM_REQUIRE(terms[i].dual_sd >= 0 && terms[i].dual_sd <= dim && terms[i].base_sd >= 0 && terms[i].base_sd <= dim, "sd out of range");
    MFEM_REQUIRE(terms[i].block >= 0 && (i == 0 || terms[i].block >= terms[i - 1].block), "terms must be sorted by block");
    const int lo = terms[i].dual_sd < terms[i].base_sd ? terms[i].dual_sd : terms[i].base_sd;
    const int hi = terms[i].dual_sd > terms[i].base_sd ? terms[i].dual_sd : terms[i].base_sd;
    smin = lo < smin ? lo : smin;
    smax = hi > smax ? hi : smax;
  }
  *mode = mo_kval_mode(smin, smax);
  const int s0 = mo_kval_first_slot(*mode);
  memset(P, 0, sizeof(*P));
  P->n = n_terms;
  for (int i = 0; i < n_terms; ++i) {
    P->ds[i] = (int8_t)(terms[i].dual_sd - s0);
    P->bs[i] = (int8_t)(terms[i].base_sd - s0);
    P->block[i] = terms[i].block;
  }
  return MFEM_OK;
}

// out_mode 0 / 1: K = K_val through the slot table; 2: K = the element-major scratch with nb blocks per row.
static int mo_kval_launch(mfem_context_s* ctx, int dim, const MeshItems& V, const KvalProgram& P, int mode, int waves, size_t per_wave,
                          const double* vals, int64_t n_units, const int32_t* slots, int64_t block_stride, double* K, int out_mode, int n_colours,
                          const int64_t* colour_offsets, int nb) {
  const int nbatch = out_mode == 0 ? n_colours : 1;
  for (int c = 0; c < nbatch; ++c) {
    const int64_t a = out_mode == 0 ? colour_offsets[c] : 0, b = out_mode == 0 ? colour_offsets[c + 1] : n_units;
    if (b <= a) continue;
    const int64_t grid = (b - a + waves - 1) / waves;
    MFEM_REQUIRE(grid < (1ll << 31), "too many items for one launch");
#define MO_LAUNCH(D, S0, NSS, AT)                                                                                                         \
  hipLaunchKernelGGL((k_mesh_kval<D, S0, NSS, AT>), dim3((unsigned)grid), dim3(64 * waves), per_wave * waves, ctx->stream, V, P, vals, \
                     n_units, slots, block_stride, K, a, b, nb)
#define MO_MODE(D, AT)                          \
  do {                                          \
    if (mode == 2) MO_LAUNCH(D, 0, 1, AT);      \
    else if (mode == 1) MO_LAUNCH(D, 1, D, AT); \
    else MO_LAUNCH(D, 0, 1 + D, AT);            \
  } while (0)
#define MO_OUT(D)                          \
  do {                                     \
    if (out_mode == 2) MO_MODE(D, 2);      \
    else if (out_mode == 1) MO_MODE(D, 1); \
    else MO_MODE(D, 0);                    \
  } while (0)
    if (dim == 2) MO_OUT(2); else MO_OUT(3);
#undef MO_OUT
#undef MO_MODE
#undef MO_LAUNCH
    MFEM_CHECK_LAUNCH();
  }
  return MFEM_OK;
}

// The scatter forms (elements and facets).
static int mo_kval(mfem_context_s* ctx, int dim, const MeshItems& V, int64_t n_items, int32_t n_terms, const mfem_kval_term* terms,
                   const double* vals, const int32_t* slots, int64_t block_stride, double* K_val, int n_colours, const int64_t* colour_offsets) {
  MFEM_REQUIRE(n_colours >= 0 && (n_colours == 0 || colour_offsets), "colour_offsets missing");
  KvalProgram P;
  int mode;
  int rc = mo_kval_terms(dim, n_terms, terms, vals, &P, &mode);
  if (rc) return rc;
  MFEM_REQUIRE(slots && K_val, "null array");
  if (n_colours > 0) {
    MFEM_REQUIRE(colour_offsets[0] == 0 && colour_offsets[n_colours] == n_items, "colour_offsets must span the items");
    for (int c = 0; c < n_colours; ++c) MFEM_REQUIRE(colour_offsets[c] <= colour_offsets[c + 1], "colour_offsets must be non-decreasing");
  }
  rc = mo_check_table(dim, V.itg, V.itp);
  if (rc) return rc;
  const int NS = mo_kval_slots(mode, dim);
  const size_t per_wave = sizeof(double) * mo_kval_doubles(dim, V.itg, V.itp, V.eindex != nullptr, NS, n_terms);
  int waves;
  rc = mo_check_waves(per_wave, "element table and coefficients", &waves);
  if (rc) return rc;
  if (n_items == 0) return MFEM_OK;
  rc = mo_kval_launch(ctx, dim, V, P, mode, waves, per_wave, vals, n_items, slots, block_stride, K_val, n_colours == 0 ? 1 : 0, n_colours,
                      colour_offsets, 0);
  if (rc) return rc;
  ++g_mesh_ops_count;
  return MFEM_OK;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
extern "C" int mfem_mesh_var_elements(mfem_context ctx, int32_t dim, int32_t itg, int32_t itp, int64_t nel, int64_t ncp, const double* ref_itp_vals,
                                      const double* itg_weight, const double* coords, const int32_t* controlpoint_IDs, int32_t index_base,
                                      int32_t n_terms, const mfem_var_term* terms, double* targets, const int32_t* elIDs, int64_t n_items) try {
  int rc = mo_mesh_args(ctx, dim, itg, itp, nel, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(n_items >= 0 && n_items <= nel, "bad sizes");
  MFEM_REQUIRE(ref_itp_vals && itg_weight && coords && controlpoint_IDs, "null array");
  return mo_var(ctx, dim, mo_elements(itg, itp, ncp, ref_itp_vals, itg_weight, coords, controlpoint_IDs, elIDs, index_base), n_items, n_terms, terms,
                targets, nullptr);
} MFEM_API_CATCH("mfem_mesh_var_elements")

extern "C" int mfem_mesh_var_facets(mfem_context ctx, int32_t dim, int32_t itg_b, int32_t itp, int32_t n_face_ids, int64_t n_facets, int64_t ncp,
                                    const double* bdy_ref_itp_vals, const double* bdy_itg_weights, const double* bdy_tangent_directions,
                                    const double* coords, const int32_t* controlpoint_IDs, const int32_t* element_ID, const int32_t* element_eindex,
                                    int32_t index_base, int32_t n_terms, const mfem_var_term* terms, double* targets, double* normal_directions,
                                    const int32_t* facetIDs, int64_t n_items) try {
  int rc = mo_mesh_args(ctx, dim, itg_b, itp, n_facets, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(n_face_ids > 0 && n_items >= 0 && n_items <= n_facets, "bad sizes");
  MFEM_REQUIRE(bdy_ref_itp_vals && bdy_itg_weights && bdy_tangent_directions && coords && controlpoint_IDs && element_ID && element_eindex,
               "null array");
  return mo_var(ctx, dim, mo_facets(dim, itg_b, itp, ncp, bdy_ref_itp_vals, bdy_itg_weights, bdy_tangent_directions, coords, controlpoint_IDs,
                                    element_ID, element_eindex, facetIDs, index_base), n_items, n_terms, terms, targets, normal_directions);
} MFEM_API_CATCH("mfem_mesh_var_facets")

extern "C" int mfem_mesh_res_elements(mfem_context ctx, int32_t dim, int32_t itg, int32_t itp, int64_t nel, int64_t ncp, const double* ref_itp_vals,
                                      const double* itg_weight, const double* coords, const int32_t* controlpoint_IDs, int32_t index_base,
                                      int32_t n_terms, const mfem_res_term* terms, const double* vals, const int32_t* elIDs,
                                      const int64_t* adj_ptr, const int32_t* adj, double* residue) try {
  int rc = mo_mesh_args(ctx, dim, itg, itp, nel, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(ref_itp_vals && itg_weight && coords && controlpoint_IDs, "null array");
  return mo_res(ctx, dim, mo_elements(itg, itp, ncp, ref_itp_vals, itg_weight, coords, controlpoint_IDs, elIDs, index_base), nel, n_terms, terms,
                vals, adj_ptr, adj, residue);
} MFEM_API_CATCH("mfem_mesh_res_elements")

extern "C" int mfem_mesh_res_facets(mfem_context ctx, int32_t dim, int32_t itg_b, int32_t itp, int32_t n_face_ids, int64_t n_facets, int64_t ncp,
                                    const double* bdy_ref_itp_vals, const double* bdy_itg_weights, const double* bdy_tangent_directions,
                                    const double* coords, const int32_t* controlpoint_IDs, const int32_t* element_ID, const int32_t* element_eindex,
                                    int32_t index_base, int32_t n_terms, const mfem_res_term* terms, const double* vals, const int32_t* facetIDs,
                                    const int64_t* adj_ptr, const int32_t* adj, double* residue) try {
  int rc = mo_mesh_args(ctx, dim, itg_b, itp, n_facets, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(n_face_ids > 0, "bad sizes");
  MFEM_REQUIRE(bdy_ref_itp_vals && bdy_itg_weights && bdy_tangent_directions && coords && controlpoint_IDs && element_ID && element_eindex,
               "null array");
  return mo_res(ctx, dim, mo_facets(dim, itg_b, itp, ncp, bdy_ref_itp_vals, bdy_itg_weights, bdy_tangent_directions, coords, controlpoint_IDs,
                                    element_ID, element_eindex, facetIDs, index_base), n_facets, n_terms, terms, vals, adj_ptr, adj, residue);
} MFEM_API_CATCH("mfem_mesh_res_facets")

extern "C" int mfem_mesh_kval_elements(mfem_context ctx, int32_t dim, int32_t itg, int32_t itp, int64_t nel, int64_t ncp, const double* ref_itp_vals,
                                       const double* itg_weight, const double* coords, const int32_t* controlpoint_IDs, int32_t index_base,
                                       int32_t n_terms, const mfem_kval_term* terms, const double* vals, const int32_t* sparse_IDs_by_el,
                                       int64_t slot_block_stride, double* K_val, const int32_t* elIDs, int64_t n_items, int32_t n_colours,
                                       const int64_t* colour_offsets) try {
  int rc = mo_mesh_args(ctx, dim, itg, itp, nel, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(n_items >= 0 && n_items <= nel, "bad sizes");
  MFEM_REQUIRE(ref_itp_vals && itg_weight && coords && controlpoint_IDs, "null array");
  return mo_kval(ctx, dim, mo_elements(itg, itp, ncp, ref_itp_vals, itg_weight, coords, controlpoint_IDs, elIDs, index_base), n_items, n_terms,
                 terms, vals, sparse_IDs_by_el, slot_block_stride, K_val, n_colours, colour_offsets);
} MFEM_API_CATCH("mfem_mesh_kval_elements")

extern "C" int mfem_mesh_kval_facets(mfem_context ctx, int32_t dim, int32_t itg_b, int32_t itp, int32_t n_face_ids, int64_t n_facets, int64_t ncp,
                                     const double* bdy_ref_itp_vals, const double* bdy_itg_weights, const double* bdy_tangent_directions,
                                     const double* coords, const int32_t* controlpoint_IDs, const int32_t* element_ID,
                                     const int32_t* element_eindex, int32_t index_base, int32_t n_terms, const mfem_kval_term* terms,
                                     const double* vals, const int32_t* sparse_IDs_by_el, int64_t slot_block_stride, double* K_val,
                                     const int32_t* facetIDs, int64_t n_items, int32_t n_colours, const int64_t* colour_offsets) try {
  int rc = mo_mesh_args(ctx, dim, itg_b, itp, n_facets, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(n_face_ids > 0 && n_items >= 0 && n_items <= n_facets, "bad sizes");
  MFEM_REQUIRE(bdy_ref_itp_vals && bdy_itg_weights && bdy_tangent_directions && coords && controlpoint_IDs && element_ID && element_eindex,
               "null array");
  return mo_kval(ctx, dim, mo_facets(dim, itg_b, itp, ncp, bdy_ref_itp_vals, bdy_itg_weights, bdy_tangent_directions, coords, controlpoint_IDs,
                                     element_ID, element_eindex, facetIDs, index_base), n_items, n_terms, terms, vals, sparse_IDs_by_el,
                 slot_block_stride, K_val, n_colours, colour_offsets);
} MFEM_API_CATCH("mfem_mesh_kval_facets")

extern "C" int mfem_mesh_kval_elements_rows(mfem_context ctx, int32_t dim, int32_t itg, int32_t itp, int64_t nel, int64_t ncp,
                                            const double* ref_itp_vals, const double* itg_weight, const double* coords,
                                            const int32_t* controlpoint_IDs, int32_t index_base, int32_t n_terms, const mfem_kval_term* terms,
                                            const double* vals, const int32_t* elIDs, int32_t n_fields, mfem_csr A, const int64_t* adj_ptr,
                                            const int32_t* adj, const uint16_t* ranks, double* K_val) try {
  int rc = mo_mesh_args(ctx, dim, itg, itp, nel, ncp, index_base);
  if (rc) return rc;
  MFEM_REQUIRE(A, "null handle");
  MFEM_REQUIRE(n_fields >= 1, "n_fields must be >= 1");
  MFEM_REQUIRE(ref_itp_vals && itg_weight && coords && controlpoint_IDs && adj_ptr && adj && ranks && K_val, "null array");
  KvalProgram P;
  int mode;
  rc = mo_kval_terms(dim, n_terms, terms, vals, &P, &mode);
  if (rc) return rc;
  if (n_fields > 4) {  // (GatherBlocks holds 4 x 4 blocks)
    mfem_set_error("%d fields: the row-owner form takes 1..4; use mfem_mesh_kval_elements", n_fields);
    return MFEM_ERR_UNSUPPORTED;
  }
  MFEM_REQUIRE(A->n == (int64_t)n_fields * ncp, "pattern rows != n_fields * ncp");
  if (A->max_row_nnz > MG_MAXROW) {
    mfem_set_error("rows of up to %d entries: the row-owner form stages a row in LDS (<= %d); use mfem_mesh_kval_elements", A->max_row_nnz, MG_MAXROW);
    return MFEM_ERR_UNSUPPORTED;
  }
  GatherBlocks B;
  memset(&B, 0, sizeof(B));
  B.nf = n_fields;
  for (int i = 0; i < n_terms; ++i) {
    if (i > 0 && terms[i].block == terms[i - 1].block) continue;
    const int fd = terms[i].block / n_fields, fb = terms[i].block % n_fields;
    MFEM_REQUIRE(fd < n_fields, "block out of range");
    B.k[fd][B.cnt[fd]] = B.nb;
    B.fb[fd][B.cnt[fd]] = fb;
    ++B.cnt[fd];
    ++B.nb;
  }
  const size_t bytes = sizeof(double) * (size_t)nel * itp * B.nb * itp;
  if (bytes > MG_SCRATCH_BUDGET) {
    mfem_set_error("element-matrix scratch of %zu bytes exceeds the 96 GiB budget; use mfem_mesh_kval_elements", bytes);
    return MFEM_ERR_UNSUPPORTED;
  }
  rc = mo_check_table(dim, itg, itp);
  if (rc) return rc;
  const int NS = mo_kval_slots(mode, dim);
  const size_t per_wave = sizeof(double) * mo_kval_doubles(dim, itg, itp, false, NS, n_terms);
  int waves;
  rc = mo_check_waves(per_wave, "element table and coefficients", &waves);
  if (rc) return rc;
  if (nel == 0) return MFEM_OK;
  rc = mfem_ws_reserve(ctx, bytes);
  if (rc) return rc;
  double* S = (double*)ctx->ws;
  const MeshItems V = mo_elements(itg, itp, ncp, ref_itp_vals, itg_weight, coords, controlpoint_IDs, elIDs, index_base);
  rc = mo_kval_launch(ctx, dim, V, P, mode, waves, per_wave, vals, nel, nullptr, 0, S, 2, 0, nullptr, B.nb);
  if (rc) return rc;
  rc = mfem_mesh_gather_launch(ctx, itp, ncp, B, A, adj_ptr, adj, ranks, S, K_val, 0);
  if (rc) return rc;
  ++g_mesh_ops_count;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_kval_elements_rows")
