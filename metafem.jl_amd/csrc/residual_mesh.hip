// Fused residual of affine weak-form terms on UNSTRUCTURED classical meshes: geometry on the fly, no stored tables.  Replaces, for
// residual terms that are affine in the fields and the nodal externals,
//   update_BasicElements / update_BasicBoundary (the per-element physical tables)     mesh/unstructured_mesh/4_Update_Integrator.jl
//   _Var_Basic per inner variable / external, the `vals = @. expr * w` broadcasts and _Res_Basic per term    05_CodeGenerator.jl:93-154
// Pass 1: a WAVE owns an element (facet):
//   1. node coordinates and the nodal values of every source array the symbols read go to the wave's LDS block;
//   2. J, det, J^-1 (facets: surface det, normals) per Gauss point (mesh_geometry.h: phase 1 of the assembly kernel, shared);
//   3. every word of every source at the Gauss points: sum_a D^c N_a(q) u[a] on the reference table, derivatives pushed forward with J^-1;
//   4. the terms, summed per dual word g = (dual field, dual word):  D[g][q] = w_q det_q sum_t (c0_t + sum_p coef_p [n_j] u_p(q));
//   5. the element vector r[f][a] = sum_q sum_g D^{s_g} N_a(q) D[g][q], with d/dx_s N_a = sum_m d/dxi_m N_a J^-1[m][s] folded into the
//      Gauss-point side, contracted on the reference table  ->  element-major scratch S[item][f][a].
// Pass 2 (k_mesh_residual_gather): a lane owns (field, control point) and sums the scratch entries of the point's adjacency list in
// ascending order into residue: no atomics, no colours, a fixed summation order (bitwise reproducible); a collapsed element (a node
// listed twice) simply has two entries in the list.
#include "mesh_geometry.h"

#define MR_MAX_ENTRIES 128  // (symbol, coefficient) pairs of all terms of one launch, after merging the terms of a dual word
#define MR_MAX_FIELDS 8     // dual fields of one launch

// The terms compiled for the kernel (built on the host per launch, passed by value; read with wave-uniform or small indices).
struct ResProgram {
  int nsym, nsrc, ngroups, nfo;
  const double* src_x[MFEM_RES_MAX_SYMBOLS];  // distinct (array, shift) sources of the symbols
  int64_t src_shift[MFEM_RES_MAX_SYMBOLS];
  int8_t sym_src[MFEM_RES_MAX_SYMBOLS], sym_word[MFEM_RES_MAX_SYMBOLS];  // source, word
  int8_t grp_sd[MFEM_RES_MAX_TERMS];       // dual word of group g (groups sorted by output field)
  int16_t grp_end[MFEM_RES_MAX_TERMS];     // entries of group g: [grp_end[g - 1], grp_end[g])
  double grp_c0[MFEM_RES_MAX_TERMS];
  int8_t ent_sym[MR_MAX_ENTRIES];          // symbol, or -1 = the constant 1
  int8_t ent_nrm[MR_MAX_ENTRIES];          // -1, or j: times n_j
  double ent_coef[MR_MAX_ENTRIES];
  int32_t fo_pos[MR_MAX_FIELDS];           // dual field position of output field fo
  int8_t fo_g0[MR_MAX_FIELDS + 1];         // groups of output field fo: [fo_g0[fo], fo_g0[fo + 1])
};
static_assert(sizeof(ResProgram) < 3500, "ResProgram travels in the kernel arguments");

static std::atomic<long long> g_mesh_residual_count{0};
extern "C" int64_t mfem_debug_mesh_residual_count(void) { return g_mesh_residual_count; }

static inline size_t mr_wave_doubles(int dim, int itg, int itp, const ResProgram& P, bool facet) {
  return (size_t)itg * (1 + dim * dim) + (size_t)itp * dim + (facet ? (size_t)itg * dim : 0) + (size_t)P.nsrc * itp +
         (size_t)(P.nsrc + P.nfo) * itg * (1 + dim) + (size_t)P.ngroups * itg;
}

// A wave per item.  Its LDS block holds the Gauss-point data only, never a basis table: the words of the sources and the element vector are
// contracted against the REFERENCE table (one copy for all items, read through the caches) and J^-1 per Gauss point.  (A physical table
// T[q][a][s] in LDS -- 17 KB per hex-20 wave -- held the kernel to 7 resident waves per CU: 12.1 ms for the 96^3 thermal residual, this form
// keeps 4-6 KB per wave.)
template <int DIM>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_residual(MeshItems V, ResProgram P, double* __restrict__ S, int64_t n_items) {
  extern __shared__ double lds[];
  constexpr int NC = 1 + DIM;  // value, d/dx_1 .. d/dx_DIM
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  const bool facet = V.eindex != nullptr;
  const size_t per_wave = (size_t)itg * (1 + DIM * DIM) + (size_t)itp * DIM + (facet ? (size_t)itg * DIM : 0) + (size_t)P.nsrc * itp +
                          (size_t)(P.nsrc + P.nfo) * itg * NC + (size_t)P.ngroups * itg;
  double* wd = lds + (size_t)w * per_wave;      // [itg]
  double* Ji = wd + itg;                        // [itg][DIM*DIM]
  double* X = Ji + (size_t)itg * DIM * DIM;     // [itp][DIM]
  double* Nq = X + (size_t)itp * DIM;           // [itg][DIM] (facets)
  double* Un = Nq + (facet ? (size_t)itg * DIM : 0);  // [nsrc][itp]
  double* Vs = Un + (size_t)P.nsrc * itp;       // [nsrc][itg][NC]: every word of every source
  double* D = Vs + (size_t)P.nsrc * itg * NC;   // [ngroups][itg]
  double* E = D + (size_t)P.ngroups * itg;      // [nfo][itg][NC]: the dual words pulled back to the reference derivatives
  const int64_t t = (int64_t)blockIdx.x * nw + w;
  if (t >= n_items) return;  // (no workgroup barrier below: a wave without an item may leave)
  const int64_t el = V.host_el ? (int64_t)V.host_el[t] - V.base : t;
  const int f = facet ? V.eindex[t] - V.base : 0;
  const double* R = V.ref + (int64_t)f * V.ref_stride;  // R[q + itg * (a + itp * c)]
  const int32_t* cpe = V.cp + (int64_t)itp * el;
  for (int i = lane; i < itp * DIM; i += 64) {
    const int a = i / DIM, d = i - a * DIM;
    X[i] = V.coords[((int64_t)cpe[a] - V.base) + (int64_t)d * V.ncp];
  }
  for (int i = lane; i < P.nsrc * itp; i += 64) {
    const int k = i / itp, a = i - k * itp;
    Un[i] = P.src_x[k][P.src_shift[k] + ((int64_t)cpe[a] - V.base)];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  mg_geometry<DIM>(V, R, X, f, lane, itg, false, Ji, wd, facet ? Nq : nullptr);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  // ---- the sources' words at the Gauss points (lane <-> (source, q)): value and reference gradient, pushed forward with J^-1
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
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  // ---- the terms of every dual word, times the weight (lane <-> q; groups in sequence: uniform entry lists)
  for (int g = 0; g < P.ngroups; ++g) {
    const int e0 = g ? P.grp_end[g - 1] : 0, e1 = P.grp_end[g];
    for (int q = lane; q < itg; q += 64) {
      double sum = P.grp_c0[g];
      for (int e = e0; e < e1; ++e) {
        double c = P.ent_coef[e];
        if (P.ent_nrm[e] >= 0) c *= Nq[q * DIM + P.ent_nrm[e]];
        const int k = P.ent_sym[e];
        if (k >= 0) c *= Vs[((size_t)P.sym_src[k] * itg + q) * NC + P.sym_word[k]];
        sum += c;
      }
      D[g * itg + q] = sum * wd[q];
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  // ---- per output field and Gauss point: the value part and J^-1 (d/dx part) -> coefficients of the reference words (lane <-> (field, q))
  for (int i = lane; i < P.nfo * itg; i += 64) {
    const int fo = i / itg, q = i - fo * itg;
    double d[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) d[c] = 0.0;
    for (int g = P.fo_g0[fo]; g < P.fo_g0[fo + 1]; ++g) {
      const double v = D[g * itg + q];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (P.grp_sd[g] == c) d[c] += v;
    }
    double* o = E + (size_t)i * NC;
    o[0] = d[0];
#pragma unroll
    for (int m = 0; m < DIM; ++m) {
      double e = 0.0;
#pragma unroll
      for (int s = 0; s < DIM; ++s) e += Ji[q * DIM * DIM + m * DIM + s] * d[1 + s];
      o[1 + m] = e;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  // ---- element vector (lane <-> (output field, node)) -> scratch, unit-stride over the nodes
  for (int i = lane; i < P.nfo * itp; i += 64) {
    const int fo = i / itp, a = i - fo * itp;
    const double* ef = E + (size_t)fo * itg * NC;
    double r = 0.0;
    for (int q = 0; q < itg; ++q) {
#pragma unroll
      for (int c = 0; c < NC; ++c) r += R[q + itg * (a + itp * c)] * ef[q * NC + c];
    }
    S[(t * P.nfo + fo) * itp + a] = r;
  }
}

// Pass 2: lane <-> (output field, control point); adjacency entries (item * itp + local node) in ascending order.
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_residual_gather(int itp, int64_t ncp, int nfo, ResProgram P, const int64_t* __restrict__ adj_ptr,
                                                                     const int32_t* __restrict__ adj, const double* __restrict__ S,
                                                                     double* __restrict__ residue) {
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
    if (j1 > j0) residue[(int64_t)P.fo_pos[fo] * ncp + node] += sum;
  }
}

// Validate the symbols and terms and compile them into a ResProgram.
static int mr_compile(int dim, bool facet, int32_t n_symbols, const mfem_res_symbol* symbols, int32_t n_terms, const mfem_affine_term* terms,
                      ResProgram* P) {
  MFEM_REQUIRE(n_symbols >= 0 && (n_symbols == 0 || symbols), "symbols missing");
  MFEM_REQUIRE(n_terms > 0 && terms, "terms missing");
  if (n_symbols > MFEM_RES_MAX_SYMBOLS || n_terms > MFEM_RES_MAX_TERMS) {
    mfem_set_error("%d symbols, %d terms: the fused residual takes up to %d and %d", n_symbols, n_terms, MFEM_RES_MAX_SYMBOLS, MFEM_RES_MAX_TERMS);
    return MFEM_ERR_UNSUPPORTED;
  }
  memset(P, 0, sizeof(*P));
  for (int k = 0; k < n_symbols; ++k) {
    MFEM_REQUIRE(symbols[k].word >= 0 && symbols[k].word <= dim, "symbol words: 0 = value, 1 + j = d/dx_j");
    MFEM_REQUIRE(symbols[k].x && symbols[k].shift >= 0, "symbol source: a device array and a shift >= 0");
  }
  for (int i = 0; i < n_terms; ++i) {
    const mfem_affine_term& T = terms[i];
    MFEM_REQUIRE(T.dual_pos >= 0 && T.dual_sd >= 0 && T.dual_sd <= dim, "term dual field / word out of range");
    MFEM_REQUIRE(T.n_pairs >= 0, "negative n_pairs");
    if (T.n_pairs > MFEM_RES_MAX_PAIRS) {
      mfem_set_error("a term of %d pairs: the fused residual takes up to %d", T.n_pairs, MFEM_RES_MAX_PAIRS);
      return MFEM_ERR_UNSUPPORTED;
    }
    for (int p = 0; p < T.n_pairs; ++p) {
      MFEM_REQUIRE(T.sym[p] >= -1 && T.sym[p] < n_symbols, "term pair: symbol index out of range");
      MFEM_REQUIRE(T.normal[p] >= -1 && T.normal[p] < dim, "term pair: normal component out of range");
      MFEM_REQUIRE(facet || T.normal[p] < 0, "normals exist on facets only");
    }
  }
  // sources: distinct (array, shift)
  int sym_map[MFEM_RES_MAX_SYMBOLS];
  for (int k = 0; k < n_symbols; ++k) {
    int s = 0;
    while (s < P->nsrc && !(P->src_x[s] == symbols[k].x && P->src_shift[s] == symbols[k].shift)) ++s;
    if (s == P->nsrc) {
      P->src_x[s] = symbols[k].x;
      P->src_shift[s] = symbols[k].shift;
      ++P->nsrc;
    }
    sym_map[k] = k;
    P->sym_src[k] = (int8_t)s;
    P->sym_word[k] = (int8_t)symbols[k].word;
  }
  P->nsym = n_symbols;
  // groups = distinct (dual field, dual word), sorted by field then word; output fields = distinct dual fields
  int order[MFEM_RES_MAX_TERMS];
  for (int i = 0; i < n_terms; ++i) order[i] = i;
  for (int i = 1; i < n_terms; ++i)  // (stable insertion sort: the terms of a group keep their order)
    for (int j = i; j > 0; --j) {
      const mfem_affine_term &A = terms[order[j - 1]], &B = terms[order[j]];
      if (A.dual_pos < B.dual_pos || (A.dual_pos == B.dual_pos && A.dual_sd <= B.dual_sd)) break;
      const int tmp = order[j - 1];
      order[j - 1] = order[j];
      order[j] = tmp;
    }
  int nent = 0;
  for (int ii = 0; ii < n_terms; ++ii) {
    const mfem_affine_term& T = terms[order[ii]];
    const bool new_group = ii == 0 || T.dual_pos != terms[order[ii - 1]].dual_pos || T.dual_sd != terms[order[ii - 1]].dual_sd;
    if (new_group) {
      if (ii == 0 || T.dual_pos != terms[order[ii - 1]].dual_pos) {
        if (P->nfo == MR_MAX_FIELDS) {
          mfem_set_error("more than %d dual fields in one fused residual launch", MR_MAX_FIELDS);
          return MFEM_ERR_UNSUPPORTED;
        }
        P->fo_pos[P->nfo] = T.dual_pos;
        P->fo_g0[P->nfo] = (int8_t)P->ngroups;
        ++P->nfo;
      }
      P->grp_sd[P->ngroups] = (int8_t)T.dual_sd;
      P->grp_c0[P->ngroups] = 0.0;
      ++P->ngroups;
    }
    const int g = P->ngroups - 1;
    P->grp_c0[g] += T.c0;
    for (int p = 0; p < T.n_pairs; ++p) {
      if (T.coef[p] == 0.0) continue;
      const int sk = T.sym[p] < 0 ? -1 : sym_map[T.sym[p]];
      const int g_begin = g ? P->grp_end[g - 1] : 0;
      int e = g_begin;
      while (e < nent && !(P->ent_sym[e] == sk && P->ent_nrm[e] == T.normal[p])) ++e;  // (merge equal monomials of a dual word)
      if (e == nent) {
        if (nent == MR_MAX_ENTRIES) {
          mfem_set_error("more than %d distinct (symbol, normal) pairs in one fused residual launch", MR_MAX_ENTRIES);
          return MFEM_ERR_UNSUPPORTED;
        }
        P->ent_sym[e] = (int8_t)sk;
        P->ent_nrm[e] = (int8_t)T.normal[p];
        P->ent_coef[e] = 0.0;
        ++nent;
      }
      P->ent_coef[e] += T.coef[p];
    }
    P->grp_end[g] = (int16_t)nent;
  }
  P->fo_g0[P->nfo] = (int8_t)P->ngroups;
  return MFEM_OK;
}

static int mr_launch(mfem_context_s* ctx, int dim, const MeshItems& V, int64_t n_items, int32_t n_symbols, const mfem_res_symbol* symbols,
                     int32_t n_terms, const mfem_affine_term* terms, const int64_t* adj_ptr, const int32_t* adj, double* residue) {
  const bool facet = V.eindex != nullptr;
  ResProgram P;
  int rc = mr_compile(dim, facet, n_symbols, symbols, n_terms, terms, &P);
  if (rc) return rc;
  if (n_items == 0) return MFEM_OK;
  const size_t per_wave = sizeof(double) * mr_wave_doubles(dim, V.itg, V.itp, P, facet);
  const size_t lds_cap = 64 * 1024;
  if (per_wave > lds_cap) {
    mfem_set_error("Gauss-point data of %zu bytes per wave: too large for the fused mesh residual (64 KB)", per_wave);
    return MFEM_ERR_UNSUPPORTED;
  }
  int waves = 4;
  while (waves > 1 && per_wave * waves > lds_cap) waves >>= 1;
  const size_t bytes = sizeof(double) * (size_t)n_items * V.itp * P.nfo;
  rc = mfem_ws_reserve(ctx, bytes);
  if (rc) return rc;
  double* S = (double*)ctx->ws;
  const int64_t grid = (n_items + waves - 1) / waves;
  MFEM_REQUIRE(grid < (1ll << 31), "too many items for one launch");
  const size_t ldsb = per_wave * waves;
  if (dim == 2)
    hipLaunchKernelGGL(k_mesh_residual<2>, dim3((unsigned)grid), dim3(64 * waves), ldsb, ctx->stream, V, P, S, n_items);
  else
    hipLaunchKernelGGL(k_mesh_residual<3>, dim3((unsigned)grid), dim3(64 * waves), ldsb, ctx->stream, V, P, S, n_items);
  MFEM_CHECK_LAUNCH();
  const int ggrid = mfem_grid_for((int64_t)P.nfo * V.ncp, MFEM_BLOCK, ctx->num_cus * 16);
  hipLaunchKernelGGL(k_mesh_residual_gather, dim3(ggrid), dim3(MFEM_BLOCK), 0, ctx->stream, V.itp, V.ncp, P.nfo, P, adj_ptr, adj, S, residue);
  MFEM_CHECK_LAUNCH();
  ++g_mesh_residual_count;
  return MFEM_OK;
}

extern "C" int mfem_mesh_residual_elements(mfem_context ctx, int32_t dim, int32_t itg, int32_t itp, int64_t nel, int64_t ncp,
                                           const double* ref_itp_vals, const double* itg_weight, const double* coords,
                                           const int32_t* controlpoint_IDs, int32_t index_base, int32_t n_symbols,
                                           const mfem_res_symbol* symbols, int32_t n_terms, const mfem_affine_term* terms,
                                           const int64_t* adj_ptr, const int32_t* adj, double* residue) try {
  MFEM_REQUIRE(ctx, "null ctx");
  MFEM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  MFEM_REQUIRE(itg > 0 && itp > 0 && nel >= 0 && ncp > 0, "bad sizes");
  MFEM_REQUIRE(index_base == 0 || index_base == 1, "index_base must be 0 or 1");
  MFEM_REQUIRE(ref_itp_vals && itg_weight && coords && controlpoint_IDs && adj_ptr && adj && residue, "null array");
  MeshItems V{itg, itp, ncp, ref_itp_vals, 0, itg_weight, 0, nullptr, 0, coords, controlpoint_IDs, nullptr, nullptr, nullptr, index_base};
  return mr_launch(ctx, dim, V, nel, n_symbols, symbols, n_terms, terms, adj_ptr, adj, residue);
} MFEM_API_CATCH("mfem_mesh_residual_elements")

extern "C" int mfem_mesh_residual_facets(mfem_context ctx, int32_t dim, int32_t itg_b, int32_t itp, int32_t n_face_ids, int64_t n_facets,
                                         int64_t ncp, const double* bdy_ref_itp_vals, const double* bdy_itg_weights,
                                         const double* bdy_tangent_directions, const double* coords, const int32_t* controlpoint_IDs,
                                         const int32_t* element_ID, const int32_t* element_eindex, int32_t index_base, int32_t n_symbols,
                                         const mfem_res_symbol* symbols, int32_t n_terms, const mfem_affine_term* terms,
                                         const int64_t* adj_ptr, const int32_t* adj, double* residue) try {
  MFEM_REQUIRE(ctx, "null ctx");
  MFEM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  MFEM_REQUIRE(itg_b > 0 && itp > 0 && n_face_ids > 0 && n_facets >= 0 && ncp > 0, "bad sizes");
  MFEM_REQUIRE(index_base == 0 || index_base == 1, "index_base must be 0 or 1");
  MFEM_REQUIRE(bdy_ref_itp_vals && bdy_itg_weights && bdy_tangent_directions && coords && controlpoint_IDs && element_ID && element_eindex &&
                   adj_ptr && adj && residue, "null array");
  const int64_t rs = (int64_t)itg_b * itp * (1 + dim), ts = (int64_t)itg_b * dim * (dim - 1);
  MeshItems V{itg_b, itp, ncp, bdy_ref_itp_vals, rs, bdy_itg_weights, (int64_t)itg_b, bdy_tangent_directions, ts, coords,
              controlpoint_IDs, element_ID, element_eindex, nullptr, index_base};
  return mr_launch(ctx, dim, V, n_facets, n_symbols, symbols, n_terms, terms, adj_ptr, adj, residue);
} MFEM_API_CATCH("mfem_mesh_residual_facets")
