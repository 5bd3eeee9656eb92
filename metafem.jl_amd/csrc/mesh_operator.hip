// Matrix-free operator on UNSTRUCTURED classical meshes: y = alpha K x + beta y and diag K for weak forms whose linear gradients have constant
// coefficients (facets: constant + linear in the outward normal), straight from coordinates, connectivity and the reference tables -- no K_val, no
// column indices, no sparse_IDs_by_el, no row ranks.  K x is the contraction the fused residual (residual_mesh.hip) evaluates,
//   sum_q D^s N_a(q) * w_q det_q * sum_terms coef [n_j(q)] D^s' x(q),
// with the field blocks of x in the role of the residual's sources.  The handle keeps the mesh and up to MOP_MAX_PARTS parts (the elements, then one
// per facet group) with their compiled terms (mesh_operator_decide.h: OpProgram).
// Pass 1 (k_mesh_operator, per part): a WAVE owns an element (facet) -- the phases of k_mesh_residual:
//   1. node coordinates and the nodal values x[base field][cp(a)] (/ dsc: the right Jacobi scaling of a solve on A D^-1) to the wave's LDS block;
//   2. J, det, J^-1 (facets: surface det, normals) per Gauss point (mesh_geometry.h);
//   3. every word of every source at the Gauss points on the reference table, derivatives pushed forward with J^-1;
//   4. per dual word g: D[g][q] = w_q det_q sum_e coef_e [n_j] u_e(q);
//   5. the element vector r[f][a] = sum_q sum_g D^{s_g} N_a(q) D[g][q], J^-1 folded into the Gauss-point side -> scratch S_part[item][f][a].
// Pass 2 (k_mesh_operator_gather): a lane owns (field, control point) and sums the scratch entries of its adjacency lists, the element part first,
// then the facet parts in the order they were added, each in ascending order: no atomics, bitwise reproducible.  It writes y = alpha sum + beta y and
// leaves the partial sums of dotw . y the Krylov kernels fold; both passes leave at once when the solve's stop flag is set.
// Diagonal (k_mesh_operator_diag): the same wave per item computes, per dual field and local node, sum_q w_q det_q sum_{terms on the diagonal block}
// coef [n_j] D^s N_a(q) D^s' N_a(q) into the same scratch; the same gather sums it.
// Variable terms (mfem_mesh_operator_set_variable_terms): a part may carry, behind the constant entries of a dual word, entries whose coefficient is
// read at every product from the caller's array vals[slot][item][q] (the layout of mfem_mesh_kval_elements: the coefficient alone, the kernel
// multiplies w_q det_q in).  Such a part launches the VAR instantiation of pass 1 and of the diagonal: phase 4 maps lanes to (dual word, q) pairs and
// adds, after the constant entries, vals[slot_e][q + itg * item] * u_e(q) in the order the terms were given; every load is unit-stride along q and
// nothing of it is staged in LDS.  A part without variable terms launches the instantiation it always did.
#include <memory>
#include <vector>
#include "mesh_geometry.h"
#include "blas1.h"
#include "mesh_operator.h"
#include "mesh_operator_decide.h"

static std::atomic<long long> g_mesh_operator_count{0};
extern "C" int64_t mfem_debug_mesh_operator_count(void) { return g_mesh_operator_count; }

struct OpPart {
  MeshItems V;
  int64_t n_items;
  const int64_t* adj_ptr;
  const int32_t* adj;
  OpProgram P;
  int32_t n_terms, n_var;                      // the caller's lists, kept so that either can be replaced without the other
  mfem_operator_term terms[MOP_MAX_TERMS];
  mfem_kval_term vterms[MOP_MAX_VAR_TERMS];
  const double* var_vals;                      // [n_var][n_items][itg], caller-owned; read at every product and diagonal
  int waves;          // of a pass-1 workgroup
  size_t lds_doubles; // of one wave
  size_t offset;      // of the part's element vectors in the scratch, in doubles
};

struct mfem_mesh_operator_s {
  mfem_operator_head head;    // MFEM_OPERATOR_MESH (operator.h)
  mfem_context_s* ctx;
  int dim, itp, n_fields, base;
  int64_t nel, ncp;
  const double* coords;
  const int32_t* cp;
  std::vector<OpPart> parts;  // [0]: the elements (n_items < 0 until they are set)
  size_t scratch_doubles;
  mfem_csr_s csr;             // pattern-less: what the Krylov loop holds in place of a matrix
};

// the handle of an entry point of this file; nullptr: none, or another kind's
static mfem_mesh_operator_s* mfem_mesh_operator_from_handle(uint64_t handle) {
  mfem_operator_head* h = (mfem_operator_head*)(uintptr_t)handle;
  return h && h->kind == MFEM_OPERATOR_MESH ? (mfem_mesh_operator_s*)h : nullptr;
}

static void mfem_mesh_operator_bind(mfem_mesh_operator_s* op, double* scratch, const double* dsc) {
  op->csr.op = &op->head;
  op->csr.op_scratch = scratch;
  op->csr.op_dsc = dsc;
}
static void mfem_mesh_operator_unbind(mfem_mesh_operator_s* op) {
  op->csr.op = nullptr;
  op->csr.op_scratch = nullptr;
  op->csr.op_dsc = nullptr;
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------------------------
template <int DIM, bool VAR>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_operator(MeshItems V, OpProgram P, const double* __restrict__ x, const double* __restrict__ dsc,
                                                              double* __restrict__ S, int64_t n_items, const int32_t* __restrict__ done_flag,
                                                              const double* __restrict__ vals) {
  extern __shared__ double lds[];
  if (done_flag && done_flag[0]) return;
  constexpr int NC = 1 + DIM;  // value, d/dx_1 .. d/dx_DIM
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  const bool facet = V.eindex != nullptr;
  const size_t per_wave = (size_t)itg * (1 + DIM * DIM) + (size_t)itp * DIM + (facet ? (size_t)itg * DIM : 0) + (size_t)P.nsrc * itp +
                          (size_t)(P.nsrc + P.nfo) * itg * NC + (size_t)P.ngroups * itg;  // (mop_wave_doubles)
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
    const int64_t j = (int64_t)P.src_pos[k] * V.ncp + ((int64_t)cpe[a] - V.base);
    Un[i] = dsc ? x[j] / dsc[j] : x[j];
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
  // ---- the terms of every dual word, times the weight
  if constexpr (VAR) {
    // lane <-> (dual word, q): the constant entries, then the variable ones, whose coefficients come from vals[slot][item][q] (unit stride along q)
    const double* vq = vals + (size_t)itg * (size_t)t;
    const size_t term_stride = (size_t)itg * (size_t)n_items;
    for (int i = lane; i < P.ngroups * itg; i += 64) {
      const int g = i / itg, q = i - g * itg;
      const int e0 = g ? P.grp_end[g - 1] : 0, ev = P.grp_var[g], e1 = P.grp_end[g];
      double sum = 0.0;
      for (int e = e0; e < ev; ++e) {
        double c = P.ent_coef[e];
        if (P.ent_nrm[e] >= 0) c *= Nq[q * DIM + P.ent_nrm[e]];
        sum += c * Vs[((size_t)P.ent_src[e] * itg + q) * NC + P.ent_word[e]];
      }
      for (int e = ev; e < e1; ++e)
        sum += vq[(size_t)P.ent_nrm[e] * term_stride + q] * Vs[((size_t)P.ent_src[e] * itg + q) * NC + P.ent_word[e]];
      D[i] = sum * wd[q];
    }
  } else {  // (lane <-> q; groups in sequence: uniform entry lists)
    for (int g = 0; g < P.ngroups; ++g) {
      const int e0 = g ? P.grp_end[g - 1] : 0, e1 = P.grp_end[g];
      for (int q = lane; q < itg; q += 64) {
        double sum = 0.0;
        for (int e = e0; e < e1; ++e) {
          double c = P.ent_coef[e];
          if (P.ent_nrm[e] >= 0) c *= Nq[q * DIM + P.ent_nrm[e]];
          sum += c * Vs[((size_t)P.ent_src[e] * itg + q) * NC + P.ent_word[e]];
        }
        D[g * itg + q] = sum * wd[q];
      }
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

// ---- the diagonal of one part: S[item][fo][a] = sum_q w_q det_q sum_{g of fo} sum_{e of g on the diagonal block} coef [n_j] D^{s_g} N_a(q) D^{word_e} N_a(q)
template <int DIM, bool VAR>
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_operator_diag(MeshItems V, OpProgram P, double* __restrict__ S, int64_t n_items,
                                                                   const double* __restrict__ vals) {
  extern __shared__ double lds[];
  constexpr int NC = 1 + DIM;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int itg = V.itg, itp = V.itp;
  const bool facet = V.eindex != nullptr;
  const size_t per_wave = (size_t)itg * (1 + DIM * DIM) + (size_t)itp * DIM + (facet ? (size_t)itg * DIM : 0);  // (mop_geo_doubles)
  double* wd = lds + (size_t)w * per_wave;
  double* Ji = wd + itg;
  double* X = Ji + (size_t)itg * DIM * DIM;
  double* Nq = X + (size_t)itp * DIM;
  const int64_t t = (int64_t)blockIdx.x * nw + w;
  if (t >= n_items) return;
  const int64_t el = V.host_el ? (int64_t)V.host_el[t] - V.base : t;
  const int f = facet ? V.eindex[t] - V.base : 0;
  const double* R = V.ref + (int64_t)f * V.ref_stride;
  const int32_t* cpe = V.cp + (int64_t)itp * el;
  for (int i = lane; i < itp * DIM; i += 64) {
    const int a = i / DIM, d = i - a * DIM;
    X[i] = V.coords[((int64_t)cpe[a] - V.base) + (int64_t)d * V.ncp];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  mg_geometry<DIM>(V, R, X, f, lane, itg, false, Ji, wd, facet ? Nq : nullptr);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < P.nfo * itp; i += 64) {
    const int fo = i / itp, a = i - fo * itp;
    double r = 0.0;
    for (int q = 0; q < itg; ++q) {
      double n[NC];  // the physical words of N_a at q
      n[0] = R[q + itg * a];
#pragma unroll
      for (int s = 0; s < DIM; ++s) {
        double g = 0.0;
#pragma unroll
        for (int m = 0; m < DIM; ++m) g += R[q + itg * (a + itp * (1 + m))] * Ji[q * DIM * DIM + m * DIM + s];
        n[1 + s] = g;
      }
      double sum = 0.0;
      for (int g = P.fo_g0[fo]; g < P.fo_g0[fo + 1]; ++g) {
        const int e0 = g ? P.grp_end[g - 1] : 0, e1 = VAR ? P.grp_var[g] : P.grp_end[g];
        double ng = 0.0, gs = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (P.grp_sd[g] == c) ng = n[c];
        for (int e = e0; e < e1; ++e) {
          if (P.src_pos[P.ent_src[e]] != P.fo_pos[fo]) continue;  // (an off-diagonal block)
          double c = P.ent_coef[e];
          if (P.ent_nrm[e] >= 0) c *= Nq[q * DIM + P.ent_nrm[e]];
          double nb = 0.0;
#pragma unroll
          for (int k = 0; k < NC; ++k)
            if (P.ent_word[e] == k) nb = n[k];
          gs += c * nb;
        }
        if constexpr (VAR) {
          for (int e = e1; e < P.grp_end[g]; ++e) {
            if (P.src_pos[P.ent_src[e]] != P.fo_pos[fo]) continue;
            double nb = 0.0;
#pragma unroll
            for (int k = 0; k < NC; ++k)
              if (P.ent_word[e] == k) nb = n[k];
            gs += vals[((size_t)P.ent_nrm[e] * (size_t)n_items + (size_t)t) * itg + q] * nb;
          }
        }
        sum += ng * gs;
      }
      r += wd[q] * sum;
    }
    S[(t * P.nfo + fo) * itp + a] = r;
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------------------------------
struct OpGather {
  int np, itp;
  struct {
    const int64_t* adj_ptr;
    const int32_t* adj;
    size_t offset;                  // of the part's element vectors in the scratch
    int nfo;
    int8_t fo_of[MOP_MAX_NFIELDS];  // the part's output index of field f, -1: the part has no dual word on f
  } p[MOP_MAX_PARTS];
};
static_assert(sizeof(OpGather) < 1024, "OpGather travels in the kernel arguments");

enum { OPG_PRODUCT = 0, OPG_DIAGONAL = 1, OPG_JACOBI = 2 };
// lane <-> row (field, control point).  mode OPG_PRODUCT: y = alpha sum + beta y (beta == 0: y is not read) and the workgroup's partial sum of dotw . y;
// OPG_DIAGONAL: y = sum; OPG_JACOBI: y = |sum| where the row has adjacency and sum != 0, else y keeps its preset (jacobi.hip's guarded rule).
__global__ __launch_bounds__(MFEM_BLOCK) void k_mesh_operator_gather(OpGather G, int64_t ncp, int64_t n, const double* __restrict__ S, double* __restrict__ y,
                                                                     double alpha, double beta, int mode, const double* __restrict__ dotw,
                                                                     double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i / ncp);
    const int64_t node = i - (int64_t)f * ncp;
    double sum = 0.0;
    bool any = false;
    for (int p = 0; p < G.np; ++p) {
      const int fo = G.p[p].fo_of[f];
      if (fo < 0) continue;
      const int64_t j0 = G.p[p].adj_ptr[node], j1 = G.p[p].adj_ptr[node + 1];
      const double* Sp = S + G.p[p].offset;
      const int nfo = G.p[p].nfo;
      any = any || j1 > j0;
      for (int64_t j = j0; j < j1; ++j) {
        const int32_t ea = G.p[p].adj[j];
        const int64_t it = ea / G.itp;
        const int a = ea - (int)it * G.itp;
        sum += Sp[(it * nfo + fo) * G.itp + a];
      }
    }
    if (mode == OPG_PRODUCT) {
      double yv = alpha * sum;
      if (beta != 0.0) yv += beta * y[i];
      y[i] = yv;
      if (dotw) dot_acc += yv * dotw[i];
    } else if (mode == OPG_DIAGONAL) {
      y[i] = sum;
    } else if (any && sum != 0.0) {
      y[i] = fabs(sum);
    }
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
static int op_refuse(int rc, const char* why) {
  mfem_set_error("matrix-free mesh operator: %s", why);
  return rc;
}

// compiles `terms` and the variable `vterms` for a part (its MeshItems already set) and decides its LDS block; the part is changed only if
// everything is accepted.  Either list may be the part's own stored copy.
static int op_set_program(mfem_mesh_operator_s* op, OpPart& part, int32_t n_terms, const mfem_operator_term* terms, int32_t n_var,
                          const mfem_kval_term* vterms, const double* vals) {
  const bool facet = part.V.eindex != nullptr;
  OpProgram P;
  const char* why = "";
  const int rc = mop_compile_mixed(op->dim, facet, op->n_fields, n_terms, terms, n_var, vterms, &P, &why);
  if (rc) return op_refuse(rc, why);
  const size_t doubles = mop_wave_doubles(op->dim, part.V.itg, part.V.itp, facet, P.nsrc, P.nfo, P.ngroups);
  const int waves = mop_waves(doubles);
  if (!waves) {
    mfem_set_error("matrix-free mesh operator: Gauss-point data of %zu bytes per wave: too large (64 KB)", doubles * sizeof(double));
    return MFEM_ERR_UNSUPPORTED;
  }
  part.P = P;
  if (n_terms > 0 && terms != part.terms) memcpy(part.terms, terms, sizeof(mfem_operator_term) * (size_t)n_terms);
  if (n_var > 0 && vterms != part.vterms) memcpy(part.vterms, vterms, sizeof(mfem_kval_term) * (size_t)n_var);
  part.n_terms = n_terms;
  part.n_var = n_var;
  part.var_vals = n_var ? vals : nullptr;
  part.waves = waves;
  part.lds_doubles = doubles;
  return MFEM_OK;
}

static void op_layout(mfem_mesh_operator_s* op) {
  int64_t n_items[MOP_MAX_PARTS];
  int nfo[MOP_MAX_PARTS];
  size_t off[MOP_MAX_PARTS];
  const int np = (int)op->parts.size();
  for (int p = 0; p < np; ++p) {
    n_items[p] = op->parts[p].n_items > 0 ? op->parts[p].n_items : 0;
    nfo[p] = op->parts[p].P.nfo;
  }
  op->scratch_doubles = mop_scratch_layout(np, n_items, nfo, op->itp, off);
  for (int p = 0; p < np; ++p) op->parts[p].offset = off[p];
  ++op->csr.op_epoch;  // (compiled terms, offsets, the instantiation and the coefficient array of a part are baked into a captured cycle)
}

extern "C" int mfem_mesh_operator_create(mfem_context ctx, int32_t dim, int32_t itp, int64_t nel, int64_t ncp, int32_t n_fields, const double* coords,
                                         const int32_t* controlpoint_IDs, int32_t index_base, uint64_t* out) try {
  MFEM_REQUIRE(out, "null out");
  *out = 0;
  MFEM_REQUIRE(ctx && coords && controlpoint_IDs, "null argument");
  MFEM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  MFEM_REQUIRE(itp > 0 && nel >= 0 && ncp > 0 && n_fields >= 1, "bad sizes");
  MFEM_REQUIRE(index_base == 0 || index_base == 1, "index_base must be 0 or 1");
  MFEM_REQUIRE(nel * (int64_t)itp < ((int64_t)1 << 31), "nel * itp must fit 31 bits (adjacency entries are 32-bit)");
  if (n_fields > MOP_MAX_NFIELDS) {
    mfem_set_error("%d fields: the matrix-free mesh operator takes up to %d", n_fields, MOP_MAX_NFIELDS);
    return MFEM_ERR_UNSUPPORTED;
  }
  mfem_host_alloc_probe();
  std::unique_ptr<mfem_mesh_operator_s> op(new mfem_mesh_operator_s());
  op->head.kind = MFEM_OPERATOR_MESH;
  op->ctx = ctx;
  op->dim = dim;
  op->itp = itp;
  op->n_fields = n_fields;
  op->base = index_base;
  op->nel = nel;
  op->ncp = ncp;
  op->coords = coords;
  op->cp = controlpoint_IDs;
  op->scratch_doubles = 0;
  memset(&op->csr, 0, sizeof(op->csr));
  op->csr.ctx = ctx;
  op->csr.serial = mfem_next_csr_serial();
  op->csr.n = (int64_t)n_fields * ncp;
  op->csr.rowptr_bits = 64;
  op->parts.resize(1);
  memset(&op->parts[0], 0, sizeof(OpPart));
  op->parts[0].n_items = -1;  // (no element part yet)
  *out = (uint64_t)(uintptr_t)op.release();
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_operator_create")

extern "C" int mfem_mesh_operator_set_elements(uint64_t handle, int32_t itg, const double* ref_itp_vals, const double* itg_weight,
                                               const int64_t* adj_ptr, const int32_t* adj, int32_t n_terms, const mfem_operator_term* terms) try {
  mfem_mesh_operator_s* op = mfem_mesh_operator_from_handle(handle);
  MFEM_REQUIRE(op, "null handle");
  MFEM_REQUIRE(itg > 0, "bad sizes");
  MFEM_REQUIRE(ref_itp_vals && itg_weight && adj_ptr && adj, "null array");
  OpPart part;
  memset(&part, 0, sizeof(part));
  part.V = MeshItems{itg, op->itp, op->ncp, ref_itp_vals, 0, itg_weight, 0, nullptr, 0, op->coords, op->cp, nullptr, nullptr, nullptr, op->base};
  part.n_items = op->nel;
  part.adj_ptr = adj_ptr;
  part.adj = adj;
  const int rc = op_set_program(op, part, n_terms, terms, 0, nullptr, nullptr);
  if (rc) return rc;
  op->parts[0] = part;
  op_layout(op);
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_operator_set_elements")

extern "C" int mfem_mesh_operator_add_facets(uint64_t handle, int32_t itg_b, int32_t n_face_ids, int64_t n_facets, const double* bdy_ref_itp_vals,
                                             const double* bdy_itg_weights, const double* bdy_tangent_directions, const int32_t* element_ID,
                                             const int32_t* element_eindex, const int64_t* adj_ptr, const int32_t* adj, int32_t n_terms,
                                             const mfem_operator_term* terms, int32_t* part_out) try {
  mfem_mesh_operator_s* op = mfem_mesh_operator_from_handle(handle);
  MFEM_REQUIRE(op, "null handle");
  if (part_out) *part_out = -1;
  MFEM_REQUIRE(itg_b > 0 && n_face_ids > 0 && n_facets >= 0, "bad sizes");
  MFEM_REQUIRE(n_facets * (int64_t)op->itp < ((int64_t)1 << 31), "n_facets * itp must fit 31 bits (adjacency entries are 32-bit)");
  MFEM_REQUIRE(bdy_ref_itp_vals && bdy_itg_weights && bdy_tangent_directions && element_ID && element_eindex && adj_ptr && adj, "null array");
  if ((int)op->parts.size() == MOP_MAX_PARTS) {
    mfem_set_error("matrix-free mesh operator: more than %d parts", MOP_MAX_PARTS);
    return MFEM_ERR_UNSUPPORTED;
  }
  const int dim = op->dim;
  const int64_t rs = (int64_t)itg_b * op->itp * (1 + dim), ts = (int64_t)itg_b * dim * (dim - 1);
  OpPart part;
  memset(&part, 0, sizeof(part));
  part.V = MeshItems{itg_b, op->itp, op->ncp, bdy_ref_itp_vals, rs, bdy_itg_weights, (int64_t)itg_b, bdy_tangent_directions, ts, op->coords,
                     op->cp, element_ID, element_eindex, nullptr, op->base};
  part.n_items = n_facets;
  part.adj_ptr = adj_ptr;
  part.adj = adj;
  const int rc = op_set_program(op, part, n_terms, terms, 0, nullptr, nullptr);
  if (rc) return rc;
  mfem_host_alloc_probe();
  op->parts.push_back(part);
  op_layout(op);
  if (part_out) *part_out = (int32_t)op->parts.size() - 1;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_operator_add_facets")

extern "C" int mfem_mesh_operator_set_terms(uint64_t handle, int32_t part, int32_t n_terms, const mfem_operator_term* terms) try {
  mfem_mesh_operator_s* op = mfem_mesh_operator_from_handle(handle);
  MFEM_REQUIRE(op, "null handle");
  MFEM_REQUIRE(part >= 0 && part < (int)op->parts.size() && op->parts[part].n_items >= 0, "no such part");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  OpPart& pt = op->parts[part];
  const int rc = op_set_program(op, pt, n_terms, terms, pt.n_var, pt.vterms, pt.var_vals);  // (the variable terms stay)
  if (rc) return rc;
  op_layout(op);
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_operator_set_terms")

extern "C" int mfem_mesh_operator_set_variable_terms(uint64_t handle, int32_t part, int32_t n_terms, const mfem_kval_term* terms,
                                                     const double* vals) try {
  mfem_mesh_operator_s* op = mfem_mesh_operator_from_handle(handle);
  MFEM_REQUIRE(op, "null handle");
  MFEM_REQUIRE(part >= 0 && part < (int)op->parts.size() && op->parts[part].n_items > 0, "no such part, or a part without items");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  MFEM_REQUIRE(n_terms >= 0 && (n_terms == 0 || (terms && vals)), "null terms or vals");
  OpPart& pt = op->parts[part];
  const int rc = op_set_program(op, pt, pt.n_terms, pt.terms, n_terms, terms, vals);  // (the constant terms stay)
  if (rc) return rc;
  op_layout(op);  // (a new epoch: no captured cycle replays the old array or the other instantiation)
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_operator_set_variable_terms")

extern "C" int mfem_mesh_operator_destroy(uint64_t handle) try {
  mfem_mesh_operator_s* op = mfem_mesh_operator_from_handle(handle);
  if (!op) return MFEM_OK;
  if (op->ctx && mfem_context_alive(op->ctx)) {
    (void)hipStreamSynchronize(op->ctx->stream);
    mfem_graphs_invalidate(op->ctx);  // (a cached cycle holds the operator's arrays)
  }
  delete op;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_mesh_operator_destroy")

static OpGather op_gather_args(const mfem_mesh_operator_s* op) {
  OpGather G;
  memset(&G, 0, sizeof(G));
  G.itp = op->itp;
  for (const OpPart& part : op->parts) {
    if (part.n_items <= 0 || part.P.nfo == 0) continue;
    auto& g = G.p[G.np++];
    g.adj_ptr = part.adj_ptr;
    g.adj = part.adj;
    g.offset = part.offset;
    g.nfo = part.P.nfo;
    for (int f = 0; f < MOP_MAX_NFIELDS; ++f) g.fo_of[f] = -1;
    for (int fo = 0; fo < part.P.nfo; ++fo) g.fo_of[part.P.fo_pos[fo]] = (int8_t)fo;
  }
  return G;
}

static int op_gather_launch(mfem_context_s* ctx, const mfem_mesh_operator_s* op, const double* S, double* y, double alpha, double beta, int mode,
                            const double* dotw, double* partials, int* n_partials, const int32_t* done_flag) {
  const int64_t n = op->csr.n;
  const int cap = ctx->num_cus * 16 < MFEM_MAX_PARTIALS ? ctx->num_cus * 16 : MFEM_MAX_PARTIALS;
  const int grid = mfem_grid_for(n, MFEM_BLOCK, cap);
  hipLaunchKernelGGL(k_mesh_operator_gather, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, op_gather_args(op), op->ncp, n, S, y, alpha, beta, mode,
                     dotw, partials, done_flag);
  MFEM_CHECK_LAUNCH();
  if (n_partials && partials) *n_partials = grid;
  return MFEM_OK;
}

// pass 1 of every part (diag: the diagonal kernel) into the scratch S
static int op_items_launch(mfem_context_s* ctx, const mfem_mesh_operator_s* op, bool diag, const double* x, const double* dsc, double* S,
                           const int32_t* done_flag) {
  for (const OpPart& part : op->parts) {
    if (part.n_items <= 0 || part.P.nfo == 0) continue;
    const bool facet = part.V.eindex != nullptr;
    const size_t doubles = diag ? mop_geo_doubles(op->dim, part.V.itg, part.V.itp, facet) : part.lds_doubles;
    const int waves = diag ? mop_waves(doubles) : part.waves;
    const int64_t grid = (part.n_items + waves - 1) / waves;
    MFEM_REQUIRE(grid < (1ll << 31), "too many items for one launch");
    const size_t ldsb = doubles * sizeof(double) * waves;
    double* Sp = S + part.offset;
    const dim3 gr((unsigned)grid), bl(64 * waves);
    const bool var = part.P.nvar > 0;  // (a part without variable terms launches the instantiation it always did)
    const double* vals = part.var_vals;
    if (diag) {
      auto k = op->dim == 2 ? (var ? k_mesh_operator_diag<2, true> : k_mesh_operator_diag<2, false>)
                            : (var ? k_mesh_operator_diag<3, true> : k_mesh_operator_diag<3, false>);
      hipLaunchKernelGGL(k, gr, bl, ldsb, ctx->stream, part.V, part.P, Sp, part.n_items, vals);
    } else {
      auto k = op->dim == 2 ? (var ? k_mesh_operator<2, true> : k_mesh_operator<2, false>)
                            : (var ? k_mesh_operator<3, true> : k_mesh_operator<3, false>);
      hipLaunchKernelGGL(k, gr, bl, ldsb, ctx->stream, part.V, part.P, x, dsc, Sp, part.n_items, done_flag, vals);
    }
    MFEM_CHECK_LAUNCH();
  }
  return MFEM_OK;
}

static int mfem_mesh_operator_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* x, double* y, double alpha, double beta, const double* dotw,
                                     double* partials, int* n_partials, const int32_t* done_flag) {
  mfem_mesh_operator_s* op = A->op && A->op->kind == MFEM_OPERATOR_MESH ? (mfem_mesh_operator_s*)A->op : nullptr;
  MFEM_REQUIRE(op && (A->op_scratch || op->scratch_doubles == 0), "the operator is not bound");
  int rc = op_items_launch(ctx, op, false, x, A->op_dsc, A->op_scratch, done_flag);
  if (!rc) rc = op_gather_launch(ctx, op, A->op_scratch, y, alpha, beta, OPG_PRODUCT, dotw, partials, n_partials, done_flag);
  if (rc) return rc;
  if (!ctx->probe_active) ++g_mesh_operator_count;
  return MFEM_OK;
}

static int mfem_mesh_operator_jacobi(mfem_context_s* ctx, mfem_mesh_operator_s* op, double* scratch, double* d) {
  int rc = op_items_launch(ctx, op, true, nullptr, nullptr, scratch, nullptr);
  if (!rc) rc = op_gather_launch(ctx, op, scratch, d, 1.0, 0.0, OPG_JACOBI, nullptr, nullptr, nullptr, nullptr);
  return rc;
}

// what the solve driver and the product dispatch hold of this kind (operator.h)
static mfem_mesh_operator_s* as_mesh(mfem_operator_head* h) { return (mfem_mesh_operator_s*)h; }
static mfem_context_s* mop_if_ctx(mfem_operator_head* h) { return as_mesh(h)->ctx; }
static mfem_csr_s* mop_if_csr(mfem_operator_head* h) { return &as_mesh(h)->csr; }
static size_t mop_if_scratch(const mfem_operator_head* h) { return ((const mfem_mesh_operator_s*)h)->scratch_doubles; }
static int mop_if_bind(mfem_operator_head* h, double* scratch, const double* dsc) { mfem_mesh_operator_bind(as_mesh(h), scratch, dsc); return MFEM_OK; }
static void mop_if_unbind(mfem_operator_head* h) { mfem_mesh_operator_unbind(as_mesh(h)); }
static int mop_if_jacobi(mfem_context_s* ctx, mfem_operator_head* h, double* scratch, double* d) { return mfem_mesh_operator_jacobi(ctx, as_mesh(h), scratch, d); }
const mfem_operator_interface* mfem_mesh_operator_interface() {  // (a function-local table: a const global of a .hip file is emitted for the device too)
  static const mfem_operator_interface I = {mop_if_ctx, mop_if_csr, mop_if_scratch, mop_if_bind, mop_if_unbind, mop_if_jacobi, mfem_mesh_operator_launch};
  return &I;
}

// the stand-alone entry points take the scratch from the context workspace, as the fused residual does
static int op_standalone(mfem_context ctx, uint64_t handle, mfem_mesh_operator_s** out) {
  mfem_mesh_operator_s* op = mfem_mesh_operator_from_handle(handle);
  MFEM_REQUIRE(ctx && op, "null handle, or not a mesh operator's");
  MFEM_REQUIRE(op->ctx == ctx, "the operator was created on another context");
  MFEM_REQUIRE(!op->csr.op, "the operator is bound to a running solve");
  const int rc = mfem_ws_reserve(ctx, op->scratch_doubles * sizeof(double));
  if (rc) return rc;
  *out = op;
  return MFEM_OK;
}

extern "C" int mfem_mesh_operator_apply(mfem_context ctx, uint64_t handle, const double* x, double* y, double alpha, double beta) try {
  mfem_mesh_operator_s* op = nullptr;
  int rc = op_standalone(ctx, handle, &op);
  if (rc) return rc;
  MFEM_REQUIRE(x && y, "null vector");
  struct Release { mfem_mesh_operator_s* op; ~Release() { mfem_mesh_operator_unbind(op); } } release{op};
  mfem_mesh_operator_bind(op, (double*)ctx->ws, nullptr);
  return mfem_spmv_launch(ctx, &op->csr, nullptr, x, y, alpha, beta, nullptr, nullptr, nullptr, nullptr);
} MFEM_API_CATCH("mfem_mesh_operator_apply")

extern "C" int mfem_mesh_operator_diagonal(mfem_context ctx, uint64_t handle, double* d) try {
  mfem_mesh_operator_s* op = nullptr;
  int rc = op_standalone(ctx, handle, &op);
  if (rc) return rc;
  MFEM_REQUIRE(d, "null vector");
  rc = op_items_launch(ctx, op, true, nullptr, nullptr, (double*)ctx->ws, nullptr);
  if (!rc) rc = op_gather_launch(ctx, op, (double*)ctx->ws, d, 1.0, 0.0, OPG_DIAGONAL, nullptr, nullptr, nullptr, nullptr);
  return rc;
} MFEM_API_CATCH("mfem_mesh_operator_diagonal")
