// Geometry on the fly for the fused kernels of unstructured classical meshes (assemble_mesh.hip: K; residual_mesh.hip: the
// residual).  A wave owns an element (or boundary facet) and, with the node coordinates in its LDS block, computes
//   phase 1: J, det, J^-1 per Gauss point (facets: tangents, surface det and, on request, the outward normal),
//   phase 2: the physical table T[q][a][s - S0] (s = value, d/dx_1 .. d/dx_dim) from the reference table (the assembly; the residual
//            contracts on the reference table and J^-1 instead),
// as update_BasicElements / update_BasicBoundary + inv_Jac + update_Basic_itgval_1 do (mesh/unstructured_mesh/
// 4_Update_Integrator.jl:2-227), without storing anything per element.
#pragma once
#include "common.h"

struct MeshItems {
  int itg, itp;
  int64_t ncp;
  const double* ref;     // [n_face_ids][itg, itp, 1 + dim]
  int64_t ref_stride;
  const double* wq;      // [n_face_ids][itg]
  int64_t w_stride;
  const double* tan;     // facets: [n_face_ids][itg, dim, dim - 1]; elements: nullptr
  int64_t tan_stride;
  const double* coords;  // SoA
  const int32_t* cp;     // [itp, nel]
  const int32_t* host_el;   // facets: element of item h; elements: nullptr
  const int32_t* eindex;    // facets: local face id of item h
  const int32_t* order;     // item processed by work unit t (colour order); nullptr = identity
  int base;
};

// The constant-coefficient terms of one launch (assemble_mesh.hip, mesh_direct.hip), sorted by sparse block; ma_terms checks and copies the caller's list.
#define MA_MAX_TERMS 48
struct ConstTerms {
  int n;
  int32_t ds[MA_MAX_TERMS], bs[MA_MAX_TERMS], block[MA_MAX_TERMS];
  double coef[MA_MAX_TERMS];
};
int ma_terms(int32_t n_terms, const mfem_const_term* terms, int dim, ConstTerms* out);

template <int DIM>
__device__ __forceinline__ double ma_inv(const double (&J)[3][3], double (&I)[3][3]) {
  if (DIM == 2) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    I[0][0] = J[1][1] / det;
    I[0][1] = -J[0][1] / det;
    I[1][0] = -J[1][0] / det;
    I[1][1] = J[0][0] / det;
    return det;
  }
  const double det = J[0][0] * J[1][1] * J[2][2] - J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] +
                     J[0][1] * J[1][2] * J[2][0] + J[0][2] * J[1][0] * J[2][1] - J[0][2] * J[1][1] * J[2][0];
  I[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) / det;
  I[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
  I[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) / det;
  I[1][0] = (J[1][2] * J[2][0] - J[2][2] * J[1][0]) / det;
  I[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
  I[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
  I[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) / det;
  I[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) / det;
  I[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) / det;
  return det;
}

// Phase 1 (lane <-> q): Ji[q][m * DIM + s] = J^-1, wd[q] = w_q det (facets: w_q * surface det), and for facets with nrm != nullptr
// nrm[q * DIM + i] = the outward unit normal, the expressions of mfem_update_basic_boundary.  R: the item's reference table, X: [itp][DIM]
// node coordinates, f: local face id (facets).  nq = itg, or 0 to skip the phase (ablation).  split_j: two lane groups share a point's
// Jacobian sum, half the nodes each (2 * itg <= 64).
template <int DIM>
__device__ __forceinline__ void mg_geometry(const MeshItems& V, const double* R, const double* X, int f, int lane, int nq, bool split_j,
                                            double* Ji, double* wd, double* nrm) {
  const int itg = V.itg, itp = V.itp;
  for (int q0 = 0; q0 < nq; q0 += 64) {
    const int hq = split_j ? lane / itg : 0, q = split_j ? lane - hq * itg : q0 + lane;
    const int half = split_j ? (itp + 1) >> 1 : itp;
    const int a_lo = hq < 2 ? hq * half : 0, a_hi = hq < 2 ? (a_lo + half < itp ? a_lo + half : itp) : 0;
    const bool qon = q < itg;
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = a_lo; a < a_hi; ++a) {
#pragma unroll
      for (int m = 0; m < DIM; ++m) {
        const double r = R[(qon ? q : 0) + itg * (a + itp * (1 + m))];
#pragma unroll
        for (int i = 0; i < DIM; ++i) J[i][m] += r * X[a * DIM + i];
      }
    }
    if (split_j) {
#pragma unroll
      for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int m = 0; m < DIM; ++m) J[i][m] += __shfl_down(J[i][m], itg);  // (group 0 takes group 1's half)
    }
    if (!qon || hq != 0) continue;
    double I[3][3];
    const double det = ma_inv<DIM>(J, I);
#pragma unroll
    for (int m = 0; m < DIM; ++m)
#pragma unroll
      for (int s = 0; s < DIM; ++s) Ji[q * DIM * DIM + m * DIM + s] = I[m][s];
    if (!V.eindex) {
      wd[q] = V.wq[q] * det;
    } else {  // surface weight: |J t1 x J t2| (3-D) or |J t1| (2-D)   4_Update_Integrator.jl:163-227
      const double* Tn = V.tan + (int64_t)f * V.tan_stride;
      double tg[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
      for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int k = 0; k < DIM - 1; ++k)
#pragma unroll
          for (int m = 0; m < DIM; ++m) tg[i][k] += J[i][m] * Tn[q + itg * (m + DIM * k)];
      double ld;
      if (DIM == 2) {
        ld = sqrt(tg[0][0] * tg[0][0] + tg[1][0] * tg[1][0]);
        if (nrm) {
          nrm[q * DIM + 0] = tg[1][0] / ld;
          nrm[q * DIM + 1] = -tg[0][0] / ld;
        }
      } else {
        const double r0 = tg[1][0] * tg[2][1] - tg[2][0] * tg[1][1];
        const double r1 = -tg[0][0] * tg[2][1] + tg[2][0] * tg[0][1];
        const double r2 = tg[0][0] * tg[1][1] - tg[1][0] * tg[0][1];
        ld = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
        if (nrm) {
          nrm[q * DIM + 0] = r0 / ld;
          nrm[q * DIM + 1] = r1 / ld;
          nrm[q * DIM + DIM - 1] = r2 / ld;
        }
      }
      wd[q] = V.wq[(int64_t)f * V.w_stride + q] * ld;
    }
  }
}

// Phase 2 (lane <-> (q, a)): Tt[(q * itp + a) * NS + s - S0], the slots S0 .. S0 + NS - 1 of the physical table.  n = itg * itp, or 0 to skip.
template <int DIM, int S0, int NS>
__device__ __forceinline__ void mg_table(const double* R, const double* Ji, double* Tt, int itg, int itp, int lane, int n) {
  for (int i = lane; i < n; i += 64) {
    const int q = i % itg, a = i / itg;
    double* o = Tt + ((size_t)q * itp + a) * NS;
    if (S0 == 0) o[0] = R[q + itg * a];
    if (NS > 1 || S0 == 1) {
      double r[3];
#pragma unroll
      for (int m = 0; m < DIM; ++m) r[m] = R[q + itg * (a + itp * (1 + m))];
#pragma unroll
      for (int s = 0; s < DIM; ++s) {
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < DIM; ++m) v += r[m] * Ji[q * DIM * DIM + m * DIM + s];
        o[(1 - S0) + s] = v;
      }
    }
  }
}

// ---- pass 2 of the row-owner forms (assemble_mesh.hip: k_mesh_gather / k_mesh_gather_nodes), shared with mesh_ops.hip ------------------------
#define MG_MAXROW 2048  // longest CSR row the gather stages in LDS
// element-matrix scratch the row-owner form may take from the context workspace (288 GB of HBM: hex-20 elasticity at 128^3 needs 60 GB)
static const size_t MG_SCRATCH_BUDGET = (size_t)96 << 30;
struct GatherBlocks {
  int nf;          // fields
  int nb;          // blocks in the scratch (runs of the term list)
  int cnt[4];      // blocks with dual field fd
  int k[4][4];     // their scratch index
  int fb[4][4];    // their base field
};
// adds (overwrite: sets) the element-major scratch S[((el * itp + a) * nb + k) * itp + b] into the rows of K_val; the launch lives with the kernels
int mfem_mesh_gather_launch(mfem_context_s* ctx, int itp, int64_t ncp, const GatherBlocks& B, mfem_csr_s* A, const int64_t* adj_ptr,
                            const int32_t* adj, const uint16_t* ranks, const double* S, double* K_val, int overwrite);
