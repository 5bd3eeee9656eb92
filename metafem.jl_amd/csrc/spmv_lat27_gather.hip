// Pass 2 of solver layout mode 4 (spmv_lat27.hip): the plain gather, the staged gather (the default) and the staged gather that ends in the residual
// update of a CG iteration.  The three kernels are written out in full: sharing the staging, the covering-block sums or the ghost-plane block between
// them through inlined helpers changed their instructions (the staged ones lose 100 of 3 100), and identical kernels outrank shorter source.
#include "blas1.h"
#include "spmv_lat27.h"

// the sums s of the column (gj, gk) of the tile layer at plane gi0 into y: the alpha / beta / dot epilogue of the two SpMV gathers
__device__ __forceinline__ void l27_store_rows(Lat27Geom G, const double (&s)[L27_TI], int gi0, int gj, int gk, double alpha, double beta,
                                               double* y, const double* dotw, double& dot_acc) {
#pragma unroll
  for (int u = 0; u < L27_TI; ++u) {
    if (gi0 + u < G.m0) {
      const int64_t r = ((int64_t)(gi0 + u) * G.m1 + gj) * G.m2 + gk;
      double yv = alpha * s[u];
      if (beta != 0.0) yv += beta * y[r];
      y[r] = yv;
      if (dotw) dot_acc += yv * dotw[r];
    }
  }
}

// pass 2: y[r] = alpha * (sum over the tiles whose block covers r, fixed order) + beta * y[r]; fused dot with dotw.  A thread owns a
// (j, k) position of the tile and its 8 lattice planes: 8 independent loads per covering tile.
// Slab with a lower neighbour (G.plo > 0): the rows of the first owned plane (an even plane: reach 2) also have entries towards the two ghost planes
// below.  No stored entry mirrors onto them (the rows that would belong to the neighbour rank), so they are taken from the caller's CSR values here.
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_lat27_gather(Lat27Geom G, const double* __restrict__ dump, double* __restrict__ y,
                                                               double alpha, double beta, const double* __restrict__ dotw,
                                                               double* __restrict__ partials, const int32_t* __restrict__ done_flag,
                                                               const RP* __restrict__ rowptr, int base, const double* __restrict__ csr_vals,
                                                               const double* __restrict__ x, const double* __restrict__ dsc) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int ntiles = G.nti * G.ntj * G.ntk;
  const int lk = threadIdx.x & (L27_TK - 1), lj = threadIdx.x >> 5;
  const int PC = L27_SJ * L27_SK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tk = tile % G.ntk, t2 = tile / G.ntk, tj = t2 % G.ntj, ti = t2 / G.ntj;
    const int gj = tj * L27_TJ + lj, gk = tk * L27_TK + lk, gi0 = ti * L27_TI;
    if (gj >= G.m1 || gk >= G.m2) continue;
    double s[L27_TI];
#pragma unroll
    for (int u = 0; u < L27_TI; ++u) s[u] = 0.0;
    // covering tiles (ti + a, tj + b, tk + c), a in {-1, 0}, b, c in {-1, 0, 1}, in this fixed order: the row's cell must exist in that tile's block
    for (int b = -1; b <= 1; ++b) {
      if ((b < 0 && (lj >= 2 || tj == 0)) || (b > 0 && (lj < L27_TJ - 2 || tj == G.ntj - 1))) continue;
      for (int c = -1; c <= 1; ++c) {
        if ((c < 0 && (lk >= 2 || tk == 0)) || (c > 0 && (lk < L27_TK - 2 || tk == G.ntk - 1))) continue;
        const int cell = (lj - L27_TJ * b + 2) * L27_SK + (lk - L27_TK * c + 2);
        if (ti > 0) {  // the tile below: its planes 8, 9 are this tile's 0, 1
          const double* d = dump + (((int64_t)(ti - 1) * G.ntj + (tj + b)) * G.ntk + (tk + c)) * L27_CELLS + cell;
          s[0] += d[8 * PC];
          s[1] += d[9 * PC];
        }
        const double* d = dump + (((int64_t)ti * G.ntj + (tj + b)) * G.ntk + (tk + c)) * L27_CELLS + cell;
#pragma unroll
        for (int u = 0; u < L27_TI; ++u) s[u] += d[u * PC];
      }
    }
    if (G.plo > 0 && ti == 0) {  // the lower ghost planes (see above): the first two of the row's five i-offsets
      int l1, n1, l2, n2;
      l27_range(gj, G.m1, l1, n1);
      l27_range(gk, G.m2, l2, n2);
      const int64_t rp = (int64_t)rowptr[(int64_t)gj * G.m2 + gk] - base;
      double acc = 0.0;
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < n1; ++b)
          for (int c = 0; c < n2; ++c) {
            const int64_t xi = l27_xindex(G, G.plo - 2 + a, (int64_t)(gj + l1 + b) * G.m2 + gk + l2 + c);
            acc += csr_vals[rp + ((int64_t)a * n1 + b) * n2 + c] * (dsc ? x[xi] / dsc[xi] : x[xi]);
          }
      s[0] += acc;
    }
    l27_store_rows(G, s, gi0, gj, gk, alpha, beta, y, dotw, dot_acc);
  }
  if (partials) {
    const double bsum = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = bsum;
  }
}

// pass 2, staged (round 4): the same sums in the same order, but every global load of a tile is in flight at once.  The kernel above walks the up to 18
// covering blocks of a row in masked code blocks, one memory round trip each (every wave holds lanes on the tile's k rim, so every wave takes at least
// three, the waves on the j rim nine: 3.1 TB/s).  Here the workgroup first copies the 4 320 (row, covering block) values of its tile -- the extended box
// (8 + 2 planes) x (8 + 2 + 2 lines) x (32 + 2 + 2 columns): own cells, the cells the tile below / beside / diagonal to it holds for these rows -- into
// LDS, 17 independent loads per thread, and the row owners then add them from LDS in the order of the kernel above (bitwise the same y).
// Measured (tools/gather_ab.py, C4): 1 % off a 200-iteration solve -- the round trips were not what bounds pass 2 (a 0.18 ms kernel of 0.56 GB).
#define L27_EJ (L27_TJ + 4)
#define L27_EK (L27_TK + 4)
#define L27_ECELLS ((L27_TI + 2) * L27_EJ * L27_EK)  // 4320
#define L27_EU ((L27_ECELLS + MFEM_BLOCK - 1) / MFEM_BLOCK)
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_lat27_gather_st(Lat27Geom G, const double* __restrict__ dump, double* __restrict__ y,
                                                                  double alpha, double beta, const double* __restrict__ dotw,
                                                                  double* __restrict__ partials, const int32_t* __restrict__ done_flag,
                                                                  const RP* __restrict__ rowptr, int base, const double* __restrict__ csr_vals,
                                                                  const double* __restrict__ x, const double* __restrict__ dsc) {
  __shared__ double E[L27_ECELLS];
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int ntiles = G.nti * G.ntj * G.ntk;
  const int lk = threadIdx.x & (L27_TK - 1), lj = threadIdx.x >> 5;
  const int PC = L27_SJ * L27_SK;
  // extended line / column e -> (neighbour offset, line or column of this tile): 0 .. T - 1 own; T, T + 1: the block below / before holds rows 0, 1;
  // T + 2, T + 3: the block after holds rows T - 2, T - 1
  auto ext = [](int e, int T, int& off, int& l) {
    if (e < T) { off = 0; l = e; }
    else if (e < T + 2) { off = -1; l = e - T; }
    else { off = 1; l = e - 4; }
  };
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (the trip count is the workgroup's: every barrier below is reached by all threads)
    const int tk = tile % G.ntk, t2 = tile / G.ntk, tj = t2 % G.ntj, ti = t2 / G.ntj;
    double t[L27_EU];
#pragma unroll
    for (int u = 0; u < L27_EU; ++u) {
      const int e = threadIdx.x + u * MFEM_BLOCK;
      t[u] = 0.0;
      if (e < L27_ECELLS) {
        const int ei = e / (L27_EJ * L27_EK), r2 = e - ei * (L27_EJ * L27_EK), ej = r2 / L27_EK, ek = r2 - ej * L27_EK;
        int b, c, sj, sk;
        ext(ej, L27_TJ, b, sj);
        ext(ek, L27_TK, c, sk);
        const int a = ei < L27_TI ? 0 : -1;  // (planes 8, 9 of the block below are this tile's planes 0, 1: the block's plane index is ei either way)
        const bool ok = (a == 0 || ti > 0) && (b == 0 || (b < 0 ? tj > 0 : tj < G.ntj - 1)) && (c == 0 || (c < 0 ? tk > 0 : tk < G.ntk - 1));
        if (ok)
          t[u] = __builtin_nontemporal_load(dump + (((int64_t)(ti + a) * G.ntj + (tj + b)) * G.ntk + (tk + c)) * L27_CELLS + ei * PC +
                                            (sj - L27_TJ * b + 2) * L27_SK + (sk - L27_TK * c + 2));
      }
    }
#pragma unroll
    for (int u = 0; u < L27_EU; ++u) {
      const int e = threadIdx.x + u * MFEM_BLOCK;
      if (e < L27_ECELLS) E[e] = t[u];
    }
    __syncthreads();
    const int gj = tj * L27_TJ + lj, gk = tk * L27_TK + lk, gi0 = ti * L27_TI;
    if (gj < G.m1 && gk < G.m2) {
      double s[L27_TI];
#pragma unroll
      for (int u = 0; u < L27_TI; ++u) s[u] = 0.0;
      for (int b = -1; b <= 1; ++b) {
        if ((b < 0 && (lj >= 2 || tj == 0)) || (b > 0 && (lj < L27_TJ - 2 || tj == G.ntj - 1))) continue;
        const int ej = b == 0 ? lj : b < 0 ? L27_TJ + lj : lj + 4;
        for (int c = -1; c <= 1; ++c) {
          if ((c < 0 && (lk >= 2 || tk == 0)) || (c > 0 && (lk < L27_TK - 2 || tk == G.ntk - 1))) continue;
          const int ek = c == 0 ? lk : c < 0 ? L27_TK + lk : lk + 4;
          const double* d = E + ej * L27_EK + ek;
          if (ti > 0) {
            s[0] += d[8 * (L27_EJ * L27_EK)];
            s[1] += d[9 * (L27_EJ * L27_EK)];
          }
#pragma unroll
          for (int u = 0; u < L27_TI; ++u) s[u] += d[u * (L27_EJ * L27_EK)];
        }
      }
      if (G.plo > 0 && ti == 0) {  // the lower ghost planes (see k_lat27_gather): the first two of the row's five i-offsets
        int l1, n1, l2, n2;
        l27_range(gj, G.m1, l1, n1);
        l27_range(gk, G.m2, l2, n2);
        const int64_t rp = (int64_t)rowptr[(int64_t)gj * G.m2 + gk] - base;
        double acc = 0.0;
        for (int a = 0; a < 2; ++a)
          for (int b = 0; b < n1; ++b)
            for (int c = 0; c < n2; ++c) {
              const int64_t xi = l27_xindex(G, G.plo - 2 + a, (int64_t)(gj + l1 + b) * G.m2 + gk + l2 + c);
              acc += csr_vals[rp + ((int64_t)a * n1 + b) * n2 + c] * (dsc ? x[xi] / dsc[xi] : x[xi]);
            }
        s[0] += acc;
      }
      l27_store_rows(G, s, gi0, gj, gk, alpha, beta, y, dotw, dot_acc);
    }
    __syncthreads();  // the staged values are consumed: the next tile's may land
  }
  if (partials) {
    const double bsum = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = bsum;
  }
}

// The fused CG iteration on the lattice tiles (one rank): pass 2 and the residual update of Jacobi-CG in one kernel.  q = A p is needed twice in a CG iteration --
// in p . q, which pass 1 now delivers (k_spmv_lat27: dotp), and in r -= alpha q -- so the sums over the covering blocks are formed here, used and never stored:
// no y written and read back, no separate gather launch (3 of the iteration's vector streams and one launch less).  Staging and summation order are
// k_lat27_gather_st's; the update arithmetic is k_cg_update's (krylov_cg.hip), operation for operation.
__global__ __launch_bounds__(MFEM_BLOCK) void k_lat27_gather_cg(Lat27Geom G, const double* __restrict__ dump, LatCgUpdate U) {
  __shared__ double E[L27_ECELLS];
  __shared__ double red[4];
  if (U.flags[F_DONE]) return;
  const double pap = U.np > 0 ? reduce_partials_bcast(U.pap_partials, U.np, red) : U.S[S_PAP];  // (as k_cg_update / k_cg_pupdate: every workgroup folds the partials itself)
  const double alpha = U.S[S_RZ0 + U.cur] / pap;
  const bool exact = U.sw && U.S[S_RR] * U.n_inv <= U.gate2;
  double rz = 0.0, rr = 0.0;
  const int ntiles = G.nti * G.ntj * G.ntk;
  const int lk = threadIdx.x & (L27_TK - 1), lj = threadIdx.x >> 5;
  const int PC = L27_SJ * L27_SK;
  auto ext = [](int e, int T, int& off, int& l) {
    if (e < T) { off = 0; l = e; }
    else if (e < T + 2) { off = -1; l = e - T; }
    else { off = 1; l = e - 4; }
  };
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (the trip count is the workgroup's: every barrier below is reached by all threads)
    const int tk = tile % G.ntk, t2 = tile / G.ntk, tj = t2 % G.ntj, ti = t2 / G.ntj;
    double t[L27_EU];
#pragma unroll
    for (int u = 0; u < L27_EU; ++u) {
      const int e = threadIdx.x + u * MFEM_BLOCK;
      t[u] = 0.0;
      if (e < L27_ECELLS) {
        const int ei = e / (L27_EJ * L27_EK), r2 = e - ei * (L27_EJ * L27_EK), ej = r2 / L27_EK, ek = r2 - ej * L27_EK;
        int b, c, sj, sk;
        ext(ej, L27_TJ, b, sj);
        ext(ek, L27_TK, c, sk);
        const int a = ei < L27_TI ? 0 : -1;
        const bool ok = (a == 0 || ti > 0) && (b == 0 || (b < 0 ? tj > 0 : tj < G.ntj - 1)) && (c == 0 || (c < 0 ? tk > 0 : tk < G.ntk - 1));
        if (ok)
          t[u] = __builtin_nontemporal_load(dump + (((int64_t)(ti + a) * G.ntj + (tj + b)) * G.ntk + (tk + c)) * L27_CELLS + ei * PC +
                                            (sj - L27_TJ * b + 2) * L27_SK + (sk - L27_TK * c + 2));
      }
    }
#pragma unroll
    for (int u = 0; u < L27_EU; ++u) {
      const int e = threadIdx.x + u * MFEM_BLOCK;
      if (e < L27_ECELLS) E[e] = t[u];
    }
    __syncthreads();
    const int gj = tj * L27_TJ + lj, gk = tk * L27_TK + lk, gi0 = ti * L27_TI;
    if (gj < G.m1 && gk < G.m2) {
      double s[L27_TI];
#pragma unroll
      for (int u = 0; u < L27_TI; ++u) s[u] = 0.0;
      for (int b = -1; b <= 1; ++b) {
        if ((b < 0 && (lj >= 2 || tj == 0)) || (b > 0 && (lj < L27_TJ - 2 || tj == G.ntj - 1))) continue;
        const int ej = b == 0 ? lj : b < 0 ? L27_TJ + lj : lj + 4;
        for (int c = -1; c <= 1; ++c) {
          if ((c < 0 && (lk >= 2 || tk == 0)) || (c > 0 && (lk < L27_TK - 2 || tk == G.ntk - 1))) continue;
          const int ek = c == 0 ? lk : c < 0 ? L27_TK + lk : lk + 4;
          const double* d = E + ej * L27_EK + ek;
          if (ti > 0) {
            s[0] += d[8 * (L27_EJ * L27_EK)];
            s[1] += d[9 * (L27_EJ * L27_EK)];
          }
#pragma unroll
          for (int u = 0; u < L27_TI; ++u) s[u] += d[u * (L27_EJ * L27_EK)];
        }
      }
#pragma unroll
      for (int u = 0; u < L27_TI; ++u) {
        if (gi0 + u < G.m0) {
          const int64_t i = ((int64_t)(gi0 + u) * G.m1 + gj) * G.m2 + gk;
          const double av = s[u];  // (A p)[i]
          double rv, z;
          if (U.zrec && U.dinv) {  // the array holds z: z -= alpha dinv .* Ap ; r = z ./ dinv for the two dot products only
            const double dv = U.dinv[i];
            z = U.r[i] - alpha * (av * dv);
            U.r[i] = z;
            rv = dv != 0.0 ? z * mfem_recip_nr(dv) : 0.0;
          } else {
            rv = U.r[i] - alpha * av;
            U.r[i] = rv;
            z = U.dinv ? rv * U.dinv[i] : rv;
          }
          rz += rv * z;
          if (exact) {
            const double tt = U.sw[i] * rv;
            rr += tt * tt;
          } else {
            rr += rv * rv;
          }
        }
      }
    }
    __syncthreads();  // the staged values are consumed: the next tile's may land
  }
  const double s0 = block_reduce_sum(rz, red);
  const double s1 = block_reduce_sum(rr, red);
  if (threadIdx.x == 0) {
    U.partials2[blockIdx.x] = s0;
    U.partials2[gridDim.x + blockIdx.x] = (U.sw && !exact) ? s1 * U.smax2 : s1;
  }
}

// persistent grid = what is resident (the staged gather holds 3 workgroups per CU at 145 VGPRs, the plain one 6: both were launched with 8)
int mfem_lat27_gather_launch(mfem_context_s* ctx, const mfem_csr_s* A, const Lat27Geom& G, bool staged, const double* x, double* y, double alpha,
                             double beta, const double* dotw, double* partials, const int32_t* done_flag, int* grid) {
  return mfem_by_rowptr(A, [&](auto w) -> int {
    using RP = decltype(w);
    auto kernel = staged ? &k_lat27_gather_st<RP> : &k_lat27_gather<RP>;
    *grid = lat_gather_grid(ctx->num_cus, mfem_resident_per_cu(reinterpret_cast<const void*>(kernel), MFEM_BLOCK, 0, 3), G.nti * G.ntj * G.ntk);
    hipLaunchKernelGGL(kernel, dim3(*grid), dim3(MFEM_BLOCK), 0, ctx->stream, G, (const double*)A->lat27.dump, y, alpha, beta, dotw, partials, done_flag,
                       (const RP*)A->rowptr, A->index_base, A->lat27.src, x, A->lat27.dsc);
    MFEM_CHECK_LAUNCH();
    return MFEM_OK;
  });
}

int mfem_lat27_gather_cg_update(mfem_context_s* ctx, mfem_csr_s* A, const LatCgUpdate& U, int grid) {
  const Lat27Geom G = lat27_geom(mfem_lat_shape(A, 0));
  hipLaunchKernelGGL(k_lat27_gather_cg, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, G, (const double*)A->lat27.dump, U);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
