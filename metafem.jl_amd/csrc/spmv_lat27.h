// What the two files of solver layout mode 4 share (spmv_lat27.hip: tables, layout passes, pass 1, plan / bind / launch; spmv_lat27_gather.hip: pass 2
// and the fused CG update): the shape of a tile's LDS blocks, where a lattice point sits in x, the reach of a row.  The tile sizes and the geometry
// record: lat_decide.h.
#pragma once
#include "common.h"
#include "krylov.h"  // LatCgUpdate, the scalar / flag slots of the Krylov loop (the fused CG update)

#define L27_PI (L27_SJ * L27_SK + 8)  // plane stride of the LDS blocks: 440 = 8 mod 16, so the 16 rows of a step (2 a PI + 2 b SK + 2 c) fall on 16 different bank pairs
#define L27_LDS_CELLS ((L27_TI + 2) * L27_PI)

// local x index at GLOBAL plane gi (owned or ghost), in-plane position ip
__device__ __forceinline__ int64_t l27_xindex(const Lat27Geom& G, int gi, int64_t ip) {
  const int64_t PL = (int64_t)G.m1 * G.m2;
  if (gi >= G.plo && gi < G.plo + G.m0) return (int64_t)(gi - G.plo) * PL + ip;
  const int side = gi < G.plo ? 0 : 1;
  const int off = side ? gi - (G.plo + G.m0) : gi - (G.plo - G.gw);
  return G.n + ((int64_t)side * G.gw + off) * PL + ip;
}

// offsets a row at lattice coordinate g (of m points) has along one direction: [lo, lo + cnt)
__device__ __forceinline__ void l27_range(int g, int m, int& lo, int& cnt) {
  if (g & 1) {
    lo = -1;
    cnt = 3;
  } else {
    lo = g >= 2 ? -2 : -g;
    const int hi = (m - 1 - g) >= 2 ? 2 : (m - 1 - g);
    cnt = hi - lo + 1;
  }
}

// Pass 2 of a product on the bound tiles of A: y = alpha * (the tiles' blocks summed) + beta * y, partial sums of y . dotw; *grid = its workgroups.
// staged: k_lat27_gather_st, else k_lat27_gather.
int mfem_lat27_gather_launch(mfem_context_s* ctx, const mfem_csr_s* A, const Lat27Geom& G, bool staged, const double* x, double* y, double alpha,
                             double beta, const double* dotw, double* partials, const int32_t* done_flag, int* grid);
