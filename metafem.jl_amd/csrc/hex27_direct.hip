#include "hex27.h"

// ---- Affine meshes (round 4): the matrix without Ke ever being stored.  On an element whose 27 nodes are an affine image of the reference nodes the Jacobian is
// one matrix and Ke = sum_t G0_t S_t -- six numbers per element (G0 = -k adj(J) adj(J)^T / det, as in k_hex27's affine branch) times six 27 x 27 reference
// integrals (products of the 1-D integrals Hex27Tables::T1, summed with the same quadrature).  When EVERY element of the launch is affine (each make_Brick mesh until a caller moves coordinates;
// tested per assembly on the coordinates themselves, k_hex27_affine_g0), the row-owner gather below computes each (row, element) run from G0 and the table instead of
// reading it from the element-major scratch: no pass 1, no 12.2 GB scratch written and read back (128^3: 10.5 -> 3 ms for the matrix).  Any non-affine element sends
// the whole assembly through the two-pass MFMA path (k_hex27, hex27_gather.hip).
// slot (optional): per element -1 (affine) or its place k in the compact scratch of the non-affine elements' Ke; elist[k] = the element's index
// (the places are handed out by an atomic counter: which element gets which place varies from run to run, what is stored there does not)
__global__ __launch_bounds__(MFEM_BLOCK) void k_hex27_affine_g0(BrickView B, double kcond, int elo, int ecnt, double* __restrict__ g,
                                                                int32_t* __restrict__ nonaffine, int32_t* __restrict__ slot,
                                                                int32_t* __restrict__ elist) {
  const int64_t nel = (int64_t)ecnt * B.ne1 * B.ne2;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nel) return;
  const int K = (int)(idx % B.ne2), J = (int)((idx / B.ne2) % B.ne1), I = elo + (int)(idx / ((int64_t)B.ne1 * B.ne2));
  auto node = [&](int a, double& x, double& y, double& z) {
    const int64_t c = brick_cindex(B, 2 * I + a % 3, 2 * J + (a / 3) % 3, 2 * K + a / 9);
    x = B.X0[c]; y = B.X1[c]; z = B.X2[c];
  };
  double x0, y0, z0, ex0, ey0, ez0, ex1, ey1, ez1, ex2, ey2, ez2;
  node(0, x0, y0, z0);
  node(2, ex0, ey0, ez0);
  node(6, ex1, ey1, ez1);
  node(18, ex2, ey2, ez2);
  ex0 -= x0; ey0 -= y0; ez0 -= z0; ex1 -= x0; ey1 -= y0; ez1 -= z0; ex2 -= x0; ey2 -= y0; ez2 -= z0;
  const double tol = 3.6e-15;  // (the test of k_hex27: 16 ulp of the coordinates' magnitude, per component)
  const double tx = tol * (fabs(x0) + fabs(ex0) + fabs(ex1) + fabs(ex2)), ty = tol * (fabs(y0) + fabs(ey0) + fabs(ey1) + fabs(ey2)),
               tz = tol * (fabs(z0) + fabs(ez0) + fabs(ez1) + fabs(ez2));
  bool affine = true;
  for (int a = 0; a < 27; ++a) {
    double mx, my, mz;
    node(a, mx, my, mz);
    const double a0 = 0.5 * (a % 3), a1 = 0.5 * ((a / 3) % 3), a2 = 0.5 * (a / 9);
    const double px = x0 + a0 * ex0 + a1 * ex1 + a2 * ex2, py = y0 + a0 * ey0 + a1 * ey1 + a2 * ey2, pz = z0 + a0 * ez0 + a1 * ez1 + a2 * ez2;
    affine = affine && fabs(mx - px) <= tx && fabs(my - py) <= ty && fabs(mz - pz) <= tz;
  }
  double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0, g5 = 0.0;
  if (affine) {
    const double j00 = ex0, j01 = ex1, j02 = ex2, j10 = ey0, j11 = ey1, j12 = ey2, j20 = ez0, j21 = ez1, j22 = ez2;
    const double det = j00 * j11 * j22 - j00 * j12 * j21 - j01 * j10 * j22 + j01 * j12 * j20 + j02 * j10 * j21 - j02 * j11 * j20;
    const double c00 = j11 * j22 - j12 * j21, c01 = j02 * j21 - j01 * j22, c02 = j01 * j12 - j11 * j02;
    const double c10 = j12 * j20 - j22 * j10, c11 = j00 * j22 - j02 * j20, c12 = j02 * j10 - j00 * j12;
    const double c20 = j10 * j21 - j11 * j20, c21 = j01 * j20 - j21 * j00, c22 = j00 * j11 - j10 * j01;
    const double sc0 = -kcond / det;
    g0 = sc0 * (c00 * c00 + c01 * c01 + c02 * c02); g1 = sc0 * (c00 * c10 + c01 * c11 + c02 * c12);
    g2 = sc0 * (c00 * c20 + c01 * c21 + c02 * c22); g3 = sc0 * (c10 * c10 + c11 * c11 + c12 * c12);
    g4 = sc0 * (c10 * c20 + c11 * c21 + c12 * c22); g5 = sc0 * (c20 * c20 + c21 * c21 + c22 * c22);
    if (slot) slot[idx] = -1;
  } else {
    const int k = atomicAdd(nonaffine, 1);
    if (slot) {
      slot[idx] = k;
      elist[k] = (int32_t)idx;
    }
  }
  double* ge = g + idx * 6;
  ge[0] = g0; ge[1] = g1; ge[2] = g2; ge[3] = g3; ge[4] = g4; ge[5] = g5;
}

// The row-owner gather of k_hex27_gather_lds with the runs computed in place.  A wave owns 8 consecutive control points per trip; thread (row, e) takes the row's
// e-th candidate element (3.4 of 8 exist on average) and computes ITS 27-entry run Ke_e[la][0..26] from registers: G0 (6 numbers) and the twelve
// 3-entry rows of the 1-D integrals that belong to its local node la = (a0, a1, a2) -- the reference integrals factor per direction,
//   Ke[la][lb] = M2 P + D2 Q + Ct2 R + C2 T,  P = g0 D0 M1 + g1 (C0 Ct1 + Ct0 C1) + g3 M0 D1,  Q = g5 M0 M1,  R = g2 C0 M1 + g4 C1 M0,  T = g2 Ct0 M1 + g4 Ct1 M0
// (X_d = the 1-D integral X at (a_d, b_d); D = l'l', M = ll, C = l'l, Ct = ll') -- and adds it into the row's box in LDS (ds_add_f64: the threads of one instruction hold
// different (row, element) pairs and the same local node b, i.e. different entries).  36 LDS reads + 27 additions per run; a first version with one lane per entry
// and the 27 x 27 x 6 table in LDS (12 reads per entry) was bound by LDS bandwidth at 6.5 ms (128^3).  The additions into one entry come in program order: the
// result is reproducible (and differs from the two-pass path's in the last bits: another summation order).
#define D27_TAB 1024  // lattice planes + lines + points whose row-box tables (lo, c, P per direction) are kept in LDS (16 bytes each); beyond: read from memory
#define D27_LDS_BYTES (sizeof(double) * (48 + D27_NODES * G27_ROW + D27_TAB) + sizeof(int32_t) * (2 * D27_TAB))
// Mixed meshes (round 5): slot_of != nullptr -- element idx is affine where slot_of[idx] < 0 (computed in place, as above) and otherwise has its Ke in the
// compact scratch `ke` at slot_of[idx] (pass 1 ran for those elements only, k_hex27<true, true> in list mode): their runs Ke[la][0..26] are streamed in by the
// half-waves exactly as in k_hex27_gather_lds (one contiguous 216-byte read per run) after the wave's in-place runs have been added.  One distorted element no
// longer sends the whole mesh through the two-pass path: the assembly costs what its affine part costs plus pass 1 + the streamed runs of the rest.
#define D27_FLIGHT 8
__global__ __launch_bounds__(D27_THREADS, 4) void k_hex27_direct(BrickView B, const Hex27Tables* __restrict__ tab, const double* __restrict__ g,
                                                              double* __restrict__ vals, int64_t row_lo, int64_t row_hi, int elo,
                                                              const int32_t* __restrict__ slot_of, const double* __restrict__ ke) {
  extern __shared__ double lds[];
  double* sT = lds;                          // [4][3][4]
  double* rows = sT + 48;                    // [D27_NODES][G27_ROW]
  int64_t* t_P = reinterpret_cast<int64_t*>(rows + D27_NODES * G27_ROW);  // [D27_TAB]: P0 | P1 | P2
  int32_t* t_lo = reinterpret_cast<int32_t*>(t_P + D27_TAB);              // [D27_TAB]: lo0 | lo1 | lo2
  int32_t* t_c = t_lo + D27_TAB;             // [D27_TAB]: c0 | c1 | c2
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < 48) sT[tid] = (&tab->T1[0][0][0])[tid];
  // the row-box tables: phase A below looks a control point's box up per direction (a chain of dependent loads when they come from memory)
  const bool tabs = B.m0 + B.m1 + B.m2 <= D27_TAB;
  const int32_t *lo0 = B.lo0, *lo1 = B.lo1, *lo2 = B.lo2, *c0 = B.c0, *c1p = B.c1, *c2p = B.c2;
  const int64_t *P0 = B.P0, *P1 = B.P1, *P2 = B.P2;
  if (tabs) {
    for (int i = tid; i < B.m0; i += D27_THREADS) { t_lo[i] = B.lo0[i]; t_c[i] = B.c0[i]; t_P[i] = B.P0[i]; }
    for (int i = tid; i < B.m1; i += D27_THREADS) { t_lo[B.m0 + i] = B.lo1[i]; t_c[B.m0 + i] = B.c1[i]; t_P[B.m0 + i] = B.P1[i]; }
    for (int i = tid; i < B.m2; i += D27_THREADS) { t_lo[B.m0 + B.m1 + i] = B.lo2[i]; t_c[B.m0 + B.m1 + i] = B.c2[i]; t_P[B.m0 + B.m1 + i] = B.P2[i]; }
    lo0 = t_lo; lo1 = t_lo + B.m0; lo2 = t_lo + B.m0 + B.m1;
    c0 = t_c; c1p = t_c + B.m0; c2p = t_c + B.m0 + B.m1;
    P0 = t_P; P1 = t_P + B.m0; P2 = t_P + B.m0 + B.m1;
  }
  __syncthreads();  // (the only workgroup barrier: from here on the waves never exchange data)
  const int64_t nblk = (row_hi - row_lo + D27_NODES - 1) / D27_NODES;
  // Phase A of a block, per thread (row nl = tid / 8, candidate element e = tid % 8): the row's box, the element, its G0 -- in registers
  struct PairPre {
    int64_t pre;
    int32_t len, c1, c2, la, b0;
    bool valid;
    double g[6];
    int32_t slot;  // >= 0: the element's place in the compact scratch (non-affine), < 0: computed in place
  };
  auto phase_a = [&](int64_t blk) -> PairPre {
    PairPre P{0, 0, 1, 1, 0, 0, false, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, -1};
    const int nl = tid >> 3, e = tid & 7;
    const int64_t row = row_lo + blk * D27_NODES + nl;
    if (row >= row_hi) return P;
    const uint32_t r32 = (uint32_t)row, pl = (uint32_t)B.plane_len, m2 = (uint32_t)B.m2;  // control-point ids fit int32
    const uint32_t q0 = r32 / pl, rem = r32 - q0 * pl, q1 = rem / m2;
    const int gg[3] = {(int)q0 + B.plo, (int)q1, (int)(rem - q1 * m2)};
    const int l0 = lo0[gg[0]], l1 = lo1[gg[1]], l2 = lo2[gg[2]];
    P.c1 = c1p[gg[1]];
    P.c2 = c2p[gg[2]];
    const int cc0 = c0[gg[0]];
    P.pre = (P0[gg[0]] - B.Pplo) * B.S1 * B.S2 + (int64_t)cc0 * (P1[gg[1]] * B.S2 + (int64_t)P.c1 * P2[gg[2]]);  // (brick_prefix)
    P.len = cc0 * P.c1 * P.c2;
    const int ed[3] = {e & 1, (e >> 1) & 1, e >> 2};
    const int ne[3] = {B.ne0, B.ne1, B.ne2};
    int E[3];
    bool valid = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (gg[d] & 1) {
        E[d] = (gg[d] - 1) >> 1;
        valid = valid && ed[d] == 0;
      } else {
        E[d] = (gg[d] >> 1) - 1 + ed[d];
      }
      valid = valid && E[d] >= 0 && E[d] < ne[d];
    }
    P.valid = valid;
    P.la = valid ? (gg[0] - 2 * E[0]) + 3 * (gg[1] - 2 * E[1]) + 9 * (gg[2] - 2 * E[2]) : 0;
    P.b0 = nl * G27_ROW + ((2 * E[0] - l0) * P.c1 + (2 * E[1] - l1)) * P.c2 + (2 * E[2] - l2);  // the element's first node in the row's box
    if (valid) {
      const int64_t eidx = ((int64_t)(E[0] - elo) * ne[1] + E[1]) * ne[2] + E[2];
      const double* ge = g + eidx * 6;
#pragma unroll
      for (int t = 0; t < 6; ++t) P.g[t] = ge[t];
      if (slot_of) P.slot = slot_of[eidx];
    }
    return P;
  };
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    for (int t = lane; t < 8 * G27_ROW; t += 64) rows[wv * 8 * G27_ROW + t] = 0.0;
    PairPre cur = phase_a(blk);  // (its loads wait behind the other waves' arithmetic: two workgroups of eight waves per CU)
    // (round 6) the wave's eight rows -- consecutive control points: back to back in the value array -- sit IN MEMORY ORDER in its LDS block (a row at its
    // prefix minus the first row's, not at a fixed 125-entry stride): the write-out below is one linear copy with 16-byte stores instead of one or two
    // stores of `len` eight-byte lanes per row (27 .. 125 entries: a third of the lanes on average)
    const uint32_t p0lo = __builtin_amdgcn_readlane((uint32_t)(uint64_t)cur.pre, 0), p0hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)cur.pre >> 32), 0);
    const int64_t pre0 = (int64_t)(((uint64_t)p0hi << 32) | p0lo);
    cur.b0 += (int)(cur.pre - pre0) - (lane >> 3) * G27_ROW;
    __builtin_amdgcn_wave_barrier();
    if (cur.valid && cur.slot < 0) {
      const int a0 = cur.la % 3, a1 = (cur.la / 3) % 3, a2 = cur.la / 9;
      double X0[4][3], X2[4][3];  // [D, M, C, Ct][b]
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          X0[x][b] = sT[(x * 3 + a0) * 4 + b];
          X2[x][b] = sT[(x * 3 + a2) * 4 + b];
        }
      const double g0 = cur.g[0], g1 = cur.g[1], g2 = cur.g[2], g3 = cur.g[3], g4 = cur.g[4], g5 = cur.g[5];
#pragma unroll
      for (int b1 = 0; b1 < 3; ++b1) {
        const double D1 = sT[(0 * 3 + a1) * 4 + b1], M1 = sT[(1 * 3 + a1) * 4 + b1], C1 = sT[(2 * 3 + a1) * 4 + b1], Ct1 = sT[(3 * 3 + a1) * 4 + b1];
#pragma unroll
        for (int b0 = 0; b0 < 3; ++b0) {
          const double D0 = X0[0][b0], M0 = X0[1][b0], C0 = X0[2][b0], Ct0 = X0[3][b0];
          const double Pq = g0 * (D0 * M1) + g1 * (C0 * Ct1 + Ct0 * C1) + g3 * (M0 * D1);
          const double Qq = g5 * (M0 * M1);
          const double Rq = g2 * (C0 * M1) + g4 * (C1 * M0);
          const double Tq = g2 * (Ct0 * M1) + g4 * (Ct1 * M0);
          double* rp = rows + cur.b0 + (b0 * cur.c1 + b1) * cur.c2;
#pragma unroll
          for (int b2 = 0; b2 < 3; ++b2) {
            const double v = X2[1][b2] * Pq + X2[0][b2] * Qq + X2[3][b2] * Rq + X2[2][b2] * Tq;
            __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double*)(rp + b2), v);
          }
        }
      }
    }
    const uint64_t stored = slot_of ? __ballot(cur.valid && cur.slot >= 0) : 0ull;  // (wave-uniform) pairs whose run sits in the scratch
    if (stored) {
      // a half-wave streams the runs of its 4 rows in, element order e = 0..7 per row: lane lb < 27 loads entry lb of a run and adds it at the slot of local
      // node lb in the row's box; what a lane needs about pair p sits in lane p's registers (the pair's own phase A): fetched with wave shuffles
      __builtin_amdgcn_wave_barrier();
      const int lb = lane & 31, hb = lane & 32;
      const bool active = lb < 27;
      const int bx = lb % 3, by = (lb / 3) % 3, bz = lb / 9;
      const int64_t my_src = ((int64_t)(cur.slot >= 0 ? cur.slot : 0) * 27 + scratch_row(cur.la)) * 27;
      const int my_lo = (int)(uint32_t)(uint64_t)my_src, my_hi = (int)(uint32_t)((uint64_t)my_src >> 32);
      uint32_t todo = hb ? (uint32_t)(stored >> 32) : (uint32_t)stored;
      while (__any(todo != 0u)) {  // (both half-waves take part in every shuffle)
        double v[D27_FLIGHT];
        int sl[D27_FLIGHT];
#pragma unroll
        for (int j = 0; j < D27_FLIGHT; ++j) {
          const bool has = todo != 0u;
          const int p = hb + (has ? __builtin_ctz(todo) : 0);
          if (has) todo &= todo - 1u;
          const uint32_t slo = (uint32_t)__shfl(my_lo, p, MFEM_WAVE), shi = (uint32_t)__shfl(my_hi, p, MFEM_WAVE);
          const int pb0 = __shfl(cur.b0, p, MFEM_WAVE), pc1 = __shfl(cur.c1, p, MFEM_WAVE), pc2 = __shfl(cur.c2, p, MFEM_WAVE);
          sl[j] = -1;
          v[j] = 0.0;
          if (has && active) {
            v[j] = __builtin_nontemporal_load(ke + (int64_t)(((uint64_t)shi << 32) | slo) + lb);
            sl[j] = pb0 + (bx * pc1 + by) * pc2 + bz;
          }
        }
#pragma unroll
        for (int j = 0; j < D27_FLIGHT; ++j)
          if (sl[j] >= 0) __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double*)(rows + sl[j]), v[j]);
      }
    }
    __builtin_amdgcn_wave_barrier();
    {
      int total = 0;  // entries of the wave's live rows (rows behind row_hi carry len = 0)
#pragma unroll
      for (int r = 0; r < 8; ++r) total += __builtin_amdgcn_readlane(cur.len, 8 * r);
      double* dst = vals + pre0;
      const double* src = rows + wv * 8 * G27_ROW;
      const int head = total > 0 ? (int)(((uintptr_t)dst >> 3) & 1) : 0, np = (total - head) >> 1;
      typedef double d27_d2 __attribute__((ext_vector_type(2)));
      for (int m = lane; m < np; m += 64) {
        const int idx = head + 2 * m;
        __builtin_nontemporal_store(d27_d2{src[idx], src[idx + 1]}, reinterpret_cast<d27_d2*>(dst + idx));
      }
      if (lane == 0 && head) __builtin_nontemporal_store(src[0], dst);
      if (lane == 1 && ((total - head) & 1)) __builtin_nontemporal_store(src[total - 1], dst + total - 1);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

int hex27_launch_g0(mfem_context_s* ctx, const BrickView& B, double kcond, int elo, int ecnt, double* g, int32_t* d_cnt, int32_t* slot, int32_t* elist) {
  const int64_t nel = (int64_t)ecnt * B.ne1 * B.ne2;
  MFEM_CHECK_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t), ctx->stream));
  hipLaunchKernelGGL(k_hex27_affine_g0, dim3((unsigned)((nel + MFEM_BLOCK - 1) / MFEM_BLOCK)), dim3(MFEM_BLOCK), 0, ctx->stream, B, kcond, elo, ecnt, g, d_cnt,
                     slot, elist);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

int hex27_launch_direct(mfem_context_s* ctx, const BrickView& B, const double* g, double* vals, int elo, const int32_t* slot_of, const double* ke) {
  MFEM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hex27_direct), hipFuncAttributeMaxDynamicSharedMemorySize, (int)D27_LDS_BYTES));
  // two 8-wave workgroups per CU (78 KB of LDS each), persistent
  hipLaunchKernelGGL(k_hex27_direct, dim3(h27_direct_grid(B.n_owned, ctx->num_cus)), dim3(D27_THREADS), D27_LDS_BYTES, ctx->stream, B, hex27_tables(), g, vals,
                     (int64_t)0, B.n_owned, elo, slot_of, ke);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
