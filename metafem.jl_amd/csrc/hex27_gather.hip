#include "hex27.h"

// Pass 2 of the two-pass assembly: a wave owns 8 consecutive control points and builds their CSR rows in LDS (four waves
// per workgroup, no workgroup barrier -- the waves never exchange data).
//   A. lane (row, e) works out the row's e-th candidate element (a mid node has one element per dimension, an
//      element-boundary node two), the offset of the 27-entry run Ke_e[la][0..26] in the scratch and the LDS slot of the
//      element's first node; a ballot gives the wave the set of (row, e) pairs that exist (3.4 of 8 on average);
//   B. each half-wave streams the runs of its 4 rows in: lane lb < 27 loads entry lb (one contiguous 216-byte read per
//      run, up to sixteen runs in flight per lane) and adds it to the row buffer at the slot of node lb.  A row's runs are taken by
//      one half-wave in element order e = 0..7, so the summation order is fixed;
//   C. the rows leave as contiguous streams.
// No index arithmetic per CSR slot, every scratch entry read once, every value written once.
#define G27_FLIGHT 16 // runs a lane has in flight (the kernel is latency-bound: 4 -> 5.8 ms, 8 -> 5.1 ms at 128^3)
__global__ __launch_bounds__(MFEM_BLOCK) void k_hex27_gather_lds(BrickView B, const double* __restrict__ ke, double* __restrict__ vals, int64_t row_lo,
                                                                  int64_t row_hi, int ring) {
  __shared__ double rows[G27_NODES * G27_ROW];
  __shared__ int64_t s_pre[G27_NODES];
  __shared__ int64_t s_src[G27_NODES * 8];
  __shared__ int32_t s_b0[G27_NODES * 8];
  __shared__ int32_t s_len[G27_NODES], s_c1[G27_NODES], s_c2[G27_NODES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int t = lane; t < 8 * G27_ROW; t += 64) rows[wv * 8 * G27_ROW + t] = 0.0;
  uint64_t pairs;
  {
    const int nl = tid >> 3, e = tid & 7;
    const int64_t row = row_lo + (int64_t)blockIdx.x * G27_NODES + nl;
    const bool live = row < row_hi;
    int g[3] = {0, 0, 0}, lo0 = 0, lo1 = 0, lo2 = 0, c1 = 1, c2 = 1;
    if (live) {
      const uint32_t r32 = (uint32_t)row, pl = (uint32_t)B.plane_len, m2 = (uint32_t)B.m2;  // control-point ids fit int32
      const uint32_t q0 = r32 / pl, rem = r32 - q0 * pl, q1 = rem / m2;
      g[0] = (int)q0 + B.plo;
      g[1] = (int)q1;
      g[2] = (int)(rem - q1 * m2);
      lo0 = B.lo0[g[0]]; lo1 = B.lo1[g[1]]; lo2 = B.lo2[g[2]];
      c1 = B.c1[g[1]]; c2 = B.c2[g[2]];
    }
    if (e == 0) {
      s_pre[nl] = live ? brick_prefix(B, g[0], g[1], g[2]) : 0;
      s_len[nl] = live ? B.c0[g[0]] * c1 * c2 : 0;
      s_c1[nl] = c1;
      s_c2[nl] = c2;
    }
    const int ed[3] = {e & 1, (e >> 1) & 1, e >> 2};
    const int ne[3] = {B.ne0, B.ne1, B.ne2};
    int E[3];
    bool valid = live;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (g[d] & 1) {
        E[d] = (g[d] - 1) >> 1;
        valid = valid && ed[d] == 0;
      } else {
        E[d] = (g[d] >> 1) - 1 + ed[d];
      }
      valid = valid && E[d] >= 0 && E[d] < ne[d];
    }
    const int la = (g[0] - 2 * E[0]) + 3 * (g[1] - 2 * E[1]) + 9 * (g[2] - 2 * E[2]);
    const int64_t eid = ((int64_t)(valid ? E[0] % ring : 0) * ne[1] + E[1]) * ne[2] + E[2];
    s_src[tid] = valid ? (eid * 27 + scratch_row(valid ? la : 0)) * 27 : 0;
    s_b0[tid] = nl * G27_ROW + ((2 * E[0] - lo0) * c1 + (2 * E[1] - lo1)) * c2 + (2 * E[2] - lo2);  // the element's first node
    pairs = __ballot(valid);
  }
  __builtin_amdgcn_wave_barrier();
  {
    const int lb = lane & 31;
    const int first = wv * 64 + (lane >> 5) * 32;  // this half-wave's 32 (row, e) pairs = 4 rows
    const bool active = lb < 27;
    const int bx = lb % 3, by = (lb / 3) % 3, bz = lb / 9;
    uint32_t todo = (lane >> 5) ? (uint32_t)(pairs >> 32) : (uint32_t)pairs;
    while (todo) {
      double v[G27_FLIGHT];
      int sl[G27_FLIGHT];
#pragma unroll
      for (int j = 0; j < G27_FLIGHT; ++j) {
        sl[j] = -1;
        v[j] = 0.0;
        if (todo) {
          const int pair = first + __builtin_ctz(todo), nl = pair >> 3;
          todo &= todo - 1;
          if (active) {
            v[j] = ke[s_src[pair] + lb];
            sl[j] = s_b0[pair] + (bx * s_c1[nl] + by) * s_c2[nl] + bz;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < G27_FLIGHT; ++j)
        if (sl[j] >= 0) rows[sl[j]] += v[j];
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (int r = 0; r < 8; ++r) {
    const int n2 = wv * 8 + r, len = s_len[n2];
    const int64_t pre = s_pre[n2];
    for (int o = lane; o < len; o += 64) vals[pre + o] = rows[n2 * G27_ROW + o];
  }
}

int hex27_launch_gather(mfem_context_s* ctx, const BrickView& B, const double* ke, double* vals, int64_t row_lo, int64_t row_hi, int ring) {
  hipLaunchKernelGGL(k_hex27_gather_lds, dim3(h27_gather_grid(row_lo, row_hi)), dim3(MFEM_BLOCK), 0, ctx->stream, B, ke, vals, row_lo, row_hi, ring);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
