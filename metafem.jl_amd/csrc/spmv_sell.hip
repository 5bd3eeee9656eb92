// Row-sorted sliced ELL (SELL-128-sigma with sigma = n) for the Krylov loop on matrices whose rows are NOT of near-uniform
// length -- hex-27 (27 / 45 / 75 / 125 entries per row depending on the node type) and every unstructured mesh.  Solver layout
// mode 3; the uniform case is spmv_ell.hip (mode 1) and spmv_dia.hip with its sweeps (mode 2), the caller-facing contract stays CSR.
// A field-major multi-field matrix on an unstructured mesh takes the node-blocked form of this layout instead: spmv_bsell.hip.
//
//   * inspector (once per pattern): rows are stably sorted by decreasing length (hipCUB radix sort of (max_len - len, row));
//     rows of equal length keep their mesh order, so the x gathers of a 128-row block stay as local as in CSR order.  Block b
//     stores K_b = its longest (= first) row's length slots, slot-major: element (row r', slot s) at ptr[b] + s * 128 + (r' & 127).
//     Padding is what is left of length changes inside a block: 0.0-0.3 % for hex-27.
//     Rows of equal length are further grouped by the signature of their diagonal list (a hash of col - row over the row): a
//     block whose 128 rows share ONE list stores that list once (K_b relative offsets) and its column stream is never read --
//     col = row + off[s].  For hex-27 that is every block away from the mesh boundary (8 node types = 8 lists).
//   * per solve: the working values are copied into that layout (one pass, like the reference's K_total[K_val_ids] gather).
//   * SpMV: a wave owns a block, a lane two neighbouring sorted rows; value / column streams are unit-stride 16-byte / 8-byte
//     loads, the row sum runs in registers in slot (= column) order, and y is written through the row permutation.
// Every host decision -- eligibility, key layout, padding limits, thresholds, which instantiation a knob value gets -- is in sell_decide.h.
#include <hipcub/hipcub.hpp>

#include "blas1.h"
#include "spmv_sell.h"

typedef double s_d2 __attribute__((ext_vector_type(2)));
typedef int s_i2 __attribute__((ext_vector_type(2)));

static std::atomic<int> g_sell_word{SELL_WORD_DEFAULT};  // the word of mfem_debug_set_sell (fields: SellKnobs)
SellKnobs mfem_sell_knobs() { return sell_knobs_decode(g_sell_word); }
extern "C" int mfem_debug_set_sell(int enable) try {
  ++mfem_debug_epoch;
  g_sell_word = enable;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_sell")
// (on a node-blocked pattern: every block reads one column per node)
extern "C" int64_t mfem_debug_sell_periodic_blocks(mfem_csr A) {
  if (!A) return -1;
  return A->sell.form == SELL_NODE_BLOCKED ? (int64_t)(int32_t)A->sell.nblk : (int64_t)A->sell.rows.periodic_blocks * (A->sell.rows.fields > 0 ? 1 : 0);
}

template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_sell_keys(int64_t n, const RP* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            int base, int maxlen, int wshift, int lenbits,
                                                            uint64_t* __restrict__ keys, int32_t* __restrict__ ids,
                                                            int32_t* __restrict__ n_ghost_rows, SellRegions G) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += stride) {
    const int64_t lo = (int64_t)rowptr[r] - base, hi = (int64_t)rowptr[r + 1] - base;
    uint32_t h = 2166136261u;  // FNV-1a over the diagonal list col - row
    bool ghost = false;        // the row reads a ghost column of a slab pattern (columns numbered behind the n owned ones)
    for (int64_t j = lo; j < hi; ++j) {
      const int64_t c = (int64_t)col[j] - base;
      ghost = ghost || c >= n;
      uint32_t d = (uint32_t)(c - r);
      for (int k = 0; k < 4; ++k) {
        h = (h ^ (d & 255u)) * 16777619u;
        d >>= 8;
      }
    }
    // ghost-reading rows sort behind all others (bit 63): the leading blocks can run while the halo exchange is in flight
    // window of the sort: 2^wshift consecutive rows, or -- lattice hint -- a cube of R^3 lattice points: the rows of all lengths (node
    // types) of one region are neighbours in the block list, so the x entries they share are fetched while they are still in the L2s
    uint64_t win = (uint64_t)(r >> wshift);
    if (G.R > 0) {
      const int64_t node = r % G.n_nodes, f = r / G.n_nodes;
      const int64_t pi = node / G.PL, rem = node - pi * G.PL;
      const int64_t pj = rem / G.m2, pk = rem - pj * G.m2;
      win = (uint64_t)(((f * G.nri + pi / G.R) * G.nrj + pj / G.R) * G.nrk + pk / G.R);
    }
    keys[r] = ((uint64_t)(ghost ? 1 : 0) << 63) | (win << (32 + lenbits)) |
              ((uint64_t)(uint32_t)(maxlen - (int32_t)(hi - lo)) << 32) | h;
    ids[r] = (int32_t)r;
    if (ghost) atomicAdd(n_ghost_rows, 1);
  }
}

// Do the diagonal-list signatures repeat?  On a lattice a row shares its list with its first or second neighbour (hex-8: every interior row; hex-27: the
// node types alternate with period 2); on an unstructured pattern practically never.  The signature is the LOW word of the sort key: where it does not
// repeat it must not take part in the sort -- rows of one length would be shuffled by a hash and the x gathers of a 128-row block, local in mesh order,
// would come from all over the vector (round 6: the hex-20 meshes of every shipped example ran this layout at 0.18 of HBM, 3 x slower than the CSR kernel).
__global__ __launch_bounds__(MFEM_BLOCK) void k_sell_sig_repeats(int64_t n, const uint64_t* __restrict__ keys, unsigned long long* __restrict__ count) {
  __shared__ double red_unused[1];
  (void)red_unused;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long c = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r + 2 < n; r += stride) {
    const uint32_t h = (uint32_t)keys[r];
    c += (h == (uint32_t)keys[r + 1] || h == (uint32_t)keys[r + 2]) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}
__global__ __launch_bounds__(MFEM_BLOCK) void k_sell_clear_sig(int64_t n, uint64_t* __restrict__ keys) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += stride) keys[r] &= 0xFFFFFFFF00000000ull;
}

// flags[b] = 1 and off[ptr[b] / 128 + s] = the common diagonal list when all 128 rows of block b have the list of its first row
template <typename RP>
__global__ __launch_bounds__(SELL_B) void k_sell_block_flags(int64_t n, int64_t nblk, const RP* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col, int base,
                                                               const int32_t* __restrict__ rowid, const int64_t* __restrict__ ptr,
                                                               int32_t* __restrict__ flags, int32_t* __restrict__ off,
                                                               int32_t* __restrict__ nreg) {
  __shared__ int bad;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int64_t rs = b * SELL_B + threadIdx.x;
    const int64_t r0 = rowid[b * SELL_B];
    const int64_t lo0 = (int64_t)rowptr[r0] - base;
    const int K = (int)((int64_t)rowptr[r0 + 1] - base - lo0);
    int fail = 0;
    if (rs < n) {
      const int64_t r = rowid[rs];
      const int64_t lo = (int64_t)rowptr[r] - base;
      if ((int)((int64_t)rowptr[r + 1] - base - lo) != K) fail = 1;
      for (int s = 0; s < K && !fail; ++s)
        if ((int64_t)col[lo + s] - r != (int64_t)col[lo0 + s] - r0) fail = 1;
    } else {
      fail = 1;
    }
    if (fail) bad = 1;
    __syncthreads();
    if (!bad) {
      const int64_t o0 = ptr[b] / SELL_B;
      for (int s = threadIdx.x; s < K; s += SELL_B) off[o0 + s] = (int32_t)((int64_t)col[lo0 + s] - base - r0);
    }
    if (threadIdx.x == 0) {
      flags[b] = bad ? 0 : 1;
      if (!bad) atomicAdd(nreg, 1);
    }
    __syncthreads();
  }
}

// K_b * 128 for every block, K_b = its longest row: the first row, except in the one block where the ghost-reading rows (sorted behind
// all others, again by decreasing length) begin
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_sell_block_sizes(int64_t n, int64_t nblk, const RP* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ rowid, int64_t* __restrict__ sizes) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nblk; b += stride) {
    int64_t K = 0;
    for (int64_t rs = b * SELL_B; rs < (b + 1) * SELL_B && rs < n; ++rs) {
      const int64_t r = rowid[rs];
      const int64_t len = (int64_t)rowptr[r + 1] - (int64_t)rowptr[r];
      K = len > K ? len : K;
    }
    sizes[b] = K * SELL_B;
  }
}

// columns (0-based; padding = the row itself) or values (padding = 0) into the sliced layout.  Four lanes per sorted row, 16 rows per
// wave pass: a lane quad reads 32 contiguous bytes of its row per step, so a row's cache line is used up by four consecutive loads of the
// same wave (with a lane per row the 64 row cursors of a wave advance 8 bytes at a time over a 64 KB working set: 10.5 ms per bind of the
// hex-27 128^3 matrix against 4.9 ms here); a store covers full 128-byte lines of four slots.
template <typename RP, typename T, bool COLS>
__global__ __launch_bounds__(MFEM_BLOCK) void k_sell_fill(int64_t n, int64_t nblk, const RP* __restrict__ rowptr,
                                                            const int32_t* __restrict__ rowid, const int64_t* __restrict__ ptr,
                                                            const T* __restrict__ src, int base, T* __restrict__ out,
                                                            const int32_t* __restrict__ col, const double* __restrict__ dsc) {
  // values only -- dsc != nullptr: entry / dsc[its column] (right Jacobi scaling folded into the copy)
  const int lane = threadIdx.x & 63, g = lane & 3;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t t = wave; t < 8 * nblk; t += nwaves) {  // a wave fills 16 rows of a block
    const int64_t b = t >> 3;
    const int64_t rs = b * SELL_B + (t & 7) * 16 + (lane >> 2);  // sorted row
    const int64_t p0 = ptr[b];
    const int Kb = (int)((ptr[b + 1] - p0) / SELL_B);
    int64_t lo = 0;
    int len = 0;
    T pad = (T)0;
    if (rs < n) {
      const int64_t r = rowid[rs];
      lo = (int64_t)rowptr[r] - base;
      len = (int)((int64_t)rowptr[r + 1] - base - lo);
      if (COLS) pad = (T)r;
    }
    T* o = out + p0 + (rs & (SELL_B - 1));
    if (!COLS && dsc) {
      for (int s = g; s < Kb; s += 4) o[(int64_t)s * SELL_B] = s < len ? (T)((double)src[lo + s] / dsc[col[lo + s] - base]) : pad;
    } else {
      // four loads of a lane in flight before the first store (round 6: one at a time -- load, wait, store -- copied the 15 GB of the hex-20 elasticity
      // matrix at 0.9 TB/s: 33.6 ms per solve)
      int s = g;
      for (; s + 12 < Kb; s += 16) {
        T t4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int su = s + 4 * u;
          t4[u] = su < len ? (COLS ? (T)(src[lo + su] - base) : src[lo + su]) : pad;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) o[(int64_t)(s + 4 * u) * SELL_B] = t4[u];
      }
      for (; s < Kb; s += 4) o[(int64_t)s * SELL_B] = s < len ? (COLS ? (T)(src[lo + s] - base) : src[lo + s]) : pad;
    }
  }
}

__global__ __launch_bounds__(MFEM_BLOCK) void k_sell_clear_flag2(int64_t nblk, int32_t* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nblk; b += stride)
    if (flags[b] == 2) flags[b] = 0;
}
// flags[b] = 2 when block b (not regular) is FIELD-PERIODIC: all 128 rows have K = F * P entries and col[f * P + t] = col[t] + f * shift for every row.
// A field-major multi-field matrix on ANY mesh has that form in its full blocks (row (g, i) lists the nodes coupled to i once per column field): the SpMV
// then reads P column slots instead of K -- a third of the column stream for three fields, 22 % of the bytes of a hex-20 elasticity product.
template <typename RP>
__global__ __launch_bounds__(SELL_B) void k_sell_block_periodic(int64_t n, int64_t nblk, const RP* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                  int base, const int32_t* __restrict__ rowid, const int64_t* __restrict__ ptr, int F,
                                                                  int64_t shift, int32_t* __restrict__ flags, int32_t* __restrict__ nper) {
  __shared__ int bad;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    if (flags[b] != 0) continue;  // (block-uniform)
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int K = (int)((ptr[b + 1] - ptr[b]) / SELL_B);
    const int64_t rs = b * SELL_B + threadIdx.x;
    int fail = (K % F != 0 || K == 0) ? 1 : 0;
    if (!fail) {
      if (rs < n) {
        const int64_t r = rowid[rs];
        const int64_t lo = (int64_t)rowptr[r] - base;
        if ((int)((int64_t)rowptr[r + 1] - base - lo) != K) fail = 1;
        const int P = K / F;
        for (int f = 1; f < F && !fail; ++f)
          for (int t = 0; t < P && !fail; ++t)
            if ((int64_t)col[lo + (int64_t)f * P + t] != (int64_t)col[lo + t] + f * shift) fail = 1;
      } else {
        fail = 1;
      }
    }
    if (fail) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0 && !bad) {
      flags[b] = 2;
      atomicAdd(nper, 1);
    }
    __syncthreads();
  }
}

// one field-periodic block: U node slots at a time, their F x U values and x entries in flight (the column slot of a node is read once for its F fields)
template <int F, int U>
__device__ __forceinline__ void sell_periodic_block(int Kb, int64_t shift, const double* __restrict__ v, const int32_t* __restrict__ c,
                                                    const double* __restrict__ x, double& acc0, double& acc1) {
  const int P = Kb / F;
  int t = 0;
  for (; t + U <= P; t += U) {
    int32_t c0[U], c1[U];
    double v0[F][U], v1[F][U], x0[F][U], x1[F][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      c0[u] = __builtin_nontemporal_load(c + (int64_t)(t + u) * SELL_B);
      c1[u] = __builtin_nontemporal_load(c + (int64_t)(t + u) * SELL_B + 64);
    }
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        v0[f][u] = __builtin_nontemporal_load(v + (int64_t)(f * P + t + u) * SELL_B);
        v1[f][u] = __builtin_nontemporal_load(v + (int64_t)(f * P + t + u) * SELL_B + 64);
      }
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x0[f][u] = x[(int64_t)c0[u] + f * shift];
        x1[f][u] = x[(int64_t)c1[u] + f * shift];
      }
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc0 += v0[f][u] * x0[f][u];
        acc1 += v1[f][u] * x1[f][u];
      }
  }
  for (; t < P; ++t) {
    const int64_t ca = c[(int64_t)t * SELL_B], cb = c[(int64_t)t * SELL_B + 64];
#pragma unroll
    for (int f = 0; f < F; ++f) {
      acc0 += __builtin_nontemporal_load(v + (int64_t)(f * P + t) * SELL_B) * x[ca + f * shift];
      acc1 += __builtin_nontemporal_load(v + (int64_t)(f * P + t) * SELL_B + 64) * x[cb + f * shift];
    }
  }
}

template <int SELL_U>
__global__ __launch_bounds__(MFEM_BLOCK) void k_spmv_sell(int64_t n, int64_t nblk, const int64_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ rowid, const int32_t* __restrict__ flags,
                                                            const int32_t* __restrict__ off, const int32_t* __restrict__ cols,
                                                            const double* __restrict__ vals, const double* __restrict__ x,
                                                            double* __restrict__ y, double alpha, double beta,
                                                            const double* __restrict__ dotw, double* __restrict__ partials,
                                                            const int32_t* __restrict__ done_flag, int64_t b_lo, int64_t b_hi, int xcd, int pF,
                                                            int64_t pshift) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // xcd != 0: workgroups with equal blockIdx % 8 share an XCD (round-robin dispatch) and walk one contiguous eighth of the blocks
  int64_t b_first = b_lo + wave, b_stride = nwaves, b_end = b_hi;
  if (xcd) {
    const int64_t x = blockIdx.x & 7, wpw = blockDim.x >> 6, nb = b_hi - b_lo;
    b_first = b_lo + nb * x / 8 + ((int64_t)(blockIdx.x >> 3) * wpw + (threadIdx.x >> 6));
    b_end = b_lo + nb * (x + 1) / 8;
    b_stride = (int64_t)(gridDim.x >> 3) * wpw;
  }
  for (int64_t b = b_first; b < b_end; b += b_stride) {  // [b_lo, b_hi): all blocks, or one part of a split (multi-rank) SpMV
    const int64_t p0 = ptr[b];
    const int Kb = (int)((ptr[b + 1] - p0) / SELL_B);
    // lane l owns the block's rows l and l + 64: the value loads of a slot are two unit-stride 512-byte runs, and the x
    // loads of same-type rows (stride 2 along the fastest lattice direction for hex-27) touch half as many lines as with
    // two consecutive rows per lane
    const int64_t rs0 = b * SELL_B + lane, rs1 = rs0 + 64;
    const double* v = vals + p0 + lane;
    const int32_t* c = cols + p0 + lane;
    double acc0 = 0.0, acc1 = 0.0;
    const int bflag = flags ? __builtin_amdgcn_readfirstlane(flags[b]) : 0;
    const bool regular = bflag == 1;  // full block, one diagonal list
    const bool periodic = bflag == 2 && (pF & 15) > 1;  // full block of a field-major multi-field matrix: the node list repeats per column field
    int64_t rid0 = 0, rid1 = 0;
    if (rs0 < n) rid0 = rowid[rs0];
    if (rs1 < n) rid1 = rowid[rs1];
    // SELL_U slots in flight per lane (the kernel is latency-bound without: one slot at a time ran at 3.0 TB/s)
    if (regular) {
      const int32_t* ob = off + __builtin_amdgcn_readfirstlane((int)(p0 / SELL_B));
      int s = 0;
      for (; s + SELL_U <= Kb; s += SELL_U) {
        double v0[SELL_U], v1[SELL_U], x0[SELL_U], x1[SELL_U];
#pragma unroll
        for (int u = 0; u < SELL_U; ++u) {
          v0[u] = __builtin_nontemporal_load(v + (int64_t)(s + u) * SELL_B);
          v1[u] = __builtin_nontemporal_load(v + (int64_t)(s + u) * SELL_B + 64);
          const int64_t o = ob[s + u];
          x0[u] = x[rid0 + o];
          x1[u] = x[rid1 + o];
        }
#pragma unroll
        for (int u = 0; u < SELL_U; ++u) {
          acc0 += v0[u] * x0[u];
          acc1 += v1[u] * x1[u];
        }
      }
      for (; s < Kb; ++s) {
        const int64_t o = ob[s];
        acc0 += __builtin_nontemporal_load(v + (int64_t)s * SELL_B) * x[rid0 + o];
        acc1 += __builtin_nontemporal_load(v + (int64_t)s * SELL_B + 64) * x[rid1 + o];
      }
    } else if (periodic) {
      const int F_ = pF & 15, pu = pF >> 4;  // (fields; node slots in flight: 0 = the default)
      if (F_ == 3) {
        // (hex-20 elasticity 96^3, one box: 2 node slots in flight 3.69 ms, 3: 3.52, 4: 3.67; the whole column stream: 4.37)
        if (pu == 1) sell_periodic_block<3, 2>(Kb, pshift, v, c, x, acc0, acc1);
        else if (pu == 2) sell_periodic_block<3, 4>(Kb, pshift, v, c, x, acc0, acc1);
        else sell_periodic_block<3, 3>(Kb, pshift, v, c, x, acc0, acc1);
      } else if (F_ == 2) sell_periodic_block<2, 3>(Kb, pshift, v, c, x, acc0, acc1);
      else sell_periodic_block<4, 2>(Kb, pshift, v, c, x, acc0, acc1);
    } else {
      int s = 0;
      for (; s + SELL_U <= Kb; s += SELL_U) {
        double v0[SELL_U], v1[SELL_U], x0[SELL_U], x1[SELL_U];
#pragma unroll
        for (int u = 0; u < SELL_U; ++u) {
          v0[u] = __builtin_nontemporal_load(v + (int64_t)(s + u) * SELL_B);
          v1[u] = __builtin_nontemporal_load(v + (int64_t)(s + u) * SELL_B + 64);
          x0[u] = x[__builtin_nontemporal_load(c + (int64_t)(s + u) * SELL_B)];
          x1[u] = x[__builtin_nontemporal_load(c + (int64_t)(s + u) * SELL_B + 64)];
        }
#pragma unroll
        for (int u = 0; u < SELL_U; ++u) {
          acc0 += v0[u] * x0[u];
          acc1 += v1[u] * x1[u];
        }
      }
      for (; s < Kb; ++s) {
        acc0 += __builtin_nontemporal_load(v + (int64_t)s * SELL_B) * x[c[(int64_t)s * SELL_B]];
        acc1 += __builtin_nontemporal_load(v + (int64_t)s * SELL_B + 64) * x[c[(int64_t)s * SELL_B + 64]];
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if ((h ? rs1 : rs0) < n) {
        const int64_t r = h ? rid1 : rid0;
        double yv = alpha * (h ? acc1 : acc0);
        if (beta != 0.0) yv += beta * y[r];
        y[r] = yv;
        if (dotw) dot_acc += yv * dotw[r];
      }
    }
  }
  if (partials) {
    const double bsum = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = bsum;
  }
}

template <typename Key>
int mfem_sell_sort_blocks(mfem_context_s* ctx, SellSortBufs<Key>& B, int64_t count, int bits, int64_t nblk, const SellBlockSizes& block_sizes,
                          int64_t* total) {
  DevBuf<char> tmp;
  size_t tb = 0, tb2 = 0;
  MFEM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, B.keys.p, B.keys2.p, B.ids.p, B.sorted.p, (int)count, 0, bits, ctx->stream));
  MFEM_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, B.sizes.p, B.ptr.p, (int)(nblk + 1), ctx->stream));
  if (tb2 > tb) tb = tb2;
  MFEM_CHECK_HIP(tmp.alloc(tb));
  MFEM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, B.keys.p, B.keys2.p, B.ids.p, B.sorted.p, (int)count, 0, bits, ctx->stream));
  MFEM_CHECK_HIP(hipMemsetAsync(B.sizes.p, 0, sizeof(int64_t) * (size_t)(nblk + 1), ctx->stream));
  block_sizes(B.sorted.p, B.sizes.p);
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, B.sizes.p, B.ptr.p, (int)(nblk + 1), ctx->stream));
  MFEM_CHECK_HIP(hipMemcpyAsync(total, B.ptr.p + nblk, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return MFEM_OK;
}
template int mfem_sell_sort_blocks<uint64_t>(mfem_context_s*, SellSortBufs<uint64_t>&, int64_t, int, int64_t, const SellBlockSizes&, int64_t*);
template int mfem_sell_sort_blocks<uint32_t>(mfem_context_s*, SellSortBufs<uint32_t>&, int64_t, int, int64_t, const SellBlockSizes&, int64_t*);

// What the stages of the row-sorted plan hand on.  Everything a stage allocates is owned here until sell_plan_rows hands it to the record.
struct MFEM_SELL_LOCAL SellRowsPlan {
  SellShape S;
  SellKnobs K;
  SellRegions G;
  int64_t nblk, total;
  SellSortBufs<uint64_t> B;
  DevBuf<int32_t> cols, flags, off;
  SellLayout::Rows R;  // (the counts; its pointers are set at the end)
};
static int32_t* sell_counter(mfem_context_s* ctx) { return ctx->d_flags + 9; }  // one-shot device counter of the stages, mirrored in ctx->h_flags[9]

// stage 1: the sort keys (ghost flag | region or window | max_len - len | signature), the identity permutation, the count of ghost-reading rows
static int sell_plan_keys(mfem_context_s* ctx, const mfem_csr_s* A, SellRowsPlan& W) {
  const int64_t n = W.S.n;
  const int grid = mfem_grid_for(n, MFEM_BLOCK, ctx->num_cus * 16);
  const int rc = W.B.alloc(n, W.nblk);
  if (rc) return rc;
  MFEM_CHECK_HIP(hipMemsetAsync(sell_counter(ctx), 0, sizeof(int32_t), ctx->stream));
  mfem_by_rowptr(A, [&](auto rp) {
    using RP = decltype(rp);
    hipLaunchKernelGGL(k_sell_keys<RP>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, n, (const RP*)A->rowptr, A->colidx, A->index_base, A->max_row_nnz,
                       sell_window_shift(W.K), sell_len_bits(A->max_row_nnz), W.B.keys.p, W.B.ids.p, sell_counter(ctx), W.G);
  });
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 9, sell_counter(ctx), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  return MFEM_OK;
}
// stage 2: signatures that do not repeat (unstructured patterns) stay out of the sort: rows of one length keep their mesh order
static int sell_plan_signatures(mfem_context_s* ctx, SellRowsPlan& W) {
  const int64_t n = W.S.n;
  const int grid = mfem_grid_for(n, MFEM_BLOCK, ctx->num_cus * 16);
  unsigned long long* d_rep = (unsigned long long*)(void*)W.B.sizes.p;  // (zeroed again by the sort before its own use)
  unsigned long long h_rep = 0;
  MFEM_CHECK_HIP(hipMemsetAsync(d_rep, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_sell_sig_repeats, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, n, W.B.keys.p, d_rep);
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(&h_rep, d_rep, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  W.R.sig_sorted = sell_signatures_repeat(n, (int64_t)h_rep) ? 1 : 0;
  if (!W.R.sig_sorted) {
    hipLaunchKernelGGL(k_sell_clear_sig, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, n, W.B.keys.p);
    MFEM_CHECK_LAUNCH();
  }
  return MFEM_OK;
}
// stage 3: the sort, K_b * 128 of every block and their prefix sums; then the interior blocks of a split product, from the ghost-reading rows
static int sell_plan_sort(mfem_context_s* ctx, const mfem_csr_s* A, SellRowsPlan& W) {
  const int rc = mfem_sell_sort_blocks<uint64_t>(ctx, W.B, W.S.n, sell_key_bits(W.S, W.K, W.G), W.nblk, [&](const int32_t* rowid, int64_t* sizes) {
    mfem_by_rowptr(A, [&](auto rp) {
      using RP = decltype(rp);
      hipLaunchKernelGGL(k_sell_block_sizes<RP>, dim3(mfem_grid_for(W.nblk, MFEM_BLOCK, ctx->num_cus * 16)), dim3(MFEM_BLOCK), 0, ctx->stream, W.S.n, W.nblk,
                         (const RP*)A->rowptr, rowid, sizes);
    });
  }, &W.total);
  if (rc) return rc;
  W.R.nb_int = sell_nb_int(W.S, ctx->h_flags[9]);
  return MFEM_OK;
}
// stage 4: the columns in the sliced layout
static int sell_plan_cols(mfem_context_s* ctx, const mfem_csr_s* A, SellRowsPlan& W) {
  MFEM_CHECK_HIP(W.cols.alloc((size_t)W.total));
  const int g2 = mfem_grid_for(8 * W.nblk * 64, MFEM_BLOCK, ctx->num_cus * 16);
  mfem_by_rowptr(A, [&](auto rp) {
    using RP = decltype(rp);
    hipLaunchKernelGGL((k_sell_fill<RP, int32_t, true>), dim3(g2), dim3(MFEM_BLOCK), 0, ctx->stream, W.S.n, W.nblk, (const RP*)A->rowptr, W.B.sorted.p,
                       W.B.ptr.p, A->colidx, A->index_base, W.cols.p, (const int32_t*)nullptr, (const double*)nullptr);
  });
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
// reads back the block count a stage's kernel left in the counter
static int sell_read_counter(mfem_context_s* ctx, int32_t* count) {
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 9, sell_counter(ctx), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  *count = ctx->h_flags[9];
  return MFEM_OK;
}
// stage 5: blocks with a single diagonal list
static int sell_plan_regular(mfem_context_s* ctx, const mfem_csr_s* A, SellRowsPlan& W) {
  MFEM_CHECK_HIP(W.flags.alloc((size_t)W.nblk));
  MFEM_CHECK_HIP(W.off.alloc((size_t)(W.total / SELL_B + 1)));
  MFEM_CHECK_HIP(hipMemsetAsync(sell_counter(ctx), 0, sizeof(int32_t), ctx->stream));
  mfem_by_rowptr(A, [&](auto rp) {
    using RP = decltype(rp);
    hipLaunchKernelGGL(k_sell_block_flags<RP>, dim3(sell_inspect_grid(W.nblk, ctx->num_cus)), dim3(SELL_B), 0, ctx->stream, W.S.n, W.nblk, (const RP*)A->rowptr,
                       A->colidx, A->index_base, W.B.sorted.p, W.B.ptr.p, W.flags.p, W.off.p, sell_counter(ctx));
  });
  MFEM_CHECK_LAUNCH();
  return sell_read_counter(ctx, &W.R.regular_blocks);
}
// stage 6: field-periodic blocks among the others (k_sell_block_periodic), for the first field count that covers enough of the blocks
static int sell_plan_periodic(mfem_context_s* ctx, const mfem_csr_s* A, SellRowsPlan& W) {
  if (!sell_periodic_may_try(W.S, W.K, W.R.regular_blocks, W.nblk)) return MFEM_OK;
  const int g3 = sell_inspect_grid(W.nblk, ctx->num_cus);
  for (int ci = 0; ci < 3 && W.R.fields == 0; ++ci) {
    const int F = SELL_PERIODIC_FIELDS[ci];
    if (!sell_fields_divide(W.S, F)) continue;
    MFEM_CHECK_HIP(hipMemsetAsync(sell_counter(ctx), 0, sizeof(int32_t), ctx->stream));
    mfem_by_rowptr(A, [&](auto rp) {
      using RP = decltype(rp);
      hipLaunchKernelGGL(k_sell_block_periodic<RP>, dim3(g3), dim3(SELL_B), 0, ctx->stream, W.S.n, W.nblk, (const RP*)A->rowptr, A->colidx, A->index_base,
                         W.B.sorted.p, W.B.ptr.p, F, W.S.n / F, W.flags.p, sell_counter(ctx));
    });
    MFEM_CHECK_LAUNCH();
    int32_t count = 0;
    const int rc = sell_read_counter(ctx, &count);
    if (rc) return rc;
    if (sell_periodic_taken(W.nblk, count)) {
      W.R.fields = F;
      W.R.shift = W.S.n / F;
      W.R.periodic_blocks = count;
    } else if (count > 0) {  // (a few blocks happened to fit: not taken -- back to "generic")
      hipLaunchKernelGGL(k_sell_clear_flag2, dim3(g3), dim3(MFEM_BLOCK), 0, ctx->stream, W.nblk, W.flags.p);
      MFEM_CHECK_LAUNCH();
    }
  }
  return MFEM_OK;
}
// The row-sorted plan: fills *L (form SELL_ROW_SORTED) unless the padding is refused.
static int sell_plan_rows(mfem_context_s* ctx, const mfem_csr_s* A, const SellShape& S, SellLayout* L) {
  SellRowsPlan W{};
  W.S = S;
  W.K = mfem_sell_knobs();
  W.G = sell_regions(S, W.K);
  W.nblk = sell_blocks(S.n);
  int rc = sell_plan_keys(ctx, A, W);
  if (!rc) rc = sell_plan_signatures(ctx, W);
  if (!rc) rc = sell_plan_sort(ctx, A, W);
  if (rc || !sell_padding_ok(S, W.G, W.total)) return rc;
  rc = sell_plan_cols(ctx, A, W);
  if (!rc) rc = sell_plan_regular(ctx, A, W);
  if (!rc) rc = sell_plan_periodic(ctx, A, W);
  if (rc) return rc;
  L->form = SELL_ROW_SORTED;
  L->total = W.total;
  L->nblk = W.nblk;
  L->rows = W.R;
  L->rows.rowid = W.B.sorted.release();
  L->rows.ptr = W.B.ptr.release();
  L->rows.cols = W.cols.release();
  L->rows.flags = W.flags.release();
  L->rows.off = W.off.release();
  return MFEM_OK;
}

// The node-blocked form first (a multi-field matrix on an unstructured mesh), else the row-sorted one.  The record is built aside: the handle
// gets it whole, and a plan that fails midway leaves the handle as mfem_sell_free does.
int mfem_sell_plan(mfem_context_s* ctx, mfem_csr_s* A) {
  if (A->sell.state != 0) return MFEM_OK;
  const SellShape S = mfem_sell_shape(A);
  const int wanted = sell_state_wanted(S);
  if (wanted != 1) {
    A->sell.state = wanted;
    return MFEM_OK;
  }
  SellLayout L{};
  int rc = mfem_bsell_plan(ctx, A, S, &L);
  if (!rc && L.form == SELL_NONE) rc = sell_plan_rows(ctx, A, S, &L);
  if (rc) return rc;
  L.state = L.form != SELL_NONE ? 1 : -1;
  A->sell = L;
  return MFEM_OK;
}

size_t mfem_sell_vals_bytes(const mfem_csr_s* A) {
  return sell_serves(A->sell.state, mfem_sell_knobs(), mfem_sell_shape(A)) ? sizeof(double) * (size_t)A->sell.total : 0;
}

int mfem_sell_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc) {
  SellLayout& L = A->sell;
  mfem_sell_unbind(A);
  if (L.state != 1 || !mfem_sell_knobs().enable || !buf) return MFEM_OK;
  if (L.form == SELL_NODE_BLOCKED) {
    const int rc = mfem_bsell_fill(ctx, A, vals, buf, dsc);
    if (rc) return rc;
  } else {
    const int g2 = mfem_grid_for(8 * L.nblk * 64, MFEM_BLOCK, ctx->num_cus * 16);
    mfem_by_rowptr(A, [&](auto rp) {
      using RP = decltype(rp);
      hipLaunchKernelGGL((k_sell_fill<RP, double, false>), dim3(g2), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, L.nblk, (const RP*)A->rowptr, L.rows.rowid,
                         L.rows.ptr, vals, A->index_base, buf, A->colidx, dsc);
    });
    MFEM_CHECK_LAUNCH();
  }
  L.vals = buf;
  L.src = vals;
  return MFEM_OK;
}

// accounting (mfem_csr_solver_layout_entries / _bytes): the padded slots, and sell_design_bytes
int64_t mfem_sell_entries(const mfem_csr_s* A) { return A->sell.total; }
int64_t mfem_sell_design_bytes(const mfem_csr_s* A) { return sell_design_bytes(A->sell, A->n); }

void mfem_sell_unbind(mfem_csr_s* A) {
  A->sell.vals = nullptr;
  A->sell.src = nullptr;
}

void mfem_sell_free(mfem_csr_s* A) {
  SellLayout& L = A->sell;
  void* const owned[] = {L.rows.cols, L.rows.rowid, L.rows.ptr, L.rows.flags, L.rows.off, L.nodes.nodeid, L.nodes.ptr, L.nodes.cols};
  for (void* p : owned)
    if (p) (void)hipFree(p);
  L = SellLayout{};  // (state 0: not planned; mfem_layout_drop has unbound the copy)
}

static auto sell_kernel(int U) -> decltype(&k_spmv_sell<5>) {
  switch (U) {
    case 4: return k_spmv_sell<4>;
    case 8: return k_spmv_sell<8>;
    case 9: return k_spmv_sell<9>;
    case 10: return k_spmv_sell<10>;
    case 15: return k_spmv_sell<15>;
    default: return k_spmv_sell<5>;
  }
}
// returns 1 if launched, 0 if another kernel should be used, <0 on error
int mfem_spmv_sell_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha,
                          double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag, int part) {
  const SellLayout& L = A->sell;
  if (!L.vals || vals != L.src) return 0;
  if (n_partials) *n_partials = 0;
  if (L.form == SELL_NODE_BLOCKED) return mfem_bsell_launch(ctx, A, x, y, alpha, beta, dotw, partials, n_partials, done_flag, part);
  const SellKnobs K = mfem_sell_knobs();
  const SellRange b = sell_part_range(part, L.rows.nb_int, L.nblk);
  if (b.hi <= b.lo) return 1;
  const int grid = mfem_grid_for((b.hi - b.lo) * 64, MFEM_BLOCK, sell_grid_cap(ctx->num_cus, K, MFEM_MAX_PARTIALS, part));
  hipLaunchKernelGGL(sell_kernel(sell_unroll_resolved(K)), dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, L.nblk, L.rows.ptr, L.rows.rowid,
                     K.offsets ? L.rows.flags : nullptr, L.rows.off, L.rows.cols, L.vals, x, y, alpha, beta, dotw, partials, done_flag, b.lo, b.hi,
                     sell_xcd_flag(K, grid), sell_periodic_word(K, L.rows.fields), L.rows.shift);
  MFEM_CHECK_LAUNCH();
  if (n_partials && partials) *n_partials = grid;
  return 1;
}
