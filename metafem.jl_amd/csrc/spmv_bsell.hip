// Node-blocked form ("BSELL", round 6) of the sliced solver layout (mode 3; the row-sorted form: spmv_sell.hip) for field-major multi-field matrices on unstructured meshes: unknown (f, i) = f * ncp + i, and the rows
// (0, i) .. (F - 1, i) of node i all list the nodes coupled to i, once per column field (what mfem_pattern_build makes for n_fields fields; checked entry
// by entry by k_bsell_check).  The row-sorted layout gives every ROW a lane: per value it reads a third of a column index (field-periodic blocks)
// and gathers one x entry -- on hex-20 elasticity 96^3 the product moved 21.2 GB for 17.7 by design (x gathers that miss the L2s) at the HBM copy rate.
// Here a lane owns a NODE: per coupled node ONE column index, F gathers of x and F x F values for the node's F row sums -- a ninth of the column stream,
// a third of the gathers.  Nodes are stably sorted by their number of coupled nodes; a block is 64 nodes; slot t of a block holds, for each of its nodes,
// the F x F values towards the node's t-th coupled node as F * F unit-stride runs of 64 doubles.
// Every host decision of this form -- who may try it, the field counts, the padding limit, which copy and which product instantiation -- is in
// sell_decide.h; the entry points of the layout (plan, bind, launch, release) are spmv_sell.hip's, which dispatch here on the form.
#include "blas1.h"
#include "spmv_sell.h"

static std::atomic<int> g_bsell_word{BSELL_WORD_DEFAULT};  // mfem_debug_set("bsell", on) (fields: BsellKnobs)
static std::atomic<long long> g_bsell_spmv_count{0};
extern "C" int mfem_debug_set_bsell(int on) {
  ++mfem_debug_epoch;
  g_bsell_word = on;
  return MFEM_OK;
}
extern "C" long long mfem_debug_bsell_spmv_count(void) { return g_bsell_spmv_count; }
extern "C" int mfem_debug_bsell_fields(mfem_csr A) { return !A ? -1 : A->sell.form == SELL_NODE_BLOCKED ? A->sell.nodes.F : 0; }

// bad[0] != 0: some node's rows do not have the node-blocked form
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_bsell_check(int64_t ncp, int F, const RP* __restrict__ rowptr, const int32_t* __restrict__ col, int base,
                                                              int32_t* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncp; i += stride) {
    const int64_t lo0 = (int64_t)rowptr[i] - base;
    const int len = (int)((int64_t)rowptr[i + 1] - base - lo0);
    bool ok = len % F == 0;
    const int L = len / F;
    for (int t = 0; ok && t < L; ++t) {
      const int64_t c = (int64_t)col[lo0 + t] - base;
      ok = c >= 0 && c < ncp;
    }
    for (int f = 0; ok && f < F; ++f) {
      const int64_t lo = (int64_t)rowptr[(int64_t)f * ncp + i] - base;
      ok = (int)((int64_t)rowptr[(int64_t)f * ncp + i + 1] - base - lo) == len;
      for (int g = 0; ok && g < F; ++g)
        for (int t = 0; ok && t < L; ++t) ok = (int64_t)col[lo + (int64_t)g * L + t] == (int64_t)col[lo0 + t] + (int64_t)g * ncp;
    }
    if (!ok) *bad = 1;
  }
}
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_bsell_keys(int64_t ncp, int F, int maxL, const RP* __restrict__ rowptr, uint32_t* __restrict__ keys,
                                                             int32_t* __restrict__ ids) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncp; i += stride) {
    keys[i] = (uint32_t)(maxL - (int)(((int64_t)rowptr[i + 1] - (int64_t)rowptr[i]) / F));
    ids[i] = (int32_t)i;
  }
}
// node slots x 64 of every block (its first node is its longest)
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_bsell_block_sizes(int64_t nblk, int F, const RP* __restrict__ rowptr, const int32_t* __restrict__ nodeid,
                                                                    int64_t* __restrict__ sizes) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nblk; b += stride) {
    const int64_t i = nodeid[b * 64];
    sizes[b] = ((int64_t)rowptr[i + 1] - (int64_t)rowptr[i]) / F * 64;
  }
}
// node-level columns, 0-based (padding: the node itself, with zero values)
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_bsell_cols(int64_t ncp, int64_t nblk, int F, const RP* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             int base, const int32_t* __restrict__ nodeid, const int64_t* __restrict__ ptr,
                                                             int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave; b < nblk; b += nwaves) {
    const int64_t p0 = ptr[b];
    const int Kb = (int)((ptr[b + 1] - p0) / 64);
    const int64_t ns = b * 64 + lane;
    int64_t lo = 0, i = 0;
    int L = 0;
    if (ns < ncp) {
      i = nodeid[ns];
      lo = (int64_t)rowptr[i] - base;
      L = (int)(((int64_t)rowptr[i + 1] - base - lo) / F);
    }
    for (int t = 0; t < Kb; ++t) out[p0 + (int64_t)t * 64 + lane] = t < L ? col[lo + t] - base : (int32_t)i;
  }
}
// values into the node-blocked layout (once per solve).  A lane quad per CSR row, 16 consecutive sorted nodes of one row field per wave pass: the quad
// reads 32 contiguous bytes of its row per step, the 16 rows' stores of one slot are 128 contiguous bytes.  dsc != nullptr: entry / dsc[its column].
template <typename RP, int F>
__global__ __launch_bounds__(MFEM_BLOCK) void k_bsell_fill(int64_t ncp, int64_t nblk, const RP* __restrict__ rowptr, const int32_t* __restrict__ nodeid,
                                                             const int64_t* __restrict__ ptr, const double* __restrict__ src, int base,
                                                             double* __restrict__ out, const int32_t* __restrict__ col, const double* __restrict__ dsc) {
  const int lane = threadIdx.x & 63, g4 = lane & 3, q = lane >> 2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p = wave; p < nblk * F * 4; p += nwaves) {
    const int64_t b = p / (F * 4);
    const int rem = (int)(p - b * (F * 4)), f = rem >> 2, sub = rem & 3;
    const int64_t p0 = ptr[b];
    const int Kb = (int)((ptr[b + 1] - p0) / 64);
    const int nl = sub * 16 + q;  // the node's lane in the product kernel
    const int64_t ns = b * 64 + nl;
    int64_t lo = 0;
    int L = 0;
    if (ns < ncp) {
      const int64_t i = nodeid[ns];
      lo = (int64_t)rowptr[(int64_t)f * ncp + i] - base;
      L = (int)(((int64_t)rowptr[(int64_t)f * ncp + i + 1] - base - lo) / F);
    }
    double* o = out + p0 * (F * F) + (int64_t)(f * F) * 64 + nl;
#pragma unroll
    for (int g = 0; g < F; ++g) {
      const double* sg = src + lo + (int64_t)g * L;
      const int32_t* cg = col + lo + (int64_t)g * L;
      double* og = o + (int64_t)g * 64;
      int t = g4;
      for (; t + 28 < Kb; t += 32) {  // eight loads of a lane in flight before the first store (four: 17.0 ms per bind of the hex-20 elasticity matrix at 96^3)
        double t8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int tu = t + 4 * u;
          t8[u] = tu < L ? (dsc ? sg[tu] / dsc[cg[tu] - base] : sg[tu]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) og[(int64_t)(t + 4 * u) * (64 * F * F)] = t8[u];
      }
      for (; t + 12 < Kb; t += 16) {
        double t4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int tu = t + 4 * u;
          t4[u] = tu < L ? (dsc ? sg[tu] / dsc[cg[tu] - base] : sg[tu]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) og[(int64_t)(t + 4 * u) * (64 * F * F)] = t4[u];
      }
      for (; t < Kb; t += 4) og[(int64_t)t * (64 * F * F)] = t < L ? (dsc ? sg[t] / dsc[cg[t] - base] : sg[t]) : 0.0;
    }
  }
}

// The same copy through an LDS transpose (round 6, for coupling lists of up to BSELL_T_MAXL nodes): a workgroup takes (block, row field f, column field g);
// its waves read the 64 nodes' g-segments of row (f, node) -- L contiguous values each, unit-stride lanes -- into LDS [node][t], then every slot t leaves
// as ONE 512-byte run of 64 lanes.  The quad-per-row form above reads 32-byte pieces and writes 128-byte pieces, 8 bytes per lane: 16.3 ms for the 15 GB
// of the hex-20 elasticity matrix at 96^3 (1.8 TB/s).
// (a first version with a workgroup per (block, f, g) ran at 15.3 ms: the copy is bound by the 1.9e9 gathers of dsc[column], not by its access pattern --
// the divisor depends on the COLUMN (g, coupled node) alone, so a workgroup now takes (block, g), gathers the divisors once into registers and walks the F
// row fields with them: a third of the gathers)
template <typename RP, int F>
__global__ __launch_bounds__(MFEM_BLOCK) void k_bsell_fill_t(int64_t ncp, int64_t nblk, const RP* __restrict__ rowptr, const int32_t* __restrict__ nodeid,
                                                               const int64_t* __restrict__ ptr, const double* __restrict__ src, int base,
                                                               double* __restrict__ out, const int32_t* __restrict__ col, const double* __restrict__ dsc,
                                                               int ldl) {
  extern __shared__ double tl[];  // [64][ldl] values, then [F][64] segment starts (int64), then [64] lengths (int)
  int64_t* s_lo = reinterpret_cast<int64_t*>(tl + (size_t)64 * ldl);
  int* s_L = reinterpret_cast<int*>(s_lo + F * 64);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int64_t job = blockIdx.x; job < nblk * F; job += gridDim.x) {
    const int64_t b = job / F;
    const int g = (int)(job - b * F);
    const int64_t p0 = ptr[b];
    const int Kb = (int)((ptr[b + 1] - p0) / 64);
    if (tid < 64) {
      const int64_t ns = b * 64 + tid;
      int L = 0;
      int64_t i = 0;
      if (ns < ncp) {
        i = nodeid[ns];
        L = (int)(((int64_t)rowptr[i + 1] - (int64_t)rowptr[i]) / F);
      }
#pragma unroll
      for (int f = 0; f < F; ++f) s_lo[f * 64 + tid] = ns < ncp ? (int64_t)rowptr[(int64_t)f * ncp + i] - base + (int64_t)g * L : 0;
      s_L[tid] = L;
    }
    __syncthreads();
    // the divisors of this wave's 16 nodes x 2 entries per lane (columns: from the node's first row -- every row field lists the same)
    double dv[4][4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int nl = w * 4 + 16 * q + u;
        const int64_t lo = s_lo[nl];
        const int L = s_L[nl];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int t = lane + 64 * h;
          dv[q][u][h] = (dsc && t < L) ? dsc[col[lo + t] - base] : 1.0;
        }
      }
    for (int f = 0; f < F; ++f) {
      // phase 1: a wave per node, four nodes' loads in flight
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double v[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int nl = w * 4 + 16 * q + u;
          const int64_t lo = s_lo[f * 64 + nl];
          const int L = s_L[nl];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int t = lane + 64 * h;
            v[u][h] = t < L ? src[lo + t] : 0.0;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int t = lane + 64 * h;
            if (t < Kb) tl[(size_t)(w * 4 + 16 * q + u) * ldl + t] = dsc ? v[u][h] / dv[q][u][h] : v[u][h];  // (zeros behind a node's own list: the block's padding)
          }
      }
      __syncthreads();
      // phase 2: a slot per wave trip, lane = node
      double* o = out + p0 * (F * F) + (int64_t)(f * F + g) * 64 + lane;
      for (int t = w; t < Kb; t += 4) o[(int64_t)t * (64 * F * F)] = tl[(size_t)lane * ldl + t];
      __syncthreads();
    }
  }
}

// y = alpha A x + beta y: a wave per block of 64 nodes, a lane per node, U node slots (their F x F values, column and F x entries) in flight
template <int F, int U>
__global__ __launch_bounds__(MFEM_BLOCK) void k_spmv_bsell(int64_t ncp, int64_t nblk, const int64_t* __restrict__ ptr, const int32_t* __restrict__ nodeid,
                                                             const int32_t* __restrict__ cols, const double* __restrict__ vals, const double* __restrict__ x,
                                                             double* __restrict__ y, double alpha, double beta, const double* __restrict__ dotw,
                                                             double* __restrict__ partials, const int32_t* __restrict__ done_flag) {
  __shared__ double red[4];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  constexpr int64_t SS = 64 * F * F;  // doubles per node slot of a block
  for (int64_t b = wave; b < nblk; b += nwaves) {
    const int64_t p0 = ptr[b];
    const int Kb = (int)((ptr[b + 1] - p0) / 64);
    const double* v = vals + p0 * (F * F) + lane;
    const int32_t* c = cols + p0 + lane;
    const int64_t ns = b * 64 + lane;
    const int64_t node = ns < ncp ? nodeid[ns] : 0;
    double acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0;
    int t = 0;
    for (; t + U <= Kb; t += U) {
      int32_t cu[U];
      double vv[U][F * F], xx[U][F];
#pragma unroll
      for (int u = 0; u < U; ++u) cu[u] = __builtin_nontemporal_load(c + (int64_t)(t + u) * 64);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int m = 0; m < F * F; ++m) vv[u][m] = __builtin_nontemporal_load(v + (int64_t)(t + u) * SS + m * 64);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int g = 0; g < F; ++g) xx[u][g] = x[(int64_t)cu[u] + (int64_t)g * ncp];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
          for (int g = 0; g < F; ++g) acc[f] += vv[u][f * F + g] * xx[u][g];
    }
    for (; t < Kb; ++t) {
      const int64_t cc = c[(int64_t)t * 64];
#pragma unroll
      for (int g = 0; g < F; ++g) {
        const double xg = x[cc + (int64_t)g * ncp];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] += __builtin_nontemporal_load(v + (int64_t)t * SS + (f * F + g) * 64) * xg;
      }
    }
    if (ns < ncp) {
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const int64_t r = (int64_t)f * ncp + node;
        double yv = alpha * acc[f];
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

// A->nb_F: the field count F (SELL_NODE_FIELDS, tried in order) for which the pattern is node-blocked, 0 if none.  Once per pattern (the check
// reads every column index: 61 ms for the 1.9e9 entries of hex-20 elasticity at 96^3).
int mfem_node_block_fields(mfem_context_s* ctx, mfem_csr_s* A) {
  if (A->nb_F > 0 || A->nb_checked) return MFEM_OK;
  A->nb_checked = 1;
  A->nb_F = 0;
  const SellShape S = mfem_sell_shape(A);
  if (!sell_node_check_possible(S)) return MFEM_OK;
  int32_t* d_bad = ctx->d_flags + 9;
  for (int ci = 0; ci < 3 && A->nb_F == 0; ++ci) {
    const int f = SELL_NODE_FIELDS[ci];
    if (!sell_fields_divide(S, f)) continue;
    const int64_t ncp = A->n / f;
    MFEM_CHECK_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), ctx->stream));
    const int grid = mfem_grid_for(ncp, MFEM_BLOCK, ctx->num_cus * 16);
    mfem_by_rowptr(A, [&](auto rp) {
      using RP = decltype(rp);
      hipLaunchKernelGGL(k_bsell_check<RP>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, ncp, f, (const RP*)A->rowptr, A->colidx, A->index_base, d_bad);
    });
    MFEM_CHECK_LAUNCH();
    MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 9, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->h_flags[9] == 0) A->nb_F = f;
  }
  return MFEM_OK;
}

// stages of the plan: nodes stably sorted by decreasing length of their coupling list, node slots x 64 of every block and their prefix sums
static int bsell_plan_sort(mfem_context_s* ctx, const mfem_csr_s* A, int F, SellSortBufs<uint32_t>& B, int64_t* slots) {
  const int64_t ncp = A->n / F, nblk = bsell_blocks(ncp);
  const int maxL = A->max_row_nnz / F;
  const int rc = B.alloc(ncp, nblk);
  if (rc) return rc;
  mfem_by_rowptr(A, [&](auto rp) {
    using RP = decltype(rp);
    hipLaunchKernelGGL(k_bsell_keys<RP>, dim3(mfem_grid_for(ncp, MFEM_BLOCK, ctx->num_cus * 16)), dim3(MFEM_BLOCK), 0, ctx->stream, ncp, F, maxL,
                       (const RP*)A->rowptr, B.keys.p, B.ids.p);
  });
  MFEM_CHECK_LAUNCH();
  return mfem_sell_sort_blocks<uint32_t>(ctx, B, ncp, sell_len_bits(maxL), nblk, [&](const int32_t* nodeid, int64_t* sizes) {
    mfem_by_rowptr(A, [&](auto rp) {
      using RP = decltype(rp);
      hipLaunchKernelGGL(k_bsell_block_sizes<RP>, dim3(mfem_grid_for(nblk, MFEM_BLOCK, ctx->num_cus * 16)), dim3(MFEM_BLOCK), 0, ctx->stream, nblk, F,
                         (const RP*)A->rowptr, nodeid, sizes);
    });
  }, slots);
}
// ... and the node-level columns
static int bsell_plan_cols(mfem_context_s* ctx, const mfem_csr_s* A, int F, const SellSortBufs<uint32_t>& B, int64_t slots, DevBuf<int32_t>& cols) {
  const int64_t ncp = A->n / F, nblk = bsell_blocks(ncp);
  MFEM_CHECK_HIP(cols.alloc((size_t)(slots > 0 ? slots : 1)));
  const int g2 = mfem_grid_for(nblk * 64, MFEM_BLOCK, ctx->num_cus * 16);
  mfem_by_rowptr(A, [&](auto rp) {
    using RP = decltype(rp);
    hipLaunchKernelGGL(k_bsell_cols<RP>, dim3(g2), dim3(MFEM_BLOCK), 0, ctx->stream, ncp, nblk, F, (const RP*)A->rowptr, A->colidx, A->index_base, B.sorted.p,
                       B.ptr.p, cols.p);
  });
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
// Plans the node-blocked layout if the pattern has its form and the padding is accepted: *L is filled then, and left alone otherwise.
int mfem_bsell_plan(mfem_context_s* ctx, mfem_csr_s* A, const SellShape& S, SellLayout* L) {
  if (!bsell_may_try(S, bsell_knobs_decode(g_bsell_word))) return MFEM_OK;
  int rc = mfem_node_block_fields(ctx, A);
  if (rc) return rc;
  const int F = A->nb_F;
  if (!bsell_enough_nodes(S, F)) return MFEM_OK;
  SellSortBufs<uint32_t> B;
  DevBuf<int32_t> cols;
  int64_t slots = 0;
  rc = bsell_plan_sort(ctx, A, F, B, &slots);
  if (rc || !bsell_padding_ok(S, F, slots)) return rc;
  rc = bsell_plan_cols(ctx, A, F, B, slots, cols);
  if (rc) return rc;
  L->form = SELL_NODE_BLOCKED;
  L->total = slots * F * F;
  L->nblk = bsell_blocks(S.n / F);
  L->nodes = {F, S.n / F, slots, B.sorted.release(), B.ptr.release(), cols.release()};
  return MFEM_OK;
}

template <typename RP> static auto bsell_fill_t_kernel(int F) -> decltype(&k_bsell_fill_t<RP, 3>) {
  return F == 3 ? k_bsell_fill_t<RP, 3> : F == 2 ? k_bsell_fill_t<RP, 2> : k_bsell_fill_t<RP, 4>;
}
template <typename RP> static auto bsell_fill_kernel(int F) -> decltype(&k_bsell_fill<RP, 3>) {
  return F == 3 ? k_bsell_fill<RP, 3> : F == 2 ? k_bsell_fill<RP, 2> : k_bsell_fill<RP, 4>;
}
// The values into the layout (once per solve): through the LDS transpose, or by lane quads (bsell_copy)
int mfem_bsell_fill(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc) {
  const SellLayout& L = A->sell;
  const SellLayout::Nodes& N = L.nodes;
  const BsellCopy C = bsell_copy(A->max_row_nnz / N.F, N.F, bsell_knobs_decode(g_bsell_word));
  mfem_by_rowptr(A, [&](auto rp) {
    using RP = decltype(rp);
    if (C.transpose)
      hipLaunchKernelGGL(bsell_fill_t_kernel<RP>(N.F), dim3(bsell_copy_grid(L.nblk, N.F, ctx->num_cus)), dim3(MFEM_BLOCK), C.lds_bytes, ctx->stream, N.ncp, L.nblk,
                         (const RP*)A->rowptr, N.nodeid, N.ptr, vals, A->index_base, buf, A->colidx, dsc, C.ldl);
    else
      hipLaunchKernelGGL(bsell_fill_kernel<RP>(N.F), dim3(mfem_grid_for(L.nblk * N.F * 4 * 64, MFEM_BLOCK, ctx->num_cus * 16)), dim3(MFEM_BLOCK), 0, ctx->stream,
                         N.ncp, L.nblk, (const RP*)A->rowptr, N.nodeid, N.ptr, vals, A->index_base, buf, A->colidx, dsc);
  });
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}

static auto bsell_kernel(BsellFU k) -> decltype(&k_spmv_bsell<3, 3>) {
  switch (k.F * 16 + k.U) {
    case 3 * 16 + 1: return k_spmv_bsell<3, 1>;
    case 3 * 16 + 2: return k_spmv_bsell<3, 2>;
    case 3 * 16 + 4: return k_spmv_bsell<3, 4>;
    case 2 * 16 + 4: return k_spmv_bsell<2, 4>;
    case 4 * 16 + 2: return k_spmv_bsell<4, 2>;
    default: return k_spmv_bsell<3, 3>;
  }
}
// The product of a bound node-blocked copy (no ghost columns: never split -- part 1 is the whole product, part 2 nothing).  Returns 1: launched.
int mfem_bsell_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* x, double* y, double alpha, double beta, const double* dotw, double* partials,
                      int* n_partials, const int32_t* done_flag, int part) {
  if (part == 2) return 1;
  const SellLayout& L = A->sell;
  const SellKnobs K = mfem_sell_knobs();
  const int grid = mfem_grid_for(L.nblk * 64, MFEM_BLOCK, sell_grid_cap(ctx->num_cus, K, MFEM_MAX_PARTIALS, 0));
  hipLaunchKernelGGL(bsell_kernel(bsell_fu_resolved(L.nodes.F, K)), dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, L.nodes.ncp, L.nblk, L.nodes.ptr,
                     L.nodes.nodeid, L.nodes.cols, L.vals, x, y, alpha, beta, dotw, partials, done_flag);
  MFEM_CHECK_LAUNCH();
  ++g_bsell_spmv_count;
  if (n_partials && partials) *n_partials = grid;
  return 1;
}
