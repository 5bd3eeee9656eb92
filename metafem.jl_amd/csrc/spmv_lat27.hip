// Symmetric lattice-tile layout for the Krylov loop on the hex-27 (order-2 Lagrange, one field) lattice matrix: solver layout mode 4.
// The caller-facing contract stays CSR (mul!, misc/04_GPU_Utils.jl:131; iterative_Solve!, solver/03_Iterative_Solvers.jl:31-49).
//
// Why: the row-sorted sliced layout (spmv_sell.hip) streams all 64 entries of an average hex-27 row and gathers x from global memory
// (10 L1 accesses per value line, 1.33 x the design bytes from HBM: profiles/r03_sell_memory_path.txt).  A hex-27 stiffness matrix
// that CG may be run on is symmetric, and its pattern is a lattice stencil whose reach depends on the parity of the node in each
// direction (even = element boundary: offsets -2..2, odd = element interior: -1..1; 8 node types, 27..125 entries per row).
//
//   * layout (per solve, one pass over the CSR values): only the diagonal and the entries with column > row are stored -- 14..63 of a
//     row's 27..125.  Rows are grouped in units of 4 x 4 x 8 lattice points = 16 rows of each of the 8 types; a wave owns a unit, four
//     lanes share a row and take every fourth stored entry, so a unit is 68 wave-wide 16-byte-per-lane... (8 bytes per lane per step,
//     two steps per 16-byte load) unit-stride steps: 34.8 KB instead of the 65.5 KB of its 8 192 entries.  No column stream: the column of
//     a slot is the row's lattice position plus a per-type table entry.
//   * SpMV, pass 1 (k_spmv_lat27): a workgroup owns a tile of 8 x 8 x 32 lattice points (16 units, 8 waves).  It stages x of the tile and
//     of the (+2, +-2, +-2) neighbourhood its stored entries reach in LDS (4 320 cells), and accumulates y in a second LDS block of
//     the same shape: for a stored entry a = A[r][c] the lane adds a x[c] to its register sum for row r and a x[r] to cell c
//     (ds_add_f64) -- the mirrored entry A[c][r] is never read.  The whole y block -- own cells and neighbourhood -- leaves as one
//     contiguous 34.6 KB run per tile.
//   * pass 2 (spmv_lat27_gather.hip): row r sums the up to 18 tiles whose block covers it, in a fixed order, applies alpha / beta and the fused
//     dot product.  No global atomics; 2.1 cells per row written and read again (+ 12 % traffic).
//   * eligibility is decided in two steps: the pattern must BE the lattice stencil (checked entry by entry once per pattern), and the values
//     of this solve must be symmetric: measured per bind with a probe product (sym_probe.hip: the layout against the CSR kernel on one
//     vector); the sliced layout serves the solve when a row of the two products differs by more than LAT_SYM_GATE (lat_decide.h) of that row's diagonal entry.  A right Jacobi scaling (bicgstabl_GS!, idrs!, cgs2! work on A D^-1, which is not
//     symmetric) is applied to x while it is staged: (A D^-1) x = A (x / d), so the stored matrix stays the symmetric A.
//   * y differs from the CSR kernel's by round-off (other summation order), and the order in which the waves of a workgroup add into
//     an LDS cell is not fixed: results are reproducible to ~1e-16 relative, not bitwise (mfem_debug_set_lat27(0) selects the sliced layout).
// The host decisions (knobs, eligibility, geometry, sizes, the split of a slab's launch): lat_decide.h.
#include "blas1.h"
#include "layouts.h"
#include "spmv_lat27.h"

typedef double l_d2 __attribute__((ext_vector_type(2)));

extern std::atomic<int64_t> g_layout_min_rows_lat27;  // spmv_ell.hip
static std::atomic<int> g_lat27_word{LAT27_WORD_DEFAULT};  // mfem_debug_set_lat27 (Lat27Knobs)
static Lat27Knobs lat27_knobs() { return lat27_knobs_decode(g_lat27_word); }
static LatShape lat27_shape(const mfem_csr_s* A) { return mfem_lat_shape(A, g_layout_min_rows_lat27); }
static std::atomic<long long> g_lat27_count{0};
extern "C" long long mfem_debug_lat27_spmv_count(void) { return g_lat27_count; }  // SpMVs the layout has served (bench.py: which kernel ran)
// what the symmetry probe of the last bind on this pattern measured (0: no bind yet)
extern "C" double mfem_debug_lat27_asymmetry(mfem_csr A) { return A ? A->lat27.asym : -1.0; }
extern "C" int mfem_debug_set_lat27(int enable) try {
  ++mfem_debug_epoch;
  g_lat27_word = enable & 15;
  return MFEM_OK;
} MFEM_API_CATCH("mfem_debug_set_lat27")

// type t = 4 (i odd) + 2 (j odd) + (k odd); steps per lane K4, stored slots Kup, group base inside a unit (doubles), table base (entries)
__constant__ int c_l27_Kup[8];
__constant__ int16_t c_l27_off[L27_TAB];   // [tb[t] + q * K4 + it]: LDS cell offset of slot it * 4 + q (0 for padding)
__constant__ int8_t c_l27_d[L27_TAB][4];   // same index: (di, dj, dk) of the slot; di = L27_PAD for padding
__constant__ int c_l27_K4[8];
__constant__ int c_l27_gb[8];
__constant__ int c_l27_tb[8];
static std::atomic<bool> g_l27_tables{false};

static int lat27_upload_tables() {
  static std::mutex mu;  // uploads from two host threads must not interleave (the tables themselves are process-wide: see the threading note in include/metafem_mi355x.h)
  std::lock_guard<std::mutex> lk(mu);
  if (g_l27_tables) return MFEM_OK;
  int Kup[8];
  int16_t off[L27_TAB];
  int8_t d[L27_TAB][4];
  if (!l27_build_tables(d, Kup)) return MFEM_ERR_INVALID;  // (spmv_lat_tables.h)
  for (int i = 0; i < L27_TAB; ++i) off[i] = d[i][0] == L27_PAD ? (int16_t)0 : (int16_t)(d[i][0] * L27_PI + d[i][1] * L27_SK + d[i][2]);
  if (hipMemcpyToSymbol(HIP_SYMBOL(c_l27_Kup), Kup, sizeof(Kup)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_l27_off), off, sizeof(off)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_l27_d), d, sizeof(d)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_l27_K4), l27_K4, sizeof(l27_K4)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_l27_gb), l27_gb, sizeof(l27_gb)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_l27_tb), l27_tb, sizeof(l27_tb)) != hipSuccess) {
    mfem_set_error("lattice-tile tables: hipMemcpyToSymbol failed");
    return MFEM_ERR_HIP;
  }
  g_l27_tables = true;
  return MFEM_OK;
}

// 1 in *bad if some row is not the lattice stencil row: length = product of the per-direction ranges, columns in lexicographic order
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_l27_verify(Lat27Geom G, const RP* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             int base, int32_t* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t PL = (int64_t)G.m1 * G.m2;
  int fail = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < G.n; r += stride) {
    const int gi = (int)(r / PL) + G.plo;  // global plane
    const int64_t rem = r % PL;
    const int gj = (int)(rem / G.m2), gk = (int)(rem - (int64_t)gj * G.m2);
    int li, ni, lj, nj, lk, nk;
    l27_range(gi, G.mg, li, ni);
    l27_range(gj, G.m1, lj, nj);
    l27_range(gk, G.m2, lk, nk);
    const int64_t lo = (int64_t)rowptr[r] - base, hi = (int64_t)rowptr[r + 1] - base;
    if (hi - lo != (int64_t)ni * nj * nk) {
      fail = 1;
      continue;
    }
    int64_t j = lo;
    for (int a = 0; a < ni; ++a)
      for (int b = 0; b < nj; ++b) {
        const int64_t c0 = l27_xindex(G, gi + li + a, (int64_t)(gj + lj + b) * G.m2 + gk + lk);
        for (int c = 0; c < nk; ++c, ++j)
          if ((int64_t)col[j] - base != c0 + c) fail = 1;
      }
  }
  if (fail) bad[0] = 1;
}

// The layout pass: a wave per unit.  stats[1] = max |A[r][c]| over the stored entries (bit pattern of a non-negative double, which orders like
// an integer).
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_l27_fill(Lat27Geom G, const RP* __restrict__ rowptr, int base,
                                                           const double* __restrict__ vals, double* __restrict__ out,
                                                           unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63, q = lane & 3, rho = lane >> 2;
  const int ra = rho >> 3, rb = (rho >> 2) & 1, rc = rho & 3;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t nunits = (int64_t)G.nui * G.nuj * G.nuk;
  double amax = 0.0;
  for (int64_t u = wave; u < nunits; u += nwaves) {
    const int uk = (int)(u % G.nuk);
    const int64_t u2 = u / G.nuk;
    const int uj = (int)(u2 % G.nuj), ui = (int)(u2 / G.nuj);
    double* ou = out + u * L27_UNIT_D;
    for (int t = 0; t < 8; ++t) {
      const int oi = ui * 4 + ((t >> 2) & 1) + 2 * ra, gj = uj * 4 + ((t >> 1) & 1) + 2 * rb, gk = uk * 8 + (t & 1) + 2 * rc;  // oi: owned plane
      const int gi = oi + G.plo;
      const bool valid = oi < G.m0 && gj < G.m1 && gk < G.m2;
      const int64_t r = ((int64_t)oi * G.m1 + gj) * G.m2 + gk;
      int li = 0, ni = 1, lj = 0, nj = 1, lk = 0, nk = 1;
      int64_t rp = 0;
      if (valid) {
        l27_range(gi, G.mg, li, ni);
        l27_range(gj, G.m1, lj, nj);
        l27_range(gk, G.m2, lk, nk);
        rp = (int64_t)rowptr[r] - base;
      }
      const int K4 = c_l27_K4[t], tb = c_l27_tb[t] + q * K4;
      double* og = ou + c_l27_gb[t] + lane * 2;
      for (int it = 0; it < K4; it += 2) {
        l_d2 pr;
        pr.x = 0.0;
        pr.y = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int di = c_l27_d[tb + it + h][0], dj = c_l27_d[tb + it + h][1], dk = c_l27_d[tb + it + h][2];
          const int ci = gi + di, cj = gj + dj, ck = gk + dk;
          if (valid && di != L27_PAD && ci < G.mg && cj >= 0 && cj < G.m1 && ck >= 0 && ck < G.m2) {  // (ci may be a ghost plane of a slab)
            const double v = vals[rp + ((int64_t)(di - li) * nj + (dj - lj)) * nk + (dk - lk)];
            double av = fabs(v);
            if (!(av == av)) av = __builtin_huge_val();  // NaN: fmax would drop it
            amax = fmax(amax, av);
            if (h) pr.y = v; else pr.x = v;
          }
        }
        *(l_d2*)(og + (int64_t)(it >> 1) * 128) = pr;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_down(amax, o, MFEM_WAVE));
  if (lane == 0) atomicMax(stats + 1, (unsigned long long)__double_as_longlong(amax));
}

// A unit's 68 steps run as 5 chunks of 16 / 10 / 10 / 16 / 16 steps (type 0; type 1; type 2; types 3 + 4; types 5 + 6 + 7: neighbours in the unit's
// storage); the values of chunk k + 1 are in flight while chunk k is worked through LDS (two register buffers that swap roles; 9 smaller chunks left
// 32 - 64 bytes per lane in flight, this keeps 80 - 128).
template <int N>
__device__ __forceinline__ void l27_load(l_d2 (&v)[8], const double* __restrict__ gv) {
#pragma unroll
  for (int u = 0; u < N / 2; ++u) v[u] = __builtin_nontemporal_load((const l_d2*)gv + u * 64);
}

// N steps of one type from v[OFF ...] (OFF in 16-byte pairs)
template <int N, int OFF>
__device__ __forceinline__ void l27_proc(const l_d2 (&v)[8], const uint32_t* __restrict__ tq, int pos, int q, const double* xs, double* ys) {
  uint32_t w[N / 2];
#pragma unroll
  for (int u = 0; u < N / 2; ++u) w[u] = tq[u];
  const double xr = xs[pos];
  double acc = 0.0;
#pragma unroll
  for (int it = 0; it < N; ++it) {
    const int o = (it & 1) ? ((int)w[it >> 1] >> 16) : (int)(int16_t)(w[it >> 1] & 0xffffu);
    const double a = (it & 1) ? v[OFF + (it >> 1)].y : v[OFF + (it >> 1)].x;
    acc += a * xs[pos + o];
    double m = a * xr;
    if (it == 0) m = q == 0 ? 0.0 : m;  // slot 0 is the diagonal: nothing to mirror
    __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double*)(ys + pos + o), m);
  }
  acc += __shfl_xor(acc, 1, MFEM_WAVE);
  acc += __shfl_xor(acc, 2, MFEM_WAVE);
  if (q == 0) __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double*)(ys + pos), acc);
}

// on entry A holds the unit's first chunk; on exit B holds the first chunk of the unit at uv_next (if any)
__device__ __forceinline__ void l27_unit(l_d2 (&A)[8], l_d2 (&B)[8], const double* __restrict__ uv, const double* __restrict__ uv_next,
                                         int p0, int q, const uint32_t* __restrict__ tabs, const double* xs, double* ys) {
  const int PI = L27_PI, PJ = L27_SK;
  l27_load<10>(B, uv + 1024);
  l27_proc<16, 0>(A, tabs + q * 8, p0, q, xs, ys);                     // type 0
  l27_load<10>(A, uv + 1664);
  l27_proc<10, 0>(B, tabs + 32 + q * 5, p0 + 1, q, xs, ys);            // type 1 (k odd)
  l27_load<16>(B, uv + 2304);
  l27_proc<10, 0>(A, tabs + 52 + q * 5, p0 + PJ, q, xs, ys);           // type 2 (j odd)
  l27_load<16>(A, uv + 3328);
  l27_proc<6, 0>(B, tabs + 72 + q * 3, p0 + PJ + 1, q, xs, ys);        // type 3
  l27_proc<10, 3>(B, tabs + 84 + q * 5, p0 + PI, q, xs, ys);           // type 4 (i odd)
  if (uv_next) l27_load<16>(B, uv_next);
  l27_proc<6, 0>(A, tabs + 104 + q * 3, p0 + PI + 1, q, xs, ys);       // type 5
  l27_proc<6, 3>(A, tabs + 116 + q * 3, p0 + PI + PJ, q, xs, ys);      // type 6
  l27_proc<4, 6>(A, tabs + 128 + q * 2, p0 + PI + PJ + 1, q, xs, ys);  // type 7
}

// What both forms of pass 1 do around their products.  x of the tile's box -- own points and the (+2, +-2, +-2) neighbourhood -- into xs, divided by d
// under a right Jacobi scaling; ys cleared.
__device__ __forceinline__ void l27_stage_x(Lat27Geom G, const double* x, const double* dsc, int ti, int tj, int tk, int tid, double* xs, double* ys) {
  const int i0 = ti * L27_TI, j0 = tj * L27_TJ - 2, k0 = tk * L27_TK - 2;
  for (int e = tid; e < L27_LDS_CELLS; e += 512) {
    const int li = e / L27_PI, r2 = e - li * L27_PI, lj = r2 / L27_SK, lk = r2 - lj * L27_SK;
    const int gi = G.plo + i0 + li, gj = j0 + lj, gk = k0 + lk;  // global plane: the two planes behind the last owned one are ghost planes
    double xv = 0.0;
    if (lj < L27_SJ && gi < G.mg && gi < G.plo + G.m0 + G.gw && gj >= 0 && gj < G.m1 && gk >= 0 && gk < G.m2) {
      const int64_t r = l27_xindex(G, gi, (int64_t)gj * G.m2 + gk);
      xv = dsc ? x[r] / dsc[r] : x[r];
    }
    xs[e] = xv;
    ys[e] = 0.0;
  }
}
// the tile's y block leaves as one contiguous run; dotp: the tile's share of x . A x beside it
__device__ __forceinline__ void l27_write_block(const double* xs, const double* ys, double* dump, int tile, int tid, double* dotp, double* dred) {
  double* dt = dump + (int64_t)tile * L27_CELLS;
  double dacc = 0.0;
  for (int e = tid; e < L27_CELLS; e += 512) {
    const int li = e / (L27_SJ * L27_SK);
    const double yv = ys[e + 8 * li];
    dt[e] = yv;
    dacc += yv * xs[e + 8 * li];
  }
  if (dotp) {  // (kernel argument: every thread of the workgroup takes the same way)
    const double d = block_reduce_sum(dacc, dred);
    if (tid == 0) dotp[tile] = d;
  }
}

// pass 1: one workgroup per tile.  dump[tile][cell] = what the tile's stored entries contribute to y on its own cells and on the
// (+2, +-2, +-2) neighbourhood.
// dsc != nullptr: the operator is A D^-1 (right Jacobi scaling, Mat_Div_Jacobi of 02_Preconditioner.jl:141-148): the stored matrix stays the
// symmetric A and x is divided by d while it is staged.
// dotp != nullptr (the fused CG iteration, no column scaling): dotp[tile] = sum over the tile's block of x(cell) * y-contribution(cell); summed over the tiles that is
// x . A x -- every contribution to y[r] sits in exactly one cell of one block, beside the x[r] the tile staged -- so the dot product of a CG iteration needs no pass 2.
__global__ __launch_bounds__(512, 4) void k_spmv_lat27(Lat27Geom G, const double* __restrict__ vals, const double* __restrict__ x,
                                                       const double* __restrict__ dsc, double* __restrict__ dump,
                                                       const int32_t* __restrict__ done_flag, int tile0, int tcount, double* __restrict__ dotp) {
  __shared__ double xs[L27_LDS_CELLS];
  __shared__ double ys[L27_LDS_CELLS];
  __shared__ uint32_t tabs[L27_TAB / 2];
  __shared__ double dred[8];
  if (done_flag && done_flag[0]) return;
  // (this launch covers the tiles [tile0, tile0 + tcount) of the i-major tile list: all of them, or the interior / boundary part of a slab's SpMV)
  int tsub;
  if (!mfem_xcd_tile(tcount, tsub)) return;
  const int tile = tile0 + tsub;
  const int tk = tile % G.ntk, t2 = tile / G.ntk, tj = t2 % G.ntj, ti = t2 / G.ntj;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6, q = lane & 3, rho = lane >> 2;
  const int ra = rho >> 3, rb = (rho >> 2) & 1, rc = rho & 3;
  // the wave's two units: (0, b, c) and (1, b, c) of the tile's 2 x 2 x 4; the second exists only if the first does
  const int ub = (wv >> 2) & 1, uc = wv & 3;
  const int ui = ti * 2, uj = tj * 2 + ub, uk = tk * 4 + uc;
  const bool e0 = uj < G.nuj && uk < G.nuk, e1 = e0 && ui + 1 < G.nui;
  const double* uv0 = vals + (((int64_t)ui * G.nuj + uj) * G.nuk + uk) * L27_UNIT_D + lane * 2;
  const double* uv1 = uv0 + (int64_t)G.nuj * G.nuk * L27_UNIT_D;
  l_d2 A[8], B[8];
  if (e0) l27_load<16>(A, uv0);  // in flight while x is staged
  for (int e = tid; e < L27_TAB / 2; e += 512)
    tabs[e] = (uint32_t)(uint16_t)c_l27_off[2 * e] | ((uint32_t)(uint16_t)c_l27_off[2 * e + 1] << 16);
  l27_stage_x(G, x, dsc, ti, tj, tk, tid, xs, ys);
  __syncthreads();
  if (e0) {
    // LDS cell of the lane's row of type (0, 0, 0) in the first unit; the other types are +1 in the odd directions, the second unit 4 planes on
    const int p0 = (2 * ra) * L27_PI + (ub * 4 + 2 * rb + 2) * L27_SK + (uc * 8 + 2 * rc + 2);
    l27_unit(A, B, uv0, e1 ? uv1 : nullptr, p0, q, tabs, xs, ys);
    if (e1) l27_unit(B, A, uv1, nullptr, p0 + 4 * L27_PI, q, tabs, xs, ys);
  }
  __syncthreads();
  l27_write_block(xs, ys, dump, tile, tid, dotp, dred);
}


// =====================================================================================================================================================
// Deterministic form of pass 1 (round 6; tables and the argument: spmv_lat_tables.h, "mode 4, deterministic order").  LANE = ROW: a wave owns the rows of
// four node types in a cube of 8 x 8 x 8 lattice points, the two waves of a cube split the types by the parity of their (j, k) column, a tile of
// 8 x 8 x 32 points = 4 cubes = 8 waves as before.  Every stored slot is one wave-wide step with a compile-time offset; the steps run phase-major -- a phase =
// the (dj, dk) of the offset -- with LDS-only barriers between phases, so every cell of the tile's y block receives its mirrored products from one wave
// per phase in program order: y is bitwise the same from run to run.  A cube's 260 steps are stored as its two waves' streams (138 + 122 steps of 64
// lanes), a pair of steps per lane side by side: each wave reads its 70 / 62 KB front to back with 16-byte loads.  bit 3 of the "lat27" knob selects
// the four-lanes-per-row kernel above (ds_add_f64 across waves: ~1e-16, not bitwise) for the A/B.
__host__ __device__ constexpr int l27d_coff(int di, int dj, int dk) { return di * L27_PI + dj * L27_SK + dk; }
__host__ __device__ constexpr int l27d_toff(int t) { return ((t >> 2) & 1) * L27_PI + ((t >> 1) & 1) * L27_SK + (t & 1); }

template <int PG, int V0, int N>
__device__ __forceinline__ void l27d_load(double (&v)[8], const double* __restrict__ sb) {
  static_assert(V0 % 2 == 0 && N % 2 == 0, "stream steps leave in pairs");
#pragma unroll
  for (int i = 0; i < N; i += 2) {
    const l_d2 pr = __builtin_nontemporal_load((const l_d2*)sb + (int64_t)((V0 + i) >> 1) * 64);
    v[i] = pr.x;
    v[i + 1] = pr.y;
  }
}
// the barriers of `n` phase changes (a phase without a step of this wave's types still has its barrier: both waves of a cube, and all cubes, meet 24 times)
template <int n>
__device__ __forceinline__ void l27d_barriers() {
  if constexpr (n > 0) {
    mfem_lds_barrier();
    l27d_barriers<n - 1>();
  }
}
template <int PG, int V0, int I, int N>
__device__ __forceinline__ void l27d_proc(const double (&v)[8], int p0, bool act, const double (&xo)[4], double (&acc)[4], const double* xs, double* ys) {
  if constexpr (I < N) {
    constexpr L27DStream S = l27d_stream(PG);
    constexpr int vv = V0 + I, q = S.q[vv], t = l27d_type(PG, q);
    constexpr int coff = l27d_toff(t) + l27d_coff(S.di[vv], S.dj[vv], S.dk[vv]);
    l27d_barriers<(vv == 0 ? S.phase[0] : S.phase[vv] - S.phase[vv > 0 ? vv - 1 : 0])>();
    if (act) {  // (wave-uniform)
      const double a = v[I];
      acc[q] += a * xs[p0 + coff];
      if constexpr (!(S.di[vv] == 0 && S.dj[vv] == 0 && S.dk[vv] == 0))
        __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double*)(ys + p0 + coff), a * xo[q]);  // (the diagonal has no mirror)
    }
    l27d_proc<PG, V0, I + 1, N>(v, p0, act, xo, acc, xs, ys);
  }
}
template <int PG, int C>
__device__ __forceinline__ void l27d_run(double (&A)[8], double (&B)[8], const double* __restrict__ sb, int p0, bool act, const double (&xo)[4],
                                         double (&acc)[4], const double* xs, double* ys) {
  constexpr int NV = l27d_stream(PG).n, NCH = (NV + 7) / 8, LAST = NCH - 1;
  constexpr int nthis = (C == LAST) ? NV - 8 * LAST : 8;
  if constexpr (C < LAST) {
    constexpr int nnext = (C + 1 == LAST) ? NV - 8 * LAST : 8;
    l27d_load<PG, (C + 1) * 8, nnext>((C & 1) ? A : B, sb);
  }
  __builtin_amdgcn_sched_barrier(0);
  l27d_proc<PG, C * 8, 0, nthis>((C & 1) ? B : A, p0, act, xo, acc, xs, ys);
#pragma unroll
  for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(acc[q]));
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (C < LAST) l27d_run<PG, C + 1>(A, B, sb, p0, act, xo, acc, xs, ys);
}
template <int PG>
__device__ __forceinline__ void l27d_wave(const double* __restrict__ sb, int p0, bool act, const double* xs, double* ys) {
  constexpr L27DStream S = l27d_stream(PG);
  double A[8], B[8];
  l27d_load<PG, 0, 8>(A, sb);
  double xo[4], acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    xo[q] = xs[p0 + l27d_toff(l27d_type(PG, q))];
    acc[q] = 0.0;
  }
  l27d_run<PG, 0>(A, B, sb, p0, act, xo, acc, xs, ys);
  l27d_barriers<L27D_NPHASE - 1 - S.phase[S.n - 1]>();  // (none: the last phase holds the diagonal of every type)
  if (act) {  // the row sums: still the last phase (own cells; the other adds into them in this phase come from this wave)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double*)(ys + p0 + l27d_toff(l27d_type(PG, q))), acc[q]);
  }
}

// pass 1, deterministic: same tile, same dump, same arguments as k_spmv_lat27
__global__ __launch_bounds__(512, 4) void k_spmv_lat27d(Lat27Geom G, const double* __restrict__ vals, const double* __restrict__ x,
                                                        const double* __restrict__ dsc, double* __restrict__ dump,
                                                        const int32_t* __restrict__ done_flag, int tile0, int tcount, double* __restrict__ dotp) {
  __shared__ double xs[L27_LDS_CELLS];
  __shared__ double ys[L27_LDS_CELLS];
  __shared__ double dred[8];
  if (done_flag && done_flag[0]) return;
  int tsub;
  if (!mfem_xcd_tile(tcount, tsub)) return;
  const int tile = tile0 + tsub;
  const int tk = tile % G.ntk, t2 = tile / G.ntk, tj = t2 % G.ntj, ti = t2 / G.ntj;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int cu = wv >> 1, pg = wv & 1;
  const int nck = (G.m2 + 7) >> 3, ncj = G.ntj;  // cubes per direction (a tile is one cube in i and j, four in k)
  const int ck = tk * 4 + cu;
  const bool act = ck < nck;
  // a cube that does not exist (lattice edge in k) is read from a place that does and not worked on
  const double* sb = vals + (act ? (((int64_t)ti * ncj + tj) * nck + ck) * (int64_t)L27D_CUBE_D : 0) + (pg ? (int64_t)l27d_stream(0).n * 64 : 0) + lane * 2;
  l27_stage_x(G, x, dsc, ti, tj, tk, tid, xs, ys);
  __syncthreads();
  {
    const int a = lane >> 4, b = (lane >> 2) & 3, c = lane & 3;
    const int p0 = (2 * a) * L27_PI + (2 * b + 2) * L27_SK + (cu * 8 + 2 * c + 2);  // the lane's row of type (0, 0, 0)
    if (pg == 0) l27d_wave<0>(sb, p0, act, xs, ys);
    else l27d_wave<1>(sb, p0, act, xs, ys);
  }
  __syncthreads();
  l27_write_block(xs, ys, dump, tile, tid, dotp, dred);
}

// the layout pass of the deterministic form: a wave per (cube, parity group), lane = row.  A lane walks the UPPER HALF of its CSR row front to back (the
// stored slots of a type in lexicographic order = ascending columns: each 128-byte line of the row is used up by 16 consecutive loads of the lane while it
// sits in the L1) and drops every value at its place in the phase-major stream (8-byte stores; the two halves of a 16-byte pair come from two steps).  A
// first version read in STREAM order -- 64 rows per instruction, each row touched again and again over 60 steps: 11.6 ms per bind of the 128^3 matrix
// against 2.65 ms of the four-lanes-per-row fill.
__constant__ uint8_t c_l27d_lex[2][4][64][4];  // [pg][q][e]: (di, dj + 2, dk + 2, stream step v) of the e-th stored slot of the wave's q-th type, lexicographic
__constant__ int c_l27d_kup[2][4];
static std::atomic<bool> g_l27d_tables{false};
static int lat27d_upload_tables() {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (g_l27d_tables) return MFEM_OK;
  static uint8_t h[2][4][64][4];
  int kup[2][4];
  memset(h, 0, sizeof(h));
  for (int pg = 0; pg < 2; ++pg) {
    const L27DStream S = l27d_stream(pg);
    for (int q = 0; q < 4; ++q) {
      const int t = l27d_type(pg, q);
      const int R0 = (t & 4) ? 1 : 2, R1 = (t & 2) ? 1 : 2, R2 = (t & 1) ? 1 : 2;
      int e = 0;
      for (int di = 0; di <= R0; ++di)
        for (int dj = -R1; dj <= R1; ++dj)
          for (int dk = -R2; dk <= R2; ++dk) {
            if (!(di > 0 || dj > 0 || (dj == 0 && dk >= 0))) continue;  // (the diagonal first: (0, 0, 0) is the smallest stored offset)
            int v = -1;
            for (int u = 0; u < S.n; ++u)
              if (S.q[u] == q && S.di[u] == di && S.dj[u] == dj && S.dk[u] == dk) v = u;
            if (v < 0 || e >= 64) {
              mfem_set_error("lattice-tile tables (deterministic form): a stored slot has no stream step");
              return MFEM_ERR_INTERNAL;
            }
            h[pg][q][e][0] = (uint8_t)di;
            h[pg][q][e][1] = (uint8_t)(dj + 2);
            h[pg][q][e][2] = (uint8_t)(dk + 2);
            h[pg][q][e][3] = (uint8_t)v;
            ++e;
          }
      kup[pg][q] = e;
    }
  }
  if (hipMemcpyToSymbol(HIP_SYMBOL(c_l27d_lex), h, sizeof(h)) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(c_l27d_kup), kup, sizeof(kup)) != hipSuccess) {
    mfem_set_error("lattice-tile tables (deterministic form): hipMemcpyToSymbol failed");
    return MFEM_ERR_HIP;
  }
  g_l27d_tables = true;
  return MFEM_OK;
}
template <typename RP>
__global__ __launch_bounds__(MFEM_BLOCK) void k_l27d_fill(Lat27Geom G, const RP* __restrict__ rowptr, int base, const double* __restrict__ vals,
                                                            double* __restrict__ out, unsigned long long* __restrict__ stats) {
  // a wave per (cube, node type): the type's 64 rows 16 at a time, FOUR LANES PER ROW reading four consecutive entries of the row's upper half (16 rows x
  // 32 bytes per load instruction: the lines in flight fit the L1 -- with a lane per row, 64 rows per instruction, the fill took 11.6 ms for the 128^3
  // matrix, 4.4 x the four-lanes-per-row fill of the other form); every value goes to its place in the phase-major stream of its row's lane
  const int lane = threadIdx.x & 63, qd = lane & 3, rho = lane >> 2;
  const int b = rho >> 2, c = rho & 3;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nci = G.nti, ncj = G.ntj, nck = (G.m2 + 7) >> 3;
  const int64_t nwork = 8 * (int64_t)nci * ncj * nck;
  const int n0 = l27d_stream(0).n;
  double amax = 0.0;
  for (int64_t u = wave; u < nwork; u += nwaves) {
    const int t = (int)(u & 7);
    const int64_t cube = u >> 3;
    const int ck = (int)(cube % nck);
    const int64_t c2 = cube / nck;
    const int cj = (int)(c2 % ncj), ci = (int)(c2 / ncj);
    const int pg = (((t >> 1) & 1) + (t & 1)) & 1;
    const int q = pg ? (t == 1 ? 0 : t == 5 ? 1 : t == 2 ? 2 : 3) : (t == 0 ? 0 : t == 4 ? 1 : t == 3 ? 2 : 3);  // (l27d_type backwards)
    double* os = out + cube * (int64_t)L27D_CUBE_D + (pg ? (int64_t)n0 * 64 : 0);
    const int kup = c_l27d_kup[pg][q];
    for (int a = 0; a < 4; ++a) {
      const int oi = ci * 8 + 2 * a + ((t >> 2) & 1), gj = cj * 8 + 2 * b + ((t >> 1) & 1), gk = ck * 8 + 2 * c + (t & 1);
      const int gi = oi + G.plo;
      const bool valid = oi < G.m0 && gj < G.m1 && gk < G.m2;
      int li = 0, ni = 1, lj = 0, nj = 1, lk = 0, nk = 1;
      int64_t rp = 0;
      if (valid) {
        l27_range(gi, G.mg, li, ni);
        l27_range(gj, G.m1, lj, nj);
        l27_range(gk, G.m2, lk, nk);
        rp = (int64_t)rowptr[((int64_t)oi * G.m1 + gj) * G.m2 + gk] - base;
      }
      double* orow = os + (a * 16 + rho) * 2;  // the row's lane in the stream
      for (int e = qd; e < kup; e += 4) {
        const int di = c_l27d_lex[pg][q][e][0], dj = (int)c_l27d_lex[pg][q][e][1] - 2, dk = (int)c_l27d_lex[pg][q][e][2] - 2, v = c_l27d_lex[pg][q][e][3];
        const int ci2 = gi + di, cj2 = gj + dj, ck2 = gk + dk;
        double val = 0.0;
        if (valid && ci2 < G.mg && cj2 >= 0 && cj2 < G.m1 && ck2 >= 0 && ck2 < G.m2) {  // (ci2 may be a ghost plane of a slab)
          val = vals[rp + ((int64_t)(di - li) * nj + (dj - lj)) * nk + (dk - lk)];
          double av = fabs(val);
          if (!(av == av)) av = __builtin_huge_val();  // NaN: fmax would drop it
          amax = fmax(amax, av);
        }
        orow[(int64_t)(v >> 1) * 128 + (v & 1)] = val;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_down(amax, o, MFEM_WAVE));
  if (lane == 0) atomicMax(stats + 1, (unsigned long long)__double_as_longlong(amax));
}

// A->lat27.state: 0 not inspected, -1 not the lattice stencil, 1 structure ok
int mfem_lat27_plan(mfem_context_s* ctx, mfem_csr_s* A) {
  if (A->lat27.state != 0) return MFEM_OK;
  if (lat27_eligible(lat27_shape(A)) == 0) return MFEM_OK;  // launch-bound sizes stay on the CSR tile kernel
  A->lat27.state = -1;
  int rc = mfem_lattice_hint_from_row0(ctx, A);  // (a caller-supplied pattern: read the lattice off row 0)
  if (rc) return rc;
  const LatShape S = lat27_shape(A);
  if (lat27_eligible(S) != 1) return MFEM_OK;
  rc = lat27_upload_tables();
  if (rc) return rc;
  const Lat27Geom G = lat27_geom(S);
  int32_t* d_bad = ctx->d_flags + 12;
  MFEM_CHECK_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), ctx->stream));
  const int grid = mfem_grid_for(A->n, MFEM_BLOCK, ctx->num_cus * 16);
  mfem_by_rowptr(A, [&](auto w) {
    using RP = decltype(w);
    hipLaunchKernelGGL(k_l27_verify<RP>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, G, (const RP*)A->rowptr, A->colidx, A->index_base, d_bad);
  });
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 12, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->h_flags[12] == 0) A->lat27.state = 1;
  return MFEM_OK;
}

size_t mfem_lat27_bytes(const mfem_csr_s* A) {
  const LatShape S = lat27_shape(A);
  return lat_serves(A->lat27.state, lat27_knobs().enable, S) ? lat27_ws_bytes(lat27_geom(S)) : 0;
}

// Makes the layout copy of `vals` in buf and binds it if the values are symmetric (mfem_sym_probe; else leaves the pattern unbound: the caller
// binds the sliced layout instead).  scratch: 3 n doubles, left dirty.  Two stream synchronisations (max |a|, the verdict).
int mfem_lat27_bind(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, double* scratch, bool allow_rem) {
  LatTiles& T = A->lat27;
  mfem_lat_unbind(A, T);
  const Lat27Knobs K = lat27_knobs();
  if (T.state != 1 || !K.enable || !buf || !scratch) return MFEM_OK;
  const Lat27Geom G = lat27_geom(lat27_shape(A));
  unsigned long long* d_stats = (unsigned long long*)(ctx->d_flags + 12);
  MFEM_CHECK_HIP(hipMemsetAsync(d_stats, 0, 2 * sizeof(unsigned long long), ctx->stream));
  T.det = K.det ? 1 : 0;  // (the form THIS copy is made in: the launches follow the copy, not the knob)
  if (T.det) {
    const int rt = lat27d_upload_tables();
    if (rt) return rt;
  }
  // a wave per (cube, node type) / per unit
  const int64_t nwaves = T.det ? 8 * (int64_t)G.nti * G.ntj * ((G.m2 + 7) / 8) : (int64_t)G.nui * G.nuj * G.nuk;
  const int grid = mfem_grid_for(nwaves * 64, MFEM_BLOCK, ctx->num_cus * 16);
  mfem_by_rowptr(A, [&](auto w) {
    using RP = decltype(w);
    hipLaunchKernelGGL(T.det ? &k_l27d_fill<RP> : &k_l27_fill<RP>, dim3(grid), dim3(MFEM_BLOCK), 0, ctx->stream, G, (const RP*)A->rowptr, A->index_base,
                       vals, buf, d_stats);
  });
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 12, d_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  double amax;
  memcpy(&amax, ctx->h_flags + 14, sizeof(double));
  T.vals = buf;
  T.dump = buf + lat27_vals_doubles(G);
  T.src = vals;
  double asym = 1.0;
  const int rc = mfem_sym_probe(ctx, A, &T, vals, scratch, amax, &asym, allow_rem ? 1 : 0);
  T.asym = asym;
  if (rc || !lat_accepts(asym)) {  // not symmetric (or NaN): the sliced layout serves this solve
    mfem_lat_unbind(A, T);
    return rc;
  }
  T.dsc = dsc;
  T.scaled = dsc ? 1 : 0;
  return MFEM_OK;
}

// returns 1 if launched, 0 if another kernel should be used, <0 on error
int mfem_spmv_lat27_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, const double* x, double* y, double alpha,
                           double beta, const double* dotw, double* partials, int* n_partials, const int32_t* done_flag, int part) {
  const LatTiles& T = A->lat27;
  if (!T.vals || vals != T.src) return 0;
  if (n_partials) *n_partials = 0;
  const Lat27Geom G = lat27_geom(lat27_shape(A));
  const LatPart P = lat_part_tiles(G.m0, G.gw, G.nti, G.ntj, G.ntk, G.plo + G.m0 < G.mg, part);
  // y == nullptr: the fused CG iteration (mfem_lat27_cg_fused) -- pass 1 alone, the tiles' blocks stay in the dump for mfem_lat27_gather_cg_update,
  // x . A x comes out as one partial per tile behind the dump (the caller reads them where mfem_lat27_dot_partials says)
  if (!y) MFEM_REQUIRE(part == 0 && dotw == x && alpha == 1.0 && beta == 0.0 && !T.dsc, "lattice tiles: pass 1 alone serves only the fused CG iteration");
  if (P.tcount > 0) {
    hipLaunchKernelGGL(T.det ? k_spmv_lat27d : k_spmv_lat27, dim3(P.grid), dim3(512), 0, ctx->stream, G, (const double*)T.vals, x, T.dsc, T.dump, done_flag,
                       P.tile0, P.tcount, y ? (double*)nullptr : T.dump + lat27_dot_offset(G));
    MFEM_CHECK_LAUNCH();
  }
  if (!y) {
    if (n_partials) *n_partials = lat27_dot_partials(G);
    if (!ctx->probe_active) ++g_lat27_count;
    return 1;
  }
  if (part == 1) return 1;  // (the gather pass belongs to part 2)
  int grid = 1;
  int rc = mfem_lat27_gather_launch(ctx, A, G, lat27_knobs().gather_staged, x, y, alpha, beta, dotw, partials, done_flag, &grid);
  if (rc) return rc;
  if (n_partials && partials) *n_partials = grid;
  if (A->rem_active) {  // A = S + N: the skew remainder of the few nonsymmetric rows (spmv_rem.hip)
    rc = mfem_rem_apply(ctx, A, x, T.dsc, y, alpha, dotw, partials, n_partials, done_flag);
    if (rc) return rc;
  }
  if (!ctx->probe_active) ++g_lat27_count;
  return 1;
}

// Accounting.  What pass 1 streams is read off the KNOB, not off the bound copy's form (nothing need be bound when bench.py asks).
int64_t mfem_lat27_design_bytes(const mfem_csr_s* A) {
  return lat27_design_bytes(lat27_geom(lat27_shape(A)), lat27_knobs().det, A->lat27.scaled != 0) + mfem_rem_design_bytes(A);
}
int64_t mfem_lat27_entries(const mfem_csr_s* A) { return lat27_entries(lat27_geom(lat27_shape(A)), lat27_knobs().det); }

// ---- the fused CG iteration (krylov_cg.hip, mfem_cg_pass): pass 1 alone (mfem_spmv_halo with y = nullptr), the dot-product partials; pass 2 + residual
// update: spmv_lat27_gather.hip
bool mfem_lat27_cg_fused(const mfem_context_s* ctx, const mfem_csr_s* A, const double* vals) {
  return lat27_cg_fusable(lat27_knobs(), A->lat27.vals && vals == A->lat27.src, A->lat27.dsc != nullptr, ctx->comm != nullptr, A->rem_active != 0);
}
const double* mfem_lat27_dot_partials(const mfem_csr_s* A, int* np) {
  const Lat27Geom G = lat27_geom(lat27_shape(A));
  *np = lat27_dot_partials(G);
  return A->lat27.dump + lat27_dot_offset(G);
}
// (accounting for bench.py) is the fused CG iteration on, and what pass 1 alone moves by design
extern "C" int mfem_debug_lat27_cg_fused(void) { return lat27_knobs().cg_fused ? 1 : 0; }
extern "C" int64_t mfem_debug_lat27_pass1_bytes(mfem_csr A) {
  if (!A || A->lat27.state != 1) return -1;
  return lat27_pass1_bytes(lat27_geom(lat27_shape(A)), lat27_knobs().det);
}
