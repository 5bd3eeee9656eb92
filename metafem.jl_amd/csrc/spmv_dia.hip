// Mode 2 of the slot-major solver layout (spmv_ell.hip, spmv_ell.h): the diagonal-slotted copy -- the inspection of the pattern, the per-solve
// copy of the values (k_dia_vals, k_symp_fill), the per-row product kernel.  The symmetric sweeps on the same copy: spmv_sym.hip.
#include "blas1.h"
#include "spmv_ell.h"

// ---------------------------------------------------------------------------------------------------------------
// Diagonal-slotted blocks.  When every entry of the matrix sits on one of D <= 32 diagonals (col - row in a fixed sorted
// offset list: any lattice stencil -- 27 for the hex-8 scalar operator), slot s of a row is "the entry on diagonal s"
// (zero if the row has none) instead of "the s-th entry".  A 128-row block whose rows only touch in-range positions is
// then REGULAR: the column of (row r, slot s) is r + off[s], the column stream is not read at all, and the gather is a
// unit-stride 16-byte load.  Blocks that contain rows pointing outside [0, n_x) on some diagonal (first / last rows) or
// entries off the diagonal list (ghost columns of a slab) stay on the generic slot-major path with explicit columns.
// The detection is an inspection of the caller's CSR pattern; nothing about the mesh is assumed.
// ---------------------------------------------------------------------------------------------------------------

// flags[b] = c + 1 when every row of the 128-row block b is regular for class c: all its entries sit on the class's
// diagonals and r + off[s] is a valid x index for EVERY listed diagonal (so the kernel may load x there even where the
// row has no entry); 0 otherwise.  nreg counts the regular blocks.
template <typename RP>
__global__ __launch_bounds__(128) void k_dia_flags(int64_t n, int64_t nx, const RP* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col, int base,
                                                     const DiaOffsets* __restrict__ Op, int32_t* __restrict__ flags,
                                                     int32_t* __restrict__ nreg) {
  const DiaOffsets& O = *Op;
  __shared__ int ok_mask;
  for (int64_t blk = blockIdx.x; blk * 128 < n; blk += gridDim.x) {
    if (threadIdx.x == 0) ok_mask = (1 << O.ncls) - 1;
    __syncthreads();
    const int64_t r = blk * 128 + threadIdx.x;
    int mask = 0;
    if (r < n) {
      const int64_t lo = (int64_t)rowptr[r] - base, hi = (int64_t)rowptr[r + 1] - base;
      for (int c = 0; c < O.ncls; ++c) {
        const int D = O.D[c];
        bool ok = r + O.off[c][0] >= 0 && r + O.off[c][D - 1] < nx;
        int s = 0;
        int64_t last = INT64_MIN;
        for (int64_t j = lo; j < hi && ok; ++j) {  // columns strictly ascending, offsets ascending: merge
          const int64_t d = (int64_t)col[j] - base - r;
          if (d <= last) ok = false;  // unsorted or duplicate columns: only the explicit-column path sums every entry
          last = d;
          while (s < D && O.off[c][s] < d) ++s;
          if (s == D || O.off[c][s] != d) ok = false;
        }
        if (ok) mask |= 1 << c;
      }
    }  // rows past n (partial last block): mask 0 -> generic path
    atomicAnd(&ok_mask, mask);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = ok_mask;
      flags[blk] = m ? __ffs(m) : 0;
      if (m) atomicAdd(nreg, 1);
    }
    __syncthreads();
  }
}

// values in diagonal slots + per-block regular flag (regular: every row r of the block has 0 <= r + off[s] < nx for all s).
// With pv != nullptr the rows of the swept lattice planes [Gm.p0, Gm.p1) go straight to the patch-major copy of the patch sweep (layout:
// k_spmv_symp) -- their 27 slots, the edge block entries they own, and the diagonal alone to the slot-major copy (k_ell_diag reads it
// there) -- instead of through the slot-major copy and a second pass (k_symp_bind): 1.97 + 1.85 ms -> one pass at 256^3.
// LPR = lanes per row: 1 (64 rows per wave tile) or 2 (32 rows); SYM: the symmetrically scaled copy -- its own instantiation, so that the plain
// copy's code is what it was (2.4 ms at 256^3; 2.7 with the test for the scaling in it)
template <typename RP, int LPR, bool SYM, bool PIPE>
__global__ __launch_bounds__(MFEM_BLOCK) void k_dia_vals(int64_t n, int64_t npad, int K, const RP* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, const double* __restrict__ vals,
                                                           int base, const DiaOffsets* __restrict__ Op,
                                                           const int32_t* __restrict__ flags, double* __restrict__ out, SympGeom Gm,
                                                           double* __restrict__ pv, const double* __restrict__ dsc,
                                                           const double* __restrict__ ssym, int fast) {
  // ssym != nullptr: the copy is S^-1 A S^-1 with ssym = 1 / S, entry * (ssym[row] * ssym[column]) with the PRODUCT of the two factors formed
  // first -- a mirrored pair is then multiplied by the same number, so a bitwise symmetric matrix stays bitwise symmetric (the scaled CG,
  // cg_variant 4).  (Multiplying by reciprocals, not dividing: 27 divisions per row cost more than the rest of the placement.)
  // dsc != nullptr: the copy is the right-Jacobi-scaled matrix, entry / dsc[its column] (Mat_Div_Jacobi folded into this pass; the
  // columns are then read for every tile)
  const DiaOffsets& O = *Op;
  extern __shared__ double lds[];
  const int64_t slo = pv ? (int64_t)Gm.p0 * Gm.PL : 0, shi = pv ? (int64_t)Gm.p1 * Gm.PL : 0;  // swept rows
  const int spNP = Gm.NR * Gm.NPk, spB = Gm.B > 0 ? Gm.B : 1, spMAIN = sp_main(spB), spLOW = sp_low(spB);
  const int64_t spT = (int64_t)spNP * (Gm.p1 - Gm.p0);
  // LPR = 2: a wave takes 32 rows at a time, two lanes per row -- lanes 0..31 walk their row's entries forward through the first half of
  // the diagonal list, lanes 32..63 walk them backward through the second half.  A lane per row (64 rows per tile) needs 12 x 64 x K
  // bytes of staging per wave: two waves per CU on 81-entry rows (4.0 ms per bind at C3 against 3.4 ms with two lanes); on 27-entry
  // rows six waves per CU are enough and the lane per row is faster (2.4 against 2.7 ms at 256^3).
  constexpr int RT = 64 / LPR, SH = LPR == 2 ? 5 : 6;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;  // (w: wave-uniform, known to the compiler)
  const int half = LPR == 2 ? lane >> 5 : 0, rl = lane & (RT - 1);
  double* T = lds + (size_t)w * RT * K;
  // columns are staged only for the Jacobi scaling pass (dsc); the placement below needs them for the few tiles that are not `full`
  // (mesh boundary) and reads those from memory -- 8 instead of 12 bytes of LDS per staged entry, half as many more waves per CU
  int32_t* Tc = reinterpret_cast<int32_t*>(lds + (size_t)nw * RT * K) + (size_t)w * RT * K;
  const bool stage_cols = !PIPE && dsc != nullptr;
  const int64_t ntiles = npad >> SH;
  constexpr int NB = 28;
  // Software pipeline (round 4; a lane per row, rows of at most NB entries, no scaling pass -- the 27-diagonal lattice copies of C2): the NEXT tile's
  // values are loaded into registers before the current tile is placed, so a wave keeps one tile of loads in flight while it reads LDS and issues
  // its 27 scattered stores -- each wave had one memory round trip per tile with nothing else outstanding (10 waves per CU).
  constexpr bool pipe = PIPE;  // (chosen at the launch: LPR == 1, no scaling pass, K <= NB)
  const int64_t tstride = (int64_t)gridDim.x * nw;
  double tvn[NB];
  int64_t s0n = 0;
  int cntn = 0;
  auto tile_span = [&](int64_t t, int64_t& s0_, int& cnt_) {
    const int64_t q0 = t << SH, qend = (q0 + RT < n) ? q0 + RT : n;
    s0_ = q0 < n ? (int64_t)rowptr[q0] - base : 0;
    cnt_ = q0 < n ? (int)((int64_t)rowptr[qend] - base - s0_) : 0;
  };
  auto prefetch = [&]() {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int i = lane + 64 * u;
#if defined(DV_ABL) && DV_ABL == 2   // (ablation: no value loads)
      tvn[u] = (double)i;
#else
      tvn[u] = i < cntn ? __builtin_nontemporal_load(vals + s0n + i) : 0.0;
#endif
    }
  };
  if (pipe) {
    const int64_t t0 = (int64_t)blockIdx.x * nw + w;
    if (t0 < ntiles) {
      tile_span(t0, s0n, cntn);
      prefetch();
    }
  }
  // fast != 0: the swept rows are filled by k_symp_fill (below) -- this launch visits only the tiles that hold other rows (the tiles [sk0, sk1) lie inside the
  // swept range and are stepped over) and leaves the swept rows of the tiles it visits alone
  const int64_t sk0 = fast ? (slo + RT - 1) >> SH : 0, sk1 = fast ? (shi >> SH > sk0 ? shi >> SH : sk0) : 0;
  for (int64_t tix = (int64_t)blockIdx.x * nw + w; tix < ntiles - (sk1 - sk0); tix += tstride) {
    const int64_t tile = tix < sk0 ? tix : tix + (sk1 - sk0);
    const int64_t r0 = tile << SH, r = r0 + rl;
    const int64_t rend = (r0 + RT < n) ? r0 + RT : n;
    int64_t lo = 0;
    int len = 0;
    if (r < n) {
      lo = (int64_t)rowptr[r] - base;
      len = (int)((int64_t)rowptr[r + 1] - base - lo);
    }
    int64_t s0;
    int cnt;  // <= RT D
    int64_t s0_next = 0;
    int cnt_next = 0;
    if (pipe) {
      s0 = s0n;
      cnt = cntn;
      if (tile + tstride < ntiles) tile_span(tile + tstride, s0_next, cnt_next);  // (these row pointers arrive beside the values in flight)
    } else {
      s0 = r0 < n ? (int64_t)rowptr[r0] - base : 0;
      cnt = r0 < n ? (int)((int64_t)rowptr[rend] - base - s0) : 0;
    }
    const int cls = __builtin_amdgcn_readfirstlane(flags[tile >> (7 - SH)]) - 1;
    // a tile of a regular block whose rows all have every diagonal of the class (cnt = RT D: away from the mesh boundary, nearly all
    // tiles): entry s of a row IS its slot s -- the columns are not needed, a third of the kernel's reads
    const bool full = cls >= 0 && cnt == RT * O.D[cls];
    if (pipe) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = lane + 64 * u;
        if (i < cnt) T[i] = tvn[u];
      }
      s0n = s0_next;
      cntn = cnt_next;
      if (tile + tstride < ntiles) prefetch();  // in flight until the next trip's LDS stores
    }
    // staging: all loads of a lane are issued before the first LDS store.  28 in flight per lane: a 64-row tile of 27-entry rows (27 per lane) is
    // ONE memory round trip, a 32-row tile of 81-entry rows two (SQ counters of the version with batches of 8: 79 % of the wave cycles waiting,
    // ~10 waves per CU with 4 KB in flight each)
    if constexpr (!PIPE)
    for (int i0 = lane; i0 < cnt; i0 += 64 * NB) {
      double tv[NB];
      int32_t tc[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + 64 * u;
        tv[u] = i < cnt ? vals[s0 + i] : 0.0;
        tc[u] = (i < cnt && stage_cols) ? col[s0 + i] : 0;
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + 64 * u;
        if (i < cnt) {
          T[i] = tv[u];
          if (stage_cols) Tc[i] = tc[u] - base;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (!PIPE && dsc) {
      // right Jacobi scaling of the staged tile, entry / dsc[column]: the gathers of 16 entries per lane are in flight together -- one more
      // memory round trip per batch of 1024 entries (dividing inside the staging loop above made every batch of its loads wait twice)
      __builtin_amdgcn_wave_barrier();
      for (int i0 = lane; i0 < cnt; i0 += 64 * 16) {
        double dd[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int i = i0 + 64 * u;
          dd[u] = i < cnt ? dsc[Tc[i]] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int i = i0 + 64 * u;
          if (i < cnt) T[i] /= dd[u];
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
    }
    const int off0 = (int)(lo - s0);
    const int dir = half ? -1 : 1;
    double sr = 1.0;
    if constexpr (SYM) sr = r < n ? ssym[r] : 1.0;
    auto sym_scaled = [&](double a, int64_t c) -> double {
      if constexpr (SYM) return a * (sr * ssym[c]);
      else return a;
    };
    auto colat = [&](int j) -> int64_t { return stage_cols ? (int64_t)Tc[off0 + j] : (int64_t)col[lo + j] - base; };
    if (cls >= 0 && r0 < shi && r0 + RT > slo) {  // a tile with swept rows (all of them in regular blocks of the 27-diagonal lattice class)
      bool sw = r >= slo && r < shi;
      int p = 0, jj = 0, kk = 0;
      if (sw) {
        p = (int)(r / Gm.PL);
        const int rem = (int)(r - (int64_t)p * Gm.PL);
        jj = rem / Gm.m2;
        kk = rem - jj * Gm.m2;
        sw = jj < Gm.ms1 && kk < Gm.ms2;  // (a rim row of a trimmed sweep goes to the slot-major copy like a row outside the swept planes; the product reads k_symp_rim_fill's copy)
      }
      if (fast && sw) len = 0;  // (k_symp_fill's row: nothing is stored for it below)
      int line = 0, pcol = 0;
      int64_t mainoff = 0, lowoff = 0, edgeoff = 0;
      if (sw) {
        const int L = SP_L * spB, band = (jj % L) / SP_L;  // the row's patch row, band and line of the band
        line = jj % L;
        pcol = kk % SP_W;
        const int64_t step = (int64_t)(p - Gm.p0) * spNP + (jj / L) * Gm.NPk + kk / SP_W;
        mainoff = step * spMAIN + band * 14 * SP_ROWS + (line - band * SP_L) * SP_W + pcol;
        lowoff = spT * spMAIN + step * spLOW + band * 13 * SP_ROWS + (line - band * SP_L) * SP_W + pcol;
        edgeoff = step * spMAIN + spB * 14 * SP_ROWS;
      }
      int j = half ? len - 1 : 0;
#pragma unroll
      for (int t = 0; t < (LPR == 2 ? 14 : 27); ++t) {  // forward lanes: slots 0..13 (all 27 with a lane per row), backward lanes: slots 26..14
        const int sl = half ? 26 - t : t;
        const bool act = half == 0 || t < 13;
        double v = 0.0;
        if (act && j >= 0 && j < len && (full || colat(j) - r == O.off[cls][sl])) {
          v = sym_scaled(T[off0 + j], r + O.off[cls][sl]);
          j += dir;
        }
        if (!act) continue;
        if (!sw) {
          DIA_ST(out + ell_base(r, K) + sl * ELL_B, v);
        } else if (!fast) {
          DIA_ST(pv + (sl < 13 ? lowoff + sl * SP_ROWS : mainoff + (sl - 13) * SP_ROWS), v);
          if (sl == 13) out[ell_base(r, K) + 13 * ELL_B] = v;  // the diagonal (offset 0 is the 14th of the 27 lattice offsets)
          if (half == 0 && t < 13) {                           // the edge block entry the row owns for this lower slot, if any
            const int e = sp_edge_of(t, line, pcol, spB);  // (line: counted over the patch's bands)
            if (e >= 0) pv[edgeoff + e] = v;
          }
        }
      }
    } else if (cls >= 0) {  // regular 128-row block of class cls: slot s = diagonal s
      const int D = O.D[cls], Dh = LPR == 2 ? (D + 1) >> 1 : D;
      if (half == 0) {
        int j = 0;
        for (int sl = 0; sl < Dh; ++sl) {
          double v = 0.0;
          if (j < len && (full || colat(j) - r == O.off[cls][sl])) {
            v = sym_scaled(T[off0 + j], r + O.off[cls][sl]);
            ++j;
          }
          DIA_ST(out + ell_base(r, K) + sl * ELL_B, v);
        }
      } else {
        int j = len - 1;
        for (int sl = D - 1; sl >= Dh; --sl) {
          double v = 0.0;
          if (j >= 0 && (full || colat(j) - r == O.off[cls][sl])) {
            v = sym_scaled(T[off0 + j], r + O.off[cls][sl]);
            --j;
          }
          DIA_ST(out + ell_base(r, K) + sl * ELL_B, v);
        }
      }
    } else {                 // generic block: slot s = s-th entry, columns come from ell_cols
      for (int sl = half; sl < K; sl += LPR) out[ell_base(r, K) + sl * ELL_B] = sl < len ? sym_scaled(T[off0 + sl], colat(sl)) : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// A value of the patch-major copy as the fill forms it: with the symmetric scaling v * (srow * sc) -- the product of the two factors first: a mirrored pair is
// multiplied by the same number --, else the plain value.  One function for k_symp_fill and k_symp_const_ref: the reference row's values are compared bit by bit.
template <bool SYM>
__device__ __forceinline__ double symp_formed(double v, double srow, double sc) {
  if constexpr (SYM) return v * (srow * sc);
  else return v;
}

// The swept rows of the patch-major copy: a workgroup of two waves per patch step (plane, strip of SP_L lines, patch column), a wave per pair of lattice lines,
// lane = line * SP_W + column -- 64 rows whose CSR values are two contiguous runs (one per line: 6.9 KB when all 32 rows have their 27 entries).  Every slot store of
// a wave is ONE aligned 512-byte piece of the copy and the two halves of each 1 KB slot are written by the same workgroup; the step's edge block (318 entries owned by
// rows of both waves) is gathered in LDS and written as one contiguous piece.  (k_dia_vals' tiles of 64 consecutive rows drift against the patch columns -- a
// 513-point line is 16 patches + 1 point -- and wrote two or three unaligned pieces per slot and the edge entries one by one; tools/copy_probe.hip, 512^3, all stores:
// 14.8 ms in that shape, 10.7 ms in this one; a plain aligned copy of the same bytes 9.4 ms.)  Two memory round trips per full tile -- the four row pointers of the
// runs (scalar loads), then the 27 values + the 27 factors of the symmetric scaling per lane, all issued before the first wait; tiles with short rows (lattice edge)
// or missing lines / columns take the general path: per-lane row pointers, masked staging, the short rows' columns decoded into slots (offset = di PL + dj m2 + dk,
// guaranteed by dia_lattice_class below) and every row expanded to its 27 slots in LDS.
// DC (with SYM; Gm.DC): the coded-diagonal form of the main part (spmv_symp.h) -- slots 14..26 per band, and the scaled diagonal a_ii * (t_i * t_i) as the signed
// byte bits(v) - bits(1.0) in the step's code block, gathered in LDS like the edge block and written as one aligned piece (cells outside the lattice: code 0).  A
// swept row whose diagonal is further than 127 ulps from the unit (the other sign, zero, absent, non-finite) raises dcbad[0]: the bind then refills in the stored
// form.  The unit is +1.0 or, with dcbad[1] set (k_symp_diag_sign: the first swept row's diagonal is negative -- the thermal K is negative definite), -1.0.  The
// slot-major copy gets the diagonal as a double either way (k_ell_diag, the rows outside the swept planes).
// Constant steps (symp_const_decide.h; sflags != nullptr): every lane compares each value it forms, by bit pattern (-0.0, NaN and an absent entry's zero all
// differ from a reference row of 27 finite entries), with the reference row's of the same slot (cref, written by k_symp_const_ref in front of this launch) and,
// coded form, its diagonal's code.  A step is flagged when all its bands took the full-tile path in both waves (whole patch, 27 entries in every row) and no lane
// met a difference: one LDS word gathers the waves' verdicts in front of the barrier that closes the step, thread 0 writes the step's byte behind it.  The
// edge block needs no look of its own: its entries are copies of the rows' lower-slot values.  The workgroup's flagged steps are added once to *scount.
template <typename RP, bool SYM, bool DC = false>
__global__ __launch_bounds__(128) void k_symp_fill(int64_t n, int K, const RP* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const double* __restrict__ vals, int base, const DiaOffsets* __restrict__ Op, int cls,
                                                    double* __restrict__ out, SympGeom Gm, double* __restrict__ pv, const double* __restrict__ ssym,
                                                    unsigned long long* __restrict__ fp, int32_t* __restrict__ dcbad, const SympConst* __restrict__ cref,
                                                    unsigned char* __restrict__ sflags, int32_t* __restrict__ scount) {
  const DiaOffsets& O = *Op;
  extern __shared__ double lds[];
  constexpr int RUN = SP_W * 27;  // entries of a full 32-row run
  constexpr int NSL = sp_nslots(DC), S0 = 27 - NSL;  // the main part holds slots S0..26 of every band
  int nocode = 0;
  const long long unit = sp_unit_bits(DC ? dcbad[1] : 0);
  // Symmetry fingerprint (round 6; fp != nullptr): are the values this pass WRITES bitwise symmetric among the swept rows?  Every stored entry (r, c), c != r,
  // both rows swept, adds  sign(c - r) * m(min, max) * bits(v)  to a 64-bit sum in wrap-around arithmetic, m a 64-bit hash of the unordered pair.  A
  // symmetric copy cancels pair by pair -- exactly, in any order (integer sums commute: no atomics on doubles, no second pass); a copy with v_rc != v_cr
  // anywhere leaves a non-zero sum unless the pairs' hashed multipliers conspire (2^-63 for a given matrix).  It replaces the separate check pass over the
  // copy (k_spmv_symp<1>: 4.6 ms of the 21 ms a 512^3 solve spends outside its iterations); the pass is still there (bit 30 of the "ell" knob) and the
  // test-suite compares the two verdicts.  Stricter than the pass (which looks at the pairs the sweep mirrors): never the other way round.  Swept: in a patch --
  // an entry towards a rim row of a trimmed sweep has no partner in this pass and is not counted.
  unsigned long long fsum = 0;
  const int64_t sw_lo = (int64_t)Gm.p0 * Gm.PL, sw_hi = (int64_t)Gm.p1 * Gm.PL;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (launched with two waves per workgroup)
  double* T = lds + (size_t)w * (2 * RUN);
  double* E = lds + 2 * (2 * RUN);  // the step's edge block (SP_EPAD entries; zero between steps: entries of rows outside the lattice and the padding stay 0)
  const int spNP = Gm.NR * Gm.NPk, spB = Gm.B, spMAIN = sp_main(spB, DC), spLOW = sp_low(spB), spEPAD = sp_epad(spB);
  signed char* const Cb = reinterpret_cast<signed char*>(E + spEPAD);  // DC: the step's code block (spB * SP_ROWS bytes; zero between steps)
  const int64_t spT = (int64_t)spNP * (Gm.p1 - Gm.p0);
  const int h = lane >> 5, c = lane & (SP_W - 1);
  const int32_t PL = (int32_t)Gm.PL, m2 = Gm.m2;
  auto uni64 = [](int64_t x) -> int64_t {  // (the same value in every lane: into scalar registers, so that what depends on it stays scalar)
    const uint32_t xl = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)x), xh = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)xh << 32) | xl);
  };
  int* const Fw = reinterpret_cast<int*>(E + spEPAD + sp_cpad(spB, DC));  // constant steps: non-zero once a wave of the step has met a difference (zero between steps)
  const bool cs = sflags != nullptr && cref->valid != 0;  // (no reference row: every step's byte is 0)
  const int ccode = DC && cs ? cref->code : 0;
  // the reference row, copied to LDS once in front of the steps and read there as broadcasts.  Read from memory inside the step, the scalar loads share their
  // counter with the LDS staging of the tile and every step waited for them (14.46 instead of 13.89 ms per fill at 512^3); held in 54 scalar registers they spill.
  double* const Cv = reinterpret_cast<double*>(Fw) + 1;
  if (threadIdx.x < 27) Cv[threadIdx.x] = cref->v[threadIdx.x];
  int nflagged = 0;
  for (int i = threadIdx.x; i < spEPAD + sp_cpad(spB, DC); i += 128) E[i] = 0.0;  // (the code block lies behind E: all-zero bytes)
  if (threadIdx.x == 0) *Fw = 0;
  __syncthreads();
  // Work item wi = (plane, q) takes patch (q + plane * rot) % NP of its plane.  Workgroups with equal blockIdx % 8 share an XCD and the grid is a multiple of 8: with
  // a patch count per plane that is a multiple of 8 too (whole patches of the usual meshes: 1024 at 512^3) a workgroup would meet the same patch, and an XCD
  // the same patch columns, in every plane -- measured at 512^3: 22.0 ms per fill that way (the 512-point lattice of --n 511, untrimmed: 21.7 ms), 13.9 ms with
  // the planes' patch orders shifted against each other (rot = 1, 3, 7, 13, NP - 1 alike), as the 1105 patches of the untrimmed plane shift by themselves
  // (profiles/r10_symp_trim_ab_512.txt).
  const int rot = spNP % 8 == 0 ? 1 : 0;
  for (int64_t wi = blockIdx.x; wi < spT; wi += gridDim.x) {  // (every barrier below is reached by both waves: the trip count is the workgroup's)
    const int64_t wpl = wi / spNP, step = wpl * spNP + (wi - wpl * spNP + wpl * rot) % spNP;
    const int kp = (int)(step % Gm.NPk);
    const int64_t q = step / Gm.NPk;
    const int prow = (int)(q % Gm.NR), pl = (int)(q / Gm.NR);
    double* const pe = pv + step * spMAIN + spB * NSL * SP_ROWS;
    int differs = cs ? 0 : 1;
    for (int band = 0; band < spB; ++band) {  // the strips of the patch one after the other: their edge entries meet in E (a strip past the lattice: nlines = 0)
    const int strip = prow * spB + band;
    const int jj0 = strip * SP_L + 2 * w, kk0 = kp * SP_W;
    const int ncol = m2 - kk0 < SP_W ? m2 - kk0 : SP_W, nlines = Gm.m1 - jj0 < 2 ? (Gm.m1 - jj0 < 1 ? 0 : 1) : 2;  // (the last strip may end before this wave's lines)
    const int64_t rb = (int64_t)(Gm.p0 + pl) * Gm.PL + (int64_t)jj0 * m2 + kk0;  // lane 0's row
    const int64_t rB = nlines == 2 ? rb + m2 : rb;                              // lane 32's row (no second line: the first again, nothing of it is used)
    int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (nlines > 0) {
      a0 = uni64((int64_t)rowptr[rb]) - base, a1 = uni64((int64_t)rowptr[rb + ncol]) - base;
      b0 = uni64((int64_t)rowptr[rB]) - base, b1 = uni64((int64_t)rowptr[rB + ncol]) - base;
    }
    const bool full = ncol == SP_W && nlines == 2 && a1 - a0 == RUN && b1 - b0 == RUN;
    const bool valid = c < ncol && h < nlines;
    const bool cmp = cs && full;  // (wave-uniform)
    if (!full) differs = 1;
    const int64_t r = rb + (int64_t)h * m2 + c;
    const int line = 2 * w + h;
    double* const pm = pv + step * spMAIN + band * NSL * SP_ROWS + line * SP_W + c;
    double* const plo = pv + spT * spMAIN + step * spLOW + band * 13 * SP_ROWS + line * SP_W + c;
    const double* Tr = T + lane * 27;
    double sc[27];
    double srow = 1.0;
    uint32_t present = 0x7FFFFFFu;
    if (full) {
      double tv[27];
      const double* vA = vals + a0 + lane;
      const double* vB = vals + b0 + lane - RUN;
      const double* v13 = h ? vB : vA;  // entries 832 .. 895 of the tile: the first run ends at 864
#pragma unroll
      for (int u = 0; u < 27; ++u) tv[u] = __builtin_nontemporal_load((u < 13 ? vA : u == 13 ? v13 : vB) + 64 * u);
      if constexpr (SYM) {
        srow = ssym[r];
#pragma unroll
        for (int u = 0; u < 27; ++u) sc[u] = ssym[r + O.off[cls][u]];
      }
#pragma unroll
      for (int u = 0; u < 27; ++u) T[lane + 64 * u] = tv[u];
      __builtin_amdgcn_wave_barrier();
    } else {
      int64_t lo = 0;
      int len = 0;
      if (valid) {
        lo = (int64_t)rowptr[r] - base;
        len = (int)((int64_t)rowptr[r + 1] - base - lo);
      }
      const int cntA = (int)(a1 - a0), cntB = nlines == 2 ? (int)(b1 - b0) : 0;  // <= RUN each (regular blocks: at most 27 entries per row)
      {
        double ta[14], tb[14];
#pragma unroll
        for (int u = 0; u < 14; ++u) {
          const int i = lane + 64 * u;
          ta[u] = i < cntA ? __builtin_nontemporal_load(vals + a0 + i) : 0.0;
          tb[u] = i < cntB ? __builtin_nontemporal_load(vals + b0 + i) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 14; ++u) {
          const int i = lane + 64 * u;
          if (i < cntA) T[i] = ta[u];
          if (i < cntB) T[RUN + i] = tb[u];
        }
      }
      // the columns of the short rows (their entries are decoded into slots below; a row of 27 entries has entry s in slot s)
      int32_t cj[27];
      const bool shortrow = valid && len < 27;
#pragma unroll
      for (int j = 0; j < 27; ++j) cj[j] = (shortrow && j < len) ? col[lo + j] - base : 0;
      __builtin_amdgcn_wave_barrier();
      const int off0 = h * RUN + (int)(lo - (h ? b0 : a0));
      double ev[27];
#pragma unroll
      for (int j = 0; j < 27; ++j) ev[j] = j < len ? T[off0 + j] : 0.0;
      __builtin_amdgcn_wave_barrier();  // every lane holds its entries: the staging area may now be overwritten by the expanded rows
      present = 0;
      if (shortrow) {
#pragma unroll
        for (int sl = 0; sl < 27; ++sl) T[lane * 27 + sl] = 0.0;
      }
#pragma unroll
      for (int j = 0; j < 27; ++j) {
        if (j < len) {
          int sl = j;
          if (shortrow) {
            const int32_t d = cj[j] - (int32_t)r;
            const int di = (2 * d > PL) - (2 * d < -PL);
            const int32_t d1 = d - di * PL;
            const int dj = (2 * d1 > m2) - (2 * d1 < -m2);
            sl = 9 * (di + 1) + 3 * (dj + 1) + (d1 - dj * m2 + 1);
          }
          T[lane * 27 + sl] = ev[j];
          present |= 1u << sl;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if constexpr (SYM) {
        srow = valid ? ssym[r] : 1.0;
#pragma unroll
        for (int u = 0; u < 27; ++u) sc[u] = valid ? ssym[r + O.off[cls][u]] : 1.0;
      }
    }
    if (valid) {
#pragma unroll
      for (int sl = 0; sl < 27; ++sl) {
        double v = 0.0;
        if (present >> sl & 1u) {
          v = Tr[sl];
          v = symp_formed<SYM>(v, srow, sc[sl]);
          if (cmp) differs |= __double_as_longlong(v) != __double_as_longlong(Cv[sl]) ? 1 : 0;
          if (fp && sl != 13) {
            const int64_t cc = r + O.off[cls][sl];
            if (cc >= sw_lo && cc < sw_hi && jj0 + h + sp_dj(sl) < Gm.ms1 && kk0 + c + sp_dk(sl) < Gm.ms2) {
              const uint64_t lo_ = (uint64_t)(sl < 13 ? cc : r), hi_ = (uint64_t)(sl < 13 ? r : cc);
              uint64_t z = lo_ * 0x9E3779B97F4A7C15ull + hi_ * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
              z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
              z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
              z = (z ^ (z >> 31)) | 1ull;
              const unsigned long long t = z * (unsigned long long)__double_as_longlong(v);
              fsum += sl < 13 ? (0ull - t) : t;
            }
          }
        }
        if (sl < 13) {
          DIA_ST(plo + sl * SP_ROWS, v);
          const int e = sp_edge_of(sl, band * SP_L + line, c, spB);
          if (e >= 0) E[e] = v;
        } else {
          if (sl >= S0) DIA_ST(pm + (sl - S0) * SP_ROWS, v);
          if (sl == 13) {
            DIA_ST(out + ell_base(r, K) + 13 * ELL_B, v);  // the diagonal also to the slot-major copy (k_ell_diag reads it there)
            if constexpr (DC) {
              int code = 0;
              if (!sp_diag_code(v, code, unit)) nocode = 1;
              else Cb[band * SP_ROWS + line * SP_W + c] = (signed char)code;
              if (cmp) differs |= code != ccode ? 1 : 0;
            }
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();  // (the wave's staging area is overwritten by its next strip)
    }
    if (sflags && __ballot(differs) != 0 && lane == 0) *Fw = 1;
    __syncthreads();
    for (int i = threadIdx.x; i < spEPAD + sp_cpad(spB, DC); i += 128) {  // (DC: the code block follows the edge block in the copy as in LDS)
      DIA_ST(pe + i, E[i]);
      E[i] = 0.0;
    }
    if (sflags && threadIdx.x == 0) {  // (the barrier below orders the reset before the next step's verdicts)
      const int f = *Fw == 0 ? 1 : 0;
      sflags[step] = (unsigned char)f;
      nflagged += f;
      *Fw = 0;
    }
    __syncthreads();
  }
  if (sflags && threadIdx.x == 0 && nflagged) atomicAdd(scount, nflagged);
  if (DC && nocode) atomicOr(dcbad, 1);
  if (fp) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fsum += __shfl_down(fsum, o, MFEM_WAVE);
    if (lane == 0 && fsum) atomicAdd(fp, fsum);
  }
}

// The compact copy of the rim rows of a trimmed sweep (symp_trim_decide.h): units of SPT_UNIT rows in the rim's enumeration, slot-major inside a unit, a lane per
// row.  The row's CSR entries are merged into the 27 lattice slots (columns and offsets both ascend; an absent entry is a stored zero) with the arithmetic of
// the other copies: entry / dsc[column], then entry * (ssym[row] * ssym[column]).  The diagonal also goes to the slot-major copy (k_ell_diag reads it there):
// k_dia_vals steps over the tiles inside the swept planes when k_symp_fill fills them.
template <typename RP>
__global__ __launch_bounds__(64) void k_symp_rim_fill(int K, const RP* __restrict__ rowptr, const int32_t* __restrict__ col, const double* __restrict__ vals,
                                                       int base, double* __restrict__ out, SympGeom Gm, double* __restrict__ rim, const double* __restrict__ dsc,
                                                       const double* __restrict__ ssym) {
  const int lane = threadIdx.x;
  for (int64_t u = blockIdx.x; u < Gm.rim_units; u += gridDim.x) {
    const int64_t g = u * SPT_UNIT + lane;
    const bool valid = g < Gm.rim_rows;
    int64_t r = 0, lo = 0;
    int len = 0;
    double sr = 1.0;
    if (valid) {
      const int pl = (int)(g / Gm.rim_pp);
      int j = 0, k = 0;
      spt_rim_row((int)(g - (int64_t)pl * Gm.rim_pp), Gm.m2, Gm.ms1, Gm.ms2, j, k);
      r = (int64_t)(Gm.p0 + pl) * Gm.PL + (int64_t)j * Gm.m2 + k;
      lo = (int64_t)rowptr[r] - base;
      len = (int)((int64_t)rowptr[r + 1] - base - lo);
      if (ssym) sr = ssym[r];
    }
    double* const dst = rim + u * SPT_UNIT_DOUBLES + lane;
    // all loads of a row are issued before the first use (a row of 27 entries, nearly all of them, has entry s in slot s: one memory round trip)
    double ev[27];
    int32_t ec[27];
#pragma unroll
    for (int e = 0; e < 27; ++e) {
      ev[e] = e < len ? vals[lo + e] : 0.0;
      ec[e] = e < len ? col[lo + e] : 0;
    }
    uint32_t slot_of = 0;  // bit sl: the row has an entry on lattice offset sl (columns and offsets both ascend)
    if (len == 27) {
      slot_of = 0x7FFFFFFu;
    } else {
      int sl = 0;
#pragma unroll
      for (int e = 0; e < 27; ++e) {
        if (e < len) {
          const int64_t d = (int64_t)ec[e] - base - r;
          while (sl < 27 && (int64_t)(sl / 9 - 1) * Gm.PL + (int64_t)(sp_dj(sl) * Gm.m2 + sp_dk(sl)) < d) ++sl;
          if (sl < 27) slot_of |= 1u << sl;
          ++sl;
        }
      }
    }
    // the e-th set bit of slot_of is entry e's slot: walk slots and entries together with compile-time register indices
    int cnt = 0;  // entries placed so far
#pragma unroll
    for (int sl = 0; sl < 27; ++sl) {
      double v = 0.0;
      if (slot_of >> sl & 1u) {
        int64_t c = 0;
#pragma unroll
        for (int e = 0; e <= sl; ++e)
          if (e == cnt) {
            v = ev[e];
            c = (int64_t)ec[e] - base;
          }
        if (dsc) v /= dsc[c];
        if (ssym) v = v * (sr * ssym[c]);
        ++cnt;
      }
      DIA_ST(dst + sl * SPT_UNIT, v);
      if (sl == 13 && valid) out[ell_base(r, K) + 13 * ELL_B] = v;
    }
  }
}

// lane <-> RPT (2 or 4) neighbouring rows; a wave covers one aligned block of 64 RPT rows; U diagonals per batch
template <int RPT, int U, bool TRIPLES = false>
__global__ __launch_bounds__(1024) void k_spmv_dia(int64_t n, int64_t npad, int K, const DiaOffsets* __restrict__ Op,
                                                           const int32_t* __restrict__ flags, const int32_t* __restrict__ cols,
                                                           const double* __restrict__ vals, const double* __restrict__ x,
                                                           double* __restrict__ y, double alpha, double beta,
                                                           const double* __restrict__ dotw, double* __restrict__ partials,
                                                           const int32_t* __restrict__ done_flag, int xcd, SpmvPart part) {
  __shared__ double red[16];
  if (done_flag && done_flag[0]) return;
  const DiaOffsets& O = *Op;
  double dot_acc = 0.0;
  // xcd > 0: workgroups with equal blockIdx % 8 share an XCD (round-robin dispatch); XCD x walks its own contiguous eighth of
  // the rows, so the x window an L2 has to hold is an eighth of the vector instead of all of it
  const int64_t rows_per_wg = (int64_t)blockDim.x * RPT;
  const int64_t nchunks = (n + rows_per_wg - 1) / rows_per_wg;
  int64_t chunk = blockIdx.x, chunk_end = nchunks, chunk_step = gridDim.x;
  if (xcd & 1) {
    const int64_t per = (nchunks + 7) / 8;
    chunk = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    chunk_end = ((blockIdx.x & 7) + 1) * per < nchunks ? ((blockIdx.x & 7) + 1) * per : nchunks;
    chunk_step = gridDim.x >> 3;
  }
  for (; chunk < chunk_end; chunk += chunk_step) {
    const int64_t r = chunk * rows_per_wg + (int64_t)threadIdx.x * RPT;
    if (r >= n) continue;
    if (spmv_part_skip(part, chunk * rows_per_wg, (chunk + 1) * rows_per_wg)) continue;  // workgroup-uniform
    dia_rows<RPT, U, TRIPLES>(r, n, npad, K, O, flags, cols, vals, x, y, alpha, beta, dotw, xcd, dot_acc);
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// the rows outside [skip_lo, skip_hi) through the plain per-row code on the slot-major copy (chunks that lie inside the range are not
// visited, rows of straddling chunks are masked)
template <bool TRIPLES>
__global__ __launch_bounds__(MFEM_BLOCK) void k_spmv_dia_outside(int64_t n, int64_t npad, int K, const DiaOffsets* __restrict__ Op,
                                                                   const int32_t* __restrict__ flags, const int32_t* __restrict__ cols,
                                                                   const double* __restrict__ vals, const double* __restrict__ x,
                                                                   double* __restrict__ y, double alpha, double beta,
                                                                   const double* __restrict__ dotw, double* __restrict__ partials,
                                                                   const int32_t* __restrict__ done_flag, int64_t skip_lo, int64_t skip_hi) {
  __shared__ double red[16];
  if (done_flag && done_flag[0]) return;
  double dot_acc = 0.0;
  const int64_t R = 2 * MFEM_BLOCK, nchunks = (n + R - 1) / R;
  int64_t cA = (skip_lo + R - 1) / R, cB = skip_hi / R;
  if (cB < cA) cB = cA;
  for (int64_t q = blockIdx.x; q < cA + (nchunks - cB); q += gridDim.x) {
    const int64_t ch = q < cA ? q : cB + (q - cA);
    const int64_t r = ch * R + 2 * (int64_t)threadIdx.x;
    if (r < n) dia_rows<2, 3, TRIPLES>(r, n, npad, K, *Op, flags, cols, vals, x, y, alpha, beta, dotw, 0, dot_acc, skip_lo, skip_hi);
  }
  if (partials) {
    const double b = block_reduce_sum(dot_acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
  }
}

// neg[0] = 1 if the stored diagonal of row r is negative (the symmetric scaling multiplies it by a square: the sign of the scaled diagonal)
template <typename RP>
__global__ __launch_bounds__(64) void k_symp_diag_sign(int64_t r, const RP* __restrict__ rowptr, const int32_t* __restrict__ col, const double* __restrict__ vals,
                                                        int base, int32_t* __restrict__ neg) {
  const int64_t lo = (int64_t)rowptr[r] - base, hi = (int64_t)rowptr[r + 1] - base;
  for (int64_t j = lo + threadIdx.x; j < hi; j += 64)
    if ((int64_t)col[j] - base == r && __double_as_longlong(vals[j]) < 0) neg[0] = 1;
}

// The reference row of the constant form (symp_const_decide.h): row r -- the centre of the swept region -- formed as k_symp_fill forms it, lane s = slot s
// (a row of 27 entries has entry s in slot s).  valid = 0 when the row is short or, coded form, its diagonal has no code counted from the unit of dcbad[1].
// One wave, in front of the fill.
template <typename RP, bool SYM, bool DC>
__global__ __launch_bounds__(64) void k_symp_const_ref(int64_t r, const RP* __restrict__ rowptr, const double* __restrict__ vals, int base,
                                                        const DiaOffsets* __restrict__ Op, int cls, const double* __restrict__ ssym,
                                                        const int32_t* __restrict__ dcbad, SympConst* __restrict__ ref) {
  const int lane = threadIdx.x;
  const int64_t lo = (int64_t)rowptr[r] - base, hi = (int64_t)rowptr[r + 1] - base;
  const bool full = hi - lo == 27;
  int code = 0;
  bool coded = true;
  if (full && lane < 27) {
    double srow = 1.0, sc = 1.0;
    if constexpr (SYM) {
      srow = ssym[r];
      sc = ssym[r + Op->off[cls][lane]];
    }
    const double v = symp_formed<SYM>(vals[lo + lane], srow, sc);
    ref->v[lane] = v;
    if (DC && lane == 13) coded = sp_diag_code(v, code, sp_unit_bits(dcbad[1]));
  }
  const bool ok = full && __ballot(!coded) == 0;
  if (lane == 13) {
    ref->code = code;
    ref->valid = ok ? 1 : 0;
  }
}

// lattice lines of odd length: the lane pair at the line's end holds the last point and a cell outside the lattice, which no row writes
// and the sweep reads as a structurally absent entry -- an explicit zero in all 27 slots of every step of the last patch column
__global__ __launch_bounds__(MFEM_BLOCK) void k_symp_zero_odd(SympGeom Gm, double* __restrict__ pv) {
  const int NP = Gm.NR * Gm.NPk, nplanes = Gm.p1 - Gm.p0, B = Gm.B, MAINB = sp_main(B, Gm.DC), LOWB = sp_low(B), NSL = sp_nslots(Gm.DC);
  const int64_t T = (int64_t)NP * nplanes, cells = (int64_t)nplanes * Gm.NS * SP_L * 27;
  const int col = Gm.ms2 - (Gm.NPk - 1) * SP_W;  // first column past the line in the last patch column (odd, < SP_W)
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cells; t += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(t % 27), line = (int)((t / 27) % SP_L);
    const int64_t q = t / (27 * SP_L);
    const int strip = (int)(q % Gm.NS), pl = (int)(q / Gm.NS);
    const int band = strip % B;
    const int64_t step = (int64_t)pl * NP + (int64_t)(strip / B) * Gm.NPk + (Gm.NPk - 1);
    const int idx = line * SP_W + col;
    if (s < 13) pv[T * MAINB + step * LOWB + band * 13 * SP_ROWS + s * SP_ROWS + idx] = 0.0;
    else if (s >= 27 - NSL) pv[step * MAINB + band * NSL * SP_ROWS + (s - (27 - NSL)) * SP_ROWS + idx] = 0.0;  // (coded form: the fill writes every code byte)
  }
}

// Candidate diagonal lists: the offsets of one full-length row from each of 8 windows along the matrix (a field-major multi-field matrix has
// one list per field)
static int dia_sample_lists(mfem_context_s* ctx, const mfem_csr_s* A, DiaOffsets& O) {
  const int K = A->ell_K;
  memset(&O, 0, sizeof(O));
  for (int wdw = 0; wdw < 8 && O.ncls < DIA_MAXC; ++wdw) {
    const int64_t centre = A->n * (2 * wdw + 1) / 16;
    const int64_t w0 = centre > 1024 ? centre - 1024 : 0;
    const int64_t wn = (A->n - w0) < 2048 ? (A->n - w0) : 2048;  // rows in the window
    if (wn <= 0) continue;
    mfem_host_alloc_probe();
    const size_t rb = A->rowptr_bits / 8;  // the window's row pointers, in the pattern's width
    std::vector<char> raw((size_t)(wn + 1) * rb);
    MFEM_CHECK_HIP(hipMemcpyAsync(raw.data(), (const char*)A->rowptr + w0 * rb, raw.size(), hipMemcpyDeviceToHost, ctx->stream));
    MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    auto win = [&](int64_t i) -> int64_t { return rb == 8 ? ((const int64_t*)raw.data())[i] : ((const int32_t*)raw.data())[i]; };
    int64_t rm = -1;
    for (int64_t i = 0; i < wn && rm < 0; ++i)
      if (win(i + 1) - win(i) == K) rm = i;
    if (rm < 0) continue;
    int32_t cbuf[DIA_MAXD];
    MFEM_CHECK_HIP(hipMemcpyAsync(cbuf, A->colidx + (win(rm) - A->index_base), sizeof(int32_t) * K, hipMemcpyDeviceToHost, ctx->stream));
    MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    int32_t cand[DIA_MAXD];
    for (int i = 0; i < K; ++i) cand[i] = (int32_t)((int64_t)cbuf[i] - A->index_base - (w0 + rm));
    bool seen = false;
    for (int c = 0; c < O.ncls && !seen; ++c) seen = memcmp(O.off[c], cand, sizeof(int32_t) * K) == 0;
    if (!seen) {
      memcpy(O.off[O.ncls], cand, sizeof(int32_t) * K);
      O.D[O.ncls] = K;
      ++O.ncls;
    }
  }
  return MFEM_OK;
}

// Which list, if any, each 128-row block obeys: leaves the lists (A->dia_dev) and the flags (A->dia_flags) on the device, *nreg = regular blocks
static int dia_flag_blocks(mfem_context_s* ctx, mfem_csr_s* A, const DiaOffsets& O, int32_t* nreg) {
  const int64_t nblk = A->ell_npad / ELL_B;
  const int64_t nx = A->n + (ctx->comm ? 2 * ctx->halo_plane_len * ctx->halo_fields : 0);  // length of the local x
  MFEM_CHECK_HIP(hipMalloc(&A->dia_flags, sizeof(int32_t) * (size_t)nblk));
  MFEM_CHECK_HIP(hipMalloc(&A->dia_dev, sizeof(DiaOffsets)));
  MFEM_CHECK_HIP(hipMemcpyAsync(A->dia_dev, &O, sizeof(DiaOffsets), hipMemcpyHostToDevice, ctx->stream));
  MFEM_CHECK_HIP(hipMemsetAsync(A->dia_flags, 0, sizeof(int32_t) * (size_t)nblk, ctx->stream));
  int32_t* d_cnt = ctx->d_flags + 9;
  MFEM_CHECK_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t), ctx->stream));
  const int g2 = (int)(nblk < (int64_t)ctx->num_cus * 64 ? nblk : (int64_t)ctx->num_cus * 64);
  mfem_by_rowptr(A, [&](auto t) {
    hipLaunchKernelGGL(k_dia_flags<decltype(t)>, dim3(g2), dim3(128), 0, ctx->stream, A->n, nx, (const decltype(t)*)A->rowptr, A->colidx, A->index_base,
                       (const DiaOffsets*)A->dia_dev, A->dia_flags, d_cnt);
  });
  MFEM_CHECK_LAUNCH();
  MFEM_CHECK_HIP(hipMemcpyAsync(ctx->h_flags + 9, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MFEM_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // also orders the H2D copy of the caller's O
  *nreg = ctx->h_flags[9];
  return MFEM_OK;
}

// do the diagonals of every list come in runs of three consecutive offsets (o, o + 1, o + 2: the fastest lattice direction)?
static bool dia_has_triples(const DiaOffsets& O, int K) {
  if (K % 3 != 0) return false;
  for (int c = 0; c < O.ncls; ++c)
    for (int i = 0; i + 2 < K; i += 3)
      if (O.off[c][i + 1] != O.off[c][i] + 1 || O.off[c][i + 2] != O.off[c][i] + 2) return false;
  return true;
}

// the list with the form of the 27-point lattice stencil, offsets di PL + dj m2 + dk (a slab has further lists for the rows next to its ghost
// planes); -1: none
static int dia_lattice_class(const DiaOffsets& O, int K, int64_t* m2_out, int64_t* PL_out) {
  for (int c = 0; c < O.ncls && K == 27; ++c) {
    if (O.D[c] != 27 || O.off[c][13] != 0 || O.off[c][14] != 1) continue;
    const int64_t m2 = *m2_out = O.off[c][16], PL = *PL_out = O.off[c][22];
    bool lattice = m2 > 2 && PL > 2 * m2;
    for (int q = 0; q < 27 && lattice; ++q)
      if (O.off[c][q] != (q / 9 - 1) * PL + ((q / 3) % 3 - 1) * m2 + (q % 3 - 1)) lattice = false;
    if (lattice) return c;
  }
  return -1;
}

// blocks [*lo, *hi): the longest run of whole blocks that are regular for list `cls` (both sweeps work on rows inside it)
static void dia_longest_run(const std::vector<int32_t>& hf, int cls, int64_t n, int64_t* best_lo, int64_t* best_hi) {
  const int64_t nblk = (int64_t)hf.size();
  int64_t lo = -1;
  *best_lo = *best_hi = 0;
  for (int64_t b = 0; b <= nblk; ++b) {
    const bool reg = b < nblk && hf[(size_t)b] == cls + 1 && (b + 1) * ELL_B <= n;
    if (reg && lo < 0) lo = b;
    if (!reg && lo >= 0) {
      if (b - lo > *best_hi - *best_lo) { *best_lo = lo; *best_hi = b; }
      lo = -1;
    }
  }
}

// Diagonal structure?  The layout is taken when at least half of the blocks are regular (the others run the explicit-column loop, as in mode 1).
int mfem_dia_plan(mfem_context_s* ctx, mfem_csr_s* A) {
  A->dia_state = -1;
  const int K = A->ell_K;
  if (K > DIA_MAXD) return MFEM_OK;
  DiaOffsets O;
  int rc = dia_sample_lists(ctx, A, O);
  if (rc || O.ncls == 0) return rc;
  int32_t nreg = 0;
  rc = dia_flag_blocks(ctx, A, O, &nreg);
  if (rc) return rc;
  const int64_t nblk = A->ell_npad / ELL_B;
  if ((double)nreg < 0.5 * (double)nblk) {
    hipFree(A->dia_flags);
    hipFree(A->dia_dev);
    A->dia_flags = nullptr;
    A->dia_dev = nullptr;
    return MFEM_OK;
  }
  A->dia_state = 1;
  A->dia_classes = O.ncls;
  A->dia_regular_blocks = nreg;
  A->dia_triples = dia_has_triples(O, K);
  // 27-point lattice stencil: candidate for the symmetric sweeps
  A->sym_state = -1;
  int64_t m2 = 0, PL = 0;
  const int lc = dia_lattice_class(O, K, &m2, &PL);
  if (lc < 0) return MFEM_OK;
  std::vector<int32_t> hf((size_t)nblk);
  MFEM_CHECK_HIP(hipMemcpy(hf.data(), A->dia_flags, sizeof(int32_t) * (size_t)nblk, hipMemcpyDeviceToHost));
  int64_t run_lo = 0, run_hi = 0;
  dia_longest_run(hf, lc, A->n, &run_lo, &run_hi);
  mfem_sym_plan(A, O.off[lc], lc, m2, PL, run_lo, run_hi);
  return MFEM_OK;
}

// The copies of a bind: the slot-major copy of `vals` into buf; with pvals the rows of the swept planes G go straight to the patch-major copy there
// instead -- by k_symp_fill (patch-aligned tiles) where its conditions hold, after k_dia_vals has done the other rows, else by k_dia_vals.
// *fp_made: the fill left the symmetry fingerprint of the swept rows, asked for with want_fp, in d_flags[16..17].
// k_symp_fill fills the swept rows of a direct bind: a lane per row (K <= 64), no column scaling pass, 32-bit row arithmetic, lattice lines and planes long
// enough for its column decoding (bit 29 of the "ell" knob turns it off)
bool mfem_dia_fill_fast(const mfem_csr_s* A, const double* dsc, bool direct) {
  return direct && A->symp_state == 1 && 8 * 64 * (size_t)A->ell_K * 2 <= 64 * 1024 && !dsc && A->n < ((int64_t)1 << 31) && A->symp_PL < ((int64_t)1 << 30) &&
         A->symp_m1 >= 3 && A->symp_m2 >= 3 && g_ell.dia_fast;
}
int mfem_dia_copy(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, const double* ssym, const SympGeom& G,
                  double* pvals, double* rim, bool want_fp, bool* fp_made, unsigned char* sflags, bool* flags_made) {
  if (flags_made) *flags_made = false;
  const DiaOffsets* O = (const DiaOffsets*)A->dia_dev;
  if (pvals && (G.ms2 & 1)) {  // lattice lines of odd length leave cells of the patch-major copy that no row writes
    const int64_t cells = (int64_t)(G.p1 - G.p0) * G.NS * SP_L * 27;
    hipLaunchKernelGGL(k_symp_zero_odd, dim3(mfem_grid_for(cells, MFEM_BLOCK, ctx->num_cus * 8)), dim3(MFEM_BLOCK), 0, ctx->stream, G, pvals);
    MFEM_CHECK_LAUNCH();
  }
  // a lane per row while at least two waves of 64-row tiles fit 64 KB of staging (K <= 42: the 27-diagonal lattice); two lanes per row,
  // 32-row tiles, beyond (the 81 diagonals of three fields)
  const size_t eb = dsc ? 12 : 8;  // 8 B value (+ 4 B column for the scaling pass) per staged entry (<= rt K per tile)
  const int lpr = eb * 64 * (size_t)A->ell_K * 2 > 64 * 1024 ? 2 : 1;
  const int rt = 64 / lpr;
  int wv = 2;  // two-wave workgroups: what fits a CU is then decided in steps of two waves (27 diagonals: 27.6 KB per workgroup, 5 per CU)
  while (wv > 1 && eb * rt * (size_t)A->ell_K * wv > 64 * 1024) wv >>= 1;
  const size_t ldsb = eb * rt * (size_t)A->ell_K * wv;
  const int64_t nt = A->ell_npad / rt;
  int g = (int)((nt + wv - 1) / wv);
  if (g > ctx->num_cus * 16) g = ctx->num_cus * 16;
  // k_symp_fill: a patch-major copy to fill, no column scaling pass, 32-bit row arithmetic, lattice lines and planes long enough for its column
  // decoding (bit 29 of the "ell" knob turns it off)
  const bool fast = pvals && mfem_dia_fill_fast(A, dsc, true);
  // the software-pipelined staging: a lane per row, rows of at most 28 entries, no scaling pass (bit 28 turns it off)
  const bool pipe = lpr == 1 && !dsc && A->ell_K <= 28 && g_ell.dia_pipe && !fast;
  const int64_t ft = (int64_t)(G.p1 - G.p0) * G.NR * G.NPk;  // the fill: patch steps, one workgroup of two waves each
  int gf = (int)(ft < (int64_t)ctx->num_cus * 20 ? ft : (int64_t)ctx->num_cus * 20);  // (5 workgroups are resident per CU: four rounds)
  if (gf < 1) gf = 1;
  unsigned long long* fpr = fast && want_fp ? (unsigned long long*)(ctx->d_flags + 16) : nullptr;
  *fp_made = fpr != nullptr;
  const bool coded = G.DC != 0;  // (decided by the bind, mfem_symp_coded_wanted: only with the fill and the symmetric scaling)
  if (coded && !(fast && ssym)) return MFEM_ERR_INVALID;
  int32_t* dcbad = ctx->d_flags + 18;  // beside the fingerprint; [19]: the unit is -1.0
  return mfem_by_rowptr(A, [&](auto t) -> int {
    using RP = decltype(t);
    auto kv = ssym ? k_dia_vals<RP, 1, true, false> : k_dia_vals<RP, 1, false, false>;
    if (lpr == 2) kv = ssym ? k_dia_vals<RP, 2, true, false> : k_dia_vals<RP, 2, false, false>;
    else if (pipe) kv = ssym ? k_dia_vals<RP, 1, true, true> : k_dia_vals<RP, 1, false, true>;
    hipLaunchKernelGGL(kv, dim3(g), dim3(64 * wv), ldsb, ctx->stream, A->n, A->ell_npad, A->ell_K, (const RP*)A->rowptr, A->colidx, vals, A->index_base,
                       O, A->dia_flags, buf, G, pvals, dsc, ssym, fast ? 1 : 0);
    MFEM_CHECK_LAUNCH();
    if (rim && G.rim_units > 0) {  // after k_dia_vals: the rim rows' diagonals of the slot-major copy are this kernel's where both write them (the same value)
      const int gr = (int)(G.rim_units < (int64_t)ctx->num_cus * 32 ? G.rim_units : (int64_t)ctx->num_cus * 32);
      hipLaunchKernelGGL(k_symp_rim_fill<RP>, dim3(gr), dim3(64), 0, ctx->stream, A->ell_K, (const RP*)A->rowptr, A->colidx, vals, A->index_base, buf, G, rim, dsc, ssym);
      MFEM_CHECK_LAUNCH();
    }
    if (!fast) return MFEM_OK;
    if (fpr) MFEM_CHECK_HIP(hipMemsetAsync(fpr, 0, sizeof(unsigned long long), ctx->stream));
    if (coded) {  // the gate's flag, and the sign of the unit the codes count from
      MFEM_CHECK_HIP(hipMemsetAsync(dcbad, 0, 2 * sizeof(int32_t), ctx->stream));
      hipLaunchKernelGGL(k_symp_diag_sign<RP>, dim3(1), dim3(64), 0, ctx->stream, (int64_t)G.p0 * G.PL, (const RP*)A->rowptr, A->colidx, vals, A->index_base, dcbad + 1);
      MFEM_CHECK_LAUNCH();
    }
    SympConst* cref = (SympConst*)(ctx->d_flags + SPC_REF_AT);
    int32_t* scount = ctx->d_flags + SPC_COUNT_AT;
    if (sflags) {  // the constant form's reference row: the centre of the swept region (middle swept plane, line ms1 / 2, point ms2 / 2), formed as the fill forms it
      const int64_t rr = (int64_t)(G.p0 + (G.p1 - G.p0) / 2) * G.PL + (int64_t)(G.ms1 / 2) * G.m2 + G.ms2 / 2;
      MFEM_CHECK_HIP(hipMemsetAsync(scount, 0, sizeof(int32_t), ctx->stream));
      const auto kr = coded ? k_symp_const_ref<RP, true, true> : ssym ? k_symp_const_ref<RP, true, false> : k_symp_const_ref<RP, false, false>;
      hipLaunchKernelGGL(kr, dim3(1), dim3(64), 0, ctx->stream, rr, (const RP*)A->rowptr, vals, A->index_base, O, A->sym_cls, ssym, (const int32_t*)dcbad, cref);
      MFEM_CHECK_LAUNCH();
      if (flags_made) *flags_made = true;
    }
    const auto kf = coded ? k_symp_fill<RP, true, true> : ssym ? k_symp_fill<RP, true> : k_symp_fill<RP, false>;
    const int fB = G.B > 0 ? G.B : 1;
    hipLaunchKernelGGL(kf, dim3(gf), dim3(128), sizeof(double) * (2 * (2 * SP_W * 27) + sp_epad(fB) + sp_cpad(fB, G.DC) + 1 + 27), ctx->stream, A->n, A->ell_K, (const RP*)A->rowptr,
                       A->colidx, vals, A->index_base, O, A->sym_cls, buf, G, pvals, ssym, fpr, dcbad, (const SympConst*)cref, sflags, scount);
    MFEM_CHECK_LAUNCH();
    return MFEM_OK;
  });
}

// all rows by the plain per-row kernel, with the shared x loads of three consecutive diagonals (`triples`) or without; `cap` workgroups at most
int mfem_dia_launch(mfem_context_s* ctx, mfem_csr_s* A, bool triples, int cap, const SpmvArgs& a) {
  const int gd = mfem_grid_for((A->n + 1) / 2, MFEM_BLOCK, cap);
  const auto k = triples ? k_spmv_dia<2, 3, true> : k_spmv_dia<2, 3, false>;
  hipLaunchKernelGGL(k, dim3(gd), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, A->ell_npad, A->ell_K, (const DiaOffsets*)A->dia_dev, A->dia_flags,
                     A->ell_cols, A->ell_vals, a.x, a.y, a.alpha, a.beta, a.dotw, a.partials, a.done_flag, (int)g_ell.xcd, a.part);
  MFEM_CHECK_LAUNCH();
  if (a.n_partials && a.partials) *a.n_partials = gd;
  return MFEM_OK;
}
// the rows outside [lo, hi) by the per-row code (the patch sweep's boundary part); *ngrid = its workgroups = the partial sums it wrote to `partials`
int mfem_dia_launch_outside(mfem_context_s* ctx, mfem_csr_s* A, const SpmvArgs& a, double* partials, int64_t lo, int64_t hi, int* ngrid) {
  const int64_t outside = (lo + 511) / 512 + (A->n - hi + 511) / 512 + 2;
  *ngrid = (int)(outside < 1 ? 1 : outside < 1024 ? outside : 1024);
  const auto k = A->dia_triples ? k_spmv_dia_outside<true> : k_spmv_dia_outside<false>;
  hipLaunchKernelGGL(k, dim3(*ngrid), dim3(MFEM_BLOCK), 0, ctx->stream, A->n, A->ell_npad, A->ell_K, (const DiaOffsets*)A->dia_dev, A->dia_flags,
                     A->ell_cols, A->ell_vals, a.x, a.y, a.alpha, a.beta, a.dotw, partials, a.done_flag, lo, hi);
  MFEM_CHECK_LAUNCH();
  return MFEM_OK;
}
