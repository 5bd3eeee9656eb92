// What the files of the slot-major solver layout share.  spmv_ell.hip: the entry points (layouts.h, common.h) and mode 1, explicit columns;
// spmv_dia.hip: mode 2, the diagonal-slotted copy, its inspection and its per-row kernel; spmv_sym.hip: the two symmetric sweeps on that
// copy.  Here: the layout's addressing, the diagonal lists, the per-row product code, the decoded "ell" knob word, the one
// decision which kernel serves a diagonal-slotted copy, and the host functions one family offers another.  The library is one code object per
// .hip file: a kernel is defined in one file and launched from that file only; other files call a host function.
#pragma once
#include <vector>

#include "layouts.h"
#include "spmv_symp.h"
#include "symp_trim_decide.h"
#include "symp_const_decide.h"
#include "symp_sched_decide.h"

// Blocked slot-major layout ("sliced ELL"): rows are grouped in blocks of ELL_B = 128 (the rows of one wave at two rows per
// lane); block b stores its K slots one after the other, element (row r, slot s) at  b * K * 128 + s * 128 + (r & 127).
// A wave therefore reads ONE contiguous K-kilobyte chunk per block and the kernel as a whole walks memory front to back
// like a copy, instead of K streams a full vector length apart.
#define ELL_B 128
__host__ __device__ __forceinline__ int64_t ell_base(int64_t r, int K) { return (r >> 7) * ((int64_t)K * ELL_B) + (r & (ELL_B - 1)); }

typedef double e_d2 __attribute__((ext_vector_type(2)));
typedef int e_i2 __attribute__((ext_vector_type(2)));
typedef double u_d2 __attribute__((ext_vector_type(2), aligned(8)));

// Several diagonal lists ("classes") may coexist: a 3-field matrix in field-major numbering has one list per row field
// ((g - f) * n_nodes + stencil offset).  Each regular block belongs to one class.
#define DIA_MAXD 96
#define DIA_MAXC 4
struct DiaOffsets {
  int ncls;
  int D[DIA_MAXC];
  int32_t off[DIA_MAXC][DIA_MAXD];
};

// geometry of the wave-private patch sweep (k_spmv_symp, spmv_sym.hip)
struct SympGeom {
  int64_t PL, nx;
  int m1, m2, p0, p1, NS, NPk;
  int nseg;  // runs per patch: a run = one patch swept through nplanes / nseg consecutive planes
  int B, NR; // bands of SP_L lines per patch (1 or 2); patch rows = ceil(NS / B): NR * NPk patches per plane (NS: strips of SP_L lines)
  int DC;    // form of the copy's main part (spmv_symp.h): 0 the diagonal stored as slot 13, 1 carried as one-byte ulp codes
  long long unit;  // DC = 1: bits of the unit the codes count from, +1.0 or -1.0 (known once the fill has run: the sweep's launches carry it)
  // swept extents (symp_trim_decide.h): the patches cover lines [0, ms1) x points [0, ms2) of a plane -- NS, NPk, NR count those -- and the other rows of
  // the swept planes, the rim, are computed row by row from a compact copy behind the patch-major one.  Lane validity, rows and x offsets use m1, m2.
  int ms1, ms2;
  int rim_pp;              // rim rows per plane
  int64_t rim_rows, rim_units;  // rim rows of all swept planes; units of SPT_UNIT rows of their copy
};
// The constant form of the patch sweep (symp_const_decide.h).  On the device (ctx->d_flags + SPC_REF_AT, written by k_symp_const_ref before the fill): the
// reference row's 27 values as the fill forms them, its diagonal's code (coded form) and whether the row had all 27 entries (and a code).  In the
// sweep's arguments (CS = 1): the same values, passed by value -- wave-uniform, they live in scalar registers.
struct SympConst {
  double v[27];
  int32_t code, valid;
};
#define SPC_COUNT_AT 20  // ctx->d_flags[20]: flagged steps of the last fill
#define SPC_REF_AT 22    // ctx->d_flags[22..77]: the SympConst (8-byte aligned)
static_assert(SPC_REF_AT % 2 == 0 && SPC_REF_AT * 4 + sizeof(SympConst) <= MFEM_NFLAGS * 4, "the reference row must fit the context's flags");
// the rows outside the swept planes, taken by the sweep's waves after their runs (unsplit SpMV): per-row code on the slot-major copy
struct SympTail {
  int on, K;
  int rim;                  // the sweep's waves also take the units of rim rows (symp_trim_decide.h) after their runs; else a launch of their own (k_symp_rim)
  int64_t n, npad, lo, hi;  // rows [lo, hi) are the sweep's
  const DiaOffsets* Op;
  const int32_t* flags;
  const int32_t* cols;
  const double* ell;
};

// the copies are written as full coalesced streams and not read again by this kernel: nontemporal stores (per-solve work of C2 3.65 -> 3.3 ms)
#if defined(DV_ABL) && DV_ABL == 1   // timing-only ablation builds (tools/ab_libs.sh; never in the product library): 1 = no stores (one per lane and tile
#define DIA_ST(p, v) do { if ((v) == 1.2345e300) __builtin_nontemporal_store((v), (p)); } while (0)  // keeps the loads alive), 3 = plain instead of nontemporal stores
#elif defined(DV_ABL) && DV_ABL == 3
#define DIA_ST(p, v) (*(p) = (v))
#else
#define DIA_ST(p, v) __builtin_nontemporal_store((v), (p))
#endif
#define SYM_LD(p) __builtin_nontemporal_load(p)  // plain loads measured slower: 0.954 vs 0.928 ms per CG iteration at 256^3

// The RPT rows r .. r + RPT - 1 of one lane (r a multiple of RPT; a wave covers aligned 128-row blocks): regular blocks by
// diagonal, the others through their explicit columns.  Shared by the plain kernel and the symmetric sweep kernel (which
// sends the chunks outside its regular range here).
template <int RPT, int U, bool TRIPLES>
__device__ __forceinline__ void dia_rows(int64_t r, int64_t n, int64_t npad, int K, const DiaOffsets& O,
                                         const int32_t* __restrict__ flags, const int32_t* __restrict__ cols,
                                         const double* __restrict__ vals, const double* __restrict__ x, double* __restrict__ y,
                                         double alpha, double beta, const double* __restrict__ dotw, int xcd, double& dot_acc,
                                         int64_t skip_lo = 0, int64_t skip_hi = 0) {  // rows in [skip_lo, skip_hi) belong to another launch
  constexpr int H = RPT / 2;  // 16-byte pairs per lane
  const double* v = vals + ell_base(r, K);
  e_d2 acc[H];
  double xself0 = 0.0, xself1 = 0.0;  // x[r], x[r + 1] when the kernel has loaded them anyway (fused w.y with w == x, as in CG)
  bool have_self = false;
#pragma unroll
  for (int h = 0; h < H; ++h) acc[h] = (e_d2){0.0, 0.0};
  // the wave's rows [b0, b0 + 64 RPT) are RPT / 2 aligned 128-row blocks: regular only if all of them are (wave-uniform)
  const int64_t blk = r / (64 * RPT) * (RPT / 2);
  const int cls = __builtin_amdgcn_readfirstlane(flags[blk]) - 1;  // wave-uniform: keeps the offset reads scalar
  bool interior = cls >= 0;
  if (RPT == 4) interior = interior && ((blk + 1) * 128 < npad) && flags[blk + 1] == cls + 1;
  const int32_t* off = O.off[cls < 0 ? 0 : cls];
  const int D = O.D[cls < 0 ? 0 : cls];
  if (interior && TRIPLES && RPT == 2) {
    // the diagonals come in runs of three consecutive offsets (o - 1, o, o + 1: the fastest lattice direction): the two
    // rows of the lane need x[r + o - 1 .. r + o + 2] for the whole run -- two 16-byte loads instead of three
    for (int s = 0; s < D; s += 3) {
      const e_d2 va = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + s * ELL_B));
      const e_d2 vb = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + (s + 1) * ELL_B));
      const e_d2 vc = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + (s + 2) * ELL_B));
      const u_d2* xp = reinterpret_cast<const u_d2*>(x + r + off[s]);
      const u_d2 xa = xp[0], xb = xp[1];
      acc[0].x += va.x != 0.0 ? va.x * xa.x : 0.0;
      acc[0].y += va.y != 0.0 ? va.y * xa.y : 0.0;
      acc[0].x += vb.x != 0.0 ? vb.x * xa.y : 0.0;
      acc[0].y += vb.y != 0.0 ? vb.y * xb.x : 0.0;
      acc[0].x += vc.x != 0.0 ? vc.x * xb.x : 0.0;
      acc[0].y += vc.y != 0.0 ? vc.y * xb.y : 0.0;
      if (off[s + 1] == 0) {  // the main diagonal's run: x[r], x[r + 1] are the lane's own entries (wave-uniform test)
        xself0 = xa.y;
        xself1 = xb.x;
        have_self = true;
      }
    }
  } else if (interior) {
    int s = 0;
    for (; s + U <= D; s += U) {
      e_d2 vv[U][H];
      u_d2 xx[U][H];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < H; ++h) {
          vv[u][h] = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + (s + u) * ELL_B) + h);
          xx[u][h] = *(reinterpret_cast<const u_d2*>(x + r + off[s + u]) + h);
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < H; ++h) {
          // a zero slot stands for "no entry": it must not pick up a non-finite x from a position the CSR row never reads
          acc[h].x += vv[u][h].x != 0.0 ? vv[u][h].x * xx[u][h].x : 0.0;
          acc[h].y += vv[u][h].y != 0.0 ? vv[u][h].y * xx[u][h].y : 0.0;
        }
    }
    for (; s < D; ++s)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const e_d2 vv = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + s * ELL_B) + h);
        const u_d2 xx = *(reinterpret_cast<const u_d2*>(x + r + off[s]) + h);
        acc[h].x += vv.x != 0.0 ? vv.x * xx.x : 0.0;
        acc[h].y += vv.y != 0.0 ? vv.y * xx.y : 0.0;
      }
  } else {  // generic block (boundary rows, ghost columns): explicit columns, compact slots
    const int32_t* c = cols + ell_base(r, K);
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        if (r + 2 * h >= npad) continue;
        const e_d2 vv = __builtin_nontemporal_load(reinterpret_cast<const e_d2*>(v + s * ELL_B) + h);
        const e_i2 cc = __builtin_nontemporal_load(reinterpret_cast<const e_i2*>(c + s * ELL_B) + h);
        acc[h].x += vv.x * x[cc.x];
        acc[h].y += vv.y * x[cc.y];
      }
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const int64_t rr = r + 2 * h;
    if (rr >= n) break;
    double y0 = alpha * acc[h].x, y1 = alpha * acc[h].y;
    const bool one = rr < skip_lo || rr >= skip_hi;
    const bool two = rr + 1 < n && (rr + 1 < skip_lo || rr + 1 >= skip_hi);
    if (beta != 0.0) {
      if (one) y0 += beta * y[rr];
      if (two) y1 += beta * y[rr + 1];
    }
    if (one) y[rr] = y0;
    if (two) y[rr + 1] = y1;
    if (dotw) {
      if (RPT == 2 && have_self && dotw == x) {  // p.Ap of CG: p[r], p[r + 1] are already in registers
        if (one) dot_acc += y0 * xself0;
        if (two) dot_acc += y1 * xself1;
      } else {
        if (one) dot_acc += y0 * dotw[rr];
        if (two) dot_acc += y1 * dotw[rr + 1];
      }
    }
  }
}

// The "ell" knob word (mfem_debug_set_ell, spmv_ell.hip), decoded once by its setter.  Read when a layout is planned and bound -- a product
// runs the kernel its bind recorded -- and, for the launch geometry alone (grid_mult, xcd, symp_tail), when a product is launched.
struct EllKnobs {
  std::atomic<int> enable{1};            // bit 0: modes 1 and 2 on
  std::atomic<int> dia{1};               // bit 1 clears it: explicit columns even when the matrix is diagonal-structured
  std::atomic<int> symp_trim{0};         // bit 2 forces the untrimmed patch sweep (every row of a swept plane in a patch), bit 3 the trimmed one at any size (0: mfem_symp_trim_wanted decides by size)
  std::atomic<int> symp_const{0};        // bit 4 forces the stored form of the patch sweep, bit 5 the constant form whatever the share of flagged steps (0: spc_gate decides; symp_const_decide.h)
  std::atomic<int> grid_mult{6};         // bits 8-15 (0 keeps the value): persistent workgroups per CU of the per-row kernels (profiles/r01_spmv_sweep.txt: 6 or 8)
  std::atomic<int> shared_x{1};          // bits 16-19 = 8 clears it: the plain per-row kernel without the shared x loads of three consecutive diagonals, no sweep
  std::atomic<int> xcd{0};               // bit 20: each XCD walks a contiguous eighth of the rows (k_spmv_dia; needs a grid that is a multiple of 8)
  std::atomic<int> symp_coded{1};        // bit 21 clears it: the scaled CG's patch-major copy keeps its diagonal as stored doubles (mfem_symp_coded_wanted)
  std::atomic<int> sym{1};               // bit 22 clears it: no symmetric sweep kernel
  std::atomic<int> symp{1};              // bit 23 clears it: the workgroup-tile sweep (k_spmv_sym27) instead of the wave-private patch sweep (k_spmv_symp)
  std::atomic<int> symp_bands{0};        // bits 24 / 25 force one / two bands of four lines per patch (0: mfem_symp_bands_wanted decides by size)
  std::atomic<int> symp_tail{1};         // bit 26 clears it: the rows outside the swept planes in a launch of their own (as in a split SpMV)
  std::atomic<int> symp_direct{1};       // bit 27 clears it: the patch-major copy made from the slot-major copy in a second pass (k_symp_bind)
  std::atomic<int> dia_pipe{1};          // bit 28 clears it: the layout copy (k_dia_vals) without its software pipeline
  std::atomic<int> dia_fast{1};          // bit 29 clears it: the swept rows by k_dia_vals' row tiles instead of k_symp_fill (then pipelined as in bit 28)
  std::atomic<int> symp_fingerprint{1};  // bit 30 clears it: the symmetry of the swept rows by the check pass (k_spmv_symp<1>) instead of the fill's fingerprint
};
extern EllKnobs g_ell;
extern std::atomic<int64_t> g_layout_min_rows_dia, g_layout_min_rows_cols;  // spmv_ell.hip

// The product kernels of a diagonal-slotted copy: the per-row kernel k_spmv_dia without / with the shared x loads of three consecutive diagonals,
// the workgroup-tile sweep, the patch sweep.  A bind records the one its values got in mfem_csr_s::dia_kernel.
enum DiaKernel : int { DIA_NONE = 0, DIA_ROWS, DIA_ROWS_TRIPLES, DIA_SYM27, DIA_SYMP };
// THE decision which of them a copy wants, from the plan and the knobs (spmv_ell.hip).  refused: the sweep whose symmetry check the values of this
// bind have just failed -- the next choice; *direct: the patch sweep's copy of the swept planes is filled straight from the CSR values.
DiaKernel mfem_dia_kernel_wanted(const mfem_csr_s* A, DiaKernel refused = DIA_NONE, bool* direct = nullptr);
// spmv_dia.hip: inspection; the copies of a bind (pvals: the swept planes G straight to the patch-major copy); all rows / the rows outside [lo, hi)
int mfem_dia_plan(mfem_context_s* ctx, mfem_csr_s* A);
int mfem_dia_copy(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc, const double* ssym, const SympGeom& G,
                  double* pvals, double* rim, bool want_fp, bool* fp_made, unsigned char* sflags = nullptr, bool* flags_made = nullptr);  // rim: the compact copy of G's rim rows (nullptr: none wanted); sflags: the step flags of the constant form (made by k_symp_fill alone)
int mfem_dia_launch(mfem_context_s* ctx, mfem_csr_s* A, bool triples, int cap, const SpmvArgs& a);
int mfem_dia_launch_outside(mfem_context_s* ctx, mfem_csr_s* A, const SpmvArgs& a, double* partials, int64_t lo, int64_t hi, int* ngrid);
// spmv_sym.hip: the two sweeps k = DIA_SYM27, DIA_SYMP -- structure, size rule, geometry, accounting, the symmetry verdict of a bind, the product
void mfem_sym_plan(mfem_csr_s* A, const int32_t* off, int lc, int64_t m2, int64_t PL, int64_t run_lo, int64_t run_hi);
bool mfem_sym_wanted(const mfem_csr_s* A, DiaKernel k);
SympGeom mfem_symp_geom(const mfem_context_s* ctx, const mfem_csr_s* A);
int64_t mfem_symp_steps(const mfem_csr_s* A, int B = 0, int trim = -1);  // patch steps of the swept planes with B bands per patch (0: mfem_symp_bands), trimmed or not (-1: mfem_symp_trim)
int mfem_symp_bands_wanted(const mfem_csr_s* A);  // the band count a bind of the patch sweep would take now
int mfem_symp_bands(const mfem_csr_s* A);         // the bound copy's band count; unbound: what a bind would take
// THE decision whether the patch sweep of a bind covers whole patches only (symp_trim_decide.h), and the bound copy's answer (unbound: what a bind would take)
int mfem_symp_trim_wanted(const mfem_csr_s* A);
int mfem_symp_trim(const mfem_csr_s* A);
int64_t mfem_symp_copy_doubles(const mfem_csr_s* A, int B, int trim);  // doubles of the patch-major copy, the rim copy behind it (stored form: the larger one) and the step flags of the constant form behind that
int64_t mfem_symp_swept_rows(const mfem_csr_s* A);                     // rows the patches cover (bound copy's geometry; unbound: what a bind would take)
// THE decision which form the main part of a patch-major copy gets (spmv_symp.h): 1 = the diagonal as one-byte ulp codes -- only where the copy is
// filled by k_symp_fill (`fast`: mfem_dia_fill_fast) with the symmetric scaling, whose diagonal is a_ii * (t_i * t_i) = 1.0 up to a few roundings
int mfem_symp_coded_wanted(DiaKernel k, bool fast, const double* ssym);
int mfem_symp_coded(const mfem_csr_s* A);         // the bound copy's form; unbound: the last patch-sweep bind's (0 before any)
bool mfem_dia_fill_fast(const mfem_csr_s* A, const double* dsc, bool direct);  // spmv_dia.hip: would k_symp_fill fill the swept rows of a bind?
int64_t mfem_sym_entries(const mfem_context_s* ctx, const mfem_csr_s* A, DiaKernel k);
int mfem_sym_verdict(mfem_context_s* ctx, mfem_csr_s* A, DiaKernel k, const double* buf, double* pvals, const SympGeom& G, bool direct, bool fp_made, bool* ok,
                     bool* dc_refused, int* dneg, bool flags_made = false, SympConst* cst = nullptr, int64_t* flagged = nullptr);
// the step flags' place in the layout's buffer: behind the patch-major copy and the rim copy of geometry G (spmv_sym.hip)
unsigned char* mfem_symp_flags_of(double* pvals, const SympGeom& G);
// THE schedule of a bound constant form's runs (symp_sched_decide.h): built from the step flags and placed behind them; A->symp_sched null where none applies
int mfem_symp_sched_bind(mfem_context_s* ctx, mfem_csr_s* A, const SympGeom& G);
int mfem_sym_launch(mfem_context_s* ctx, mfem_csr_s* A, DiaKernel k, const SpmvArgs& a);
