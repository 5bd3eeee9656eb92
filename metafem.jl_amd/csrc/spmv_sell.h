// What the two forms of solver layout mode 3 share: spmv_sell.hip (row-sorted; the entry points of layouts.h, the knob word, the sort) and
// spmv_bsell.hip (node-blocked).  The decisions and the record of a plan: sell_decide.h.  Nothing here joins the library's dynamic symbols.
#pragma once
#include <functional>

#include "layouts.h"

#define MFEM_SELL_LOCAL __attribute__((visibility("hidden")))

extern std::atomic<int64_t> g_layout_min_rows_cols;  // spmv_ell.hip
MFEM_SELL_LOCAL SellKnobs mfem_sell_knobs();         // what mfem_debug_set_sell last set (spmv_sell.hip)
static inline SellShape mfem_sell_shape(const mfem_csr_s* A) {
  return {A->n, A->ncols, A->nnz, A->max_row_nnz, A->lat_m1, A->lat_m2, A->lat_fields, g_layout_min_rows_cols.load()};
}

// The buffers of a plan's sort: (keys, ids) are sorted into (keys2, sorted); sizes and ptr have a slot per block and one more.
template <typename Key> struct MFEM_SELL_LOCAL SellSortBufs {
  DevBuf<Key> keys, keys2;
  DevBuf<int32_t> ids, sorted;
  DevBuf<int64_t> sizes, ptr;
  int alloc(int64_t count, int64_t nblk) {
    MFEM_CHECK_HIP(keys.alloc((size_t)count));
    MFEM_CHECK_HIP(keys2.alloc((size_t)count));
    MFEM_CHECK_HIP(ids.alloc((size_t)count));
    MFEM_CHECK_HIP(sorted.alloc((size_t)count));
    MFEM_CHECK_HIP(sizes.alloc((size_t)(nblk + 1)));
    MFEM_CHECK_HIP(ptr.alloc((size_t)(nblk + 1)));
    return MFEM_OK;
  }
};
// Stable radix sort of `count` (keys, ids) by the low `bits` key bits (equal keys keep their mesh order); then block_sizes(sorted, sizes) launches
// the kernel that writes the entries of each of the nblk blocks, ptr becomes their exclusive sum and *total = ptr[nblk].  One scratch allocation
// (the larger of sort and scan), one stream synchronisation, at the end.  Key = uint64_t (rows) and uint32_t (nodes): spmv_sell.hip.
using SellBlockSizes = std::function<void(const int32_t* sorted, int64_t* sizes)>;
template <typename Key>
MFEM_SELL_LOCAL int mfem_sell_sort_blocks(mfem_context_s* ctx, SellSortBufs<Key>& B, int64_t count, int bits, int64_t nblk, const SellBlockSizes& block_sizes,
                                          int64_t* total);

// The node-blocked form (spmv_bsell.hip).  The plan fills *L (form SELL_NODE_BLOCKED) if the pattern has the form and its padding is accepted,
// and leaves it alone otherwise; bind and launch are for a handle whose sell.form is SELL_NODE_BLOCKED.
MFEM_SELL_LOCAL int mfem_bsell_plan(mfem_context_s* ctx, mfem_csr_s* A, const SellShape& S, SellLayout* L);
MFEM_SELL_LOCAL int mfem_bsell_fill(mfem_context_s* ctx, mfem_csr_s* A, const double* vals, double* buf, const double* dsc);
MFEM_SELL_LOCAL int mfem_bsell_launch(mfem_context_s* ctx, mfem_csr_s* A, const double* x, double* y, double alpha, double beta, const double* dotw,
                                      double* partials, int* n_partials, const int32_t* done_flag, int part);
