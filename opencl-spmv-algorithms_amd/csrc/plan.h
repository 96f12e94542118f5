// plan.h — struct spmv_plan, private to the library: built and run by
// plan.hip, which also holds the balanced multi-vector mode
// (spmv_plan_prepare_multi); extended with the transposed product y = A^T x by
// transpose.hip and with the symmetric product by symmetric.hip.  Each of the
// three modes keeps what its prepare built in one state struct, freed by
// "free the pointers, destroy the inner plan, assign a fresh struct", and
// counts its bytes in that struct's `owned`, never in the plan's.
#pragma once

#include <stdio.h>

#include "common.h"

namespace spmv {
// What spmv_plan_prepare_transpose built (transpose.hip).  The old mode is
// freed before the new one is built (peak memory: one mode), so a failed
// prepare leaves SPMV_T_NONE.
struct TransposeState {
    int32_t mode = 0;         // enum spmv_transpose_mode
    int32_t xcap = 0;         // scatter: LDS accumulator entries of a run (widest window that fits the cap)
    int64_t blocks = 0, lds_blocks = 0, flush = 0;
    // scatter, multi-vector run (csr_t_multi_kernel of width 1, 2, 4, 8): the
    // widest column span that fits the width's cap, and the blocks that fit
    int32_t mxcap[4] = {0, 0, 0, 0};
    int64_t mlds[4] = {0, 0, 0, 0};
    void *win = nullptr;      // scatter: int2 {lo, hi} column range per row block
    int64_t *ptr = nullptr;   // copy: A^T as CSR (ptr[n_cols+1], col/val[nnz])
    int32_t *col = nullptr;
    double *val = nullptr;
    spmv_plan *inner = nullptr;  // copy: the forward CSR plan over A^T
    size_t owned = 0;
};

// What spmv_plan_prepare_multi built (plan.hip): built aside and swapped in
// on success, so a failed prepare leaves the plan as it was.
struct MultiState {
    int32_t mode = 0;                // enum spmv_multi_mode
    spmv_multi_opts req = {-1, -1};  // the options as asked for (-1: the rule)
    int32_t seg_len = 0;             // resolved; the resolved long_len is bal.long_len
    int64_t long_entries = 0;
    MultiBalance bal;                // counts, device tables, partial workspace (plan-owned)
    size_t owned = 0;
};

// What spmv_plan_prepare_symmetric built (symmetric.hip).  A new mode is
// built into a fresh SymState and swapped in on success, so a failed prepare
// leaves the plan as it was.
struct SymState {
    int32_t mode = 0;         // enum spmv_symmetric_mode
    int32_t xcap = 0;         // fused: widest union window that fits the cap
    int64_t blocks = 0, win_blocks = 0, flush = 0;
    // fused, multi-vector run (csr_sym_multi_kernel of width 1, 2, 4, 8): the
    // widest union that fits the width's cap, the blocks that fit and the Y
    // rows the flushes address per pass
    int32_t mxcap[4] = {0, 0, 0, 0};
    int64_t mwin[4] = {0, 0, 0, 0}, mflush[4] = {0, 0, 0, 0};
    void *win = nullptr;      // fused: int2 {lo, hi} union window per row block
    int64_t nnz_a = 0;        // expand: entries of A = S + S^T - diag S
    int64_t *ptr = nullptr;   // expand: A as CSR (ptr[n+1], col/val[nnz_a])
    int32_t *col = nullptr;
    double *val = nullptr;
    spmv_plan *inner = nullptr;  // expand: the forward CSR plan over A
    size_t owned = 0;
};
}  // namespace spmv

struct spmv_plan {
    int fmt;  // SPMV_FMT_*
    int path; // PlanPath (plan.hip)
    spmv_dims d;
    spmv_plan_opts o;
    // the caller's arrays (device)
    const int64_t *ptr = nullptr;  // CSR row_ptr / SELL slice_ptr / CMRS strip_ptr
    const int32_t *row = nullptr, *col = nullptr, *perm = nullptr;
    const uint8_t *rin = nullptr;
    const double *val = nullptr;
    // geometry
    int32_t K = 0, C = 0, sigma = 0, ki = 0, h = 0, lanes = 0, variant = 0, xwin_rows = 0;
    int64_t ld = 0, n_slices = 0, n_strips = 0;
    int32_t bsr_b = 0;    // BSR: the block size (ptr = brow_ptr, col = bcol, val = bval)
    int64_t n_brows = 0;  // BSR: block rows
    // owned by the plan (device)
    void *win = nullptr;
    int32_t xcap = 0;
    void *head = nullptr;
    size_t head_bytes = 0;
    void *tails = nullptr;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    int32_t *own_lo = nullptr;
    int32_t *big = nullptr;
    int64_t big_len = 0, big_tiles = 0, big_tile = 0;
    int32_t split_T = 0;
    bool tiles_planned = false;  // tiled CMRS: the tile -> first-strip table filled at build
    int64_t n_chunks = 0;
    int32_t *chunk_slice = nullptr, *chunk_k0 = nullptr;
    uint16_t *col16 = nullptr;  // SELL16: offsets from each workgroup's window base
    uint16_t *cwin16 = nullptr;  // CSR x windows: col[e] - (the base of e's window), or NULL
    int32_t *hcol = nullptr;  // the columns with hot ids (plan-owned), or NULL
    int32_t *hot = nullptr;   // hot[H]: the hot columns in rank order
    int64_t H = 0;
    size_t owned = 0;
    char kernel[64] = "";
    char desc[320] = "";
    spmv::TransposeState t;  // the transposed product (spmv_plan_prepare_transpose)
    spmv::MultiState m;      // the balanced multi-vector mode (spmv_plan_prepare_multi)
    spmv::SymState sym;      // the symmetric product (spmv_plan_prepare_symmetric)
};

namespace spmv {
// frees what spmv_plan_prepare_multi built on this plan (the plan's device is current)
void plan_multi_free(spmv_plan *p);
// frees what spmv_plan_prepare_transpose built (the plan's device is current)
void plan_transpose_free(spmv_plan *p);
// frees what spmv_plan_prepare_symmetric built (the plan's device is current)
void plan_symmetric_free(spmv_plan *p);

// ---- the lifecycle vocabulary of the plans and their three modes (plan.hip)
// One counted device allocation: hipMalloc of `bytes` (16 at the least) into
// *dst, `bytes` added to *owned; `who` = the entry point, for the message.
int owned_alloc(void **dst, size_t bytes, size_t *owned, const char *who);

// A step failed with rc: runs `cleanup`, which may overwrite the last error,
// and returns rc with the step's own message.
template <typename F>
int fail_after(int rc, F &&cleanup)
{
    char keep[512];
    snprintf(keep, sizeof keep, "%s", spmv_last_error());
    cleanup();
    return fail_msg(rc, keep);
}

// A TransposeState or SymState: the device arrays freed, the inner plan
// destroyed, a fresh struct assigned.
template <typename S>
void mode_state_free(S *s)
{
    if (s->inner)
        spmv_plan_destroy(s->inner);
    for (void *q : {s->win, (void *)s->ptr, (void *)s->col, (void *)s->val})
        if (q)
            (void)hipFree(q);
    *s = S{};
}

// The blocks of a downloaded {lo, hi} table (windows_download) that have
// entries and span at most `cap` columns: their number, the sum of their spans
// and the widest of them.
struct WindowTally {
    int64_t blocks = 0, spans = 0;
    int32_t widest = 0;
};
WindowTally windows_tally(const int2 *h, int64_t n, int32_t cap);

// Y[i*ldy + j] = 0.0 for i < n, j < k on `st`, the first step of the scattering
// multi-vector runs (transpose.hip): a memset when ldy == k, else a kernel that
// leaves the gaps alone.  `who` = the entry point, for the message.
int zero_cols(int64_t n, int32_t k, double *Y, int64_t ldy, hipStream_t st, const char *who);
}  // namespace spmv
