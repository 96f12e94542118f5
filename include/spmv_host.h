/*
 * spmv_host.h — host side of the MI355X SpMV suite (libspmv_host.so).
 *
 * Replaces the reference's host layers L1-L3:
 *   - Matrix Market reading with the reference's acceptance semantics
 *     (reference inc/helper_functions.h:134-165, mmio/mmio.c:96-217,
 *      entry lines "%d %d %lg", csr.c:81);
 *   - the per-format builders that the reference interleaves with fscanf
 *     (reference coo.c:79-84, csr.c:68-91, ell.c:68-164,
 *      sigma_c.c:71-202, cmrs.c:72-117), re-designed for wave64 layouts
 *     and without the reference's empty-row / last-row assumptions;
 *   - the OpenMP CPU loops (reference coo.c:280-300, csr.c:285-309,
 *     ell.c:357-383, cmrs.c:319-345; the reference has none for SELL);
 *   - the run-time result check (reference inc/helper_functions.h:184-236);
 *   - synthetic generators for the configs in BASELINE.json.
 *
 * All functions take caller-allocated arrays ("plan" functions return the
 * sizes to allocate) so the same calls serve the C drivers and ctypes.
 * Return values are spmv_rc.h codes unless stated otherwise.
 */
#ifndef SPMV_HOST_H
#define SPMV_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "spmv_rc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------ Matrix Market ---*/
typedef struct spmv_mtx_info {
    int64_t n_rows;
    int64_t n_cols;
    int64_t nnz;   /* entries listed in the file (= entries multiplied)   */
    int symmetric; /* symmetric / skew / hermitian banner: entries are    */
                   /* taken literally, never mirrored (reference A12)     */
    int pattern;   /* pattern banner: every entry's value is 1.0          */
    int integer;   /* integer banner: values parsed as numbers            */
} spmv_mtx_info;

/* Banner + size line only.  SPMV_FILE_ERROR if the file is missing, the
 * banner is malformed, or the matrix is complex or dense (array).       */
int spmv_mtx_read_info(const char *path, spmv_mtx_info *info);
/* Banner + size + exactly info->nnz entries in FILE ORDER, converted to
 * 0-based.  row/col/val must hold info->nnz elements (read_info first).
 * Out-of-range indices or a short file give SPMV_FILE_ERROR.            */
int spmv_mtx_read(const char *path, spmv_mtx_info *info, int32_t *row,
                  int32_t *col, double *val);
/* Writes a coordinate real file with %.17g values (exact round trip).   */
int spmv_mtx_write(const char *path, int64_t n_rows, int64_t n_cols,
                   int64_t nnz, const int32_t *row, const int32_t *col,
                   const double *val, int symmetric);

/* Binary cache of a parsed file: header + row, col,
 * val arrays in file order.  The drivers' --cache option keeps PATH.bin
 * next to PATH and reads it instead of the text when it is newer.       */
int spmv_bin_write(const char *path, const spmv_mtx_info *info,
                   const int32_t *row, const int32_t *col, const double *val);
int spmv_bin_read_info(const char *path, spmv_mtx_info *info);
int spmv_bin_read(const char *path, spmv_mtx_info *info, int32_t *row,
                  int32_t *col, double *val);

/* ------------------------------------------------------------ formats ---*/
/* COO sorted by row, stable (file order kept inside a row).             */
int spmv_coo_sort_by_row(int64_t n_rows, int64_t nnz, const int32_t *row,
                         const int32_t *col, const double *val,
                         int32_t *row_out, int32_t *col_out, double *val_out);
/* CSR from COO in any order: stable counting sort by row; empty rows ok.
 * row_ptr[n_rows+1], col_out[nnz], val_out[nnz].                        */
int spmv_csr_from_coo(int64_t n_rows, int64_t nnz, const int32_t *row,
                      const int32_t *col, const double *val,
                      int64_t *row_ptr, int32_t *col_out, double *val_out);
/* A^T as CSR from the CSR of an n_rows x n_cols matrix (row_ptr[0] = 0):
 * stable counting sort by column.  t_ptr[n_cols+1], t_col[nnz] (row ids of
 * A), t_val[nnz]; inside a row of A^T the entries keep their position in A's
 * CSR (increasing row of A, duplicates in their CSR order) — element for
 * element the device builder spmv_dev_csr_transpose (spmv_ext.h).
 * SPMV_OTHER_ERROR for negative sizes, n_rows > INT32_MAX, a column outside
 * [0, n_cols) or a NULL array that would be read or written.             */
int spmv_csr_transpose(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr,
                       const int32_t *col, const double *val,
                       int64_t *t_ptr, int32_t *t_col, double *t_val);
/* The matrix a half-stored symmetric COO describes, A = S + S^T - diag(S), for
 * a square n x n S of any pattern (lower, upper or mixed): every off-diagonal
 * entry (i, j, v) also stands for (j, i, v), diagonal entries count once,
 * duplicates and entries stored on both sides each count as listed (the
 * Matrix Market expansion).  Skew-symmetric and hermitian meanings are not
 * covered: spmv_mtx_info.symmetric does not tell the banners apart.
 * Output: the nnz input entries in input order, then (col, row, val) of every
 * off-diagonal input entry in input order; *nnz_out = their count.  With
 * row_out == NULL only the count is written.  spmv_csr_from_coo of the output
 * (stable) defines the expanded CSR, element for element what
 * spmv_plan_prepare_symmetric(SPMV_S_EXPAND) builds on the device (spmv.h).
 * SPMV_OTHER_ERROR for negative sizes, an index outside [0, n) or a NULL
 * array that would be read or written.                                     */
int spmv_coo_symmetrize(int64_t n, int64_t nnz, const int32_t *row, const int32_t *col,
                        const double *val, int64_t *nnz_out, int32_t *row_out,
                        int32_t *col_out, double *val_out);
/* Entries of every CSR row reordered by increasing column (stable).  With
 * degree-relabelled columns (spmv_column_relabel) a long row then reads x
 * from its dense hot prefix in address order.  Changes each row's
 * summation order (not the products): y within the parity rule.          */
int spmv_csr_sort_rows(int64_t n_rows, const int64_t *row_ptr, int32_t *col, double *val);
/* Row-length statistics of a CSR matrix. */
int spmv_csr_row_stats(int64_t n_rows, const int64_t *row_ptr,
                       int64_t *min_len, int64_t *max_len, double *mean_len);
/* CSR kernel variant for this matrix (include/spmv.h): 4 = entry-balanced
 * tiled (spmv_csr_run_tiled) when the longest row exceeds both 4,096
 * entries and 64x the mean (a row-per-group kernel would then wait on one
 * group), else 0 (the library's row-group default).                    */
int spmv_csr_pick_variant(int64_t n_rows, const int64_t *row_ptr);
/* The rule itself, from the longest row (max_len) and the entry count:
 * shared with the CSR plan of spmv.h, which finds max_len on the device. */
int spmv_csr_variant_rule(int64_t n_rows, int64_t nnz, int64_t max_len);

/* Hot columns for spmv_csr_run_tiled_hot: the H most frequent columns in
 * decreasing count (ties: lower column first) into hot[], and col_out
 * (may alias col) = col with every hot column c renumbered n_cols +
 * rank(c).  H_req > 0 takes min(H_req, non-empty columns); H_req = 0 is
 * the rule: 2^19 columns (4 MiB of x, one XCD's L2; halved down to 2^16
 * while above nnz / 32) when n_cols > 2^21,
 * they hold at least half of the entries and at least 8 entries each on
 * average (the table fill re-reads each once), else none (col_out = col).
 * hot[] holds max(H_req, 2^19) entries.  Returns H, -1 on bad input.    */
int64_t spmv_hot_columns(int64_t n_cols, int64_t nnz, const int32_t *col, int64_t H_req, int32_t *hot,
                         int32_t *col_out);
/* 0 when spmv_hot_columns(n_cols, ..., H_req, ...) returns 0 whatever the
 * columns (the rule never tables a matrix of <= 2^21 columns): lets a
 * caller skip fetching the columns.                                      */
int spmv_hot_columns_possible(int64_t n_cols, int64_t H_req);

/* Big-tile plan of the entry-balanced CSR (spmv_csr_run_tiled_plan):
 * with tiles of `tile` entries (spmv_csr_tiled_tile), every tile owning
 * more than `cap` rows (the rows whose first offset lies in it; the last
 * tile also the trailing rows) and at most 65,536 gets the list of its
 * owned rows that have entries in it, as int32 pairs {row - first owned
 * row, a | b << 16} with [a, b) relative to the tile start.  Layout
 * (int32): idx[tiles] (-1 or the big tile's number k), start[nbig + 1]
 * (absolute, even positions), then the pairs.  plan = NULL returns the
 * length only.  Returns the int32 length, -1 on bad input.                */
int64_t spmv_csr_tiled_bigplan(int64_t n_rows, const int64_t *row_ptr, int64_t tile, int32_t cap,
                               int32_t *plan);

/* Long-row plan of the balanced multi-vector CSR run
 * (spmv_plan_prepare_multi, spmv.h).  A row is long when it holds more than
 * long_len entries; every long row, in increasing row order, is cut into
 * segments of seg_len consecutive entries (the row's last segment holds the
 * rest, 1..seg_len).  Segment s covers entries [seg_beg[s], seg_beg[s] +
 * seg_cnt[s]).  A row of one segment has seg_dest[s] = the row (its sums go
 * straight to Y); a row of more segments takes consecutive partial slots in
 * segment order and seg_dest[s] = ~slot.  long_row[i] / long_first[i], i <
 * n_long, are the long rows and the first slot of each; the slots of row i
 * are [long_first[i], long_first[i+1]) (none for a row of one segment), and
 * the closing entry i = n_long holds row -1 and n_slots.
 * Two calls: with the five arrays NULL only the counts are written; then
 * seg_beg[n_seg] (int64), seg_cnt / seg_dest[n_seg], long_row /
 * long_first[n_long + 1] (int32).  SPMV_OTHER_ERROR with nothing written:
 * n_rows < 0, NULL row_ptr or count pointer, decreasing row_ptr, long_len <
 * 0, seg_len < 1, some but not all arrays NULL, a long row past INT32_MAX,
 * more than INT32_MAX segments.                                          */
int spmv_csr_multi_plan(int64_t n_rows, const int64_t *row_ptr, int32_t long_len, int32_t seg_len, int64_t *n_long,
                        int64_t *n_seg, int64_t *n_slots, int64_t *seg_beg, int32_t *seg_cnt, int32_t *seg_dest,
                        int32_t *long_row, int32_t *long_first);

/* Degree-ordered column relabel (power-law columns, x replicated): the
 * columns ranked by decreasing entry count (ties: lower column first;
 * columns without entries last, in id order).  order[rank] = column,
 * newid[column] = rank, and col_out (may alias col) = newid[col].  The
 * relabelled matrix A' = A·Pᵀ takes x' = P·x (x'[k] = x[order[k]]) and
 * gives the same y in the same row order, bit for bit with any kernel
 * whose per-row summation order does not depend on column ids: the hot
 * columns are x'[0..H) (no per-run hot-table fill) and the touched part of
 * x is one dense prefix.  Returns the number of non-empty columns, -1 on
 * bad input.                                                             */
int64_t spmv_column_relabel(int64_t n_cols, int64_t nnz, const int32_t *col, int32_t *order, int32_t *newid,
                            int32_t *col_out);
/* The same with a choice of tie order among equal counts: ties = 0 lower
 * column first (spmv_column_relabel), 1 first appearance in col (for a
 * row-major CSR col: the first row that uses the column, so the low-degree
 * columns of neighbouring rows share x' lines).  -1 on bad input.        */
int64_t spmv_column_relabel_ex(int64_t n_cols, int64_t nnz, const int32_t *col, int32_t *order, int32_t *newid,
                               int32_t *col_out, int32_t ties);

/* ELL, column-major with leading dimension ld = round_up(N, 64) and
 * k-interleave ki (spmv.h).  K = round_up(max row length, ki).
 * spmv_ell_plan gives K and ld; arrays are ld*K elements.               */
int spmv_ell_plan(int64_t n_rows, const int64_t *row_ptr, int32_t ki,
                  int32_t *K, int64_t *ld);
int spmv_ell_fill(int64_t n_rows, const int64_t *row_ptr, const int32_t *col,
                  const double *val, int32_t K, int64_t ld, int32_t ki,
                  int32_t *col_out, double *val_out);

/* SELL-C-sigma: rows sorted by decreasing length inside windows of sigma
 * rows (sigma = 1: no sorting, the reference's sigma_c.c:48 behaviour;
 * sigma must be 1 or a multiple of C), slices of C rows, slice width =
 * round_up(longest row of the slice, ki).  Plan returns n_slices and the
 * stored element count; perm has n_slices*C entries.                    */
int spmv_sell_plan(int64_t n_rows, const int64_t *row_ptr, int32_t C,
                   int32_t sigma, int32_t ki, int64_t *n_slices,
                   int64_t *stored);
int spmv_sell_fill(int64_t n_rows, const int64_t *row_ptr, const int32_t *col,
                   const double *val, int32_t C, int32_t sigma, int32_t ki,
                   int64_t n_slices, int64_t *slice_ptr, int32_t *perm,
                   int32_t *col_out, double *val_out);

/* CMRS: strips of h rows (1..64), n_strips = ceil(N/h).  The CSR arrays
 * are reused unchanged; this builds strip_ptr[n_strips+1] and
 * row_in_strip[nnz].                                                    */
int spmv_cmrs_build(int64_t n_rows, const int64_t *row_ptr, int32_t h,
                    int64_t *strip_ptr, uint8_t *row_in_strip);
/* 1 = entry-balanced (spmv_cmrs_run_tiled) when the longest strip exceeds
 * both 4,096 entries and 64x the mean strip, else 0 (spmv_cmrs_run).    */
int spmv_cmrs_pick_variant(int64_t n_strips, const int64_t *strip_ptr);
/* The rule from the longest strip and the entry count (the CMRS plan).  */
int spmv_cmrs_variant_rule(int64_t n_strips, int64_t nnz, int64_t max_len);

/* SELL split plan for wide slices (spmv_sell_run_split).  _auto gives T
 * (slot columns kept by the main kernel, a multiple of ki) or 0 when no
 * slice is wider than both 1,024 and 16x the mean width.  _plan lists the
 * chunks [k0, k0+T) beyond the first T columns of every slice (T = 256), in slice
 * order, and returns their count (arrays may be NULL: count only); -1 on
 * bad arguments.                                                        */
int32_t spmv_sell_split_auto(int64_t n_slices, const int64_t *slice_ptr, int32_t C, int32_t ki);
int64_t spmv_sell_split_plan(int64_t n_slices, const int64_t *slice_ptr, int32_t C, int32_t T,
                             int32_t *chunk_slice, int32_t *chunk_k0);

/* HYB = ELL + COO tail: the first K entries of every
 * row in the column-major ELL layout of spmv_ell_fill (ld, ki), the rest
 * as a row-sorted COO tail.  K_req > 0 forces K (rounded up to ki); 0
 * picks the K that minimises stored bytes (12 per ELL slot, 16 per tail
 * entry) plus 32 MB when both parts are non-empty (the second kernel's
 * fixed cost): K = 0 (all tail) or the longest row (no tail) where the
 * split does not save more.  Fill: ell_col/ell_val[K*ld],
 * tail_row/col/val[tail_nnz].                                            */
int spmv_hyb_plan(int64_t n_rows, const int64_t *row_ptr, int32_t ki, int32_t K_req, int32_t *K,
                  int64_t *ld, int64_t *tail_nnz);
int spmv_hyb_fill(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                  int32_t K, int64_t ld, int32_t ki, int32_t *ell_col, double *ell_val,
                  int32_t *tail_row, int32_t *tail_col, double *tail_val);

/* CSR with compressed 16-bit column indices: the
 * CSR entries are cut into 64-entry blocks (entry p in block p/64).  A
 * block whose columns span < 65536 stores blk_base = its smallest column
 * and col_off[p] = col[p] - blk_base; any other block stores its columns
 * whole in col_esc[slot*64 .. +64) and blk_base = -1 - slot.  row_ptr and
 * val are CSR's.  Plan: n_blocks = ceil(nnz/64), n_esc escaped blocks.
 * Fill: blk_base[n_blocks], col_off[nnz], col_esc[n_esc*64].            */
int spmv_csr16_plan(int64_t nnz, const int32_t *col, int64_t *n_blocks, int64_t *n_esc);
int spmv_csr16_fill(int64_t nnz, const int32_t *col, int32_t *blk_base, uint16_t *col_off,
                    int32_t *col_esc);

/* Column-grouped CSR (CSRG) for gather-bound power-law matrices (R-MAT,
 * BASELINE.json configs[3]).  x is cut into `groups` (1..64) groups of
 * whole 128-byte lines (16 columns): the line c/16 belongs to group
 * spmv_csrg_group(c, groups), a hash, so hot and cold lines spread evenly.
 * The entries are stored group after group; inside a group, as a CSR over
 * the PAIRS (row, group) that hold entries, rows ascending, each pair's
 * entries in CSR order.  A run sums every pair (the groups one after
 * another, so the x lines being gathered stay in the L2s) and then adds
 * each row's pair sums in group order, block by block of
 * SPMV_CSRG_ROWS rows: blk_off[g*(nb+1) + b] is the first pair of group g
 * whose row is >= b*SPMV_CSRG_ROWS (nb = ceil(n_rows / SPMV_CSRG_ROWS)),
 * pair_row[p] the pair's row modulo SPMV_CSRG_ROWS.  Plan: n_pairs.
 * Fill: pair_ptr[n_pairs+1], col_g/val_g[nnz], blk_off[groups*(nb+1)],
 * pair_row[n_pairs].                                                    */
/* fixed (no -D override): the host fill, the device reduce and the Python
 * binding (spmv_csrg_block_rows) must agree on it */
#define SPMV_CSRG_ROWS 4096 /* also in spmv.h */
int32_t spmv_csrg_block_rows(void); /* SPMV_CSRG_ROWS as built into libspmv_host */
int32_t spmv_csrg_group(int32_t col, int32_t groups);
int spmv_csrg_plan(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, int32_t groups,
                   int64_t *n_pairs);
int spmv_csrg_fill(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                   int32_t groups, int64_t *pair_ptr, int32_t *col_g, double *val_g,
                   int32_t *blk_off, uint16_t *pair_row);

/* ----------------------------------------------------- multi-GPU shard ---
 * Row-range partition for one process per GPU: `parts`
 * contiguous ranges [bounds[p], bounds[p+1]) holding about nnz/parts
 * entries each; every inner boundary is a multiple of `align` (use the
 * SELL sigma, 1024, so sorting windows never straddle two GPUs).
 * bounds has parts+1 entries, bounds[0] = 0, bounds[parts] = n_rows.    */
int spmv_partition_rows(int64_t n_rows, const int64_t *row_ptr, int parts,
                        int64_t align, int64_t *bounds);
/* The entries of rows [lo, hi) in FILE ORDER with rows renumbered to the
 * shard (row - lo), for a device that owns those rows; returns the count
 * (output arrays NULL: count only), -1 on bad arguments.  Every entry
 * lands in exactly one shard of a partition, so the shards' y slices,
 * written at y + lo, reassemble y.                                      */
int64_t spmv_coo_row_shard(int64_t nnz, const int32_t *row, const int32_t *col, const double *val,
                           int64_t lo, int64_t hi, int32_t *row_out, int32_t *col_out, double *val_out);
/* Same cut, balancing entries + row_weight per row (a row costs the
 * kernels about as much as row_weight entries: its offset, its y store and
 * its reduction; 0 = spmv_partition_rows).                              */
int spmv_partition_rows_weighted(int64_t n_rows, const int64_t *row_ptr, int parts, int64_t align,
                                 double row_weight, int64_t *bounds);
/* Profile-guided re-cut: old_bounds (old_parts + 1) with the measured time
 * of each old shard (old_ms) give every row the cost rate_g * (entries +
 * row_weight) of the old shard g holding it (rate_g = ms_g / that shard's
 * entries + row_weight * rows); the new `parts` ranges hold equal shares
 * of that cost, aligned as spmv_partition_rows.  For shards whose cost per
 * entry differs (R-MAT hub shards against shards of short rows).         */
int spmv_partition_rows_calibrated(int64_t n_rows, const int64_t *row_ptr, int parts, int64_t align,
                                   double row_weight, int old_parts, const int64_t *old_bounds,
                                   const double *old_ms, int64_t *bounds);

/* ------------------------------------------------------ block CSR (BSR) ---
 * One int32 column per b x b block instead of one per entry, for matrices
 * with b unknowns per node (3-dof FEM).  The layout is scipy's
 * bsr_matrix.data[blk, r, c] and rocSPARSE's row-major one:
 *   brow_ptr[n_brows + 1]  int64, n_brows = ceil(n_rows / b)
 *   bcol[n_blocks]         int32, strictly ascending inside a block row
 *   bval[n_blocks * b * b] double, bval[(blk*b + r)*b + c] = entry
 *                          (I*b + r, bcol[blk]*b + c) of block row I
 * The last block row and the last block column may be partial.  Slots outside
 * the matrix and slots without an entry hold +0.0.
 *
 * THE FILL-IN RULE, a real difference from CSR: a slot without an entry
 * multiplies 0.0 by an x value of its block column.  For finite x no result
 * changes.  A non-finite x[c] reaches every scalar row of every block row that
 * has a block in c's block column (0.0 * inf = NaN), and a row whose exact
 * result is -0.0 may come out +0.0.  Slots outside the matrix are never
 * multiplied: no x at or past n_cols is read.
 *
 * spmv_bsr_plan counts the blocks of a CSR matrix (columns in any order
 * inside a row, duplicates allowed); spmv_bsr_fill writes the three arrays,
 * duplicates of one (i, j) added into their slot in CSR order.  1 <= b <=
 * SPMV_BSR_MAX_B.  SPMV_OTHER_ERROR with nothing written: b out of range,
 * negative sizes, row_ptr not nondecreasing from a non-negative start, a
 * column outside [0, n_cols), n_cols > INT32_MAX - 8, or a NULL array that
 * would be read or written.                                               */
#define SPMV_BSR_MAX_B 8
int spmv_bsr_plan(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr, const int32_t *col, int32_t b,
                  int64_t *n_brows, int64_t *n_blocks);
int spmv_bsr_fill(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr, const int32_t *col, const double *val,
                  int32_t b, int64_t *brow_ptr, int32_t *bcol, double *bval);
/* y = A x from the BSR arrays: the plain serial loop, block after block in
 * storage order, the CPU statement of a BSR plan's run (spmv_plan_bsr,
 * spmv.h), never a device fallback.  Writes y[0 .. n_rows) only (rows of empty
 * block rows get 0.0) and reads x[0 .. n_cols) only: the partial last block
 * row and block column are cut, not hidden behind their stored 0.0.
 * SPMV_OTHER_ERROR, before y is touched: b out of range, negative sizes,
 * n_brows != ceil(n_rows / b), offsets not nondecreasing, a block column
 * outside [0, ceil(n_cols / b)), n_cols > INT32_MAX - 8, or a NULL array that
 * would be read or written.                                               */
int spmv_cpu_bsr(int64_t n_rows, int64_t n_cols, int32_t b, int64_t n_brows, const int64_t *brow_ptr,
                 const int32_t *bcol, const double *bval, const double *x, double *y);

/* ---------------------------------------------------------- CPU loops ---
 * OpenMP restatements of the reference's compute_using_cpu loops, with
 * zero-initialised output (the reference accumulated into malloc'd
 * memory, reference csr.c:102).  `threads` <= 0 uses omp_get_max_threads.
 * They are the CPU baseline the drivers print, never a device fallback. */
int spmv_cpu_coo(int64_t n_rows, int64_t nnz, const int32_t *row,
                 const int32_t *col, const double *val, const double *x,
                 double *y, int threads);
int spmv_cpu_csr(int64_t n_rows, const int64_t *row_ptr, const int32_t *col,
                 const double *val, const double *x, double *y, int threads);
/* Y = A X for k >= 1 vectors stored row-major, the layout of
 * spmv_plan_run_multi (spmv.h): X[c*ldx + j], Y[r*ldy + j], j < k,
 * ldx >= k, ldy >= k.  Writes Y[r*ldy + j] for j < k only and reads nothing
 * of X outside [c*ldx, c*ldx + k).  SPMV_OTHER_ERROR for k < 1, a leading
 * dimension below k or a NULL array that would be read or written.        */
int spmv_cpu_csr_multi(int64_t n_rows, const int64_t *row_ptr, const int32_t *col,
                       const double *val, int32_t k, const double *X, int64_t ldx,
                       double *Y, int64_t ldy);
/* y = A^T x (x[n_rows], y[n_cols]): zeroes y[0 .. n_cols), then scatters
 * val * x[row] row by row.  Serial and deterministic: the CPU statement of
 * spmv_plan_run_t (spmv.h), never a device fallback.  SPMV_OTHER_ERROR for
 * negative sizes, a column outside [0, n_cols) or a NULL array that would be
 * read or written (nothing of y past a bad entry's row is touched).       */
int spmv_cpu_csr_t(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr,
                   const int32_t *col, const double *val, const double *x, double *y);
/* y = (S + S^T - diag S) x on the half storage S (n x n CSR, any pattern;
 * spmv_coo_symmetrize has the definition): zeroes y[0 .. n), then one serial
 * pass in which entry (r, c, v) adds v x[c] to y[r] and, when c != r, v x[r]
 * to y[c].  The CPU statement of spmv_plan_run_sym (spmv.h) and the CPU
 * baseline of ./bin/csr --symmetric, never a device fallback.
 * SPMV_OTHER_ERROR for a negative size, a column outside [0, n) or a NULL
 * array that would be read or written.                                     */
int spmv_cpu_csr_sym(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val,
                     const double *x, double *y);
/* Y = (S + S^T - diag S) X for k >= 1 vectors stored row-major, the layout of
 * spmv_plan_run_sym_multi (spmv.h): X[c*ldx + j], Y[i*ldy + j], c, i < n,
 * j < k; ldx >= k, ldy >= k.  Serial, the k-vector form of spmv_cpu_csr_sym:
 * column j has that loop's bits on column j.  Writes nothing for j >= k or at
 * or past row n and reads nothing of X outside [c*ldx, c*ldx + k).  The CPU
 * statement of spmv_plan_run_sym_multi and the checker of
 * tools/spmvsym_bench.py --vectors, never a device fallback.
 * SPMV_OTHER_ERROR, before Y is touched, for a negative size, k < 1, a leading
 * dimension below k, a column outside [0, n) or a NULL array that would be
 * read or written.                                                          */
int spmv_cpu_csr_sym_multi(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val,
                           int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy);
/* Block-Jacobi preconditioner M = blockdiag(D_0, D_1, ...) of a square CSR
 * matrix (rows 0 .. n-1; the host statement of spmv_bjacobi_create,
 * spmv_ext.h).  1 <= bs <= 16, n_blocks = ceil(n / bs), block q covers rows
 * [q*bs, min(n, (q+1)*bs)).  D_q[r][c] is the sum, in storage order, of the
 * entries of row q*bs + r whose column equals col_base + q*bs + c (duplicates
 * add); col_base is where the rows' own columns start (a row shard in the
 * gathered layout of iterate.py: rank * pad; otherwise 0).  symmetric_half
 * != 0: the arrays hold the stored half S of a symmetric matrix and every
 * off-diagonal entry inside a block also counts at its mirrored place,
 * diagonal entries once (spmv_coo_symmetrize's meaning).  Entries outside a
 * row's own block are ignored, out-of-range columns included; a short last
 * block is completed with the identity.
 * inv[(q*bs + r)*bs + c] = D_q^-1 by Gauss-Jordan elimination with partial
 * pivoting (the first largest entry of the column), multiply-adds as fma().  A
 * block that meets a zero or non-finite pivot, or whose inverse has a
 * non-finite element, becomes the identity and is counted in
 * *singular_blocks (the identity keeps M positive definite).
 * SPMV_OTHER_ERROR, before anything is written, for a negative n or col_base,
 * bs outside 1..16 or a NULL array that would be read or written.          */
int spmv_bjacobi_build(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val,
                       int32_t bs, int64_t col_base, int32_t symmetric_half, double *inv,
                       int64_t *singular_blocks);
/* Z = M^-1 R for k >= 1 vectors stored row-major (R[i*ldr + j], Z[i*ldz + j],
 * i < n, j < k; ldr, ldz >= k) with inv from spmv_bjacobi_build: for row i of
 * block q, s = inv[i*bs] * R[(q*bs)*ldr + j], then for c = 1 .. bs-1 in order
 * s = fma(inv[i*bs + c], R[(q*bs + c)*ldr + j], s); in a short last block only
 * the columns that exist are read.  This fixes the bits of every element: the
 * CPU statement of spmv_bjacobi_apply_multi (spmv_ext.h).  R and Z must not
 * overlap.  SPMV_OTHER_ERROR, before Z is touched, for a negative n, bs outside
 * 1..16, k < 1, a leading dimension below k or a NULL array that would be read
 * or written.                                                                */
int spmv_cpu_bjacobi_apply_multi(int64_t n, int32_t bs, const double *inv, int32_t k,
                                 const double *R, int64_t ldr, double *Z, int64_t ldz);
/* One step of the Chebyshev recurrence for A z = r over B = M^-1 A, M the block
 * Jacobi preconditioner above (iterate.Chebyshev computes the scalars a, b from
 * the bounds of B's spectrum; AZ holds A Z of the current iterate).  For row i
 * of block q and column j < k:
 *   t_c = R[c][j] - AZ[c][j] over the rows c of the block (AZ == NULL, "step 0":
 *   t_c = R[c][j]); s = inv[i*bs] * t_0, then s = fma(inv[i*bs + c], t_c, s) in
 *   column order (spmv_cpu_bjacobi_apply_multi's chain, short last block
 *   included);
 *   step 0:    d = b * s;                     D[i][j] = d, Zout[i][j] = d
 *              (a, the old D and Zin are not read; Zin may be NULL);
 *   otherwise: d = fma(a, D[i][j], b * s);    D[i][j] = d,
 *              Zout[i][j] = Zin[i][j] + d.
 * This fixes the bits of every element: the CPU statement of
 * spmv_bjacobi_cheb_step_multi (spmv_ext.h).  Zout may be Zin itself (with the
 * same leading dimension); no other overlap is allowed.  Nothing is read
 * outside columns [0, k) of a row or at or past row n, nothing is written for
 * j >= k.  SPMV_OTHER_ERROR, before anything is written, for a negative n, bs
 * outside 1..16, k < 1, a leading dimension below k, a NULL array that would be
 * read or written, or Zout == Zin with two leading dimensions.              */
int spmv_cpu_bjacobi_cheb_step_multi(int64_t n, int32_t bs, const double *inv, int32_t k, double a,
                                     double b, const double *R, int64_t ldr, const double *AZ,
                                     int64_t ldaz, double *D, int64_t ldd, const double *Zin,
                                     int64_t ldzin, double *Zout, int64_t ldzout);
/* The two vector statements of a BiCGSTAB iteration (iterate.bicgstab_multi) on
 * row-major blocks of k >= 1 vectors (V[i*ld + j], i < n, j < k <= ld), with
 * HOST arrays of k scalars.  ratio(a, b) is a / b, and 0.0 when b == 0.0.
 * update: alpha_j = ratio(a_num[j], a_den[j]), omega_j = ratio(w_num[j], w_den[j]),
 *   X[i][j] = fma(omega_j, Sh[i][j], fma(alpha_j, Ph[i][j], X[i][j]))
 *   R[i][j] = fma(-omega_j, T[i][j], R[i][j])
 *   Sh may be R itself (same leading dimension): an element of Sh is read
 *   before that element of R is written.  No other overlap is allowed.
 * dir: beta_j = ratio(rho_new[j], rv[j]) * ratio(tt[j], ts[j]),
 *      omega_j = ratio(ts[j], tt[j]),
 *   P[i][j] = fma(beta_j, fma(-omega_j, V[i][j], P[i][j]), R[i][j])
 * These fix the bits of every element: the CPU statements of
 * spmv_bicgstab_update_dot_multi and spmv_bicgstab_dir_multi (spmv_ext.h; the
 * sums of the former are fixed by spmv_dot_multi).  Nothing is read or written
 * outside columns [0, k) of a row or at or past row n.  SPMV_OTHER_ERROR,
 * before anything is written, for a negative n, k < 1, a leading dimension
 * below k, a NULL array that would be read or written, or Sh == R with two
 * leading dimensions.                                                       */
int spmv_cpu_bicgstab_update_multi(int64_t n, int32_t k, const double *a_num, const double *a_den,
                                   const double *w_num, const double *w_den, const double *Ph,
                                   int64_t ldph, const double *Sh, int64_t ldsh, const double *T,
                                   int64_t ldt, double *X, int64_t ldx, double *R, int64_t ldr);
int spmv_cpu_bicgstab_dir_multi(int64_t n, int32_t k, const double *rho_new, const double *rv,
                                const double *tt, const double *ts, const double *V, int64_t ldv,
                                const double *R, int64_t ldr, double *P, int64_t ldp);
/* The block combine of the LOBPCG eigensolver (iterate.lobpcg) on row-major
 * blocks (V[i*ld + j], i < n, j < k <= ld): with S = [A0 A1 A2] side by side
 * (ka0 + ka1 + ka2 columns; ka = 0: the operand is absent and its pointer
 * ignored) and C a row-major (ka0 + ka1 + ka2) x kc matrix,
 *   Y[i][c] = s after  s = 0.0;  s = fma(S[i][r], C[r*kc + c], s), r = 0, 1, ...
 * This fixes the bits of every element: the CPU statement of
 * spmv_block_combine_multi (spmv_ext.h).  A zero in C does not skip a term, so
 * an Inf or NaN in S[i][r] reaches every Y[i][c].  A row of S is read before
 * that row of Y is written; Y must not overlap an operand otherwise.  Nothing is
 * read or written outside the columns of a row or at or past row n.
 * SPMV_OTHER_ERROR, before anything is written, for a negative n, kc outside
 * 1..8, a ka outside 0..8 or all three 0, a leading dimension below its width,
 * or a NULL array that would be read or written.                             */
int spmv_cpu_block_combine_multi(int64_t n, int32_t kc, const double *C, int32_t ka0, const double *A0,
                                 int64_t lda0, int32_t ka1, const double *A1, int64_t lda1, int32_t ka2,
                                 const double *A2, int64_t lda2, double *Y, int64_t ldy);
/* The three basis statements of restarted GMRES (iterate.gmres): V is a
 * row-major block (V[i*ldv + j], i < n, j < c <= ldv, 1 <= c <= 32), w, w_out,
 * t and v single columns with a leading dimension of their own (element i at
 * [i*ld], ld >= 1), h, y and s HOST arrays of c, c and 1 doubles.
 * project:   w_out[i] = s after  s = w[i];  s = fma(-h[j], V[i][j], s), j = 0, 1, ...
 *            (w_out may be w itself: an element is read before it is written)
 * combine:   t[i] = s after  s = 0.0;  s = fma(V[i][j], y[j], s), j = 0, 1, ...
 * normalize: v[i] = w[i] * r,  r = 1 / sqrt(s[0]), and 0.0 when s[0] <= 0.0;
 *            copy, if not NULL, is a contiguous vector that receives the same
 *            values; v may be w.
 * These fix the bits of every element: the CPU statements of
 * spmv_krylov_project_dot (its w_out; its sums are fixed by spmv_dot_multi),
 * spmv_krylov_combine and spmv_krylov_normalize (spmv_ext.h).  Nothing else is
 * read or written.  SPMV_OTHER_ERROR, before anything is written, for a
 * negative n, c outside 1..32, ldv < c, another leading dimension below 1 or a
 * NULL array that would be read or written.                                 */
int spmv_cpu_krylov_project(int64_t n, int32_t c, const double *V, int64_t ldv, const double *h,
                            const double *w, int64_t ldw, double *w_out, int64_t ldo);
int spmv_cpu_krylov_combine(int64_t n, int32_t c, const double *V, int64_t ldv, const double *y,
                            double *t, int64_t ldt);
int spmv_cpu_krylov_normalize(int64_t n, const double *s, const double *w, int64_t ldw, double *v,
                              int64_t ldv, double *copy);
/* Y = A^T X for k >= 1 vectors stored row-major, the layout of
 * spmv_plan_run_t_multi (spmv.h): X[r*ldx + j], r < n_rows; Y[c*ldy + j],
 * c < n_cols; j < k; ldx >= k, ldy >= k.  Serial: zeroes Y[c*ldy + j], j < k,
 * then scatters row by row in CSR order, so column j has the bits of
 * spmv_cpu_csr_t on column j.  Writes nothing for j >= k or at or past row
 * n_cols and reads nothing of X outside [r*ldx, r*ldx + k).
 * SPMV_OTHER_ERROR for negative sizes, k < 1, a leading dimension below k, a
 * column outside [0, n_cols) or a NULL array that would be read or written. */
int spmv_cpu_csr_t_multi(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr,
                         const int32_t *col, const double *val, int32_t k, const double *X,
                         int64_t ldx, double *Y, int64_t ldy);
int spmv_cpu_ell(int64_t n_rows, int32_t K, int64_t ld, int32_t ki,
                 const int32_t *col, const double *val, const double *x,
                 double *y, int threads);
int spmv_cpu_sell(int64_t n_rows, int32_t C, int32_t ki, int64_t n_slices,
                  const int64_t *slice_ptr, const int32_t *perm,
                  const int32_t *col, const double *val, const double *x,
                  double *y, int threads);
int spmv_cpu_cmrs(int64_t n_rows, int32_t h, int64_t n_strips,
                  const int64_t *strip_ptr, const uint8_t *row_in_strip,
                  const int32_t *col, const double *val, const double *x,
                  double *y, int threads);
int spmv_cpu_threads(void);

/* ------------------------------------------------------ result check ---
 * The reference's check_result (inc/helper_functions.h:184-236): y_ref
 * is accumulated sequentially in FILE ORDER.  Returns the number of rows
 * that fail; *first_bad gets the first failing row (-1 if none).
 * abs_tol > 0: the reference's |y - y_ref| <= 1e-6 rule;
 * rel_tol > 0: |y - y_ref| <= rel_tol * max(|y_ref|, sum_j |a_ij x_j|).  */
int64_t spmv_check(int64_t n_rows, int64_t nnz, const int32_t *row,
                   const int32_t *col, const double *val, const double *x,
                   const double *y, double abs_tol, double rel_tol,
                   int64_t *first_bad, double *y_ref_at_bad);

/* --------------------------------------------------------- generators ---
 * Deterministic (splitmix64 counter-based), identical on every host.
 *
 * cant-like stand-in for SuiteSparse cant (N = M = 62,451 = 3 dof x
 * 9x9x257 nodes, 27-node neighbourhood).  The pattern is thinned
 * symmetrically to exactly 4,007,383 entries (2,034,917 in the lower
 * triangle incl. diagonal) — the real cant's counts.  mode:
 *   0 = full pattern, row-major order          ("cant-sorted" shape)
 *   1 = full pattern, column-major order       ("cant" shape)
 *   2 = lower triangle only, column-major order (SuiteSparse storage;
 *       banner symmetric — the reference multiplies it literally)
 * `copies` > 1 stacks that many independent copies block-diagonally.
 * Call with row == NULL to get *nnz only.                              */
int spmv_gen_cantlike(int mode, int64_t copies, int64_t *n_rows,
                      int64_t *nnz, int32_t *row, int32_t *col, double *val);
/* R-MAT (a,b,c,d) = (0.57,0.19,0.19,0.05) on 2^scale ids, rejection to
 * [0,n); exactly nnz entries, duplicates kept; values uniform [-1,1).
 * Entries in generation order.                                         */
int spmv_gen_rmat(int64_t n, int64_t nnz, int scale, uint64_t seed,
                  int32_t *row, int32_t *col, double *val);
/* Banded: row i has 16 entries at columns (i + o) mod n, o in -8..7,
 * directly in CSR form (row_ptr[n+1], col[16n], val[16n]).             */
int spmv_gen_banded_csr(int64_t n, uint64_t seed, int64_t row_begin,
                        int64_t row_end, int64_t *row_ptr, int32_t *col,
                        double *val);
/* Uniformly random sparse matrix with row lengths in [min_len,max_len]
 * (test helper for ragged inputs), CSR order.                          */
int spmv_gen_random(int64_t n_rows, int64_t n_cols, int64_t min_len,
                    int64_t max_len, uint64_t seed, int64_t *nnz,
                    int32_t *row, int32_t *col, double *val);
/* splitmix64 of (seed, index), exported for tests. */
uint64_t spmv_splitmix64(uint64_t seed, uint64_t index);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HOST_H */
