/*
 * doda_spconv.h — companion C ABI of libdoda_hip.so: the rest of the spconv v1.2 surface a network can name beside the layers of
 * the core header — the rulebook of a transposed sparse convolution (SparseConvTranspose3d), indice max pooling for fp32 and bf16
 * rows without float atomics, and the moves between a sparse tensor and its dense volume (SparseConvTensor.dense / from_dense).
 * The arithmetic of the transposed convolution is the core header's: doda_spconv_gather_ex and doda_spconv_wgrad_multi over the
 * pair of tables built here, exactly as for the generic strided convolution.
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device pointers +
 * sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises; sizes, element sizes and
 * null pointers are checked on the host before anything launches (DODA_ERR_INVALID, DODA_ERR_UNSUPPORTED, DODA_ERR_WORKSPACE); a
 * count of zero is DODA_OK with nothing but the documented fills.  The core header's surface (ABI 12) and the other companions are
 * unchanged; this header carries its own version, DODA_SPCONV_ABI_VERSION.
 *
 * elem_bytes is 4 (fp32) or 2 (bf16) everywhere.  Indices are int32 [rows][4] = (batch, x, y, z).  No kernel here uses a float
 * atomic or an atomic cursor: every result is a function of the inputs alone, bit for bit.
 */
#ifndef DODA_SPCONV_H
#define DODA_SPCONV_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_SPCONV_ABI_VERSION 1

#define DODA_SPCONV_MAX_KERNEL_VOLUME 27   /* most kernel offsets of a rulebook built here (as the core header's generic builder) */
#define DODA_SPCONV_DENSE_CHUNK 1024       /* cells per workgroup of the from-dense passes; the workspace holds one count per chunk */

int32_t doda_spconv_abi_version(void);

/* ---- transposed convolution rulebook -------------------------------------------------------------------------------------------
 * Input p reaches the output cell q = p * stride - padding + k * dilation through kernel offset k (row-major offset index), for
 * the q inside out_shape = (in - 1) * stride - 2 * padding + kernel + output_padding (the formula ignores dilation: positions
 * beyond it are dropped).  Only reached cells exist.  Outputs are numbered in first-touch order of the serial scan: inputs
 * ascending, each input's positions from its upper bound p * stride - padding + (kernel - 1) * dilation downwards, last axis
 * fastest.  The two calls mirror doda_rulebook_conv_assign / doda_rulebook_conv_tables: the first counts the outputs (*count_out,
 * device int32, and out_shape_h, host int32 [3]), the second writes out_indices [m_out][4], tbl [K][ld_out] (the input row that
 * feeds output t through offset o, or -1) and tbl_rev [K][ld_in] (the output that input j reaches through offset o, or -1) from
 * the same workspace, which must not be touched in between.  For a fixed offset p -> q is injective, so no table entry is written
 * twice.  DODA_ERR_INVALID: a null host array, m < 0, kernel / stride / dilation < 1, padding or output_padding < 0, an output
 * extent < 1 or >= 2^31, ld_out < m_out, ld_in < m, a null device pointer with m > 0.  DODA_ERR_UNSUPPORTED: K >
 * DODA_SPCONV_MAX_KERNEL_VOLUME or m * K >= 2^30.  DODA_ERR_WORKSPACE: ws_bytes below doda_rulebook_deconv_workspace_bytes(m, K)
 * (which is 0 for an unsupported size).  DODA_ERR_GRID_TOO_LARGE as in the core header.  m == 0: *count_out = 0. */
size_t doda_rulebook_deconv_workspace_bytes(int32_t m, int32_t K);
int doda_rulebook_deconv_assign(const int32_t *indices, int32_t m, const int32_t *shape_h, int32_t batch, const int32_t *ksize_h,
                                const int32_t *stride_h, const int32_t *pad_h, const int32_t *dil_h, const int32_t *outpad_h,
                                int32_t *out_shape_h, int32_t *count_out, void *ws, size_t ws_bytes, doda_stream_t stream);
int doda_rulebook_deconv_tables(const int32_t *indices, int32_t m, const int32_t *shape_h, int32_t batch, const int32_t *ksize_h,
                                const int32_t *stride_h, const int32_t *pad_h, const int32_t *dil_h, const int32_t *outpad_h,
                                int32_t m_out, int32_t *out_indices, int32_t *tbl, int32_t ld_out, int32_t *tbl_rev, int32_t ld_in,
                                void *ws, size_t ws_bytes, doda_stream_t stream);

/* ---- indice max pooling ----------------------------------------------------------------------------------------------------------
 * Forward, over tbl [K][ld] of the outputs: y[t][ch] = max(0, max over o of x[tbl[o][t]][ch]) — upstream's semantics, the output
 * starts at 0; entries outside [0, n_in) are skipped; NaN never wins.  Rows move as 16-byte pieces where c * elem_bytes is a
 * multiple of 16 (and x, y are 16-byte aligned), element by element otherwise.
 * Backward, input-stationary over tbl_rev [K][ld] of the inputs: dx[j][ch] = sum over o of dy[t][ch] * [x[j][ch] == y[t][ch]] with
 * t = tbl_rev[o][j] (entries outside [0, n_out) are skipped), accumulated in fp32 in ascending o, rounded once, every dx row
 * written exactly once: no atomic, and dx needs no zero fill.
 * DODA_ERR_INVALID: c <= 0, K <= 0, a negative row count, ld below the rows the table covers, a null pointer that the sizes make
 * necessary.  DODA_ERR_UNSUPPORTED: elem_bytes not 2 or 4. */
int doda_maxpool_fwd(const void *x, int32_t c, int32_t elem_bytes, const int32_t *tbl, int32_t ld, int32_t K, int32_t n_in,
                     int32_t n_out, void *y, doda_stream_t stream);
int doda_maxpool_bwd(const void *x, const void *y, const void *dy, int32_t c, int32_t elem_bytes, const int32_t *tbl_rev, int32_t ld,
                     int32_t K, int32_t n_in, int32_t n_out, void *dx, doda_stream_t stream);

/* ---- dense volume <-> rows -------------------------------------------------------------------------------------------------------
 * The volume is [batch][X][Y][Z][c] (channels_first == 0) or [batch][c][X][Y][Z] (channels_first != 0); shape_h = host {X, Y, Z}.
 * doda_dense_scatter zero-fills the whole volume and writes row r at indices[r]; rows outside the grid are skipped; indices must
 * be unique (two rows of one cell: either may win).  doda_dense_gather reads row r back from indices[r] (zeros for a row outside
 * the grid): the gradient of the scatter, and the scatter is the gradient of the gather.  Bits move unchanged.  In the
 * channels-first layout one lane handles one row and writes channel after channel, so a wavefront writes one channel of 64
 * consecutive rows at a time.
 * DODA_ERR_INVALID: m < 0, c <= 0, batch or an extent < 1, a volume of 4e18 bytes or more, a null shape_h or volume, a null rows /
 * indices with m > 0.  DODA_ERR_UNSUPPORTED: elem_bytes not 2 or 4. */
int doda_dense_scatter(const void *rows, const int32_t *indices, int32_t m, int32_t c, int32_t elem_bytes, int32_t batch,
                       const int32_t *shape_h, int32_t channels_first, void *volume, doda_stream_t stream);
int doda_dense_gather(const void *volume, const int32_t *indices, int32_t m, int32_t c, int32_t elem_bytes, int32_t batch,
                      const int32_t *shape_h, int32_t channels_first, void *rows, doda_stream_t stream);

/* from_dense over a channels-last volume of `cells` = batch * X * Y * Z cells: a cell is active iff any of its c channels is
 * non-zero (-0 counts as zero, NaN as non-zero).  doda_from_dense_count stores the active cells of every chunk of
 * DODA_SPCONV_DENSE_CHUNK cells in the workspace and their total in *count_out (device int32); doda_from_dense_emit, given that
 * total as m_out after the caller's one read-back, writes the active cells in ascending (row-major) cell order: indices
 * [m_out][4] and their feature rows [m_out][c], by a stable compaction over the stored counts (no scan launch, no atomic cursor).
 * DODA_ERR_INVALID: c <= 0, batch or an extent < 1, a null pointer, m_out < 0.  DODA_ERR_UNSUPPORTED: elem_bytes not 2 or 4, or
 * more than 2^31 - 1 - DODA_SPCONV_DENSE_CHUNK cells.  DODA_ERR_WORKSPACE: ws_bytes below doda_from_dense_workspace_bytes(cells) (0 for an unsupported count). */
size_t doda_from_dense_workspace_bytes(int64_t cells);
int doda_from_dense_count(const void *volume, int32_t c, int32_t elem_bytes, int32_t batch, const int32_t *shape_h,
                          int32_t *count_out, void *ws, size_t ws_bytes, doda_stream_t stream);
int doda_from_dense_emit(const void *volume, int32_t c, int32_t elem_bytes, int32_t batch, const int32_t *shape_h, int32_t m_out,
                         int32_t *indices, void *rows, const void *ws, size_t ws_bytes, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_SPCONV_H */
