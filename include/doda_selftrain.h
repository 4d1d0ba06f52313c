/*
 * doda_selftrain.h — companion C ABI of libdoda_hip.so: pseudo-label generation for the self-training
 * stage (reference tool/st.py:345-366,403-405, util/pseudo_labels_util.py, model/unet.py:115-132).
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C",
 * plain device pointers + sizes, an explicit HIP stream, an int status.  Nothing here allocates device
 * memory or synchronises.  The core header's surface (ABI 12) is unchanged; this header carries its own
 * version, DODA_ST_ABI_VERSION, and the same library exports both.
 *
 * The store: one (class uint8, confidence fp32) pair per target point, dataset-wide per rank.  The
 * per-class quantile of the reference (pandas groupby + list.sort over every point, then
 * sorted[max(1, int(r * n)) - 1]) becomes an exact radix select over the fp32 bit patterns of the
 * confidences (positive floats order as their uint32 bits): DODA_ST_RADIX_LEVELS passes of
 * DODA_ST_RADIX_BITS bits each, the host picking per class the bin that holds the wanted rank between
 * passes.  Histograms are int64 and order-independent, so they sum exactly across ranks.
 */
#ifndef DODA_SELFTRAIN_H
#define DODA_SELFTRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_ST_ABI_VERSION 1

#define DODA_ST_MAX_CLASSES 32
#define DODA_ST_RADIX_BITS 8      /* bins per class and level: 1 << DODA_ST_RADIX_BITS */
#define DODA_ST_RADIX_LEVELS 4    /* 4 x 8 bits = the whole fp32 key */

int32_t doda_st_abi_version(void);

/* Replaces the confidence / prediction of model/unet.py:115-132 (softmax(output).max(1)) and the point scores of
 * model/unet.py:62-64 (Linear applied to out.features[p2v]) at VOXEL level: every point of a voxel has its voxel's logits.
 * feats [m, c] bf16 (elem_bytes 2) or fp32 (4), c in {16, 32}; weight fp32 [n_cls, c] (rounded to bf16 first for bf16
 * features, as doda_head_ce_fwd does), bias fp32 [n_cls] or NULL, 2 <= n_cls <= DODA_ST_MAX_CLASSES.
 * pred int32 [m] = argmax (lowest index on ties) — bit-identical to doda_head_ce_fwd's pred on the same inputs;
 * conf fp32 [m] = 1 / sum_k exp(z_k - z_max). */
int doda_st_voxel_confidence(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                             int32_t n_cls, int32_t *pred, float *conf, doda_stream_t stream);

/* Replaces the per-point gather of tool/st.py's test_model_fn + util/pseudo_labels_util.py:93-104 (the groupby that files every
 * target point's confidence under its predicted class): for i < n_points, store_cls[offset + i] = pred[p2v[i]] and
 * store_conf[offset + i] = conf[p2v[i]]; p2v int32 [n_points] indexes pred / conf [m].  hist (or NULL): int64
 * [n_cls][1 << DODA_ST_RADIX_BITS], ADDED to: the level-0 histogram of the points written (doda_st_radix_hist, level 0).
 * store_len: the store's length (offset + n_points must fit). */
int doda_st_point_store(const int32_t *pred, const float *conf, int32_t m, const int32_t *p2v, int64_t n_points, int32_t n_cls,
                        uint8_t *store_cls, float *store_conf, int64_t store_len, int64_t offset, int64_t *hist,
                        doda_stream_t stream);

/* Replaces the per-class sort of util/pseudo_labels_util.py:105-142 by one radix level: for every stored point i < n with
 * class c = store_cls[i] whose key (the bits of store_conf[i]) agrees with prefix[c] above this level's bits
 * (key >> (32 - 8 * level) == prefix[c]; every point at level 0), hist[c][(key >> (24 - 8 * level)) & 255] += 1.
 * prefix: int32 [n_cls] (bit pattern; -1 = class finished, counts nothing; ignored at level 0); hist int64
 * [n_cls][256], ADDED to.  0 <= level < DODA_ST_RADIX_LEVELS. */
int doda_st_radix_hist(const uint8_t *store_cls, const float *store_conf, int64_t n, int32_t n_cls, int32_t level,
                       const int32_t *prefix, int64_t *hist, doda_stream_t stream);

/* Replaces model/unet.py:127-132 (confidence_mask = confidence > thres[pseudo_label]; pseudo_labels[~mask] = ignore) and the
 * class histogram of util/pseudo_labels_util.py:39-40: labels[i] = store_conf[i] > thres[store_cls[i]] ? store_cls[i] : ignore
 * (uint8), kept[c] += points of class c kept.  thres fp32 [n_cls]: the strict lower bounds (a float64 threshold rounded toward
 * -inf to fp32 compares the same against every fp32 confidence); kept int64 [n_cls], ADDED to; 0 <= ignore <= 255. */
int doda_st_label(const uint8_t *store_cls, const float *store_conf, int64_t n, int32_t n_cls, const float *thres, int32_t ignore,
                  uint8_t *labels, int64_t *kept, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_SELFTRAIN_H */
