/*
 * oneshotdet_hip_class_sweep.h — C-ABI of liboneshotdet_hip.so, sixth part: the class sweep, K category slots (support sets) per
 * target image in one pass.  The target pyramid is computed once per image; the two places where it enters the per-(image,
 * category) work read ONE pyramid from K rows.  Same conventions as oneshotdet_hip.h (raw device pointers, asynchronous on
 * `stream`, 0 = OK / negative = OSD_ERR_*); paths relative to the reference's maskrcnn_benchmark/.  The ABI version is unchanged.
 */
#ifndef ONESHOTDET_HIP_CLASS_SWEEP_H
#define ONESHOTDET_HIP_CLASS_SWEEP_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Query vectors a workgroup of osd_correlate_levels_sweep stages in LDS, and products it stores per 16-byte load of x. */
#define OSD_CLASS_SWEEP_GROUP 8

/* OSD_CLASS_SWEEP_GROUP, from the built library (the binding and the tests read it here). */
int osd_class_sweep_group(void);

/* modeling/detector/generalized_rcnn.py:307-311 run `classes` times on the same image, in one launch for all levels:
 *   xs[l] [n][hw_l][c] (dtype), qs[l] [n*classes][c] fp32, ys[l] [n*classes][hw_l][c] (dtype),
 *   ys[l][b*classes + k] = xs[l][b] * qs[l][b*classes + k]   (broadcast over the pixels)
 * A workgroup stages up to OSD_CLASS_SWEEP_GROUP query vectors of its image in LDS, loads each 16-byte chunk of x once and stores
 * one product per staged vector; the last group of an image is short when `classes` is no multiple of the group.  Per element
 * the arithmetic is osd_correlate_levels' (fp32 product, then the store conversion): the same bits as that entry on `classes`
 * times replicated xs, and with classes == 1 its result.  Levels with hws[l] <= 0 are skipped.  Channel rule as
 * osd_correlate_levels.  OSD_ERR_INVALID_ARG for null arrays or tensors, n < 0, classes < 1, a bad channel count or dtype; nothing
 * is launched then.  n == 0 is a no-op. */
int osd_correlate_levels_sweep(int n_levels, const void* const* xs, const float* const* qs, void* const* ys, const int32_t* hws,
                               int n, int classes, int c, int dtype, void* stream);

/* modeling/poolers.py:93-124 run for `sets_per_image` ROI sets on the same image: osd_roi_pool_levels with level maps
 * xs[l] [n_sets / sets_per_image][h_l][w_l][c]; ROI set j (boxes [n_sets][max_rois][4], counts [n_sets] or null) reads image
 * j / sets_per_image.  y, y_stride and level_out as osd_roi_pool_levels.  The same device code as that entry, so the same bits as
 * that entry on replicated maps.  OSD_ERR_INVALID_ARG as osd_roi_pool_levels, and for sets_per_image < 1 or
 * n_sets % sets_per_image != 0; nothing is launched then. */
int osd_roi_pool_levels_sweep(int n_levels, const void* const* xs, const int32_t* hs, const int32_t* ws, const float* scales,
                              const float* boxes, const int32_t* counts, void* y, int n_sets, int sets_per_image, int c,
                              int max_rois, int pool, int sampling_ratio, int y_stride, int32_t* level_out, int dtype,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_CLASS_SWEEP_H */
